/*
 * svt_hip_cfl.h -- C-ABI of the batched chroma-from-luma prediction and of the alpha search of the MI355X path.
 *
 * svt_hip_cfl_pred_batch.  One job = one chroma block of a 4:2:0 picture, both chroma planes: what compute_cfl_ac_components
 * (Source/Lib/Codec/product_coding_loop.c:3751-3786) and av1_cost_calc_cfl (:3453-3617) do between the luma reconstruction and the chroma
 * prediction, bit-exact with the reference's C path at 8 bits (uint8 planes) and 10 bits (packed uint16 planes):
 *   sub-sampling  svt_cfl_luma_subsampling_420_{lbd,hbd}_c (Codec/intra_prediction.c:420-443): over the 2W x 2H luma samples at
 *                 (luma_x, luma_y) of the luma plane, q3 = (a + b + c + d) << 1 per 2x2.  The host passes the origin rounded the reference's way
 *                 ((org >> 3) << 3 for the sub-8 luma blocks, :3758); the luma extent is always twice the chroma block (:3769-3770)
 *   average       svt_subtract_average_c (:448-465): avg = (sum + ((W * H) >> 1)) >> (log2 W + log2 H), ac = q3 - (int16_t)avg
 *   prediction    svt_cfl_predict_{lbd,hbd}_c (C_DEFAULT/cfl_c.c) per requested alpha_q3 and per plane:
 *                 clip_pixel_highbd(ROUND_POWER_OF_TWO_SIGNED(alpha_q3 * ac, 6) + dc, bit_depth), dc the job's block of that plane's
 *                 DC-prediction plane (svt_hip_intra_pred_batch can have written it)
 * The prediction for alpha_q3[k] of a job goes to dst_offset[p] + k * slot_stride of plane p's destination (the plane svt_hip_rd_batch reads:
 * every slot is one SvtHipTxJob.pred_offset), its rows dst_stride apart.  W and H are each 4, 8, 16 or 32: the reference allows CfL up to 32x32
 * luma, i.e. the nine {4, 8, 16}^2 chroma shapes; 32 is what CFL_BUF_LINE admits and the _c leaves accept.
 *
 * The kernel reads no luma sample outside the job's 2W x 2H extent and none outside the luma plane's width x height; a lane loads the
 * 8 x 2 samples under its four chroma samples and nothing else.
 *
 * Defined where the reference is not.  A job gets status 0xFF, writes nothing else and reads nothing outside the planes, when its luma extent
 * leaves the luma plane (luma_x / luma_y negative, luma_x + 2W > luma_width, luma_y + 2H > luma_height), its DC block leaves a DC plane
 * (dc_samples), or any of its n_alpha slots ends outside a destination (dst_samples).  Every other job writes status 0.  Slots of one batch
 * that overlap each other are the caller's error: the bytes there are those of one of the writers.
 *
 * svt_hip_cfl_pick_alpha_batch.  One block = one call of md_cfl_rd_pick_alpha (Codec/product_coding_loop.c:3624-3748), replayed over a complete
 * cost table instead of interleaved with the evaluations: the reference runs av1_cost_calc_cfl once per alpha it tries, here every alpha of
 * every block has been one job of svt_hip_rd_batch / svt_hip_coeff_rate_batch.  Slot k of a plane is alpha_q3 = k - 16 (the list -16 .. 16 of
 * svt_hip_cfl_pred_batch), SVT_HIP_CFL_SLOTS per plane:
 *   bits[(b * 2 + plane) * 33 + k]                 as svt_hip_coeff_rate_batch writes it
 *   dist[((b * 2 + plane) * 33 + k) * dist_stride] DIST_CALC_RESIDUAL as the reference's loop sees it; dist_stride 0 counts as 1, 2 reads the
 *                                                  first column of SvtHipRdBatchDesc.dist_coeff in place; the caller's shifts of the
 *                                                  distortion stay with the caller
 *   mode_bits[b]                                   intra_uv_mode_fac_bits[CFL_ALLOWED][pred_mode][UV_CFL_PRED]
 *   alpha_fac_bits[8][2][16]                       MdRateEstimationContext.cfl_alpha_fac_bits
 * The replay keeps the reference's order (plane, then sign NEG / POS, then c), the `c > itr_th && progress < c` break, the
 * PLANE_SIGN_TO_JOINT_SIGN pairing over i with the strict `>=` comparisons, the best_rd_uv[js][!plane] == MAX_MODE_COST test and
 * mode_rd = RDCOST(lambda, mode_bits, 0).  The break only skips evaluations, so the replay on the full table gives the reference's result.
 * The reference's `coeff_bits == INT64_MAX` tests cannot fire: svt_aom_full_loop_uv never produces that value, and the replay has no such
 * branch.
 *
 * Per block: best_rd (SVT_HIP_CFL_MAX_MODE_COST when no pair was found), cfl_alpha_idx and cfl_alpha_signs -- 0, 0 when
 * best_rd == MAX_MODE_COST, where the reference leaves its two outputs untouched: defined here -- and a status byte:
 *   bit 0 (SVT_HIP_CFL_PICK_TRUNCATED)  n_mag < 16 and a magnitude loop reached c == n_mag where the reference's break would not have fired: the
 *                                       reference would have evaluated an alpha the table does not hold, so the result may differ from its
 *   0xFF (SVT_HIP_CFL_PICK_UNDEFINED)   a bits entry the replay reads is UINT64_MAX (svt_hip_coeff_rate_batch's undefined job): best_rd =
 *                                       MAX_MODE_COST, idx = signs = 0
 *
 * Out of scope: 4:2:2 / 4:4:4 sub-sampling, 12-bit, the encode pass's own call (Codec/coding_loop.c:240; the `ac` output is what it needs), and
 * pointer-level leaves for the rtcd entries (one call per block; the batch is the boundary).
 */
#ifndef SVT_HIP_CFL_H
#define SVT_HIP_CFL_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_CFL_SLOTS 33 /* CFL_MAGS_SIZE: alpha_q3 -16 .. 16 */
#define SVT_HIP_CFL_OK 0
#define SVT_HIP_CFL_UNDEFINED 0xFF
#define SVT_HIP_CFL_PICK_TRUNCATED 1
#define SVT_HIP_CFL_PICK_UNDEFINED 0xFF
#define SVT_HIP_CFL_MAX_MODE_COST (13754408443200ull * 8) /* MAX_MODE_COST, Codec/coding_unit.h:38 */

typedef struct SvtHipCflPredJob {
    int32_t  luma_x, luma_y; /* the first of the job's 2W x 2H luma samples in the luma plane */
    uint32_t dc_offset[2];   /* of the block's first sample in each plane's DC plane, in samples */
    uint32_t dst_offset[2];  /* of slot 0's first sample in each plane's destination, in samples */
} SvtHipCflPredJob;

typedef struct SvtHipCflPlane { /* one chroma plane: Cb, Cr */
    const void *dc;          /* device pointer: the DC-prediction plane */
    uint32_t    dc_stride;   /* in samples */
    uint32_t    dst_stride;  /* in samples */
    uint64_t    dc_samples;  /* samples the DC plane holds from `dc` on: a block that does not end inside is undefined */
    void       *dst;         /* device pointer: the prediction plane the slots go to */
    uint64_t    dst_samples; /* samples the destination holds from `dst` on: a slot that does not end inside makes the job undefined */
} SvtHipCflPlane;

typedef struct SvtHipCflPredDesc {
    uint8_t  bit_depth;      /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  width, height;  /* of the chroma block, each 4, 8, 16 or 32, shared by the batch */
    uint8_t  n_alpha;        /* 1 .. 33 */
    uint32_t n_jobs;
    int8_t   alpha_q3[SVT_HIP_CFL_SLOTS]; /* each -16 .. 16, in any order; the alpha search passes -16 .. 16 */
    uint8_t  reserved[7];
    const void *luma;        /* device pointer: the luma plane's sample (0, 0) */
    uint32_t luma_stride;    /* in samples */
    uint32_t luma_width, luma_height; /* in samples: no read leaves them */
    uint32_t slot_stride;    /* in samples: slot k of a job starts k * slot_stride behind its slot 0 */
    SvtHipCflPlane plane[2];
    const SvtHipCflPredJob *jobs; /* device pointer, n_jobs entries */
    uint8_t *status;         /* device pointer, [n_jobs]: SVT_HIP_CFL_OK / SVT_HIP_CFL_UNDEFINED */
    int16_t *ac;             /* optional device pointer, 8-byte aligned: [n_jobs][H][W] the AC of the sub-sampled luma, for tests and the encode pass;
                              * an undefined job's block is not written */
} SvtHipCflPredDesc;

typedef struct SvtHipCflPickDesc {
    uint32_t n_blocks;
    uint32_t lambda;         /* full_lambda_md[] of the depth */
    uint8_t  itr_th;         /* cfl_ctrls.itr_th: 1 or 2 (set_cfl_ctrls, Codec/enc_mode_config.c:6432-6445); 0 .. 16 accepted */
    uint8_t  n_mag;          /* magnitudes the table holds per sign, 1 .. 16: slots 16 - n_mag .. 16 + n_mag are read */
    uint8_t  reserved[2];
    uint32_t dist_stride;
    const uint64_t *bits;    /* device pointers */
    const uint64_t *dist;
    const int32_t  *mode_bits;      /* [n_blocks] */
    const int32_t  *alpha_fac_bits; /* [8][2][16] */
    uint64_t *best_rd;       /* [n_blocks] */
    uint8_t  *cfl_alpha_idx; /* [n_blocks]: (u << 4) + v, ModeDecisionCandidate.cfl_alpha_idx */
    uint8_t  *cfl_alpha_signs; /* [n_blocks]: the joint sign */
    uint8_t  *status;        /* [n_blocks] */
} SvtHipCflPickDesc;

/* Enqueues one batch on the context stream (asynchronous).  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and enqueues nothing when
 * svt_hip_cfl_pred_check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_cfl_pred_batch(SvtHipContext *ctx, const SvtHipCflPredDesc *d);
/* Host-only validation: a null descriptor or luma / jobs / status / a plane's dc or dst; a bit_depth other than 8 / 10; a width or height other
 * than 4 / 8 / 16 / 32; n_alpha 0 or above 33; an alpha outside -16 .. 16; a zero luma_stride, luma_width, luma_height, dc_stride, dst_stride or
 * slot_stride, a luma_stride below luma_width, zero dc_samples or dst_samples; an `ac` that is not 8-byte aligned; a destination range
 * (dst_samples from dst) that overlaps a DC plane or the luma plane: the jobs of one batch must not read what the batch writes. */
int    svt_hip_cfl_pred_check_desc(const SvtHipCflPredDesc *d);
/* Enqueues the alpha search of n_blocks blocks, one lane per block.  Returns SVT_HIP_ERR_BAD_PARAM and enqueues nothing for a null pointer
 * (all eight are mandatory), itr_th > 16, n_mag 0 or above 16; n_blocks == 0 returns 0 and enqueues nothing. */
int    svt_hip_cfl_pick_alpha_batch(SvtHipContext *ctx, const SvtHipCflPickDesc *d);
/* sizeof / offsetof as compiled, for the bindings: what = 0 the prediction descriptor, 1 its job, 2 its plane, 3 the pick descriptor; `field` < 0
 * the size, else the offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_cfl_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
