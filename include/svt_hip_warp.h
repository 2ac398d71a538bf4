/*
 * svt_hip_warp.h -- C-ABI of the batched warped-motion prediction, of the local-warp model fit and of its MV refinement of the MI355X path.
 *
 * svt_hip_warp_pred_batch.  One job = svt_av1_warp_plane (Source/Lib/Codec/warped_motion.c:681-895) on one plane of one block, as
 * plane_warped_motion_prediction calls it (Codec/enc_inter_prediction.c:2040-2145), over svt_av1_warp_affine_c (:569-679) and
 * svt_av1_highbd_warp_affine_c (:714-819); bit-exact with them for 8-bit planes (uint8) and 10-bit planes (packed uint16):
 *   tile       every 8x8 tile of the block projects its centre: src = (j + 4) << ss, dst = mat * src, x4 = dst_x >> ss_x, y4 = dst_y >> ss_y,
 *              (ix4, sx4) / (iy4, sy4) the integer and the 16-bit fractional part; sx4 += -4 * (alpha + beta), sy4 += -4 * (gamma + delta), both
 *              rounded down to a multiple of 64.  (p_col, p_row) is the block's origin on the plane itself
 *   filter     15 rows x 8 columns of an 8-tap horizontal filter (row k, column l: filter ROUND(sx4 + beta * (k + 4) + alpha * (l + 4), 10) + 64 of
 *              the 193 Warped_Filters of the AV1 specification), round_0 = 3, then 8 x 8 of the vertical one on gamma / delta
 *   single     vertical round 14 - round_0, clip(sum - (1 << (bd - 1)) - (1 << bd))
 *   compound   round_1 = 7: the first reference into the intermediate, the second averaged into it, (a + b) >> 1 or
 *              (a * fwd_offset + b * bck_offset) >> 4 on the eight pairs of quant_dist_lookup_table, then the two offsets off, a round shift
 *              by 4 and the clip.  One job computes both references: the intermediate stays in registers
 *   ROTZOOM    wmmat[4] = -wmmat[3], wmmat[5] = wmmat[2], as svt_warp_plane rewrites them; the four shear parameters are used as given
 * Block sizes on the plane: the 17 AV1 shapes with both dimensions in {8, 16, 32, 64, 128}.  A dimension below 8 never reaches the warp filter in
 * the reference: blk_geom->bwidth < 8 has no local warp (Codec/adaptive_mv_pred.c:1706), and the chroma of a luma block below 16x16 takes
 * chroma_plane_warped_motion_prediction_sub8x8 (enc_inter_prediction.c:1887, :2883), the translational predictor svt_hip_inter_pred_batch is.
 *
 * References.  width x height of a SvtHipWarpRef are the PICTURE's on this plane: the filter clamps every sample coordinate to
 * [0, width - 1] x [0, height - 1], so it never reads the padding and nothing about it is undefined in the reference.  The reference encoder
 * reads 10-bit planes as a split 8 + 2-bit pair; the packed value is the contract here, as in svt_hip_pred.h.
 *
 * The model of a reference is the job's own SvtHipWarpModel, or models[model_index[r]] with SVT_HIP_WARP_MODEL{0,1}_FROM_ARRAY: the array
 * svt_hip_warp_model_batch writes.  Status per job:
 *   0     SVT_HIP_WARP_OK
 *   0xFE  SVT_HIP_WARP_NO_MODEL: a model taken from the array has valid == 0; nothing else is written, so a chain needs no host look at the fit
 *   0xFF  SVT_HIP_WARP_UNDEFINED, nothing else written: width x height is not one of the 17 sizes, a reference or a used model index is outside
 *         its table, the block does not end inside dst_samples, comp_mode > 1 or (comp_mode 1) fwd_offset / bck_offset is not one of the eight
 *         pairs, wmtype is neither ROTZOOM nor AFFINE, a shear parameter is not a multiple of 64, or the four fail is_affine_shear_allowed
 *         (warped_motion.c:357-363).  The reference only asserts that the filter index stays in [0, 192]; the kernel refuses instead of reading
 *         past the table
 *
 * svt_hip_warp_model_batch.  One job = the MV-dependent half of svt_aom_warped_motion_parameters (Codec/adaptive_mv_pred.c:1736-1754):
 * svt_aom_select_samples (warped_motion.c:924-972) when n_samples > 1, svt_find_projection = find_affine_int + svt_get_shear_params (:365-483,
 * :898-921) with resolve_divisor_64 / _32 and the USE_LIMITED_PREC_MULT 0 forms of get_mult_shift_* (:277-289), and the two band tests unless
 * shut_approx.  The MV-independent half stays on the host: wm_find_samples over the neighbour arrays and the min_neighbour_perc test; the host
 * passes n_samples = 0 when either leaves the candidate without a model.  Samples are what av1_find_samples writes (1/8 sample, relative to
 * the block); the arithmetic is the reference's 32-bit one, which its asserts (LS_MAT_MIN .. LS_MAT_MAX) keep free of overflow.
 * Per job one SvtHipWarpModel: wmtype = AFFINE, num_samples as the reference sets *num_samples (whether or not the fit is valid), valid, and
 * the matrix and the four shear parameters -- all zero when valid == 0, where the reference leaves them half-written: defined here.
 * Status 0, or 0xFF and no record written: bwidth x bheight is not one of the 17 sizes, n_samples > 8, a used mv_index outside mv_array.
 *
 * svt_hip_wm_refine_batch.  One job = the search loop of svt_aom_wm_motion_refinement (Codec/mode_decision.c:2082-2204) for one block: the centre
 * and its four (refine_diag: eight) neighbours, the steps shifted by mv_prec_shift, offset (0, 0) in the first iteration only; mv_record with
 * its skip rule (a position is recorded BEFORE its fit is tested) and the prev_mv skip; up to `iterations` rounds, stopping when the centre does
 * not move.  Per tested MV: the fit above (an invalid fit is skipped); the 8-bit luma non-compound warp of the block at (blk_org_x, blk_org_y),
 * never written to memory; svt_aom_variance{W}x{H} of it against the source block as an int (sse - (uint32_t)((int64_t)sum * sum / (W * H)));
 * plus the MV rate against pred_mv: svt_aom_mv_err_cost (mvjcost / mvcost[2] / error_per_bit, the latter raised to at least 1 as the
 * reference does) or, with approx_inter_rate, svt_aom_mv_err_cost_light (Codec/av1me.c:229-252: 1296 + 50 * (|dcol| + |drow|)); strict `<`
 * against best_cost, which starts at INT_MAX.  MV components are int16 and wrap as the reference's Mv fields do.
 * Per job: best_mv = (row, col), the layout svt_hip_md_subpel_batch writes and svt_hip_warp_model_batch / svt_hip_inter_pred_batch read;
 * best_cost (INT_MAX, with the start MV, when no position had a valid fit); n_checked (tot_checked_pos).  Status 0, or 0xFF and nothing else
 * written: bwidth x bheight is not one of the 17 sizes, n_samples > 8, ref outside the table, a used mv_index outside mv_array, or the source
 * block does not end inside src_samples.  What stays on the host, after the sync the candidate needs anyway: svt_aom_choose_best_av1_mv_pred
 * and the is_valid_mv_diff test.
 *
 * Out of scope: the masked second reference (av1_make_masked_warp_inter_predictor), 12-bit, 4:2:2 and
 * 4:4:4 (ss_x != ss_y is computed as the formulas say but not pinned on the reference), scaled references, and pointer-level leaves for
 * svt_av1_warp_affine (one call per block; the batch is the boundary).  Global-motion estimation (global_me.c) is svt_hip_gm.h: its refinement warps
 * whole pictures with the tile arithmetic of these entries (csrc/warp_core.h).
 */
#ifndef SVT_HIP_WARP_H
#define SVT_HIP_WARP_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_WARP_MAX_REFS 8
#define SVT_HIP_WARP_NO_REF 0xFF          /* SvtHipWarpPredJob.ref[1] of a single-reference job */
#define SVT_HIP_WARP_MODEL0_FROM_ARRAY 1  /* SvtHipWarpPredJob.flags: the model of reference 0 is models[model_index[0]] */
#define SVT_HIP_WARP_MODEL1_FROM_ARRAY 2  /* the same for reference 1 */
#define SVT_HIP_WARP_MV_FROM_ARRAY 1      /* SvtHipWarpModelJob.flags: the MV is mv_array[mv_index] */
#define SVT_HIP_WARP_OK 0
#define SVT_HIP_WARP_NO_MODEL 0xFE
#define SVT_HIP_WARP_UNDEFINED 0xFF
#define SVT_HIP_WARP_ROTZOOM 2            /* TransformationType */
#define SVT_HIP_WARP_AFFINE 3
#define SVT_HIP_WARP_MAX_SAMPLES 8        /* LEAST_SQUARES_SAMPLES_MAX */

typedef struct SvtHipWarpModel { /* EbWarpedMotionParams, and what the fit says about it */
    int32_t  wmmat[6];
    int16_t  alpha, beta, gamma, delta;
    uint8_t  wmtype;          /* SVT_HIP_WARP_ROTZOOM / _AFFINE */
    uint8_t  valid;           /* written by svt_hip_warp_model_batch; read only for a model taken from the array */
    uint16_t num_samples;     /* written by svt_hip_warp_model_batch */
    uint32_t reserved;
} SvtHipWarpModel;

typedef struct SvtHipWarpRef {
    const void *plane;        /* device pointer to the first sample of the padded plane (uint8, or uint16 at 10 bits) */
    uint32_t    stride;       /* in samples */
    uint16_t    org_x, org_y; /* the picture's sample (0, 0) is plane[org_y * stride + org_x] */
    uint16_t    width, height; /* of the PICTURE on this plane: the limits every sample coordinate is clamped to */
    uint16_t    rows;         /* rows the padded plane holds */
    uint16_t    reserved;
} SvtHipWarpRef;

typedef struct SvtHipWarpPredJob {
    uint32_t dst_offset;      /* of the block's first sample in the destination plane, in samples */
    int16_t  p_col, p_row;    /* the block's origin on the plane (a sub-sampled plane's own coordinates) */
    uint8_t  width, height;   /* on this plane: one of the 17 sizes */
    uint8_t  ref[2];          /* indices into SvtHipWarpPredDesc.refs; ref[1] = SVT_HIP_WARP_NO_REF: single reference */
    uint8_t  flags;           /* SVT_HIP_WARP_MODEL*_FROM_ARRAY */
    uint8_t  comp_mode;       /* compound jobs: 0 average, 1 distance-weighted */
    uint8_t  fwd_offset, bck_offset; /* comp_mode 1 */
    uint32_t model_index[2];  /* per reference, with its flag */
    SvtHipWarpModel model[2]; /* per reference, without its flag */
} SvtHipWarpPredJob;

typedef struct SvtHipWarpPredDesc {
    uint8_t  bit_depth;       /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  ss_x, ss_y;      /* the plane's sub-sampling, 0 or 1 */
    uint8_t  n_refs;          /* 1..SVT_HIP_WARP_MAX_REFS */
    uint32_t n_jobs;
    SvtHipWarpRef refs[SVT_HIP_WARP_MAX_REFS];
    void    *dst;             /* device pointer: the prediction plane (the one svt_hip_rd_batch reads) */
    uint32_t dst_stride;      /* in samples */
    uint32_t reserved;
    uint64_t dst_samples;     /* samples the destination holds from `dst` on: a block that does not end inside is undefined */
    const SvtHipWarpPredJob *jobs; /* device pointer, n_jobs entries */
    const SvtHipWarpModel *models; /* optional device pointer, n_models entries: svt_hip_warp_model_batch's output */
    uint32_t n_models;
    uint32_t reserved2;
    uint8_t *status;          /* device pointer, [n_jobs] */
} SvtHipWarpPredDesc;

typedef struct SvtHipWarpModelJob {
    int32_t  pts[2 * SVT_HIP_WARP_MAX_SAMPLES];       /* (x, y) per sample, as av1_find_samples leaves them; not modified */
    int32_t  pts_inref[2 * SVT_HIP_WARP_MAX_SAMPLES];
    uint16_t blk_org_x, blk_org_y; /* the block's luma origin in the picture: mi_col = blk_org_x >> 2, mi_row = blk_org_y >> 2 */
    uint8_t  bwidth, bheight; /* blk_geom->bwidth / bheight: one of the 17 sizes */
    uint8_t  n_samples;       /* 0..8, before svt_aom_select_samples; 0: no model (valid = 0, num_samples = 0) */
    uint8_t  flags;           /* SVT_HIP_WARP_MV_FROM_ARRAY */
    int16_t  mv[2];           /* (row, col) in 1/8 luma sample */
    uint32_t mv_index;
} SvtHipWarpModelJob;

typedef struct SvtHipWarpModelDesc {
    uint32_t n_jobs;
    uint8_t  shut_approx;     /* non-zero: the two band tests are skipped */
    uint8_t  reserved;
    uint16_t lower_band_th, upper_band_th; /* wm_ctrls.lower_band_th / upper_band_th */
    uint16_t reserved2;
    uint32_t n_mvs;
    const SvtHipWarpModelJob *jobs; /* device pointer, n_jobs entries */
    const int16_t *mv_array;  /* optional device pointer, [n_mvs][2] = (row, col): the layout svt_hip_md_subpel_batch's best_mv has */
    SvtHipWarpModel *models;  /* device pointer, [n_jobs] */
    uint8_t *status;          /* device pointer, [n_jobs]: SVT_HIP_WARP_OK / SVT_HIP_WARP_UNDEFINED */
} SvtHipWarpModelDesc;

#define SVT_HIP_WM_START_FROM_ARRAY 1     /* SvtHipWmRefineJob.flags: the start MV is mv_array[mv_index] */
#define SVT_HIP_WM_MAX_ITERATIONS 16

typedef struct SvtHipWmRefineJob {
    int32_t  pts[2 * SVT_HIP_WARP_MAX_SAMPLES];       /* as in SvtHipWarpModelJob: every tested MV starts from these samples */
    int32_t  pts_inref[2 * SVT_HIP_WARP_MAX_SAMPLES];
    uint32_t src_offset;      /* input_origin_index: the block's top-left sample in the source plane */
    uint16_t blk_org_x, blk_org_y; /* ctx->blk_org_x / _y: the block's luma origin in the picture */
    uint8_t  bwidth, bheight; /* one of the 17 sizes */
    uint8_t  n_samples;       /* 0..8; 0: no position is valid */
    uint8_t  flags;           /* SVT_HIP_WM_START_FROM_ARRAY */
    int16_t  start_mv[2];     /* (row, col): cand->mv[list_idx] */
    int16_t  pred_mv[2];      /* (row, col): cand->pred_mv[list_idx], what the MV rate is measured against */
    uint32_t mv_index;
    uint8_t  ref;             /* index into SvtHipWmRefineDesc.refs */
    uint8_t  reserved[7];
} SvtHipWmRefineJob;

typedef struct SvtHipWmRefineDesc {
    uint32_t n_jobs;
    uint8_t  iterations;      /* wm_ctrls.refinement_iterations, 1..SVT_HIP_WM_MAX_ITERATIONS */
    uint8_t  refine_diag;     /* wm_ctrls.refine_diag */
    uint8_t  mv_prec_shift;   /* 0 with allow_high_precision_mv, else 1 */
    uint8_t  shut_approx;
    uint16_t lower_band_th, upper_band_th;
    uint8_t  approx_inter_rate; /* non-zero: svt_aom_mv_err_cost_light */
    uint8_t  n_refs;          /* 1..SVT_HIP_WARP_MAX_REFS */
    uint8_t  waves_per_job;   /* 0: the default (4); 1 or 4: the waves that share a job's tiles.  Measured (profiles/r10_warp.txt): four waves halve
                               * the time of 64x64 blocks, one wave is 2.3 times faster on 16x16 blocks -- pass 1 for batches of blocks below 32x32 */
    uint8_t  reserved;
    int32_t  error_per_bit;   /* full_lambda_md[EB_8_BIT_MD] >> RD_EPB_SHIFT; 0 counts as 1 */
    uint32_t src_stride;      /* in samples */
    const uint8_t *src;       /* device pointer: input_pic->buffer_y (8-bit) */
    uint64_t src_samples;     /* samples the source holds from `src` on */
    SvtHipWarpRef refs[SVT_HIP_WARP_MAX_REFS]; /* 8-bit luma planes */
    const SvtHipWmRefineJob *jobs; /* device pointer, n_jobs entries */
    const int16_t *mv_array;  /* optional device pointer, [n_mvs][2] = (row, col) */
    uint32_t n_mvs;
    uint32_t reserved2;
    const int32_t *mvjcost;   /* device pointer, 4 entries; unused with approx_inter_rate */
    const int32_t *mvcost[2]; /* device pointers to the CENTRE entries of the row / column tables, indices [-16384, 16384] */
    int16_t  *best_mv;        /* outputs, device pointers: [n_jobs][2] = (row, col) */
    int32_t  *best_cost;      /* [n_jobs] */
    uint32_t *n_checked;      /* [n_jobs] */
    uint8_t  *status;         /* [n_jobs] */
} SvtHipWmRefineDesc;

/* Enqueues the refinements of n_jobs jobs, a workgroup per job, its waves sharing the tiles of every warp.  Returns SVT_HIP_ERR_BAD_PARAM and
 * enqueues nothing for: a null src / jobs / best_mv / best_cost / n_checked / status; iterations outside 1..16; mv_prec_shift > 1; waves_per_job
 * other than 0, 1, 4; n_refs outside 1..8 or a reference svt_hip_warp_check_desc would refuse; a zero src_stride or src_samples; n_mvs without
 * mv_array; a negative error_per_bit; a null cost table without approx_inter_rate.  n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_wm_refine_batch(SvtHipContext *ctx, const SvtHipWmRefineDesc *d);
int    svt_hip_wm_refine_check_desc(const SvtHipWmRefineDesc *d);

/* Enqueues one batch on the context stream (asynchronous); one workgroup of four waves per job, a wave per 8x8 tile at a time.  Returns
 * SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and enqueues nothing when svt_hip_warp_check_desc refuses the descriptor; n_jobs == 0 returns 0
 * and enqueues nothing. */
int    svt_hip_warp_pred_batch(SvtHipContext *ctx, const SvtHipWarpPredDesc *d);
/* Host-only validation: null descriptor or dst / jobs / status, bit_depth other than 8 / 10, ss_x / ss_y > 1, n_refs outside
 * 1..SVT_HIP_WARP_MAX_REFS, a reference with a null plane, a zero stride, width or height, or a picture that lies outside its plane
 * (org_x + width > stride, org_y + height > rows), a zero dst_stride or dst_samples, n_models without models. */
int    svt_hip_warp_check_desc(const SvtHipWarpPredDesc *d);
/* Enqueues the fits of n_jobs jobs, one lane per job.  Returns SVT_HIP_ERR_BAD_PARAM and enqueues nothing for a null jobs / models / status or
 * n_mvs without mv_array; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_warp_model_batch(SvtHipContext *ctx, const SvtHipWarpModelDesc *d);
/* sizeof / offsetof as compiled, for the bindings: what = 0 the prediction descriptor, 1 its job, 2 the reference, 3 the model, 4 the model
 * descriptor, 5 its job, 6 the refinement descriptor, 7 its job; `field` < 0 the size, else the offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_warp_layout(int what, int field);
/* the 193 x 8 filter table and the 257 divisor multipliers as the kernels hold them, for the tests (host copies) */
const int16_t  *svt_hip_warp_filter_table(void);
const uint16_t *svt_hip_warp_div_lut(void);

#ifdef __cplusplus
}
#endif
#endif
