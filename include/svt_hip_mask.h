/*
 * svt_hip_mask.h -- C-ABI of the masked predictions of the MI355X path and of the searches that pick their parameters: masked compound
 * (COMPOUND_WEDGE, COMPOUND_DIFFWTD), inter-intra (smooth and wedge), pick_interinter_wedge, pick_interinter_seg and inter_intra_search.
 * With them an inter candidate of any compound type reaches svt_hip_rd_batch's prediction plane without leaving the device.
 *
 * svt_hip_masked_pred_batch   one job = svt_aom_enc_make_inter_predictor (Source/Lib/Codec/enc_inter_prediction.c:3274-3391) on one plane of
 *     one block, is_masked_compound = 0 for the first reference and 1 for the second (av1_make_masked_scaled_inter_predictor, :52-166), for
 *     unscaled references, translational motion and the packed 16-bit layout -- the scope of svt_hip_pred.h.  Both references are convolved
 *     into the CONV_BUF_TYPE intermediate (round_0 = 3, round_1 = 7, do_average = 0), then svt_aom_build_masked_compound_no_round
 *     (Codec/inter_prediction.c:2227-2268) blends them: svt_aom_lowbd_blend_a64_d16_mask_c / svt_aom_highbd_blend_a64_d16_mask_c
 *     (Codec/blend_a64_mask.c:34-195), all four subw / subh branches, the mask stride the luma block's width.
 *       wedge    the mask is svt_aom_get_contiguous_soft_mask(wedge_index, wedge_sign, luma bsize): a window of the twelve 64 x 64 primaries
 *                (init_wedge_primary_masks, get_wedge_mask_inplace, Codec/inter_prediction.c:1982-2087), which the library keeps once and
 *                indexes in place (direction, x_offset, y_offset from the codebooks, sign XOR sign-flip); the nine sizes with wedges
 *       DIFFWTD  a luma batch (plane 0) computes the mask from the two intermediates (svt_av1_build_compound_diffwtd_mask_d16_c,
 *                C_DEFAULT/inter_prediction_c.c:15-40: round = 4 + (bd - 8), base 38, DIFF_FACTOR 16, and the inverse) and, when the
 *                descriptor has a mask buffer, stores its luma_width x luma_height bytes at mask_buf + mask_offset; a chroma batch
 *                (plane != 0) reads it from there with the blend's sub-sampling rule; the 17 sizes with min(w, h) >= 8.
 *                Jobs of one batch run concurrently and a batch is all luma or all chroma: a chroma job reads its mask as a batch enqueued
 *                EARLIER on the stream left it (the same mask_buf and mask_offset); no job reads what a job of its own batch writes.
 * svt_hip_interintra_blend_batch   one job = svt_aom_combine_interintra / svt_aom_combine_interintra_highbd (Codec/inter_prediction.c:
 *     2181-2214,2341-2372) on one plane of one block: AOM_BLEND_A64 (svt_aom_blend_a64_mask_c, svt_aom_highbd_blend_a64_mask_c,
 *     Codec/blend_a64_mask.c:201-299) of an intra and an inter prediction block with build_smooth_interintra_mask (:2144-2179) of the plane's
 *     block size, or with the wedge of the luma block size and subw / subh.  The destination may be the inter plane at the same offset.
 *     Luma sizes 8x8 .. 32x32 (svt_aom_is_interintra_allowed_bsize) and their sub-sampled chroma sizes down to 4x4.
 * svt_hip_mask_search_batch   one job per luma block, kind
 *       0  pick_interinter_wedge -> pick_wedge (Codec/enc_inter_prediction.c:383-446): sign_limit, svt_av1_wedge_compute_delta_squares_c with
 *          its saturation to int16, per wedge svt_av1_wedge_sign_from_residuals_c on the sign-0 mask and svt_av1_wedge_sse_from_residuals_c
 *          (Codec/inter_prediction.c:2330-2339, the clamp of 64 r1 + m d to int16 included) on the chosen sign's; rd = sse, strict <
 *       1  pick_interinter_seg (:498-544): both masks of svt_av1_build_compound_diffwtd_mask{,_highbd}_c on the pixel predictions
 *          (Codec/inter_prediction.c:61-151), the same SSE, strict <
 *       2  inter_intra_search with use_rd_model = 0 (Codec/mode_decision.c:383-480): the four smooth blends against the source (svt_aom_sse /
 *          svt_aom_highbd_sse), then, if ii_wedge_mode != 0, pick_interintra_wedge -> pick_wedge_fixed_sign with sign 0 on the best mode's
 *          intra block; use_wedge_interintra = (ii_wedge_mode == 1 || rd_wedge < best_rd)
 *     Kinds 0 and 1 run the tail of svt_aom_calc_pred_masked_compound first (:4726-4769): the SAD of pred0 against pred1; below
 *     width * height * pred0_to_pred1_mult the job writes exit = 1 and nothing else of its record.
 *     The reference's floating-point curve-fit model (model_rd_with_curvfit: inter_comp_ctrls.use_rate = 1, inter_intra_comp_ctrls.
 *     use_rd_model = 1) stays on the host: a descriptor that sets use_rate or use_rd_model is refused.
 * Bit-exact with the reference's C path for 8-bit planes (uint8) and 10-bit planes (packed uint16).
 *
 * Out of scope: the curve-fit rate model and model_rd_for_sb_with_curvfit, masked compound on warped references
 * (av1_make_masked_warp_inter_predictor), scaled references, 12-bit, OBMC (svt_hip_obmc.h), and everything svt_hip_pred.h leaves out.
 *
 * A job gets status 0xFF, and writes nothing else, when
 *   prediction  a wedge on a luma size without wedges; wedge_index >= 16, wedge_sign or mask_type > 1; comp_type > 1; DIFFWTD on a luma size
 *               below 8; the plane's block is not the luma block sub-sampled by ss_x / ss_y, or is below 4; a DIFFWTD job whose mask does not
 *               end inside mask_buf, or a chroma DIFFWTD job without mask_buf; result_index outside the result array (or no array); a single
 *               reference (ref[1] = SVT_HIP_INTER_PRED_NO_REF); every condition svt_hip_inter_pred_batch refuses
 *   blend       a luma size outside the seven; the plane's block not the sub-sampled luma block or below 4; interintra_mode > 3,
 *               use_wedge > 1, (with a wedge) wedge_index >= 16 or wedge_sign > 1; a block that does not end inside its plane (of the four
 *               intra blocks the one read); result_index outside the array
 *   search      kind > 2; a size outside the kind's (0: the nine wedge sizes, 1: the 17 DIFFWTD sizes, 2: the seven inter-intra sizes);
 *               ii_wedge_mode > 2; a block that does not end inside its plane
 * Every other job writes status 0.
 */
#ifndef SVT_HIP_MASK_H
#define SVT_HIP_MASK_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_pred.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_MASK_WEDGE 0   /* comp_type: COMPOUND_WEDGE */
#define SVT_HIP_MASK_DIFFWTD 1 /* comp_type: COMPOUND_DIFFWTD */
#define SVT_HIP_MASK_PARAMS_FROM_ARRAY 4 /* a flags bit next to SVT_HIP_INTER_PRED_MV*_FROM_ARRAY: the parameters are results[result_index] */
#define SVT_HIP_MASK_OK 0
#define SVT_HIP_MASK_UNDEFINED 0xFF
#define SVT_HIP_MASK_SEARCH_WEDGE 0      /* kind: pick_interinter_wedge */
#define SVT_HIP_MASK_SEARCH_DIFFWTD 1    /* kind: pick_interinter_seg */
#define SVT_HIP_MASK_SEARCH_INTERINTRA 2 /* kind: inter_intra_search */

/* What one search job leaves, and what a prediction / blend job with SVT_HIP_MASK_PARAMS_FROM_ARRAY takes its parameters from. */
typedef struct SvtHipMaskSearchResult {
    int64_t best_rd;             /* kind 0 / 1: the winner's rd (= sse); kind 2: the best smooth mode's */
    int64_t rd_wedge;            /* kind 2: pick_interintra_wedge's rd, INT64_MAX when ii_wedge_mode = 0; kinds 0 / 1: 0 */
    int8_t  wedge_index;         /* kind 0; kind 2: interintra_wedge_index, -1 when no wedge search ran */
    uint8_t wedge_sign;          /* kind 0 */
    uint8_t mask_type;           /* kind 1: DIFFWTD_38 = 0, DIFFWTD_38_INV = 1 */
    uint8_t interintra_mode;     /* kind 2: II_DC_PRED 0, II_V_PRED 1, II_H_PRED 2, II_SMOOTH_PRED 3 */
    uint8_t use_wedge_interintra; /* kind 2 */
    uint8_t exit;                /* kinds 0 / 1: 1 = the gate of svt_aom_calc_pred_masked_compound fired: the only field written */
    uint8_t reserved[2];
} SvtHipMaskSearchResult;

/* ---- masked compound prediction ---- */
typedef struct SvtHipMaskedPredJob {
    SvtHipInterPredJob pred;     /* as svt_hip_pred.h: both references used; comp_mode, fwd_offset, bck_offset ignored; flags may carry
                                    SVT_HIP_MASK_PARAMS_FROM_ARRAY */
    uint8_t  comp_type;          /* SVT_HIP_MASK_WEDGE / SVT_HIP_MASK_DIFFWTD */
    uint8_t  wedge_index, wedge_sign; /* wedge (unless PARAMS_FROM_ARRAY) */
    uint8_t  mask_type;          /* DIFFWTD, luma (unless PARAMS_FROM_ARRAY); a chroma job reads the mask as stored */
    uint8_t  luma_width, luma_height; /* of the luma block: the wedge window and the mask stride */
    uint8_t  reserved[2];
    uint32_t mask_offset;        /* DIFFWTD: of the block's mask in mask_buf, in bytes */
    uint32_t result_index;       /* with PARAMS_FROM_ARRAY */
} SvtHipMaskedPredJob;

typedef struct SvtHipMaskedPredDesc {
    uint8_t  bit_depth;          /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  ss_x, ss_y;         /* the plane's sub-sampling, 0 or 1; 0 for plane 0 */
    uint8_t  n_refs;             /* 1..SVT_HIP_INTER_PRED_MAX_REFS */
    uint32_t n_jobs;
    SvtHipInterPredRef refs[SVT_HIP_INTER_PRED_MAX_REFS];
    void    *dst;                /* device pointer: the prediction plane */
    uint32_t dst_stride;         /* in samples */
    uint8_t  plane;              /* 0 luma (computes and stores DIFFWTD masks), 1 / 2 chroma (reads them) */
    uint8_t  reserved[3];
    uint64_t dst_samples;        /* samples the destination holds from `dst` on */
    const SvtHipMaskedPredJob *jobs; /* device pointer, n_jobs entries */
    const int16_t *mv_array;     /* optional device pointer, [n_mvs][2] = (row, col) */
    uint32_t n_mvs;
    uint32_t n_results;
    const SvtHipMaskSearchResult *results; /* optional device pointer, n_results entries: what svt_hip_mask_search_batch wrote */
    uint8_t *mask_buf;           /* optional device pointer: the DIFFWTD masks, written by luma batches, read by chroma batches */
    uint64_t mask_bytes;         /* bytes mask_buf holds */
    uint8_t *status;             /* device pointer, [n_jobs] */
} SvtHipMaskedPredDesc;

/* Enqueues one batch on the context stream (asynchronous); one wave per job.  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and
 * enqueues nothing when svt_hip_masked_pred_check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_masked_pred_batch(SvtHipContext *ctx, const SvtHipMaskedPredDesc *d);
/* Host-only validation: what svt_hip_inter_pred_check_desc refuses, plane > 2, a luma batch with sub-sampling, n_results without results,
 * mask_bytes without mask_buf. */
int    svt_hip_masked_pred_check_desc(const SvtHipMaskedPredDesc *d);
/* sizeof / offsetof as compiled: what = 0 the descriptor, 1 the job, 2 SvtHipMaskSearchResult; `field` as svt_hip_inter_pred_layout */
size_t svt_hip_masked_pred_layout(int what, int field);

/* ---- inter-intra combination ---- */
typedef struct SvtHipInterIntraJob {
    uint32_t intra_offset[4];    /* of the intra block of II_DC_PRED, II_V_PRED, II_H_PRED, II_SMOOTH_PRED in the intra plane, in samples: the job
                                    reads the one of its interintra_mode (the search's layout: a job that takes its mode from the array names all four) */
    uint32_t inter_offset, dst_offset; /* of the block's first sample in the inter plane and in the destination, in samples */
    uint32_t result_index;       /* with SVT_HIP_MASK_PARAMS_FROM_ARRAY */
    uint8_t  width, height;      /* of the block on this plane */
    uint8_t  luma_width, luma_height;
    uint8_t  interintra_mode;    /* 0..3 (unless PARAMS_FROM_ARRAY): which intra block, and the smooth mask of a job without a wedge */
    uint8_t  use_wedge;          /* 1: the wedge mask (unless PARAMS_FROM_ARRAY) */
    uint8_t  wedge_index, wedge_sign; /* wedge_index unless PARAMS_FROM_ARRAY; wedge_sign is the job's own (INTERINTRA_WEDGE_SIGN = 0) */
    uint8_t  flags;              /* SVT_HIP_MASK_PARAMS_FROM_ARRAY */
    uint8_t  reserved[3];
} SvtHipInterIntraJob;

typedef struct SvtHipInterIntraDesc {
    uint8_t  bit_depth;
    uint8_t  reserved[3];
    uint32_t n_jobs;
    const void *intra;           /* device pointers: the plane svt_hip_intra_pred_batch wrote, */
    const void *inter;           /* the plane svt_hip_inter_pred_batch wrote, */
    void    *dst;                /* and the destination, which may be `inter` itself with equal offsets and strides */
    uint32_t intra_stride, inter_stride, dst_stride, n_results; /* strides in samples */
    uint64_t intra_samples, inter_samples, dst_samples;
    const SvtHipInterIntraJob *jobs;
    const SvtHipMaskSearchResult *results; /* optional */
    uint8_t *status;
} SvtHipInterIntraDesc;

int    svt_hip_interintra_blend_batch(SvtHipContext *ctx, const SvtHipInterIntraDesc *d);
/* Host-only validation: null descriptor or intra / inter / dst / jobs / status, bit_depth other than 8 / 10, a zero stride or sample count,
 * n_results without results. */
int    svt_hip_interintra_blend_check_desc(const SvtHipInterIntraDesc *d);
size_t svt_hip_interintra_blend_layout(int what, int field); /* what = 0 the descriptor, 1 the job */

/* ---- the searches ---- */
typedef struct SvtHipMaskSearchJob {
    uint32_t src_offset;         /* of the block's first sample in the source plane, in samples */
    uint32_t pred0_offset, pred1_offset; /* kinds 0 / 1: pred0 and pred1; kind 2: pred1 is the inter prediction, pred0_offset unused */
    uint32_t intra_offset[4];    /* kind 2: the intra blocks of II_DC_PRED, II_V_PRED, II_H_PRED, II_SMOOTH_PRED in the intra plane */
    uint8_t  width, height;
    uint8_t  kind;               /* SVT_HIP_MASK_SEARCH_* */
    uint8_t  ii_wedge_mode;      /* kind 2: inter_intra_comp_ctrls.wedge_mode_sq / _nsq of the block's shape: 0, 1 or 2 */
} SvtHipMaskSearchJob;

typedef struct SvtHipMaskSearchDesc {
    uint8_t  bit_depth;
    uint8_t  pred0_to_pred1_mult; /* inter_comp_ctrls.pred0_to_pred1_mult: 0 / 1 / 4 in the reference; 0 never exits */
    uint8_t  use_rate;           /* inter_comp_ctrls.use_rate: must be 0, the curve-fit model stays on the host */
    uint8_t  use_rd_model;       /* inter_intra_comp_ctrls.use_rd_model: must be 0, the same */
    uint32_t n_jobs;
    const void *src, *pred0, *pred1, *intra; /* device pointers; pred0 / intra may be null when no job of the batch reads them */
    uint32_t src_stride, pred0_stride, pred1_stride, intra_stride; /* in samples */
    uint64_t src_samples, pred0_samples, pred1_samples, intra_samples;
    const SvtHipMaskSearchJob *jobs;
    SvtHipMaskSearchResult *results; /* device pointer, [n_jobs] */
    uint8_t *status;             /* device pointer, [n_jobs] */
} SvtHipMaskSearchDesc;

int    svt_hip_mask_search_batch(SvtHipContext *ctx, const SvtHipMaskSearchDesc *d);
/* Host-only validation: null descriptor or src / pred1 / jobs / results / status, bit_depth other than 8 / 10, use_rate or use_rd_model set
 * (the curve-fit model stays on the host), a zero stride or sample count of a plane that is given. */
int    svt_hip_mask_search_check_desc(const SvtHipMaskSearchDesc *d);
size_t svt_hip_mask_search_layout(int what, int field); /* what = 0 the descriptor, 1 the job */

/* The library's host copies, for the fixture to pin: the twelve 64 x 64 primaries [sign][direction][64 * 64] (directions in
 * WedgeDirectionType's order) and the sign-flip table [9][16], sizes in the order 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32, 8x32, 32x8. */
const uint8_t *svt_hip_wedge_primaries(void);
const uint8_t *svt_hip_wedge_signflip(void);

#ifdef __cplusplus
}
#endif
#endif
