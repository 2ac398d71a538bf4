/*
 * svt_hip_gm.h -- C-ABI of the device side of global-motion estimation (Source/Lib/Codec/global_me.c:139-467) of the MI355X path: the refinement of
 * the integerized models and the correspondences taken from the ME results.
 *
 * What stays on the host: FAST corner detection and svt_av1_determine_correspondence (gm levels 1 and 2), RANSAC (determine_gm_params),
 * svt_aom_gm_get_params_cost, and the model loop and the thresholds of compute_global_motion.  The host passes its own correspondences and models
 * in; the refinement does not care where they came from.
 *
 * svt_hip_gm_refine_batch.  One job = one call of svt_av1_refine_integerized_param (Codec/global_motion.c:114-206) for one (reference, start
 * model), ERRORADV_BORDER 0, 8-bit luma, no sub-sampling; bit-exact with it over the _c kernels.
 *   pic_sad     svt_nxm_sad_kernel of the whole reference picture against the source (global_me.c:354), summed in uint32 and wrapping as the
 *               reference's does.  The entry computes it.  A job whose pic_sad is 0 gets status SVT_HIP_GM_IDENTICAL, the identity model
 *               (wmtype 0, valid 1) and best_error 0, and no evaluation runs for it (:357-360)
 *   evaluation  svt_av1_warp_error (Codec/enc_warped_motion.c:22-98).  When svt_get_shear_params refuses the parameters -- wmmat[2] <= 0, or
 *               is_affine_shear_allowed -- the error is 1, so a refused candidate is nearly always accepted: that is the reference's contract.
 *               Otherwise the sum, over the selected 32x32 blocks, of the SAD between the warped reference and the source: per 8x8 tile the
 *               arithmetic of svt_hip_warp_pred_batch's single prediction.  Blocks at the right and bottom edge are cropped to the picture; a tile
 *               that straddles the edge is computed whole and summed over its inside columns and rows.  With chess_refn the even block rows start
 *               at the second block column, the odd ones at the first, both take every other block, and the sum is doubled
 *   early exit  the reference's evaluation returns its partial sum as soon as that exceeds best_error.  Partial sums never decrease, so the exit
 *               fires if and only if the full, undoubled sum exceeds best_error; then the partial return and the full error are both > best_error,
 *               and all that is ever done with the value is `< best_error` and, for the first evaluation, AOMMIN(., best_frame_error).  The entry
 *               computes the full sum always and gives identical outputs; tools/gen_gm_golden.py checks this on every evaluation of every case
 *   search      force_wmtype; the first evaluation; best_error = AOMMIN(it, best_frame_error); with rfn_early_exit, unless
 *               e < 0.50 && e * params_cost < 15000 for e = (double)best_error / pic_sad (IEEE double on the device), the job ends here with the
 *               matrix as force_wmtype left it and wmtype as the job gave it.  Then for step = 16, 8, .. (n_refinements of them) and every
 *               parameter p of the type (2, 4 or 6): the candidates add_param_offset(p, cur, -step) and (p, cur, +step), each accepted on a strict
 *               `<` against the running best_error, so the right one must beat the left strictly.  At the end force_wmtype and get_wmtype
 *   ROTZOOM     the state is the whole EbWarpedMotionParams: svt_av1_warp_error calls svt_get_shear_params BEFORE svt_warp_plane, and only the
 *               latter rewrites wmmat[4] = -wmmat[3], wmmat[5] = wmmat[2].  gamma and delta of an evaluation therefore come from the wmmat[4],
 *               wmmat[5] the previous evaluation that reached the warp left behind, accepted or not; a refused candidate rewrites nothing.  The
 *               samples are warped with the fresh matrix and those gamma / delta.  Carried through the rounds as the reference carries it
 * Per job: a SvtHipWarpModel (svt_hip_warp_pred_batch takes it with SVT_HIP_WARP_MODEL0_FROM_ARRAY) with the final matrix, wmtype as the reference
 * leaves it (0 IDENTITY .. 3 AFFINE), the four shear parameters of the final matrix (0 when wmmat[2] <= 0) and valid = what svt_get_shear_params
 * says of it; best_error; pic_sad; status; and, when round_error is non-null, round_error[job][61] = what each evaluation would have returned
 * without its early exit: index 0 the first, 1 + 2k and 2 + 2k the left and right of the job's round k, -1 for rounds that did not run.
 * Status: SVT_HIP_GM_OK, SVT_HIP_GM_IDENTICAL, or SVT_HIP_GM_UNDEFINED with nothing else written: ref >= n_refs or wmtype outside 1..3.
 *
 * On the device the left and right evaluation of a round run in one launch over (32x32 blocks) x (2 sides) x (jobs); a one-lane-per-job decision
 * kernel between two launches applies the two decisions in the reference's order and sets up the next round's candidates.  Rounds follow each
 * other by stream order alone.  Sums are 64-bit integer atomics, one per workgroup, so the results do not depend on arrival order.  The entry
 * enqueues 6 * n_refinements rounds, the most a job can have; a job whose rounds are over costs every workgroup an immediate return.
 *
 * svt_hip_gm_correspondence_batch.  One call = correspondence_from_mvs (global_motion.c:236-337) for up to 8 (list, ref) pairs of one picture,
 * read from the device-resident SvtHipMeResults arrays of the asynchronous ME entries, and the three picture sums of global_me.c:162-169.
 * Entries are in the reference's order (b64 raster, then the block index within the b64: RANSAC's sampling depends on it).  Per block: skipped
 * when its origin lies at or beyond the aligned size; the PU index folded as :263-269 when 8x8 or 16x16 results are not kept; the first
 * uni-predictive candidate whose list and reference match gives the MV; the four values are shifted each on its own, (pos) >> shift and
 * (pos + mv) >> shift (arithmetic).  A caller with an adaptive down-sampling level passes shift 0 and shifts on the host.
 */
#ifndef SVT_HIP_GM_H
#define SVT_HIP_GM_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_warp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_GM_OK 0
#define SVT_HIP_GM_IDENTICAL 1
#define SVT_HIP_GM_UNDEFINED 0xFF
#define SVT_HIP_GM_TRANSLATION 1          /* TransformationType; ROTZOOM and AFFINE are SVT_HIP_WARP_ROTZOOM / _AFFINE */
#define SVT_HIP_GM_MAX_REFINEMENTS 5
#define SVT_HIP_GM_ROUND_ERRORS 61        /* 1 + 2 * 5 * 6 */
#define SVT_HIP_GM_MAX_PAIRS 8
#define SVT_HIP_GM_MAX_JOBS 65535         /* per refine batch */

typedef struct SvtHipGmRefineJob {
    int32_t wmmat[6];         /* the start model, as svt_av1_convert_model_to_params and svt_aom_upscale_wm_params leave it */
    int32_t params_cost;      /* svt_aom_gm_get_params_cost of the start model */
    uint8_t ref;              /* index into SvtHipGmRefineDesc.refs */
    uint8_t wmtype;           /* 1 TRANSLATION, 2 ROTZOOM, 3 AFFINE */
    uint8_t reserved[2];
    int64_t best_frame_error; /* the reference passes INT64_MAX (RANSAC_NUM_MOTIONS is 1) */
} SvtHipGmRefineJob;

typedef struct SvtHipGmRefineDesc {
    uint32_t n_jobs;
    uint8_t  n_refs;          /* 1..SVT_HIP_WARP_MAX_REFS */
    uint8_t  n_refinements;   /* gm_ctrls.params_refinement_steps, 0..SVT_HIP_GM_MAX_REFINEMENTS */
    uint8_t  chess_refn;
    uint8_t  rfn_early_exit;  /* gm_ctrls.rfn_early_exit */
    SvtHipWarpRef src;        /* the source plane (8-bit luma); width x height is the picture's */
    SvtHipWarpRef refs[SVT_HIP_WARP_MAX_REFS]; /* the reference planes, all of the source's picture size */
    const SvtHipGmRefineJob *jobs; /* device pointer, n_jobs entries */
    void     *work;           /* device pointer: svt_hip_gm_refine_work_bytes(n_jobs) bytes of scratch, 8-byte aligned; the entry clears it */
    SvtHipWarpModel *models;  /* outputs, device pointers: [n_jobs] */
    int64_t  *best_error;     /* [n_jobs] */
    uint32_t *pic_sad;        /* [n_jobs] */
    uint8_t  *status;         /* [n_jobs] */
    int64_t  *round_error;    /* optional: [n_jobs][SVT_HIP_GM_ROUND_ERRORS] */
} SvtHipGmRefineDesc;

typedef struct SvtHipGmPair {
    uint8_t list, ref;        /* list_idx, ref_idx */
    uint8_t reserved[2];
} SvtHipGmPair;

typedef struct SvtHipGmCorrDesc {
    uint16_t aligned_width, aligned_height; /* of the picture: the b64 grid is ceil(. / 64) each way */
    uint8_t  enable_me_8x8, enable_me_16x16;
    uint8_t  max_cand, max_refs, max_l0;    /* as in SvtHipMePictureDesc */
    uint8_t  n_pu;            /* PUs per b64 the ME results keep: 85, 21 or 5 */
    uint8_t  method;          /* 0 MV_64x64, 1 MV_32x32, 2 MV_16x16, 3 MV_8x8 */
    uint8_t  shift;           /* 0..2 */
    uint32_t n_pairs;         /* 0..SVT_HIP_GM_MAX_PAIRS */
    uint32_t cap;             /* entries per pair in corr: at least (1 << 2 * method) * b64 count */
    SvtHipGmPair pairs[SVT_HIP_GM_MAX_PAIRS];
    SvtHipMeResults me;       /* device pointers: total_me_candidate_index, me_candidate_array, me_mv_array, rc_me_distortion,
                               * stationary_block_present_sb, rc_me_allow_gm are read */
    int32_t  *corr;           /* outputs, device pointers: [n_pairs][cap][4] = (x, y, rx, ry); entries past count are not written */
    uint32_t *count;          /* [n_pairs] */
    uint32_t *sums;           /* [3] = total_me_sad (wrapping), total_stationary_sb, total_gm_sbs */
} SvtHipGmCorrDesc;

/* Enqueues the refinements of n_jobs jobs on the context stream (asynchronous).  Returns SVT_HIP_ERR_BAD_PARAM and enqueues nothing for what
 * svt_hip_gm_refine_check_desc refuses; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_gm_refine_batch(SvtHipContext *ctx, const SvtHipGmRefineDesc *d);
/* Host-only validation: a null descriptor, jobs, work, models, best_error, pic_sad or status; a work pointer that is not 8-byte aligned; n_jobs above
 * SVT_HIP_GM_MAX_JOBS; n_refs outside 1..8; n_refinements > 5; a source or
 * reference plane svt_hip_warp_check_desc would refuse (null, zero stride or size, picture outside its plane); a reference whose picture size
 * differs from the source's. */
int    svt_hip_gm_refine_check_desc(const SvtHipGmRefineDesc *d);
/* Bytes of SvtHipGmRefineDesc.work for a batch of n_jobs jobs */
size_t svt_hip_gm_refine_work_bytes(uint32_t n_jobs);

/* Enqueues one call on the context stream (asynchronous), one workgroup per pair and one for the sums.  Returns SVT_HIP_ERR_BAD_PARAM and enqueues
 * nothing for what svt_hip_gm_corr_check_desc refuses.  n_pairs == 0 still computes the sums. */
int    svt_hip_gm_correspondence_batch(SvtHipContext *ctx, const SvtHipGmCorrDesc *d);
/* Host-only validation: a null descriptor, corr (with n_pairs), count (with n_pairs), sums or one of the six ME arrays; a zero aligned size;
 * method > 3; shift > 2; n_pairs > 8; n_pu other than 85 (both kept), 21 (no 8x8) or 5 (neither) as enable_me_8x8 / enable_me_16x16 say; a zero
 * max_cand or max_refs; cap below (1 << 2 * method) * b64 count; a pair with list > 1, or whose MV slot (list ? max_l0 : 0) + ref lies outside
 * max_refs. */
int    svt_hip_gm_corr_check_desc(const SvtHipGmCorrDesc *d);

/* sizeof / offsetof as compiled, for the bindings: what = 0 the refinement descriptor, 1 its job, 2 the correspondence descriptor, 3 the pair;
 * `field` < 0 the size, else the offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_gm_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
