/*
 * svt_hip_ifs.h -- C-ABI of the batched interpolation-filter search of the MI355X path, and of the step that hands the chosen filters to the
 * prediction batches that follow it on the device.
 *
 * One job = one call of interpolation_filter_search (Source/Lib/Codec/enc_inter_prediction.c:2436-2577, called at :5068-5096) for the luma
 * block of one candidate, with interpolation_filter == SWITCHABLE:
 *   order     filter_sets[i], i = 0..8: [i][0] the y filter, [i][1] the x filter (Codec/filter.h:63-67), each of EIGHTTAP_REGULAR,
 *             EIGHTTAP_SMOOTH, MULTITAP_SHARP; pairs of unequal filters are skipped when enable_dual_filter == 0
 *   rate      svt_av1_get_switchable_rate (:2146-2165): the sum over dir < (enable_dual_filter ? 2 : 1) of
 *             switchable_interp_fac_bits[pred_ctx[dir]][av1_extract_interp_filter(filters, dir)]; dir 0 reads the y filter
 *   predict   the pair's luma prediction, exactly what svt_hip_inter_pred_batch computes for the embedded job with these filters
 *             (svt_hip_pred.h): unscaled, translational, non-masked; single, or compound with average or distance-weighted weights
 *   model     model_rd_for_sb, plane 0 (:2266-2388): shift = subsampled_distortion && height > 16; the SSE over width x (height >> shift)
 *             with both strides << shift, then << shift; plus (uint64_t)(psy energy * psy_rd) over the same view, then << shift
 *             (get_svt_psy_full_dist, Codec/psy_rd.c:135-293); skip_sse_rd_model: rate 0, dist = sse * 10; else model_rd_from_sse (:2244-2264)
 *             on ROUND_POWER_OF_TWO(sse, 2 * (bit_depth - 8)) with simple_model_rd_from_var = 0: svt_av1_model_rd_from_var_lapndz and
 *             model_rd_norm (:2167-2242), the var == 0 case, the MAX_XSQ_Q10 clamp and the 64-bit division included, then dist <<= 4
 *   cost      RDCOST(lambda, rate of the pair + model rate, dist); (rd * smooth_bias_pct) / 100 when either filter is EIGHTTAP_SMOOTH and
 *             smooth_bias_pct != 0; with spy_rd (rd * 75) / 100 when either is MULTITAP_SHARP, then (rd * 80) / 100 when either is
 *             EIGHTTAP_REGULAR (:2545-2559)
 *   winner    strict < against the running best, which starts from ~0: the first minimum
 * All outputs are integers and bit-exact with the reference's C path, 8-bit planes (uint8) and 10-bit planes (packed uint16), the 22 block
 * sizes.  The reference's is_pred_buffer_ready short-cut only spares it a prediction it already has; it changes no result and is not here.
 *
 * These keep the host path: candidates whose IFS prediction includes a mask, the OBMC blend or inter-intra (the reference passes motion_mode
 * / is_interintra_used down at 8 bits); the EB_DUAL_BIT_MD switch of reference pictures (the host simply names the 8-bit planes in `refs`);
 * planes 1 and 2 of model_rd_for_sb (never reached from IFS); simple_model_rd_from_var; scaled references; 12-bit.
 *
 * A job gets status 0xFF, and writes nothing else, in each case in which svt_hip_inter_pred_batch says so for the embedded job (its
 * filter_x / filter_y are ignored; the destination is only checked when dst is given), when a pred_ctx is >= 16, or when src_offset plus the
 * block leaves the source plane (src_samples).  Every other job writes status 0.
 */
#ifndef SVT_HIP_IFS_H
#define SVT_HIP_IFS_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_pred.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_IFS_PAIRS 9            /* DUAL_FILTER_SET_SIZE */
#define SVT_HIP_IFS_CONTEXTS 16        /* SWITCHABLE_FILTER_CONTEXTS */
#define SVT_HIP_IFS_MODEL_ENTRIES 104  /* of each table of model_rd_norm */
#define SVT_HIP_IFS_OK 0
#define SVT_HIP_IFS_UNDEFINED 0xFF
#define SVT_HIP_IFS_SKIPPED UINT64_MAX /* rd / sse of a pair the search skipped */

typedef struct SvtHipIfsJob {
    SvtHipInterPredJob pred;  /* as for svt_hip_inter_pred_batch on the luma plane; filter_x / filter_y are ignored, MV*_FROM_ARRAY reads
                                 SvtHipIfsDesc.mv_array, dst_offset is where the winner's prediction goes */
    uint32_t src_offset;      /* of the block's first sample in the source plane, in samples: input_offset of model_rd_for_sb */
    uint8_t  pred_ctx[2];     /* svt_aom_get_pred_context_switchable_interp for dir 0 and dir 1 (neighbour logic: the host's) */
    uint8_t  reserved[2];
} SvtHipIfsJob;

typedef struct SvtHipIfsResult {
    uint64_t best_rd;         /* the winner's cost after the biases */
    uint32_t interp_filters;  /* av1_make_interp_filters(y, x): y | x << 16 */
    int32_t  switchable_rate; /* the winner's: what the host adds to fast_luma_rate */
    uint8_t  filter_x, filter_y; /* the two bytes SvtHipInterPredJob wants, in its order */
    uint8_t  winner;          /* index into filter_sets */
    uint8_t  reserved[5];
} SvtHipIfsResult;

typedef struct SvtHipIfsDesc {
    uint8_t  bit_depth;       /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  n_refs;          /* 1..SVT_HIP_INTER_PRED_MAX_REFS */
    uint8_t  enable_dual_filter;    /* seq_header.enable_dual_filter */
    uint8_t  subsampled_distortion; /* ifs_ctrls.subsampled_distortion */
    uint8_t  skip_sse_rd_model;     /* ifs_ctrls.skip_sse_rd_model */
    uint8_t  spy_rd;          /* non-zero: static_config.spy_rd > 0, the 75 % / 80 % biases */
    uint8_t  reserved[2];
    uint32_t n_jobs;
    uint32_t n_mvs;
    SvtHipInterPredRef refs[SVT_HIP_INTER_PRED_MAX_REFS]; /* as SvtHipInterPredDesc.refs, luma planes */
    const void *src;          /* device pointer: the source luma plane (enhanced_pic, or input_frame16bit at 10 bits) */
    uint32_t src_stride;      /* in samples */
    uint32_t dst_stride;      /* in samples */
    uint64_t src_samples;     /* samples the source holds from `src` on */
    void    *dst;             /* optional device pointer: the prediction plane the winner's luma goes to; null: search only */
    uint64_t dst_samples;
    const SvtHipIfsJob *jobs; /* device pointer, n_jobs entries */
    const int16_t *mv_array;  /* optional device pointer, [n_mvs][2] = (row, col) */
    int32_t  quantizer;       /* y_dequant_qtx[base_q_idx][1] of the bit depth's Dequants */
    uint32_t lambda;          /* full_lambda_divided of :2452 */
    uint32_t smooth_bias_pct; /* ifs_smooth_bias[picture_qp] when sharpness_ctrls.ifs && is_noise_level, else 0: off */
    uint32_t reserved2;
    double   psy_rd;          /* get_hvs_modulation_factor's result; <= 0: no psy term */
    const int32_t *switchable_interp_fac_bits; /* device pointer, [16][3]: md_rate_est_ctx->switchable_interp_fac_bitss */
    SvtHipIfsResult *results; /* device pointer, [n_jobs] */
    uint64_t *rd;             /* optional device pointer, [n_jobs][9]: every pair's cost after the biases; SVT_HIP_IFS_SKIPPED for a skipped pair */
    uint64_t *sse;            /* optional device pointer, [n_jobs][9]: every pair's SSE after the psy term and the shift, before the model */
    uint8_t *status;          /* device pointer, [n_jobs] */
} SvtHipIfsDesc;

typedef struct SvtHipIfsPatch {
    uint32_t result_index;    /* which SvtHipIfsResult */
    uint32_t record_index;    /* which record gets its filter_x / filter_y */
} SvtHipIfsPatch;

typedef struct SvtHipIfsScatterDesc {
    uint32_t n_patches, n_results, n_records;
    uint32_t record_stride;   /* bytes from one record to the next: sizeof(SvtHipInterPredJob), sizeof(SvtHipMaskedPredJob), ... */
    uint32_t filter_x_offset; /* of the record's filter_x byte; filter_y is the next byte */
    uint32_t reserved;
    const SvtHipIfsPatch  *patches;       /* device pointer, [n_patches] */
    const SvtHipIfsResult *results;       /* device pointer, [n_results]: svt_hip_ifs_batch's */
    const uint8_t         *result_status; /* device pointer, [n_results]: svt_hip_ifs_batch's status */
    void    *base;            /* device pointer: the first record */
    uint8_t *status;          /* device pointer, [n_patches]: 0, or 0xFF for a patch that wrote nothing */
} SvtHipIfsScatterDesc;

/* Enqueues one batch on the context stream (asynchronous); one wave per job.  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and
 * enqueues nothing when svt_hip_ifs_check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_ifs_batch(SvtHipContext *ctx, const SvtHipIfsDesc *d);
/* Host-only validation: null descriptor or src / jobs / results / status / switchable_interp_fac_bits, bit_depth other than 8 / 10, n_refs
 * outside 1..SVT_HIP_INTER_PRED_MAX_REFS, a reference svt_hip_inter_pred_check_desc would refuse, a zero src_stride or src_samples, dst with a
 * zero dst_stride or dst_samples, n_mvs without mv_array, a quantizer outside 1..32767, smooth_bias_pct above 1000. */
int    svt_hip_ifs_check_desc(const SvtHipIfsDesc *d);
/* Enqueues the scatter on the context stream (asynchronous), one lane per patch, ordinary vector stores: for every patch whose result has
 * status 0 the result's filter_x / filter_y go to the record's two bytes and the patch's status is 0.  A patch whose result_index or
 * record_index is out of range, or whose result failed, writes nothing to the records and gets status 0xFF.  Two patches of one record:
 * either may win.  Refused (SVT_HIP_ERR_BAD_PARAM): a null pointer, record_stride 0, filter_x_offset + 2 > record_stride. */
int    svt_hip_ifs_scatter_filters(SvtHipContext *ctx, const SvtHipIfsScatterDesc *d);
/* The tables of model_rd_norm as compiled: which = 0 rate_tab_q10, 1 dist_tab_q10, 2 xsq_iq_q10, SVT_HIP_IFS_MODEL_ENTRIES entries each;
 * null for any other `which` */
const int32_t *svt_hip_ifs_model_table(int which);
/* sizeof / offsetof as compiled: what = 0 the descriptor, 1 the job, 2 the result, 3 the patch, 4 the scatter descriptor; `field` < 0 the
 * size, else the offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_ifs_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
