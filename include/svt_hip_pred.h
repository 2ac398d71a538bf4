/*
 * svt_hip_pred.h -- C-ABI of the batched sub-pel inter prediction of the MI355X path.
 *
 * One job = svt_aom_enc_make_inter_predictor (Source/Lib/Codec/enc_inter_prediction.c:3274-3391) on one plane of one block, once for a
 * single reference or twice for a compound of two, for unscaled, translational, non-masked prediction:
 *   position  compute_subpel_params' unscaled branch (:3200-3211): clamp_mv_to_umv_border_sb (:30-50) on the job's four mb_to_*_edge values
 *             (luma 1/8 units, as MacroBlockD holds them) and the plane's ss_x / ss_y, the (int16_t) cast of the doubled MV included;
 *             pos = origin + (mv_q4 >> 4), subpel = mv_q4 & 15
 *   filters   av1_get_convolve_filter_params (Codec/inter_prediction.h:137-153): an x and a y filter per job (dual filter), all 16 phases of
 *             EIGHTTAP_REGULAR / EIGHTTAP_SMOOTH / MULTITAP_SHARP / BILINEAR; a dimension <= 4 takes sub_pel_filters_4 /
 *             sub_pel_filters_4smooth, decided per dimension
 *   single    svt_aom_convolve[sx != 0][sy != 0][0]: svt_av1_convolve_2d_copy_sr_c, _x_sr_c, _y_sr_c, _2d_sr_c (Codec/inter_prediction.c:311-418)
 *             and svt_av1_highbd_convolve_*_sr_c (:670-777), each with its own rounding; ConvolveParams from get_conv_params_no_round
 *             (Codec/convolve.h:40-64): round_0 = 3, round_1 = 11
 *   compound  svt_av1_jnt_convolve_{2d_copy,x,y,2d}_c (:494-668) and svt_av1_highbd_jnt_convolve_*_c (:852-1020), round_1 = 7: the first
 *             reference into the CONV_BUF_TYPE intermediate, the second averaged into it, (a + b) >> 1 or
 *             (a * fwd_offset + b * bck_offset) >> DIST_PRECISION_BITS; each reference takes the variant its own MV selects.  One job computes
 *             both references: the intermediate stays in registers.
 * Bit-exact with the reference's C path for 8-bit planes (uint8) and 10-bit planes (packed uint16), the 22 AV1 block sizes.
 *
 * Out of scope: scaled references (svt_av1_convolve_2d_scale*, super-res / resize) (masked compound and inter-intra are svt_hip_mask.h, OBMC is svt_hip_obmc.h,
 * the choice of filter_x / filter_y by interpolation_filter_search is svt_hip_ifs.h, whose scatter entry writes the two bytes of these job records),
 * global-motion estimation (its refinement and MV correspondences are svt_hip_gm.h; warped motion is svt_hip_warp.h), intra-BC's bilinear path, the split 8 + 2-bit reference layout (src_ptr_2b, svt_aom_pack_block), the light-PD
 * predictors, 12-bit, and pointer-level leaves for the convolve rtcd entries (one call per block; the batch is the boundary).
 *
 * Defined where the reference is not: the reference relies on the picture padding covering the clamped block plus the filter reach; the
 * kernel clamps every source coordinate to the padded plane instead, which changes nothing whenever the reference's reads are inside it.
 * A job gets status 0xFF, and writes nothing else, when: a reference index is outside the table, width x height is not a block size, a
 * filter is > 3, a used mv_index is outside mv_array (or mv_array is null), comp_mode is > 1 or (comp_mode 1) fwd_offset / bck_offset is
 * not one of the eight pairs of quant_dist_lookup_table, or its block does not end inside the destination (dst_samples).  Every other job
 * writes status 0.
 */
#ifndef SVT_HIP_PRED_H
#define SVT_HIP_PRED_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_INTER_PRED_MAX_REFS 8
#define SVT_HIP_INTER_PRED_NO_REF 0xFF   /* SvtHipInterPredJob.ref[1] of a single-reference job */
#define SVT_HIP_INTER_PRED_MV0_FROM_ARRAY 1 /* SvtHipInterPredJob.flags: mv of reference 0 is mv_array[mv_index[0]] */
#define SVT_HIP_INTER_PRED_MV1_FROM_ARRAY 2 /* the same for reference 1 */
#define SVT_HIP_INTER_PRED_OK 0
#define SVT_HIP_INTER_PRED_UNDEFINED 0xFF

typedef struct SvtHipInterPredRef {
    const void *plane;        /* device pointer to the first sample of the PADDED plane (uint8, or uint16 at 10 bits) */
    uint32_t    stride;       /* in samples */
    uint16_t    org_x, org_y; /* the picture's sample (0, 0) is plane[org_y * stride + org_x] */
    uint16_t    width, height; /* of the padded plane: the limits every source coordinate is clamped to */
    uint32_t    reserved;
} SvtHipInterPredRef;

typedef struct SvtHipInterPredJob {
    uint32_t dst_offset;      /* of the block's first sample in the destination plane, in samples */
    int16_t  org_x, org_y;    /* pre_x / pre_y: the block's origin in the plane (a sub-sampled plane's own coordinates) */
    uint8_t  width, height;   /* blk_width / blk_height on this plane: one of the 22 block sizes */
    uint8_t  filter_x, filter_y; /* InterpFilter: 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR */
    uint8_t  ref[2];          /* indices into SvtHipInterPredDesc.refs; ref[1] = SVT_HIP_INTER_PRED_NO_REF: single reference */
    uint8_t  flags;           /* SVT_HIP_INTER_PRED_MV*_FROM_ARRAY */
    uint8_t  comp_mode;       /* compound jobs: 0 average, 1 distance-weighted (use_dist_wtd_comp_avg) */
    int16_t  mv[2][2];        /* per reference (row, col) in 1/8 luma sample, as MV holds them */
    uint32_t mv_index[2];     /* per reference, with its flag: the MV's index in mv_array */
    int32_t  mb_to_left_edge, mb_to_right_edge, mb_to_top_edge, mb_to_bottom_edge; /* MacroBlockD's, luma 1/8 units */
    uint8_t  fwd_offset, bck_offset; /* comp_mode 1: what svt_av1_dist_wtd_comp_weight_assign hands the host */
    uint8_t  reserved[6];
} SvtHipInterPredJob;

typedef struct SvtHipInterPredDesc {
    uint8_t  bit_depth;       /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  ss_x, ss_y;      /* the plane's sub-sampling, 0 or 1 */
    uint8_t  n_refs;          /* 1..SVT_HIP_INTER_PRED_MAX_REFS */
    uint32_t n_jobs;
    SvtHipInterPredRef refs[SVT_HIP_INTER_PRED_MAX_REFS];
    void    *dst;             /* device pointer: the prediction plane (the one svt_hip_rd_batch reads) */
    uint32_t dst_stride;      /* in samples */
    uint32_t reserved;
    uint64_t dst_samples;     /* samples the destination holds from `dst` on: a block that does not end inside is undefined */
    const SvtHipInterPredJob *jobs; /* device pointer, n_jobs entries */
    const int16_t *mv_array;  /* optional device pointer, [n_mvs][2] = (row, col): the layout svt_hip_md_subpel_batch's best_mv has */
    uint32_t n_mvs;
    uint32_t reserved2;
    uint8_t *status;          /* device pointer, [n_jobs]: SVT_HIP_INTER_PRED_OK / SVT_HIP_INTER_PRED_UNDEFINED */
} SvtHipInterPredDesc;

/* Enqueues one batch on the context stream (asynchronous); one wave per job.  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and
 * enqueues nothing when svt_hip_inter_pred_check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing.
 * A null context or descriptor leaves "<entry>: null context or descriptor", here and in every other svt_hip_*_batch entry that takes a descriptor. */
int    svt_hip_inter_pred_batch(SvtHipContext *ctx, const SvtHipInterPredDesc *d);
/* Host-only validation: null descriptor or dst / jobs / status, bit_depth other than 8 / 10, ss_x / ss_y > 1, n_refs outside
 * 1..SVT_HIP_INTER_PRED_MAX_REFS, a reference with a null plane, a zero stride, a stride below its width, or an origin outside the plane,
 * a zero dst_stride or dst_samples, n_mvs without mv_array. */
int    svt_hip_inter_pred_check_desc(const SvtHipInterPredDesc *d);
/* sizeof / offsetof as compiled, for the bindings: what = 0 the descriptor, 1 the job, 2 the reference; `field` < 0 the size, else the
 * offset of the field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_inter_pred_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
