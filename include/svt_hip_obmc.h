/*
 * svt_hip_obmc.h -- C-ABI of the four overlapped block motion compensation (OBMC_CAUSAL) batches of the MI355X path: the neighbour strips, the
 * blend over the block's own prediction, the weighted target of the OBMC motion search, and that search.
 *
 * The reference precomputes once per block and reuses per candidate (svt_aom_precompute_obmc_data, Source/Lib/Codec/enc_inter_prediction.c:
 * 1820-1885); the first three entries keep that split and share one device array of block records, SvtHipObmcBlock, which the host fills (the
 * fourth, svt_hip_obmc_search_batch, is the OBMC motion search on what the target batch wrote: see its declaration):
 *   neighbours  svt_hip_obmc_neighbour_batch = build_prediction_by_above_preds / _left_preds (:1133-1417): per overlappable neighbour one
 *               svt_aom_enc_make_inter_predictor, single reference, unscaled, translational, into the above / left strip buffer (obmc_buff_0 / _1:
 *               stride = the luma width, Y at 0, Cb at w * h, Cr at 2 * w * h).  One job = one plane of one block.
 *                 size     above: (size * 4) >> ss_x wide, clamp(h >> (ss_y + 1), 4, 64 >> (ss_y + 1)) high; left: the transpose.  The filter
 *                          tables (a dimension <= 4 takes the 4-tap ones) and clamp_mv_to_umv_border_sb's margins use this size
 *                 edges    per neighbour (:743-777, 1339-1344, 1381-1386), derived from the record's unmodified edges: above
 *                          left = -32 * (mi_col + rel), right = far + (n4_w - rel - size) * 32, bottom += (h - min(h / 2, 32)) * 8; left
 *                          top = -32 * (mi_row + rel), bottom = far + (n4_h - rel - size) * 32, right += (w - min(w / 2, 32)) * 8
 *                 origin   luma (org + rel * 4); chroma ((x >> 3) << 3) >> ss (:1055-1062), in the picture and in the strip alike
 *                 skip     svt_av1_skip_u4x4_pred_in_obmc with DISABLE_CHROMA_U8X8_OBMC = 0: a plane block of 4x4 / 8x4 / 4x8 has no above
 *                          strips and keeps its left ones
 *   blend       svt_hip_obmc_blend_batch = av1_build_obmc_inter_prediction (:1430-1579), in place on the prediction plane
 *               svt_hip_inter_pred_batch wrote: the above spans with svt_aom_blend_a64_vmask / svt_aom_highbd_blend_a64_vmask_16bit over
 *               (min(h, 64) >> 1) >> ss_y rows, then the left spans with the hmask forms over (min(w, 64) >> 1) >> ss_x columns, on the result of
 *               the above pass; the mask is svt_av1_get_obmc_mask(rows or columns).  One job = one plane of one block.
 *   target      svt_hip_obmc_target_batch = calc_target_weighted_pred with svt_av1_calc_target_weighted_pred_above_c / _left_c (:1581-1638,
 *               1756-1816), luma only: wsrc and mask, int32[w * h] each, from the 8-bit source plane and the luma strips.  A 10-bit strip sample
 *               is first reduced to sample >> 2, the 8-bit part svt_aom_un_pack2d leaves (:1857-1874).  One job = one block.
 * Spans may leave gaps (an intra neighbour, the max_neighbor_obmc cap): a gap is neither predicted, blended nor weighted.  Bit-exact with
 * the reference's C path at 8 bits (uint8) and 10 bits (packed uint16) for the 14 luma sizes with min(w, h) >= 8 and max(w, h) <= 64.
 *
 * Stays on the host: foreach_overlappable_nb_above / _left (:673-741) -- the mode-info walk, is_neighbor_overlappable, the mi_step == 1
 * pairing, the max_neighbor_obmc cap and the picture-edge cut -- whose outcome is the record's span list.  The fourth entry,
 * svt_hip_obmc_search_batch, is the OBMC motion search on what the target batch wrote (described at its declaration).  Out of scope: the 128-sample
 * sizes, svt_aom_choose_best_av1_mv_pred and the corrupted_mv_check after the search, scaled references, the 8-bit-MD-on-10-bit path
 * (use_precomputed_obmc = 0), 12-bit, warped or compound neighbours beyond mv[0] / ref_frame[0].
 *
 * Defined where the reference is not: every source coordinate is clamped to the padded plane, as in svt_hip_pred.h.  A job gets status
 * 0xFF, and writes nothing else, when: its block index is outside the block array; width x height is not one of the 14 sizes; n_above or
 * n_left is > 4; a span has an odd rel_pos (the walk's pairing makes it even), a size that is not 2, 4, 8 or 16 (a block's side), leaves the
 * block, or does not lie after the span before it; (neighbours) a span's reference index is outside the table, its filter is > 3 or its mv_index, where
 * flagged, is outside mv_array; the block's strip area, its block in the destination or the source, or its wsrc / mask area does not end inside its buffer.
 * Every other job writes status 0.
 */
#ifndef SVT_HIP_OBMC_H
#define SVT_HIP_OBMC_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"
#include "svt_hip_pred.h"
#include "svt_hip_pme.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_OBMC_MAX_NEIGHBOURS 4   /* max_neighbor_obmc's largest entry */
#define SVT_HIP_OBMC_MV_FROM_ARRAY 1    /* SvtHipObmcNeighbour.flags: the MV is mv_array[mv_index] */
#define SVT_HIP_OBMC_OK 0
#define SVT_HIP_OBMC_UNDEFINED 0xFF

typedef struct SvtHipObmcNeighbour {
    uint8_t  rel_pos, size;      /* rel_mi_col / rel_mi_row and AOMMIN(n4, mi_step), in 4-sample units: rel_pos even, size 2, 4, 8 or 16 */
    uint8_t  ref;                /* index into SvtHipObmcNeighbourDesc.refs: the plane of ref_frame[0] */
    uint8_t  filter_x, filter_y; /* the neighbour's own interp_filters (InterpFilter 0..3) */
    uint8_t  flags;              /* SVT_HIP_OBMC_MV_FROM_ARRAY */
    int16_t  mv[2];              /* mv[0] as (row, col) in 1/8 luma sample */
    uint16_t reserved;
    uint32_t mv_index;           /* with the flag: the MV's index in mv_array */
} SvtHipObmcNeighbour;

typedef struct SvtHipObmcBlock {
    int16_t  org_x, org_y;       /* the block's origin in the picture, luma samples (multiples of 4) */
    uint8_t  width, height;      /* luma: one of the 14 sizes */
    uint8_t  n_above, n_left;    /* 0..SVT_HIP_OBMC_MAX_NEIGHBOURS spans each, in ascending position */
    int32_t  mb_to_left_edge, mb_to_right_edge, mb_to_top_edge, mb_to_bottom_edge; /* MacroBlockD's before OBMC's adjustments, luma 1/8 units */
    uint32_t strip_offset;       /* of the block's area (3 * width * height samples) in both strip buffers, in samples */
    uint32_t reserved;
    SvtHipObmcNeighbour above[SVT_HIP_OBMC_MAX_NEIGHBOURS], left[SVT_HIP_OBMC_MAX_NEIGHBOURS];
} SvtHipObmcBlock;

typedef struct SvtHipObmcJob {
    uint32_t block;              /* index into the block array */
    uint32_t offset;             /* blend: of the block's first sample in the prediction plane, in samples; target: of the block's w * h values
                                    in wsrc and mask; neighbours: unused */
} SvtHipObmcJob;

typedef struct SvtHipObmcNeighbourDesc {
    uint8_t  bit_depth;          /* 8: planes and strips are uint8; 10: uint16 */
    uint8_t  ss_x, ss_y;         /* the plane's sub-sampling, 0 or 1 */
    uint8_t  plane;              /* 0 luma, 1 Cb, 2 Cr: the strip area's third the job writes */
    uint8_t  n_refs;             /* 1..SVT_HIP_INTER_PRED_MAX_REFS */
    uint8_t  reserved[3];
    uint32_t n_jobs, n_blocks;
    SvtHipInterPredRef refs[SVT_HIP_INTER_PRED_MAX_REFS]; /* this plane of every reference picture */
    const SvtHipObmcBlock *blocks; /* device pointer, n_blocks entries */
    const SvtHipObmcJob   *jobs;   /* device pointer, n_jobs entries */
    void    *above, *left;       /* device pointers: the two strip buffers */
    uint64_t strip_samples;      /* samples each strip buffer holds */
    const int16_t *mv_array;     /* optional device pointer, [n_mvs][2] = (row, col), svt_hip_md_subpel_batch's best_mv layout */
    uint32_t n_mvs;
    uint32_t reserved2;
    uint8_t *status;             /* device pointer, [n_jobs] */
} SvtHipObmcNeighbourDesc;

typedef struct SvtHipObmcBlendDesc {
    uint8_t  bit_depth;
    uint8_t  ss_x, ss_y;
    uint8_t  plane;
    uint32_t n_jobs, n_blocks;
    uint32_t dst_stride;         /* in samples */
    const SvtHipObmcBlock *blocks;
    const SvtHipObmcJob   *jobs; /* offset: the block's first sample in dst */
    const void *above, *left;    /* the strip buffers svt_hip_obmc_neighbour_batch wrote, at this bit depth */
    uint64_t strip_samples;
    void    *dst;                /* device pointer: the prediction plane, blended in place */
    uint64_t dst_samples;
    uint8_t *status;
} SvtHipObmcBlendDesc;

typedef struct SvtHipObmcTargetDesc {
    uint8_t  strip_bit_depth;    /* 8 or 10: of the strip buffers; the source is 8-bit either way */
    uint8_t  reserved[3];
    uint32_t n_jobs, n_blocks;
    uint32_t src_stride;         /* in samples */
    const SvtHipObmcBlock *blocks;
    const SvtHipObmcJob   *jobs; /* offset: the block's first value in wsrc and mask */
    const void *above, *left;
    uint64_t strip_samples;
    const uint8_t *src;          /* device pointer: the picture's sample (0, 0) of the 8-bit source luma plane */
    uint64_t src_samples;        /* samples the source holds from `src` on */
    int32_t *wsrc, *mask;        /* device pointers, out_values int32 each */
    uint64_t out_values;
    uint8_t *status;
} SvtHipObmcTargetDesc;

#define SVT_HIP_OBMC_MAX_FPEL_RANGE 64   /* fpel_search_range the search accepts (the reference's levels use 8 and 16) */

typedef struct SvtHipObmcSearchJob {
    uint32_t target_offset;      /* of the block's w * h values in wsrc and mask (what svt_hip_obmc_target_batch's job named) */
    uint32_t ref_offset;         /* of the co-located block's first sample in the reference plane, in samples */
    uint8_t  width, height;      /* luma: one of the 14 sizes */
    uint8_t  reserved[2];
    SvtHipMv start_mv;           /* best_pred_mv, 1/8 sample */
    SvtHipMv ref_mv;             /* *ref_mv, 1/8 sample */
    int32_t  col_min, col_max, row_min, row_max; /* x->mv_limits as single_motion_search computes them, before svt_av1_set_mv_search_range (full-pel) */
    uint32_t reserved2;
} SvtHipObmcSearchJob;

typedef struct SvtHipObmcSearchResult {
    int32_t  fullpel_value;      /* what svt_av1_obmc_full_pixel_search returns (0 at refine levels 2 / 4, which do not call it) */
    uint32_t besterr;            /* what svt_av1_find_best_obmc_sub_pixel_tree_up returns */
    int32_t  distortion;         /* its *distortion */
    uint32_t sse1;               /* its *sse1 */
    int32_t  rate_mv;            /* svt_av1_mv_bit_cost (MV_COST_WEIGHT) or svt_av1_mv_bit_cost_light of the final MV */
    uint32_t reserved;
} SvtHipObmcSearchResult;

typedef struct SvtHipObmcSearchDesc {
    uint8_t  ref_bit_depth;      /* 8: the search works on 8-bit reference planes, as the reference's does */
    uint8_t  refine_level;       /* 0..4: 0 / 1 / 3 full-pel and sub-pel, 2 / 4 sub-pel only from start_mv >> 3 */
    uint8_t  fpel_search_diag;   /* obmc_ctrls.fpel_search_diag: 8 sites a step instead of 4 */
    uint8_t  approx_inter_rate;  /* the light rate forms */
    uint8_t  allow_hp;           /* allow_high_precision_mv: three sub-pel rounds instead of two */
    uint8_t  reserved[3];
    uint32_t n_jobs;
    uint32_t fpel_search_range;  /* obmc_ctrls.fpel_search_range, <= SVT_HIP_OBMC_MAX_FPEL_RANGE */
    int32_t  sadpb;              /* x->sadperbit16 */
    int32_t  error_per_bit;      /* x->errorperbit */
    uint32_t ref_stride;         /* in samples */
    uint32_t reserved2;
    const uint8_t *ref;          /* device pointer: the reference plane's buffer */
    uint64_t ref_samples;        /* samples it holds: every read of a job must lie inside */
    const int32_t *wsrc, *mask;  /* device pointers: what svt_hip_obmc_target_batch wrote */
    uint64_t target_values;
    const int32_t *mvjcost;      /* device pointer, 4 entries (not read with approx_inter_rate) */
    const int32_t *mvcost[2];    /* device pointers to the CENTRE entries of the row / column tables, indices [-16384, 16384] */
    const SvtHipObmcSearchJob *jobs;
    int16_t *best_mv;            /* device pointer, [n_jobs][2] = (row, col): the layout svt_hip_md_subpel_batch's best_mv has */
    SvtHipObmcSearchResult *results; /* device pointer, [n_jobs] */
    uint8_t *status;
} SvtHipObmcSearchDesc;

/* One wave per job: single_motion_search for OBMC_CAUSAL (Codec/mode_decision.c:2290-2398) = svt_av1_set_mv_search_range +
 * svt_av1_obmc_full_pixel_search (Codec/av1me.c:721-776) at refine levels 0 / 1 / 3, svt_av1_find_best_obmc_sub_pixel_tree_up (:963-1132) with
 * forced_stop 0, iters_per_step 2, USE_8_TAPS, and the MV's rate.  A job gets status 0xFF and writes nothing else when its size is not one of the 14,
 * its wsrc / mask values do not end inside target_values, or a position the search can reach would read outside [ref, ref + ref_samples): from the
 * (clamped) start fpel_search_range samples of full-pel movement, then up to 14 / 8 sample of sub-pel movement either way (two samples down to the
 * floor, one up) and the 8-tap reach (3 before, 4 after), i.e. range + 5 rows and columns before the co-located block and range + 5 after it. */
int    svt_hip_obmc_search_batch(SvtHipContext *ctx, const SvtHipObmcSearchDesc *d);
/* refuses: null descriptor or pointer (ref, wsrc, mask, jobs, best_mv, results, status; mvjcost / mvcost without approx_inter_rate), ref_bit_depth
 * other than 8, refine_level > 4, fpel_search_range > SVT_HIP_OBMC_MAX_FPEL_RANGE, zero ref_stride / ref_samples / target_values */
int    svt_hip_obmc_search_check_desc(const SvtHipObmcSearchDesc *d);

/* Each enqueues one batch on the context stream (asynchronous); one wave per job.  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and
 * enqueues nothing when its check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_obmc_neighbour_batch(SvtHipContext *ctx, const SvtHipObmcNeighbourDesc *d);
int    svt_hip_obmc_blend_batch(SvtHipContext *ctx, const SvtHipObmcBlendDesc *d);
int    svt_hip_obmc_target_batch(SvtHipContext *ctx, const SvtHipObmcTargetDesc *d);
/* Host-only validation: a null descriptor or mandatory pointer (blocks, jobs, the strip buffers, status; dst; src, wsrc, mask), a bit depth
 * other than 8 / 10, ss_x / ss_y > 1, plane > 2, a luma batch with sub-sampling, n_refs outside 1..SVT_HIP_INTER_PRED_MAX_REFS or a reference
 * svt_hip_inter_pred_check_desc would refuse, zero n_blocks, strides or sample counts, n_mvs without mv_array. */
int    svt_hip_obmc_neighbour_check_desc(const SvtHipObmcNeighbourDesc *d);
int    svt_hip_obmc_blend_check_desc(const SvtHipObmcBlendDesc *d);
int    svt_hip_obmc_target_check_desc(const SvtHipObmcTargetDesc *d);
/* sizeof / offsetof as compiled, for the bindings: what = 0 the neighbour descriptor, 1 the blend descriptor, 2 the target descriptor, 3 the
 * block record, 4 a neighbour, 5 the job, 6 the search descriptor, 7 the search job, 8 the search result; `field` < 0 the size, else the offset of the field-th member in declaration order ((size_t)-1 past
 * the last) */
size_t svt_hip_obmc_layout(int what, int field);
/* Host copy of the 1-D mask rows (the AV1 specification's Obmc_Mask_2 .. _32; svt_av1_get_obmc_mask): 64 bytes, the row of length n at [n, 2n),
 * byte 0 unused (0) and byte 1 the row of length 1 */
const uint8_t *svt_hip_obmc_masks(void);

#ifdef __cplusplus
}
#endif
#endif
