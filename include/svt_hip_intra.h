/*
 * svt_hip_intra.h -- C-ABI of the batched intra prediction of the MI355X path.
 *
 * One job = one call of build_intra_predictors (8-bit, uint8 planes) or build_intra_predictors_high (10-bit, packed uint16 planes)
 * (Source/Lib/Codec/enc_intra_prediction.c:60-436) for one transform block of one plane:
 *   edges      the needed edges per mode (extend_modes[]; a directional mode overrides them from p_angle, filter-intra needs all three), the
 *              early constant fill (above_ref[0] / 129, left_ref[0] / 127; base + 1 / base - 1 at 10 bits, base = 128 << (bd - 8)), the edge
 *              extension (replication of the last available sample up to txh + txw on the left and txw + txh above; the fallbacks
 *              above_ref[0], left_ref[0], base +- 1) and the corner's four values
 *   directional p_angle = mode_to_angle_map[mode] + 3 * angle_delta; unless disable_edge_filter: filter_intra_edge_corner, svt_av1_filter_intra_edge
 *              with svt_aom_intra_edge_filter_strength, svt_av1_upsample_intra_edge when svt_aom_use_intra_edge_upsample says so; then
 *              svt_av1_dr_prediction_z1 / _z2 / _z3 with eb_dr_intra_derivative (Codec/intra_prediction.c:146-413, :2273-2422,
 *              C_DEFAULT/intra_prediction_c.c); 90 and 180 are the V and H predictors
 *   others     svt_aom_dc_pred[n_left_px > 0][n_top_px > 0] (128, left, top, full: (sum + count / 2) / count as the C bodies divide),
 *              SMOOTH / SMOOTH_V / SMOOTH_H with sm_weight_arrays, PAETH with its tie order (Codec/intra_prediction.c:1023-1348)
 *   filter-intra svt_av1_filter_intra_predictor_c / svt_aom_highbd_filter_intra_predictor: 4x2 sub-blocks, seven taps of
 *              eb_av1_filter_intra_taps, ROUND_POWER_OF_TWO_SIGNED(.., 4), clipped
 * Bit-exact with the reference's C path, the 19 transform sizes (4x4 .. 64x64, the 1:4 shapes included).
 *
 * The neighbours come from the neighbour plane (the reconstruction in a closed loop, the source in an open one):
 *   above_ref[i] = nbr[(nbr_y - 1) * stride + nbr_x + i], left_ref[i] = nbr[(nbr_y + i) * stride + nbr_x - 1], above_ref[-1] the corner.
 * The kernel reads no sample the reference does not read: of the n_top_px (+ n_topright_px) above and the n_left_px (+ n_bottomleft_px) on the
 * left those the mode needs, and the corner only when n_top_px > 0 && n_left_px > 0 and the mode needs it.  A block on the plane's first row
 * or column whose count on that side is 0 reads nothing outside the plane.
 *
 * The four counts and filt_type come from the host: svt_aom_intra_has_top_right / svt_aom_intra_has_bottom_left and the have_top / xr / yd
 * arithmetic of svt_av1_predict_intra_block, and get_filt_type (whether the above or the left neighbour is smooth), are table logic that stays
 * with the encoder.
 *
 * Palette is svt_hip_palette_search_batch / svt_hip_palette_pred_batch (svt_hip_palette.h), which write the same prediction plane.
 * Out of scope: intra-BC, the inter-intra blend, 12-bit, the availability derivation above, pointer-level leaves for the intra rtcd
 * entries (one call per block; the batch is the boundary), and svt_hip_tpl_dispense at TPL level 1 (its open-loop path upsamples the edges but
 * predicts with upsample 0: another contract).  Chroma-from-luma is svt_hip_cfl_pred_batch (svt_hip_cfl.h), which reads the DC plane this batch
 * writes.
 *
 * Defined where the reference is not.  A job gets status 0xFF, writes nothing else and reads nothing, when: tx_size > 18 or mode > 12; a
 * directional mode (1..8) with |angle_delta| > 3; filter_intra_mode > 5; a filter-intra job (filter_intra_mode < 5) with a side > 32 or
 * mode != DC_PRED; n_top_px > txw, n_topright_px > txw, or n_topright_px > 0 with n_top_px != txw; n_left_px > txh, n_bottomleft_px > txh, or
 * n_bottomleft_px > 0 with n_left_px != txh; a neighbour sample the reference would read lies outside the neighbour plane; or its block does
 * not end inside the destination (dst_samples).  Every other job writes status 0.
 */
#ifndef SVT_HIP_INTRA_H
#define SVT_HIP_INTRA_H

#include <stdint.h>
#include <stddef.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_INTRA_PRED_NO_FILTER_INTRA 5 /* SvtHipIntraPredJob.filter_intra_mode: FILTER_INTRA_MODES, no filter-intra */
#define SVT_HIP_INTRA_PRED_OK 0
#define SVT_HIP_INTRA_PRED_UNDEFINED 0xFF

typedef struct SvtHipIntraPredJob {
    uint32_t dst_offset;        /* of the block's first sample in the destination plane, in samples */
    int32_t  nbr_x, nbr_y;      /* the block's top-left sample in the neighbour plane */
    uint8_t  tx_size;           /* TxSize, 0..18 */
    uint8_t  mode;              /* PredictionMode 0..12: DC, V, H, D45, D135, D113, D157, D203, D67, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH */
    int8_t   angle_delta;       /* -3..3, read for the directional modes (1..8) alone */
    uint8_t  filter_intra_mode; /* 0..4 a FilterIntraMode, 5 none */
    uint8_t  n_top_px, n_topright_px, n_left_px, n_bottomleft_px; /* what svt_av1_predict_intra_block passes down */
    uint8_t  filt_type;         /* get_filt_type's result: 0, or non-zero when the above or left neighbour is smooth */
    uint8_t  reserved[3];
} SvtHipIntraPredJob;

typedef struct SvtHipIntraPredDesc {
    uint8_t  bit_depth;           /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  disable_edge_filter; /* !seq_header->enable_intra_edge_filter, for the whole batch */
    uint8_t  reserved[2];
    uint32_t n_jobs;
    const void *nbr;              /* device pointer: the neighbour plane's sample (0, 0) */
    uint32_t nbr_stride;          /* in samples */
    uint32_t nbr_width, nbr_height; /* in samples: no read leaves them */
    uint32_t reserved2;
    void    *dst;                 /* device pointer: the prediction plane (the one svt_hip_rd_batch reads) */
    uint32_t dst_stride;          /* in samples */
    uint32_t reserved3;
    uint64_t dst_samples;         /* samples the destination holds from `dst` on: a block that does not end inside is undefined */
    const SvtHipIntraPredJob *jobs; /* device pointer, n_jobs entries */
    uint8_t *status;              /* device pointer, [n_jobs]: SVT_HIP_INTRA_PRED_OK / SVT_HIP_INTRA_PRED_UNDEFINED */
} SvtHipIntraPredDesc;

/* Enqueues one batch on the context stream (asynchronous); one wave per job.  Returns SVT_HIP_ERR_BAD_PARAM (and svt_hip_last_error) and
 * enqueues nothing when svt_hip_intra_pred_check_desc refuses the descriptor; n_jobs == 0 returns 0 and enqueues nothing. */
int    svt_hip_intra_pred_batch(SvtHipContext *ctx, const SvtHipIntraPredDesc *d);
/* Host-only validation: a null descriptor or nbr / dst / jobs / status, a bit_depth other than 8 / 10, a zero nbr_stride, nbr_width,
 * nbr_height or dst_stride, an nbr_stride below nbr_width, zero dst_samples, a destination range (dst_samples from dst) that overlaps the
 * neighbour plane: the jobs of one batch must not read what the batch writes. */
int    svt_hip_intra_pred_check_desc(const SvtHipIntraPredDesc *d);
/* sizeof / offsetof as compiled, for the bindings: what = 0 the descriptor, 1 the job; `field` < 0 the size, else the offset of the
 * field-th member in declaration order ((size_t)-1 past the last) */
size_t svt_hip_intra_pred_layout(int what, int field);

#ifdef __cplusplus
}
#endif
#endif
