/*
 * svt_hip_dsp.h -- C-ABI of the MI355X mode-decision RD kernels (residual, forward / inverse integer AV1
 * transforms, quantize + dequantize, coefficient-domain and pixel-domain distortion, SATD).
 *
 * The batched entry svt_hip_rd_batch evaluates, for every job, one iteration of the reference's tx_type_search
 * loop body (Source/Lib/Codec/product_coding_loop.c:4764-4934):
 *     svt_residual_kernel8bit/16bit  (Codec/pic_operators.c:101-148)
 *  -> svt_aom_estimate_transform / svt_av1_fwd_txfm2d_{WxH} (+ svt_handle_transform{64..}) (Codec/transforms.c:2259-2631,3158)
 *  -> svt_aom_satd                                          (Codec/common_dsp_rtcd.c:70-77)
 *  -> svt_aom_quantize_b / svt_aom_highbd_quantize_b / svt_av1_quantize_fp / svt_av1_highbd_quantize_fp
 *                                                           (Codec/full_loop.c:29-198,282-474)
 *  -> svt_full_distortion_kernel32_bits                     (Codec/pic_operators.c:150-172)
 *  -> svt_av1_inv_txfm2d_add_{WxH}                          (Codec/inv_transforms.c:2459-2716)
 *  -> svt_spatial_full_distortion_kernel / svt_full_distortion_kernel16_bits (picture_operators_c.c:65-83, pic_operators.c:174-197)
 * The rate half of that loop body -- svt_aom_txb_estimate_coeff_bits, RDCOST and the choice of the winning tx_type -- is
 * svt_hip_coeff_rate_batch below; it reads the qcoeff / eob arrays svt_hip_rd_batch writes, on the device.  Between the two sits RDOQ,
 * svt_hip_rdoq_batch (svt_av1_optimize_b behind its gates, Codec/full_loop.c:1127-1336,1764-1817): it rewrites the "fp" quantizer's qcoeff /
 * dqcoeff / eob in place and renews dist_coeff and cul_level.  The early exits of the search stay on the host.
 *
 * Also here: the forward and the inverse transform as batches of their own (svt_hip_fwd_txfm_batch, svt_hip_inv_txfm_batch), the
 * coefficient rate estimation with the RD cost and the winning candidate (svt_hip_coeff_rate_batch), RDOQ (svt_hip_rdoq_batch), batched block statistics incl. the PSYEX psy-RD term and distortion facades (svt_hip_block_stats_batch, svt_hip_spy_rd_bias),
 * full-pel prediction from ME results (svt_hip_fullpel_pred{,_batch}) and the scan-order / size helpers.
 */
#ifndef SVT_HIP_DSP_H
#define SVT_HIP_DSP_H

#include <stdint.h>
#include "svt_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TxSize / TxType use the reference's enum values (Codec/definitions.h): TX_4X4=0 ... TX_64X16=18; DCT_DCT=0 ... H_FLIPADST=15 */
#define SVT_HIP_TX_SIZES_ALL 19
#define SVT_HIP_TX_TYPES 16

/* Per-qindex quantizer rows as MacroblockPlane / Dequants hold them (Codec/full_loop.c:1627-1685): [0] = DC, [1] = AC */
typedef struct SvtHipQuantRow {
    int16_t zbin[2], round[2], quant[2], quant_shift[2]; /* "b" quantizer */
    int16_t round_fp[2], quant_fp[2];                    /* "fp" quantizer */
    int16_t dequant[2];
} SvtHipQuantRow;

typedef struct SvtHipTxJob {
    uint32_t src_offset;  /* sample offset of the block's top-left sample in the source plane   */
    uint32_t pred_offset; /* sample offset in the prediction plane (and in the recon plane)       */
    uint8_t  tx_type;
    uint8_t  quant_row;   /* index into SvtHipRdBatchDesc.quant_rows */
    uint8_t  pf_shape;    /* EB_TRANS_COEFF_SHAPE (Codec/definitions.h): 0 DEFAULT, 1 N2, 2 N4, 3 ONLY_DC -- the partial-frequency
                           * forward transforms av1_estimate_transform_{N2,N4,ONLY_DC} (Codec/transforms.c:2633-2948) */
    uint8_t  reserved;
} SvtHipTxJob;

typedef struct SvtHipRdBatchDesc {
    uint8_t  bit_depth;     /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  quant_kind;    /* 0 = "b" (zbin / quant_shift), 1 = "fp", 2 = "fp" with the log-scale of the size forced to 0: the TPL
                             * dispenser calls plain svt_av1_quantize_fp for every transform size (get_quantize_error, Codec/src_ops_process.c:225-249) */
    uint8_t  tx_size;       /* TxSize shared by every job of this call (one kernel instantiation per size) */
    uint8_t  reserved;
    uint32_t n_jobs;
    uint32_t src_stride, pred_stride; /* in samples */
    const void           *src, *pred; /* device pointers */
    void                 *recon;      /* device pointer or NULL; same geometry as pred */
    const SvtHipTxJob    *jobs;       /* device pointer, n_jobs entries */
    const SvtHipQuantRow *quant_rows; /* device pointer */
    uint32_t              n_quant_rows;
    /* per-job outputs (device pointers; eob .. sse mandatory) */
    uint16_t *eob;                    /* [n_jobs] */
    uint32_t *satd;                   /* [n_jobs] svt_aom_satd of the kept coefficients */
    uint64_t *dist_coeff;             /* [n_jobs][2] {sum (coeff - dqcoeff)^2, sum coeff^2} */
    uint64_t *three_quad_energy;      /* [n_jobs] energy of the frequencies a 64-point size discards (0 otherwise) */
    uint64_t *sse;                    /* [n_jobs] sum (src - recon)^2 */
    int32_t  *coeff, *qcoeff, *dqcoeff; /* optional: [n_jobs][min(W,32)*min(H,32)] packed like the reference */
    /* optional quantization matrices of this tx_size (device pointers, min(W,32)*min(H,32) bytes each, AOM_QM_BITS = 5 fixed
     * point: pcs->ppcs->gqmatrix / giqmatrix[level][plane][adjusted_tx_size], full_loop.c:1606-1613); applied to the jobs with
     * a 2-D tx_type (tx_type < IDTX), like the reference; NULL = flat */
    const uint8_t *qmatrix, *iqmatrix;
    /* optional, [n_jobs] (device pointer): svt_av1_compute_cul_level(scan, qcoeff, &eob) (Codec/full_loop.c:1449-1466) -- the value
     * svt_aom_quantize_inv_quantize returns when rate_est_ctrls.update_skip_ctx_dc_sign_ctx is set (:1832-1836): min(63, sum |qcoeff|)
     * with the DC sign in bits 6-7 (negative: | 64, positive: + 128); feeds the entropy contexts of the next block's rate estimate */
    uint8_t *cul_level;
} SvtHipRdBatchDesc;

/* Enqueues one batch on the context stream (asynchronous).  Every pointer in `d` is a DEVICE pointer.
 * Returns non-zero (and leaves nothing enqueued) when the descriptor fails validation.
 * Every svt_hip_*_batch entry of this header that takes a descriptor leaves "<entry>: null context or descriptor" in svt_hip_last_error for a null argument. */
int svt_hip_rd_batch(SvtHipContext *ctx, const SvtHipRdBatchDesc *d);

/* ---- forward transform alone ------------------------------------------------------------------------------------
 * svt_av1_fwd_txfm2d_{W}x{H}{,_N2,_N4} (Codec/transforms.c:2259-2631,5202-5425,6769-6990) on an int16 residual plane: the FULL W x H
 * coefficient array per job, row-major (what the per-size pointers return; packing the 64-point sizes is svt_handle_transform*). */
typedef struct SvtHipFwdTxBatchDesc {
    uint8_t  tx_size, reserved[3];
    uint32_t n_jobs;
    uint32_t residual_stride;    /* in samples */
    const int16_t     *residual; /* device pointers */
    const SvtHipTxJob *jobs;     /* src_offset: the block in `residual`; tx_type; pf_shape 0 / 1 / 2 = full / _N2 / _N4, 3 = the DC coefficient alone
                                  * (av1_estimate_transform_ONLY_DC, transforms.c:2925-2946); only its two low bits are read */
    int32_t           *coeff;    /* [n_jobs][W * H] */
} SvtHipFwdTxBatchDesc;
int svt_hip_fwd_txfm_batch(SvtHipContext *ctx, const SvtHipFwdTxBatchDesc *d);

/* ---- inverse transform + reconstruction alone ------------------------------------------------------------------
 * The tail of the RD chain on caller-supplied dequantized coefficients: svt_av1_inv_txfm2d_add_{W}x{H} (Codec/inv_transforms.c:
 * 2459-2716) = recon = clip(pred + inverse(dqcoeff)), read and write planes separate (may alias), as svt_aom_inv_transform_recon /
 * svt_aom_inv_transform_recon8bit drive it in the encode pass (inv_transforms.c:3087-3192). */
typedef struct SvtHipInvTxBatchDesc {
    uint8_t  bit_depth;    /* 8 or 10: clamp ranges of the stages and of the output */
    uint8_t  sample_bytes; /* 1: uint8 planes (bit_depth 8 only); 2: uint16 planes (the `_c` entries' layout for either depth) */
    uint8_t  tx_size;      /* shared by the batch */
    uint8_t  reserved;
    uint32_t n_jobs;
    uint32_t pred_stride, recon_stride; /* in samples */
    const void        *pred;            /* device pointers */
    void              *recon;
    const SvtHipTxJob *jobs;            /* pred_offset: the block in `pred`; src_offset: the block in `recon`; tx_type */
    const int32_t     *dqcoeff;         /* [n_jobs][min(W,32) * min(H,32)] packed like the reference's inverse entries take them */
} SvtHipInvTxBatchDesc;
int svt_hip_inv_txfm_batch(SvtHipContext *ctx, const SvtHipInvTxBatchDesc *d);

/* ---- batched block statistics ---------------------------------------------------------------------------------
 * Per job: SAD, SSE, variance and Hadamard SATD of (src block - ref block).  Restates
 *   svt_nxm_sad_kernel_helper_c / svt_aom_sad_16b_kernel_c          (C_DEFAULT/compute_sad_c.c:20-56,209)
 *   svt_spatial_full_distortion_kernel_c / svt_full_distortion_kernel16_bits_c / svt_aom_sse_c
 *                                                                   (C_DEFAULT/picture_operators_c.c:65-83, Codec/pic_operators.c:174-197)
 *   svt_aom_variance{W}x{H}_c, svt_aom_sub_pixel_variance{W}x{H}_c  (C_DEFAULT/variance.c:256-318)
 *   hadamard_path_c = residual -> svt_aom_hadamard_NxN -> svt_aom_satd over <= 32x32 tiles
 *                                                                   (Codec/enc_mode_config.c:2151-2217)
 *   svt_psy_distortion / svt_psy_distortion_hbd / get_svt_psy_full_dist  (Codec/psy_rd.c:135-293)                           */
typedef struct SvtHipBlockJob {
    uint32_t src_offset, ref_offset; /* sample offsets of the block's top-left sample in the two planes */
    uint8_t  width, height;          /* 1..128 */
    uint8_t  subpel_x, subpel_y;     /* 0..7: the src block is first interpolated at this 1/8-sample phase with the 2-tap bilinear
                                      * filters of svt_aom_sub_pixel_variance{W}x{H}_c (C_DEFAULT/variance.c:28-75,308-318;
                                      * filter.h:39-48): horizontal pass on height+1 rows, then vertical.  (0,0) = src as is */
} SvtHipBlockJob;

typedef struct SvtHipBlockStatsDesc {
    uint8_t  bit_depth;   /* 8: planes are uint8; 10: planes are uint16 */
    uint8_t  temporal_layer_index; /* pcs->temporal_layer_index (0..5), read for facade_dist only */
    uint8_t  spy_rd;               /* EbSvtAv1EncConfiguration.spy_rd (API/EbSvtAv1Enc.h:1020), read for facade_dist only */
    uint8_t  reserved;
    uint32_t n_jobs;
    uint32_t src_stride, ref_stride; /* in samples */
    const void           *src, *ref; /* device pointers */
    const SvtHipBlockJob *jobs;      /* device pointer, n_jobs entries */
    /* per-job outputs, device pointers; any of them may be NULL (not computed) */
    uint32_t *sad;      /* sum |src - ref| */
    uint64_t *sse;      /* sum (src - ref)^2, 64-bit */
    uint32_t *variance; /* sse32 - sum^2 / (w*h), the svt_aom_variance* return value (32-bit wrap like the reference) */
    uint32_t *var_sse;  /* the `sse` out-parameter of svt_aom_variance* (32-bit) */
    uint32_t *satd;     /* hadamard_path_c of a square block (4..128); 0 for other shapes; 8-bit planes only */
    /* PSYEX psy-RD term (Codec/psy_rd.c:135-293): src = input, ref = reconstruction; width and height multiples of 4 */
    double    psy_rd;     /* strength; only used for psy_dist */
    uint64_t *psy_energy; /* svt_psy_distortion / svt_psy_distortion_hbd */
    uint64_t *psy_dist;   /* get_svt_psy_full_dist: (uint64_t)(psy_energy * psy_rd), one fp64 multiply */
    /* PSYEX distortion facades (C_DEFAULT/picture_operators_c.c:85-174), src = input, ref = prediction or reconstruction */
    uint64_t      *psy_sse;       /* svt_spatial_psy_distortion_kernel_c: sse + (uint64_t)(psy_energy * psy_rd) when psy_rd > 0 */
    const uint8_t *pred_mode;     /* [n_jobs] PredictionMode of the candidate, device pointer; mandatory with facade_dist */
    const uint8_t *compound_type; /* [n_jobs] CompoundType, device pointer; mandatory with facade_dist */
    uint64_t      *facade_dist;   /* svt_spatial_full_distortion_kernel_facade: the SSE with the spy-rd mode biases */
    /* svt_aom_highbd_10_variance{W}x{H}_c (Codec/svt_psnr.c:139-177), 10-bit planes only: sse and sum are brought back to the
     * 8-bit scale with rounding ((sse + 8) >> 4, (sum + 2) >> 2) before sse - sum^2 / (w*h), clamped at 0 */
    uint32_t *variance10, *var_sse10;
    /* Optional hierarchical jobs: `n_pyramids` 64x64 regions (device array `pyramids`; width = height = 64, no sub-pixel view).  One wave
     * reads a region's samples ONCE and produces the outputs of its 85 nested square blocks -- the 64x64, its 4 32x32, 16 16x16 and 64 8x8
     * blocks, each level in raster order: SAD / sum / SSE (hence every variance and facade output) and the PSYEX psy energy (a sum over
     * 8x8 tiles for every block size, psy_rd.c:135-274) add up the tree; hadamard_path's SATD is evaluated per size from one staged
     * residual (a 64x64 SATD is the sum of its four 32x32 tiles', enc_mode_config.c:2151-2217).  Region k writes output slots
     * pyramid_out_base + 85 k .. + 84 of the same output arrays (pred_mode / compound_type are read at those slots); plain jobs keep
     * slots 0 .. n_jobs - 1.  Results are those of 85 plain jobs. */
    uint32_t              n_pyramids, pyramid_out_base;
    const SvtHipBlockJob *pyramids;
} SvtHipBlockStatsDesc;
#define SVT_HIP_PYRAMID_BLOCKS 85

/* The integer biases svt_spatial_full_distortion_kernel_facade applies to an SSE (picture_operators_c.c:130-171): host-only
 * arithmetic, for callers that already hold the SSE (e.g. SvtHipRdBatchDesc.sse).  mode / compound_type are the reference's
 * PredictionMode / CompoundType enumerators; temporal_layer_index <= 5. */
uint64_t svt_hip_spy_rd_bias(uint64_t sse, uint32_t area_width, uint32_t area_height, uint8_t mode, uint8_t compound_type,
                             uint8_t temporal_layer_index, double psy_rd, uint8_t spy_rd);

/* Enqueues one batch on the context stream (asynchronous); one wave per job. */
int svt_hip_block_stats_batch(SvtHipContext *ctx, const SvtHipBlockStatsDesc *d);

/* Flat jobs one wave of that launch works through, one after the other: 4, or 1 for a hadamard_path batch (d->satd set) of too few jobs to
 * give every compute unit several four-job waves.  The launch itself asks this function; outputs do not depend on the answer.  Reads
 * d->satd and d->n_jobs only; 0 for a null argument. */
uint32_t svt_hip_block_stats_jobs_per_wave(SvtHipContext *ctx, const SvtHipBlockStatsDesc *d);

/* ---- batched SSIM distortion (--tune 2 / 3 / 4) -------------------------------------------------------------------
 * Per job, src = input, ref = prediction or reconstruction:
 *   ssim       the block mean ssim() / ssim_hbd() returns (Codec/mode_decision.c:4781-4878): 8x8 tiles when both sides are multiples
 *              of 8, else 4x4 tiles; each tile's similarity() (Codec/enc_dec_process.c:709-735) clamped to [0, 1], the scores added in
 *              raster order, divided by the tile count
 *   ssim_dist  svt_spatial_full_distortion_ssim_kernel (mode_decision.c:4879-4921): (uint64_t)((1 - ssim) * w * h * 100 * 7 * m), m = 1
 *              (8-bit) or 8 (10-bit), plus (uint64_t)(svt_psy_distortion{,_hbd} * psy_rd) when psy_rd > 0.  The callers' own shifts
 *              (<<= 4 ...) stay with the callers.
 * Sides are multiples of 4 in 4..128 (the callers pass cropped transform sizes); subpel_x / subpel_y must be 0.  Bit-exact with the
 * reference's fp64 arithmetic.  The psy term reads whole 8x8 (4x4) tiles, past a cropped block's right / bottom edge like the reference.
 * Optional pyramids: 64x64 regions, each read once for the 85 nested blocks in the layout of SvtHipBlockStatsDesc's (slots pyramid_out_base
 * + 85 k ...); their results equal 85 plain jobs. */
typedef struct SvtHipSsimBatchDesc {
    uint8_t  bit_depth; /* 8: planes are uint8; 10: planes are uint16 (at most 10 bits per sample) */
    uint8_t  reserved[3];
    uint32_t n_jobs;
    uint32_t src_stride, ref_stride;  /* in samples */
    const void           *src, *ref;  /* device pointers */
    const SvtHipBlockJob *jobs;       /* device pointer, n_jobs entries */
    double                psy_rd;     /* strength of the psy term; <= 0: none */
    /* per-job outputs, device pointers, at least one of them */
    double               *ssim;
    uint64_t             *ssim_dist;
    uint32_t              n_pyramids, pyramid_out_base;
    const SvtHipBlockJob *pyramids;   /* device pointer, n_pyramids 64x64 regions */
} SvtHipSsimBatchDesc;

/* Enqueues one batch on the context stream (asynchronous); one wave per job or region.  Returns non-zero and enqueues nothing when the
 * descriptor fails validation (null context / pointers, no output, bit depth other than 8 or 10).  The jobs live in device memory, where the
 * host cannot read them without waiting: check a host copy with svt_hip_ssim_check_jobs before uploading it.  A job that fails that check
 * anyway reads no sample and gets ssim = -1, ssim_dist = UINT64_MAX. */
int    svt_hip_ssim_batch(SvtHipContext *ctx, const SvtHipSsimBatchDesc *d);
/* Host arrays: non-zero (and svt_hip_last_error) when a job's sides are not multiples of 4 in 4..128 or its subpel is set; with
 * `pyramids` != 0, when a region is not 64x64. */
int    svt_hip_ssim_check_jobs(const SvtHipBlockJob *jobs, uint32_t n_jobs, int pyramids);
size_t svt_hip_ssim_desc_size(void); /* sizeof(SvtHipSsimBatchDesc) as compiled */

/* ---- coefficient rate estimation, RD cost and the winning candidate -------------------------------------------------
 * Per job, svt_aom_txb_estimate_coeff_bits of one plane (Codec/rd_cost.c:1405-1450) behind the two short-cuts of tx_type_search
 * (Codec/product_coding_loop.c:4947-4952):
 *   bits     luma, (coeff_rate_est_lvl >= 2 || == 0) && eob < th:  6000 + eob * 1000,  th = (tx_width * tx_height) >> 6 (real dimensions)
 *            luma, coeff_rate_est_lvl == 0:                        3000 + eob * 100
 *            eob == 0:                                             av1_cost_skip_txb = txb_skip_cost[txb_skip_ctx][1]
 *            else svt_av1_cost_coeffs_txb with allow_update_cdf == 0 (rd_cost.c:434-559), luma << mds_subres_step; chroma carries no
 *            transform-type rate, no shift and no short-cut
 *   rd_cost  RDCOST(lambda, bits, dist) (Codec/rd_cost.h:37) = ((bits * lambda + 256) >> 9) + (dist << 7); the caller's own shifts of
 *            the distortion and its three_quad_energy addition stay with the caller
 * and per group of consecutive jobs (the candidates of one block), the first strict minimum of rd_cost in job order.  That is
 * tx_type_search's best_tx_type (product_coding_loop.c:4976-4985) exactly when txt_ctrls.early_exit_coeff_th == 0 &&
 * txt_ctrls.early_exit_dist_th == 0 (no candidate is skipped behind a good one, :4987-5002), ssim_level <= SSIM_LVL_1 (the search
 * compares SSD costs), and the caller lists a block's candidates in the reference's group order (the tx_type_group loop's).  The
 * search's early_cost > best_cost skip (:4941-4945) never changes the winner: RDCOST is monotone in the rate.
 * Bit-exact: integer, table-driven arithmetic whose 32-bit sums are order-free. */
typedef struct SvtHipLvMapCoeffCost { /* LvMapCoeffCost (Codec/md_rate_estimation.h:41-49) */
    int32_t txb_skip_cost[13][2];
    int32_t base_eob_cost[4][3];
    int32_t base_cost[42][8];
    int32_t eob_extra_cost[22][2];
    int32_t dc_sign_cost[3][2];
    int32_t lps_cost[21][26];
} SvtHipLvMapCoeffCost;
typedef struct SvtHipLvMapEobCost { /* LvMapEobCost (:37-39) */
    int32_t eob_cost[2][11];
} SvtHipLvMapEobCost;
/* The four members of MdRateEstimationContext the estimate reads (Codec/md_rate_estimation.h:127-133), same element types and bounds: a
 * host copies them member by member.  Lives in DEVICE memory, uploaded by the caller; changes once per picture. */
typedef struct SvtHipRateTables {
    SvtHipLvMapCoeffCost coeff_fac_bits[5][2];          /* [TX_SIZES][PLANE_TYPES] */
    SvtHipLvMapEobCost   eob_frac_bits[7][2];
    int32_t intra_tx_type_fac_bits[3][4][13][17];      /* [EXT_TX_SETS_INTRA][EXT_TX_SIZES][INTRA_MODES][CDF_SIZE(TX_TYPES)] */
    int32_t inter_tx_type_fac_bits[4][4][17];          /* [EXT_TX_SETS_INTER][EXT_TX_SIZES][CDF_SIZE(TX_TYPES)] */
} SvtHipRateTables;

typedef struct SvtHipRateJob {
    uint8_t tx_type;      /* below 16 */
    uint8_t txb_skip_ctx; /* 0..12: ctx->luma_txb_skip_context / cb_ / cr_ */
    uint8_t dc_sign_ctx;  /* 0..2:  ctx->luma_dc_sign_context / cb_ / cr_ */
    uint8_t is_inter;     /* is_inter_mode(cand->pred_mode) */
    uint8_t intra_dir;    /* 0..12, read for intra luma jobs only: cand->pred_mode, or fimode_to_intradir[cand->filter_intra_mode] when that is set;
                           * any value on inter and chroma jobs */
    uint8_t reserved[3];
} SvtHipRateJob;

typedef struct SvtHipCoeffRateDesc {
    uint8_t  tx_size;                  /* TxSize shared by every job of this call */
    uint8_t  plane_type;               /* 0 PLANE_TYPE_Y, 1 PLANE_TYPE_UV, shared */
    uint8_t  reduced_tx_set;           /* frm_hdr->reduced_tx_set */
    uint8_t  coeff_rate_est_lvl;       /* ctx->rate_est_ctrls.coeff_rate_est_lvl: selects the short-cuts above (luma); 1 = none */
    uint8_t  mds_fast_coeff_est_level; /* ctx->mds_fast_coeff_est_level, not 0 */
    uint8_t  mds_subres_step;          /* ctx->mds_subres_step, 0..2 */
    uint8_t  reserved[2];
    uint32_t n_jobs, n_groups;
    const SvtHipRateJob    *jobs;      /* device pointers */
    const SvtHipRateTables *tables;
    const int32_t  *qcoeff;            /* [n_jobs][min(W,32)*min(H,32)]: SvtHipRdBatchDesc.qcoeff; 16-byte aligned where that is 256 coefficients or more */
    const uint16_t *eob;               /* [n_jobs]: SvtHipRdBatchDesc.eob */
    uint64_t       *bits;              /* [n_jobs] */
    /* optional: rd_cost[j] = RDCOST(lambda, bits[j], dist[j * dist_stride]); dist_stride 0 counts as 1, 2 reads the first column of
     * SvtHipRdBatchDesc.dist_coeff in place */
    uint32_t        lambda, dist_stride;
    const uint64_t *dist;
    uint64_t       *rd_cost;           /* [n_jobs] */
    /* optional, needs rd_cost: jobs group_start[g] .. group_start[g + 1] - 1 are the candidates of block g (ascending; an end beyond n_jobs is
     * cut there).  best_job[g] is the job index of the first strict minimum of rd_cost, best_cost[g] its cost; a group that is empty or
     * whose jobs are all undefined reports 0xFFFFFFFF and UINT64_MAX. */
    const uint32_t *group_start;       /* [n_groups + 1] */
    uint32_t       *best_job;          /* [n_groups] */
    uint64_t       *best_cost;         /* [n_groups] */
} SvtHipCoeffRateDesc;

/* Enqueues one batch on the context stream (asynchronous).  Returns non-zero and enqueues nothing when the descriptor fails validation: a
 * null context, descriptor or mandatory pointer (jobs, tables, qcoeff, eob, bits), tx_size >= 19, plane_type > 1, mds_subres_step > 2,
 * mds_fast_coeff_est_level == 0, a qcoeff that is not 16-byte aligned for a size of 256 coefficients or more, rd_cost without dist, groups without rd_cost (or without one of
 * group_start, best_job, best_cost).
 * The jobs live in device memory, where the host cannot refuse them.  Where the reference is undefined -- eob above the coefficient count or
 * a zero coefficient at scan[eob - 1] (it indexes base_eob_cost[..][-1]), a context or tx_type outside its table, an intra_dir above 12 on an intra luma job (the only jobs that read it) -- a job that
 * would take the table path reads no table out of range and reports bits = rd_cost = UINT64_MAX (the convention of svt_hip_ssim_batch); its
 * neighbours are not affected. */
int    svt_hip_coeff_rate_batch(SvtHipContext *ctx, const SvtHipCoeffRateDesc *d);
size_t svt_hip_coeff_rate_desc_size(void); /* sizeof(SvtHipCoeffRateDesc) as compiled */
size_t svt_hip_rate_tables_size(void);     /* sizeof(SvtHipRateTables) as compiled */

/* ---- RDOQ: the trellis pass over quantised coefficients ---------------------------------------------------------------
 * Per job, the part of svt_aom_quantize_inv_quantize that follows the first ("fp") quantizer call when is_encode_pass == 0
 * (Codec/full_loop.c:1764-1817, then :1832-1836), on the coeff / qcoeff / dqcoeff / eob arrays svt_hip_rd_batch writes with quant_kind 1:
 *   eob_perc = eob * 100 / (tx_width * tx_height) on the real dimensions
 *   eob_perc >= eob_th       RDOQ is off for the job and the reference re-quantizes with the "b" quantizer: status 2.  With the fallback
 *                            arrays (the same jobs through svt_hip_rd_batch with quant_kind 0) the job's outputs become theirs; without
 *                            them the job is left untouched
 *   eob_perc >= eob_fast_th  svt_fast_optimize_b = update_coeff_eob_fast (:1092-1126) first: un-weighted dequant, zbin = dq +
 *                            ROUND_POWER_OF_TWO(dq * 70, 7)
 *   eob != 0                 svt_av1_optimize_b (:1127-1336) with rdmult = ((lambda * plane_rd_mult[is_inter][plane_type] * rweight) / 100 + 2)
 *                            >> MAX(2, sharpness), plane_rd_mult = {17, 13}, {16, 10} (TUNE_CHROMA_SSIM == 1); a job's `sharp` flag sets
 *                            rweight = 0 and switches eob shortening and update_skip off (:1169-1182); eob_fast_inter / eob_fast_intra are its
 *                            fast_mode (trims again, skips the update_coeff_eob loop)
 *   cul_level                svt_av1_compute_cul_level of the result
 * Bit-exact.  Decided on the host and therefore not carried: rdoq_ctrls.dct_dct_only, skip_uv, ctx->mds_skip_rdoq and lossless segments
 * are known per job there -- the caller simply does not list those jobs; rdoq_ctrls.satd_factor is 255 and early_exit_th is 0 at every RDOQ
 * level (set_rdoq_controls, Codec/enc_mode_config.c:3336-3418), and eob_cost < 0 never holds.  The encode-pass branch
 * (svt_av1_perform_noise_normalization, the 16-bit-pipeline quantizer choice) is not part of this entry. */
typedef struct SvtHipRdoqJob {
    uint8_t tx_type;      /* below 16 */
    uint8_t txb_skip_ctx; /* 0..12 */
    uint8_t dc_sign_ctx;  /* 0..2 */
    uint8_t is_inter;     /* pred_mode >= NEARESTMV */
    uint8_t quant_row;    /* index into quant_rows */
    uint8_t flags;        /* bit 0 = sharp: use_sharpness && delta_q_present && plane == 0 && (sb qindex - quantizer_to_qindex[picture_qp] < 0 ||
                           * sharp_tx), evaluated by the host */
    uint8_t reserved[2];
} SvtHipRdoqJob;

typedef struct SvtHipRdoqDesc {
    uint8_t  tx_size;        /* TxSize shared by every job of this call */
    uint8_t  plane_type;     /* 0 PLANE_TYPE_Y, 1 PLANE_TYPE_UV, shared */
    uint8_t  sharpness;      /* 0..7: static_config.sharpness */
    uint8_t  eob_fast_inter; /* rdoq_ctrls.eob_fast_{y,uv}_inter of this plane type */
    uint8_t  eob_fast_intra; /* rdoq_ctrls.eob_fast_{y,uv}_intra */
    uint8_t  eob_th;         /* rdoq_ctrls.eob_th, 255 = off (as set_rdoq_controls writes it) */
    uint8_t  eob_fast_th;    /* rdoq_ctrls.eob_fast_th, 255 = off */
    uint8_t  reserved;
    uint32_t n_jobs;
    uint32_t lambda;
    const SvtHipRdoqJob    *jobs;        /* device pointers */
    const SvtHipRateTables *tables;
    const SvtHipQuantRow   *quant_rows;  /* only `dequant` is read */
    uint32_t                n_quant_rows, reserved2;
    const uint8_t          *iqmatrix;    /* optional, as SvtHipRdBatchDesc.iqmatrix: applied to the 2-D tx types only (get_dqv) */
    const int32_t          *coeff;       /* [n_jobs][min(W,32)*min(H,32)] */
    int32_t                *qcoeff, *dqcoeff; /* in place */
    uint16_t               *eob;         /* [n_jobs], in place */
    /* optional outputs */
    uint8_t  *status;                    /* [n_jobs] 0 optimised; 1 eob == 0 on entry or after the fast trim (nothing else done); 2 the eob_th gate
                                          * fired; 0xFF undefined input */
    uint64_t *dist_coeff;                /* [n_jobs][2] svt_full_distortion_kernel32_bits of the final coeff / dqcoeff, the meaning of
                                          * SvtHipRdBatchDesc.dist_coeff: svt_hip_coeff_rate_batch reads it with dist_stride 2 */
    uint8_t  *cul_level;                 /* [n_jobs] */
    /* optional fallback behind the eob_th gate, all three or none: the arrays svt_hip_rd_batch writes for the same jobs with quant_kind 0 */
    const int32_t  *qcoeff_b, *dqcoeff_b;
    const uint16_t *eob_b;
} SvtHipRdoqDesc;

/* Enqueues one batch on the context stream (asynchronous).  Returns non-zero and enqueues nothing when the descriptor fails validation: a null
 * context, descriptor or mandatory pointer (jobs, tables, quant_rows, coeff, qcoeff, dqcoeff, eob), tx_size >= 19, plane_type > 1,
 * sharpness > 7, n_quant_rows == 0, a fallback with one of its three arrays missing.  (The kernel loads single coefficients: no alignment
 * beyond the element's is asked for.)
 * The jobs live in device memory, where the host cannot refuse them.  Where the reference is undefined -- eob above the coefficient count, a zero
 * coefficient at scan[eob - 1], a context or tx_type outside its table, quant_row >= n_quant_rows -- a job writes nothing but status 0xFF; its
 * neighbours are not affected.  A job behind the eob_th gate without fallback arrays writes nothing but status 2.  dist_coeff and cul_level are
 * written for status 0 and 1, and for status 2 with fallback arrays. */
int    svt_hip_rdoq_batch(SvtHipContext *ctx, const SvtHipRdoqDesc *d);
size_t svt_hip_rdoq_desc_size(void); /* sizeof(SvtHipRdoqDesc) as compiled */

/* The launch of svt_hip_coeff_rate_batch and svt_hip_rdoq_batch.  Both pack the jobs of a batch into waves (four jobs of 16 coefficients, two
 * of 32, one of any other size: a pack) and launch at most 2048 workgroups of four waves; wave v of workgroup b takes the packs b * 4 + v,
 * b * 4 + v + grid * 4, ... -- more than one of them (a second "trip") once a batch holds more than grid * 4 packs.
 * svt_hip_context_set_lvmap_max_grid lowers (or raises) that limit of 2048 for the context's later batches; 0 restores it.  The results do
 * not depend on it: it is there so that a small batch can walk the loop as a picture-sized one does.
 * svt_hip_lvmap_plan is host arithmetic alone (no context, no device): what a batch of n_jobs jobs of tx_size would launch under the limit
 * max_grid (0: 2048) -- the workgroups, the packs and the jobs per pack.  Non-zero for tx_size >= 19 or a null output. */
int svt_hip_context_set_lvmap_max_grid(SvtHipContext *ctx, uint32_t max_grid);
int svt_hip_lvmap_plan(uint32_t tx_size, uint32_t n_jobs, uint32_t max_grid, uint32_t *grid, uint32_t *n_packs, uint32_t *jobs_per_pack);

/* Full-pel motion-compensated prediction from ME results: every 16x16 PU copies the block of `ref` displaced by its
 * best integer MV (sb_best_mv = SvtHipMeResults.sb_best_mv, device pointer; list / ref_idx select the reference).
 * ref / pred are device planes of `bit_depth` 8 (uint8) or 10 (uint16), strides in samples, no padding needed
 * (coordinates are clamped to the picture).  The integer-MV case of inter prediction; feeds svt_hip_rd_batch. */
int svt_hip_fullpel_pred(SvtHipContext *ctx, const void *ref, uint32_t ref_stride, uint32_t width, uint32_t height, uint8_t bit_depth,
                         const uint32_t *sb_best_mv, uint8_t list, uint8_t ref_idx, uint32_t b64_row_start, uint32_t b64_row_count,
                         void *pred, uint32_t pred_stride); /* b64_row_count == 0: all rows from b64_row_start */

/* Several pictures in one launch (at most SVT_HIP_PRED_MAX_JOBS): all share the plane geometry; per job the reference plane, the
 * MV array, the prediction plane and the row band.  Host array of jobs holding device pointers. */
#define SVT_HIP_PRED_MAX_JOBS 16
typedef struct SvtHipPredJob {
    const void     *ref;
    const uint32_t *sb_best_mv;
    void           *pred;
    uint32_t        b64_row_start, b64_row_count; /* count 0: all rows from b64_row_start */
    uint8_t         list, ref_idx, reserved[6];
} SvtHipPredJob;
int svt_hip_fullpel_pred_batch(SvtHipContext *ctx, uint32_t ref_stride, uint32_t width, uint32_t height, uint8_t bit_depth, uint32_t pred_stride,
                               uint32_t n_jobs, const SvtHipPredJob *jobs);

/* get_hvs_modulation_factor (Codec/psy_rd.c:295-307): the psy-rd strength every psy call site passes on (e.g. product_coding_loop.c:972,
 * 4618): x0.4 on intra (I-slice) pictures, x0.75 / x0.9 / x0.95 on temporal layers 0 / 1 / 2, unchanged above.  Host arithmetic (one fp64
 * multiply, same operand order as the reference). */
double svt_hip_hvs_modulation_factor(double psy_rd, int is_islice, uint8_t temporal_layer_index);

/* Scan order of (tx_size, tx_type) as av1_scan_orders holds it (Codec/coefficients.h:2197); returns the length. */
int svt_hip_scan_order(int tx_size, int tx_type, int16_t *scan, int16_t *iscan);
int svt_hip_tx_size_wide(int tx_size);
int svt_hip_tx_size_high(int tx_size);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_DSP_H */
