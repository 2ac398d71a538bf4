#!/usr/bin/env python3
"""Writes tests/golden/mask.npz: the reference encoder's own masked-prediction results on the cases of tests/mask_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or bench.py.
It compiles a harness of its own into a temporary directory outside the tree (gcc, -O2) and links it with the reference's
Codec/enc_inter_prediction.c, Codec/blend_a64_mask.c, C_DEFAULT/inter_prediction_c.c, C_DEFAULT/compute_sad_c.c and the two rtcd files where they
lie.  The first translation unit #includes Codec/inter_prediction.c where it lies, because the primaries, the sign-flip table and the contiguous
masks are static, installs the _c kernels in the rtcd pointers, runs svt_av1_init_wedge_masks and drives
  prediction       svt_aom_enc_make_inter_predictor with is_masked_compound 0 for the first reference, then 1 for the second with the job's
                   InterInterCompoundData, the luma bsize, the plane and a seg_mask buffer: a luma DIFFWTD job fills it, the chroma job of the same
                   block is handed the buffer the luma job left; everything else as tools/gen_inter_pred_golden.py drives the non-masked case
  blend            svt_aom_combine_interintra / svt_aom_combine_interintra_highbd on the job's three blocks, in place when the job is
  compound search  svt_aom_calc_pred_masked_compound with ctx->cmp_store pre-filled with the candidate's two MVs and the scripted prediction blocks,
                   so that it skips its predictions and runs the gate and the residuals; then, unless it reports the exit,
                   svt_aom_search_compound_diff_wedge; use_rate = 0
A second translation unit #includes Codec/mode_decision.c where it lies and calls the static inter_intra_search with use_rd_model = 0;
svt_aom_inter_prediction is a stand-in there that copies the scripted inter block (the real one of Codec/enc_inter_prediction.c is compiled under
another name), and svt_aom_combine_interintra{,_highbd} is the first unit's.  Whatever else the link still wants gets a stand-in that aborts.

The fixture holds numbers only: the CRC-32 of the reference's twelve primaries, of its wedge_signflip_lookup rows of the nine sizes and of the
9 x 32 contiguous masks; per prediction / blend batch a CRC-32 per job of the block, per luma DIFFWTD batch a CRC-32 per job of the mask; one whole
block per size and depth; per search batch every output of every job (exit, wedge_index, wedge_sign, mask_type / interintra_mode,
use_wedge_interintra, interintra_wedge_index -- the reference returns no rd).  --check recomputes everything and compares it with the committed
file instead of writing it; either way the restatement of tests/mask_cases.py is compared with the reference on every job, every prediction job's
reads are checked to lie inside its padded plane, and the conditions of the planted search inputs are asserted on the reference's results."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import inter_pred_cases as ip  # noqa: E402
import mask_cases as mc  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include "inter_prediction.c"
#include <stdlib.h>
#include <string.h>
#include "sequence_control_set.h"
#include "pcs.h"
#include "md_process.h"
#include "enc_inter_prediction.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "compute_sad.h"

static SequenceControlSet *g_scs;
static ScaleFactors        g_sf;
static ConvBufType         g_tmp[128 * 128] __attribute__((aligned(32)));

static BlockSize bsize_of(int w, int h) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h) return (BlockSize)b;
    return BLOCK_INVALID;
}

static void plain_memcpy(void *dst, void const *src, size_t size) { memcpy(dst, src, size); } /* what svt_memcpy_c is */

int harness_init(void) {
    svt_memcpy = plain_memcpy;
    svt_aom_convolve[0][0][0] = svt_av1_convolve_2d_copy_sr_c; svt_aom_convolve[1][0][0] = svt_av1_convolve_x_sr_c;
    svt_aom_convolve[0][1][0] = svt_av1_convolve_y_sr_c; svt_aom_convolve[1][1][0] = svt_av1_convolve_2d_sr_c;
    svt_aom_convolve[0][0][1] = svt_av1_jnt_convolve_2d_copy_c; svt_aom_convolve[1][0][1] = svt_av1_jnt_convolve_x_c;
    svt_aom_convolve[0][1][1] = svt_av1_jnt_convolve_y_c; svt_aom_convolve[1][1][1] = svt_av1_jnt_convolve_2d_c;
    svt_aom_convolveHbd[0][0][0] = svt_av1_highbd_convolve_2d_copy_sr_c; svt_aom_convolveHbd[1][0][0] = svt_av1_highbd_convolve_x_sr_c;
    svt_aom_convolveHbd[0][1][0] = svt_av1_highbd_convolve_y_sr_c; svt_aom_convolveHbd[1][1][0] = svt_av1_highbd_convolve_2d_sr_c;
    svt_aom_convolveHbd[0][0][1] = svt_av1_highbd_jnt_convolve_2d_copy_c; svt_aom_convolveHbd[1][0][1] = svt_av1_highbd_jnt_convolve_x_c;
    svt_aom_convolveHbd[0][1][1] = svt_av1_highbd_jnt_convolve_y_c; svt_aom_convolveHbd[1][1][1] = svt_av1_highbd_jnt_convolve_2d_c;
    svt_aom_lowbd_blend_a64_d16_mask = svt_aom_lowbd_blend_a64_d16_mask_c; svt_aom_highbd_blend_a64_d16_mask = svt_aom_highbd_blend_a64_d16_mask_c;
    svt_aom_blend_a64_mask = svt_aom_blend_a64_mask_c; svt_aom_highbd_blend_a64_mask = svt_aom_highbd_blend_a64_mask_c;
    svt_av1_build_compound_diffwtd_mask_d16 = svt_av1_build_compound_diffwtd_mask_d16_c;
    svt_av1_build_compound_diffwtd_mask = svt_av1_build_compound_diffwtd_mask_c;
    svt_av1_build_compound_diffwtd_mask_highbd = svt_av1_build_compound_diffwtd_mask_highbd_c;
    svt_av1_wedge_sse_from_residuals = svt_av1_wedge_sse_from_residuals_c; svt_av1_wedge_sign_from_residuals = svt_av1_wedge_sign_from_residuals_c;
    svt_av1_wedge_compute_delta_squares = svt_av1_wedge_compute_delta_squares_c; svt_aom_sum_squares_i16 = svt_aom_sum_squares_i16_c;
    svt_aom_subtract_block = svt_aom_subtract_block_c; svt_aom_highbd_subtract_block = svt_aom_highbd_subtract_block_c;
    svt_nxm_sad_kernel = svt_nxm_sad_kernel_helper_c; sad_16b_kernel = svt_aom_sad_16b_kernel_c;
    svt_aom_sse = svt_aom_sse_c; svt_aom_highbd_sse = svt_aom_highbd_sse_c;
    svt_av1_init_wedge_masks();
    if (!g_scs) g_scs = calloc(1, sizeof(*g_scs));
    if (!g_scs) return 1;
    svt_av1_setup_scale_factors_for_frame(&g_sf, 192, 128, 192, 128);
    return av1_is_scaled(&g_sf) ? 2 : 0;
}

/* prim: [2][6][64 * 64]; flip: [9][16]; contig: the 9 x 32 contiguous masks; sizes: 9 x (w, h) */
int harness_tables(uint8_t *prim, uint8_t *flip, uint8_t *contig, const int *sizes) {
    memcpy(prim, wedge_mask_obl, sizeof(wedge_mask_obl));
    for (int s = 0; s < 9; s++) {
        const BlockSize b = bsize_of(sizes[2 * s], sizes[2 * s + 1]);
        if (b == BLOCK_INVALID || svt_aom_get_wedge_bits_lookup(b) != 4) return 1;
        memcpy(flip + 16 * s, wedge_signflip_lookup[b], 16);
        for (int k = 0; k < 16; k++)
            for (int sign = 0; sign < 2; sign++) {
                memcpy(contig, svt_aom_get_contiguous_soft_mask(k, sign, b), sizes[2 * s] * sizes[2 * s + 1]);
                contig += sizes[2 * s] * sizes[2 * s + 1];
            }
    }
    int others = 0; /* the sizes without wedges */
    for (int b = 0; b < BlockSizeS_ALL; b++) others += svt_aom_get_wedge_bits_lookup((BlockSize)b) == 0;
    return others == BlockSizeS_ALL - 9 ? 0 : 2;
}

/* p: width, height, org_x, org_y, filter_x, filter_y, mv0 row, mv0 col, mv1 row, mv1 col, the four edges (left, right, top, bottom), ss_x, ss_y,
 *    bit_depth, plane, luma width, luma height, comp_type (0 wedge, 1 diffwtd), wedge_index, wedge_sign, mask_type.
 * src0 / src1: the picture's sample (0, 0) in the (padded) reference planes; strides in samples; seg_mask: luma width x luma height bytes. */
int harness_masked_predict(const int *p, uint8_t *src0, uint8_t *src1, int src_stride, uint8_t *dst, int dst_stride, uint8_t *seg_mask) {
    const int              bd = p[16], is16 = bd > 8;
    const BlockSize        bsize = bsize_of(p[18], p[19]);
    MacroBlockD            xd;
    InterInterCompoundData comp;
    ConvolveParams         cp = get_conv_params_no_round(0, 0, 0, g_tmp, 128, 1, bd);
    InterpFilters          filters = av1_make_interp_filters((InterpFilter)p[5], (InterpFilter)p[4]);
    if (bsize == BLOCK_INVALID) return 1;
    memset(&xd, 0, sizeof(xd));
    memset(&comp, 0, sizeof(comp));
    xd.mb_to_left_edge = p[10]; xd.mb_to_right_edge = p[11]; xd.mb_to_top_edge = p[12]; xd.mb_to_bottom_edge = p[13];
    comp.type = p[20] ? COMPOUND_DIFFWTD : COMPOUND_WEDGE;
    comp.wedge_index = (int8_t)p[21]; comp.wedge_sign = (int8_t)p[22]; comp.mask_type = (DIFFWTD_MASK_TYPE)p[23];
    for (int k = 0; k < 2; k++) {
        MV mv;
        mv.row = (int16_t)p[6 + 2 * k]; mv.col = (int16_t)p[7 + 2 * k];
        svt_aom_enc_make_inter_predictor(g_scs, k ? src1 : src0, NULL, dst, (int16_t)p[3], (int16_t)p[2], mv, &g_sf, &cp, filters, &comp, seg_mask, 192, 128,
                                         (uint8_t)p[0], (uint8_t)p[1], bsize, &xd, src_stride, dst_stride, (uint8_t)p[17], (uint32_t)p[15], (uint32_t)p[14],
                                         (uint8_t)bd, 0, (uint8_t)k, (uint8_t)is16);
    }
    return 0;
}

/* p: bit_depth, interintra_mode, use_wedge, wedge_index, wedge_sign, luma width, luma height, width, height; strides in samples */
int harness_interintra(const int *p, uint8_t *dst, int dst_stride, const uint8_t *inter, int inter_stride, const uint8_t *intra, int intra_stride) {
    const BlockSize bsize = bsize_of(p[5], p[6]), plane_bsize = bsize_of(p[7], p[8]);
    if (bsize == BLOCK_INVALID || plane_bsize == BLOCK_INVALID) return 1;
    if (p[0] > 8)
        svt_aom_combine_interintra_highbd((InterIntraMode)p[1], (uint8_t)p[2], (uint8_t)p[3], (uint8_t)p[4], bsize, plane_bsize, dst, dst_stride, inter,
                                          inter_stride, intra, intra_stride, p[0]);
    else
        svt_aom_combine_interintra((InterIntraMode)p[1], (int8_t)p[2], p[3], p[4], bsize, plane_bsize, dst, dst_stride, inter, inter_stride, intra,
                                   intra_stride);
    return 0;
}

/* p: bit_depth, width, height, kind (0 wedge, 1 diffwtd), pred0_to_pred1_mult; src: the block's first sample, stride in samples; pred0 / pred1:
 * contiguous blocks; out: exit, wedge_index, wedge_sign, mask_type */
int harness_compound_search(const int *p, uint8_t *src, int src_stride, uint8_t *pred0, uint8_t *pred1, int *out) {
    PictureControlSet       *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    ModeDecisionCandidate   *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    EbPictureBufferDesc     *pic  = (EbPictureBufferDesc *)calloc(1, sizeof(*pic));
    EbObjectWrapper         *wrap = (EbObjectWrapper *)calloc(1, sizeof(*wrap));
    EbReferenceObject       *ref  = (EbReferenceObject *)calloc(1, sizeof(*ref));
    int16_t                 *res  = (int16_t *)calloc(2 * 128 * 128, sizeof(int16_t));
    BlockGeom                geo;
    if (!pcs || !ppcs || !ctx || !cand || !pic || !wrap || !ref || !res) return 2;
    memset(&geo, 0, sizeof(geo));
    geo.bwidth = (uint8_t)p[1]; geo.bheight = (uint8_t)p[2]; geo.bsize = bsize_of(p[1], p[2]);
    if (geo.bsize == BLOCK_INVALID) return 3;
    pcs->ppcs = ppcs; pcs->scs = g_scs;
    wrap->object_ptr = ref; /* reference_picture stays NULL: no prediction is made */
    for (int l = 0; l < 2; l++)
        for (int i = 0; i < 4; i++) pcs->ref_pic_ptr_array[l][i] = wrap;
    pic->buffer_y = src; pic->stride_y = (uint16_t)src_stride;
    ppcs->enhanced_pic = pic; pcs->input_frame16bit = pic;
    ctx->hbd_md = p[0] > 8 ? EB_10_BIT_MD : EB_8_BIT_MD;
    ctx->blk_geom = &geo;
    ctx->residual1 = res; ctx->diff10 = res + 128 * 128;
    ctx->inter_comp_ctrls.pred0_to_pred1_mult = (uint8_t)p[4];
    ctx->inter_comp_ctrls.use_rate = 0;
    cand->ref_frame_type = LAST_FRAME;
    cand->mv[0].as_int = 0x00010002; cand->mv[1].as_int = 0x00030004;
    ctx->cmp_store.pred0_cnt = ctx->cmp_store.pred1_cnt = 1;
    ctx->cmp_store.pred0_buf[0] = pred0; ctx->cmp_store.pred1_buf[0] = pred1;
    ctx->cmp_store.pred0_mv[0].as_int = cand->mv[0].as_int; ctx->cmp_store.pred1_mv[0].as_int = cand->mv[1].as_int;
    cand->interinter_comp.type = p[3] ? COMPOUND_DIFFWTD : COMPOUND_WEDGE;
    cand->interinter_comp.wedge_index = 0xFF; cand->interinter_comp.wedge_sign = 0xFF; cand->interinter_comp.mask_type = (DIFFWTD_MASK_TYPE)0xEE;
    out[0] = svt_aom_calc_pred_masked_compound(pcs, ctx, cand);
    if (!out[0]) svt_aom_search_compound_diff_wedge(pcs, ctx, cand);
    out[1] = cand->interinter_comp.wedge_index; out[2] = cand->interinter_comp.wedge_sign; out[3] = (int)cand->interinter_comp.mask_type;
    free(pcs); free(ppcs); free(ctx); free(cand); free(pic); free(wrap); free(ref); free(res);
    return 0;
}
"""

HARNESS_II = r"""
#include "mode_decision.c"
#include <string.h>

static const uint8_t *g_inter; /* the scripted inter block, contiguous */
static int            g_bytes;

EbErrorType svt_aom_inter_prediction(SequenceControlSet *scs, PictureControlSet *pcs, uint32_t interp_filters, BlkStruct *blk_ptr, uint8_t ref_frame_type,
                                     MvUnit *mv_unit, uint8_t use_intrabc, MotionMode motion_mode, uint8_t use_precomputed_obmc, struct ModeDecisionContext *ctx,
                                     uint8_t compound_idx, InterInterCompoundData *interinter_comp, NeighborArrayUnit *recon_neigh_y,
                                     NeighborArrayUnit *recon_neigh_cb, NeighborArrayUnit *recon_neigh_cr, uint8_t is_interintra_used,
                                     InterIntraMode interintra_mode, uint8_t use_wedge_interintra, int32_t interintra_wedge_index, uint16_t pu_origin_x,
                                     uint16_t pu_origin_y, uint8_t bwidth, uint8_t bheight, EbPictureBufferDesc *ref_pic_list0,
                                     EbPictureBufferDesc *ref_pic_list1, EbPictureBufferDesc *prediction_ptr, uint16_t dst_origin_x, uint16_t dst_origin_y,
                                     uint32_t component_mask, uint8_t bit_depth, uint8_t is_16bit_pipeline) {
    (void)scs; (void)pcs; (void)interp_filters; (void)blk_ptr; (void)ref_frame_type; (void)mv_unit; (void)use_intrabc; (void)use_precomputed_obmc; (void)ctx;
    (void)compound_idx; (void)interinter_comp; (void)recon_neigh_y; (void)recon_neigh_cb; (void)recon_neigh_cr; (void)interintra_mode;
    (void)use_wedge_interintra; (void)interintra_wedge_index; (void)pu_origin_x; (void)pu_origin_y; (void)ref_pic_list0; (void)ref_pic_list1; (void)bit_depth;
    (void)is_16bit_pipeline;
    if (motion_mode != SIMPLE_TRANSLATION || is_interintra_used || dst_origin_x || dst_origin_y || component_mask != PICTURE_BUFFER_DESC_LUMA_MASK ||
        prediction_ptr->stride_y != bwidth || g_bytes != bwidth * bheight * (bit_depth > 8 ? 2 : 1))
        abort();
    memcpy(prediction_ptr->buffer_y, g_inter, g_bytes);
    return EB_ErrorNone;
}

/* p: bit_depth, width, height, ii_wedge_mode; src: the block's first sample, stride in samples; inter and the four intra blocks contiguous;
 * out: interintra_mode, use_wedge_interintra, interintra_wedge_index */
int harness_interintra_search(const int *p, uint8_t *src, int src_stride, const uint8_t *inter, uint8_t *intra0, uint8_t *intra1, uint8_t *intra2,
                              uint8_t *intra3, int *out) {
    PictureControlSet       *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    SequenceControlSet      *scs  = (SequenceControlSet *)calloc(1, sizeof(*scs));
    ModeDecisionContext     *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    ModeDecisionCandidate   *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    MdRateEstimationContext *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    EbPictureBufferDesc     *pic  = (EbPictureBufferDesc *)calloc(1, sizeof(*pic));
    EbObjectWrapper         *wrap = (EbObjectWrapper *)calloc(1, sizeof(*wrap));
    EbReferenceObject       *ref  = (EbReferenceObject *)calloc(1, sizeof(*ref));
    uint8_t                 *intra[4] = {intra0, intra1, intra2, intra3};
    BlockGeom                geo;
    if (!pcs || !ppcs || !scs || !ctx || !cand || !rate || !pic || !wrap || !ref) return 2;
    memset(&geo, 0, sizeof(geo));
    geo.bwidth = (uint8_t)p[1]; geo.bheight = (uint8_t)p[2]; geo.bsize = BLOCK_INVALID; geo.shape = PART_N;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == p[1] && block_size_high[b] == p[2]) geo.bsize = (BlockSize)b;
    if (geo.bsize == BLOCK_INVALID) return 3;
    pcs->ppcs = ppcs; pcs->scs = scs;
    wrap->object_ptr = ref; /* reference_picture stays NULL */
    for (int l = 0; l < 2; l++)
        for (int i = 0; i < 4; i++) pcs->ref_pic_ptr_array[l][i] = wrap;
    pic->buffer_y = src; pic->stride_y = (uint16_t)src_stride;
    ppcs->enhanced_pic = pic; pcs->input_frame16bit = pic;
    ctx->hbd_md = p[0] > 8 ? EB_10_BIT_MD : EB_8_BIT_MD;
    ctx->blk_geom = &geo; ctx->md_rate_est_ctx = rate; ctx->intrapred_buf = intra;
    ctx->inter_intra_comp_ctrls.use_rd_model = 0;
    ctx->inter_intra_comp_ctrls.wedge_mode_sq = (uint8_t)p[3]; ctx->inter_intra_comp_ctrls.wedge_mode_nsq = (uint8_t)(p[3] ^ 3); /* PART_N reads _sq */
    cand->ref_frame_type = LAST_FRAME;
    cand->interintra_mode = (InterIntraMode)0xEE; cand->interintra_wedge_index = -1; cand->use_wedge_interintra = 0xEE;
    g_inter = inter; g_bytes = p[1] * p[2] * (p[0] > 8 ? 2 : 1);
    inter_intra_search(pcs, ctx, cand);
    out[0] = (int)cand->interintra_mode; out[1] = cand->use_wedge_interintra; out[2] = cand->interintra_wedge_index;
    free(pcs); free(ppcs); free(scs); free(ctx); free(cand); free(rate); free(pic); free(wrap); free(ref);
    return 0;
}
"""

SOURCES = ["Codec/enc_inter_prediction.c", "Codec/blend_a64_mask.c", "C_DEFAULT/inter_prediction_c.c", "C_DEFAULT/compute_sad_c.c", "Codec/aom_dsp_rtcd.c",
           "Codec/common_dsp_rtcd.c"]


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    # the real svt_aom_inter_prediction gets another name: the second unit's stand-in takes its place
    rename = {"Codec/enc_inter_prediction.c": ["-Dsvt_aom_inter_prediction=svt_aom_inter_prediction_real"]}
    L = refbuild.build(ref, tmp, "maskref", SOURCES, [("harness", HARNESS), ("harness_ii", HARNESS_II)], source_flags=rename, standins=True)
    P = C.c_void_p
    L.harness_tables.argtypes = [P, P, P, P]
    L.harness_masked_predict.argtypes = [P, P, P, C.c_int, P, C.c_int, P]
    L.harness_interintra.argtypes = [P, P, C.c_int, P, C.c_int, P, C.c_int]
    L.harness_compound_search.argtypes = [P, P, C.c_int, P, P, P]
    L.harness_interintra_search.argtypes = [P, P, C.c_int, P, P, P, P, P, P]
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def reference_pred_block(L, b, planes, j, seg_mask):
    bd = b["bit_depth"]
    dt = np.uint16 if bd > 8 else np.uint8
    p = j["pred"]
    w, h = int(p["width"]), int(p["height"])
    widx, wsign, mtype = mc.job_params(j, int(p["flags"]), b["results"])
    mvs = [ip.job_mv(p, k, b["mv_array"]) for k in range(2)]
    a = np.array([w, h, p["org_x"], p["org_y"], p["filter_x"], p["filter_y"], mvs[0][0], mvs[0][1], mvs[1][0], mvs[1][1], p["mb_to_left_edge"],
                  p["mb_to_right_edge"], p["mb_to_top_edge"], p["mb_to_bottom_edge"], b["ss_x"], b["ss_y"], bd, b["plane"], j["luma_width"], j["luma_height"],
                  j["comp_type"], widx, wsign, mtype], np.int32)
    srcs = []
    for k in range(2):
        pl, ox, oy = planes[int(p["ref"][k])]
        assert pl.dtype == dt
        srcs.append(pl.ctypes.data + (oy * pl.shape[1] + ox) * pl.itemsize)
    stride = planes[0][0].shape[1]
    assert all(pl.shape[1] == stride for pl, _, _ in planes)
    out = np.full((h, w), 0xA5A5 if bd > 8 else 0xA5, dt)
    rc = L.harness_masked_predict(a.ctypes.data, srcs[0], srcs[1], stride, out.ctypes.data, w, seg_mask.ctypes.data)
    assert rc == 0
    return out.astype(np.uint16)


def generate_pred(L, out):
    samples = {(name, i): key for key, name, i in mc.pred_sample_jobs()}
    masks_left, mismatch, n_jobs = {}, [], 0
    for name in mc.pred_batch_names():
        b = mc.pred_batch(name)
        planes = mc.pred_planes(b)
        want, defined, want_masks, events = mc.pred_restated(name)
        crcs, mask_crcs, left = [], [], []
        for i, j in enumerate(b["jobs"]):
            if not defined[i] or not events[i]["inside"]:
                raise RuntimeError(f"{name} job {i}: not defined, or the block plus the filter reach leaves the padded plane")
            lw, lh = int(j["luma_width"]), int(j["luma_height"])
            seg = masks_left[b["mask_from"]][i].copy() if b["mask_from"] else np.full(lw * lh, 0xA5, np.uint8)
            before = seg.copy()
            blk = reference_pred_block(L, b, planes, j, seg)
            if not np.array_equal(blk, want[i]):
                mismatch.append((name, i, int(np.count_nonzero(blk != want[i]))))
            if j["comp_type"] == mc.DIFFWTD and b["plane"] == 0:
                o = int(j["mask_offset"])
                if not np.array_equal(seg, want_masks[o:o + lw * lh]):
                    mismatch.append((name, i, "mask"))
                mask_crcs.append(mc.crc8(seg))
            elif not np.array_equal(seg, before):
                raise RuntimeError(f"{name} job {i}: the reference wrote seg_mask")
            left.append(seg)
            crcs.append(ip.crc(blk))
            if (name, i) in samples:
                out[samples[(name, i)]] = blk
        masks_left[name] = left
        out[f"crc_{name}"] = np.array(crcs, np.uint32)
        if mask_crcs:
            out[f"maskcrc_{name}"] = np.array(mask_crcs, np.uint32)
        n_jobs += len(crcs)
    if mismatch:
        raise RuntimeError(f"the prediction restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    return n_jobs


def generate_blend(L, out):
    mismatch, n_jobs = [], 0
    for name in mc.blend_batch_names():
        b = mc.blend_by_name(name)
        want = mc.blend_restated(name)
        isz = b["intra"].itemsize
        crcs = []
        for in_place in (False, True):
            for i, j in enumerate(b["jobs"]):
                w, h = int(j["width"]), int(j["height"])
                a = np.array([b["bit_depth"], j["interintra_mode"], j["use_wedge"], min(int(j["wedge_index"]), 15), min(int(j["wedge_sign"]), 1), j["luma_width"],
                              j["luma_height"], w, h], np.int32)
                inter = b["inter"].copy()
                dst = inter if in_place else np.zeros((h, w), inter.dtype)
                d_ptr, d_stride = (dst.ctypes.data + int(j["dst_offset"]) * isz, dst.shape[1]) if in_place else (dst.ctypes.data, w)
                rc = L.harness_interintra(a.ctypes.data, d_ptr, d_stride, inter.ctypes.data + int(j["inter_offset"]) * isz, inter.shape[1],
                                          b["intra"].ctypes.data + int(j["intra_offset"][int(j["interintra_mode"])]) * isz, b["intra"].shape[1])
                assert rc == 0
                blk = mc.block_of(dst, j["dst_offset"], w, h).astype(np.uint16) if in_place else dst.astype(np.uint16)
                if not np.array_equal(blk, want[i]):
                    mismatch.append((name, i, in_place))
                if not in_place:
                    crcs.append(ip.crc(blk))
        out[f"crc_{name}"] = np.array(crcs, np.uint32)
        n_jobs += len(crcs)
    if mismatch:
        raise RuntimeError(f"the blend restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    return n_jobs


def reference_search(L, sb):
    """[n][4] int32 per job: kinds 0 / 1: exit, wedge_index, wedge_sign, mask_type; kind 2: interintra_mode, use_wedge_interintra, wedge_index, 0"""
    bd = sb.bit_depth
    dt = np.uint16 if bd > 8 else np.uint8
    ref = np.zeros((len(sb.jobs), 4), np.int32)
    src = sb.planes["src"]
    for i, j in enumerate(sb.jobs):
        w, h, kind = int(j["width"]), int(j["height"]), int(j["kind"])
        blk = lambda name, o: np.ascontiguousarray(mc.block_of(sb.planes[name], o, w, h).astype(dt))
        o = np.zeros(4, np.int32)
        s_ptr = src.ctypes.data + int(j["src_offset"]) * src.itemsize
        p1 = blk("pred1", j["pred1_offset"])
        if kind <= 1:
            p0 = blk("pred0", j["pred0_offset"])
            a = np.array([bd, w, h, kind, sb.mult], np.int32)
            rc = L.harness_compound_search(a.ctypes.data, s_ptr, src.shape[1], p0.ctypes.data, p1.ctypes.data, o.ctypes.data)
        else:
            intra = [blk("intra", x) for x in j["intra_offset"]]
            a = np.array([bd, w, h, j["ii_wedge_mode"]], np.int32)
            rc = L.harness_interintra_search(a.ctypes.data, s_ptr, src.shape[1], p1.ctypes.data, *(x.ctypes.data for x in intra), o.ctypes.data)
        if rc:
            raise RuntimeError(f"{sb.name} job {i}: the harness returned {rc}")
        ref[i] = o
    return ref


def generate_search(L, out):
    bad, n_jobs = [], 0
    refs = {}
    for name, sb in mc.search_batches().items():
        ref = reference_search(L, sb)
        want = mc.reference_outputs(sb, mc.search_restated(name)[0])
        bad += [(name, i, ref[i].tolist(), want[i].tolist()) for i in range(len(ref)) if not np.array_equal(ref[i], want[i])]
        out[f"search_{name}"] = refs[name] = ref
        n_jobs += len(ref)
    if bad:
        raise RuntimeError(f"the search restatement differs from the reference on {len(bad)} jobs, first: {bad[:6]}")
    # the conditions of the planted inputs, on the reference's results
    missing = []
    for r in ("full8", "mid10", "mid8"):
        planted = mc.planted_wedge_batch(r)[1]
        won = sum(tuple(int(v) for v in a[1:3]) == p for a, p in zip(refs[f"planted_wedge_{r}"], planted))
        if won != len(planted) or len(planted) != 288:
            missing.append(f"planted_wedge_{r}: {won} of {len(planted)} planted wedges win")
    ev = {r: mc.search_restated(f"planted_wedge_{r}")[1] for r in mc.RANGES}  # the restatement equals the reference on these jobs (above)
    if not all(e["clamp"] for e in ev["full10"]):
        missing.append("planted_wedge_full10: the int16 clamp does not fire in every job")
    if any(e["clamp"] for e in ev["mid10"]) or any(e["ds_saturated"] for e in ev["mid8"]):
        missing.append("the clamp fires on [384, 640) planes, or the delta squares saturate on [96, 160) planes")
    if sum(e["ds_saturated"] for e in ev["full8"]) < 280:
        missing.append("the delta squares saturate in fewer than 280 of the full-range 8-bit jobs")
    for bd in (8, 10):
        planted = mc.planted_seg_batch(bd)[1]
        if [int(a[3]) for a in refs[f"planted_seg_{bd}"][:len(planted)]] != planted:
            missing.append(f"planted_seg_{bd}: a planted mask type loses")
        info = mc.ii_batch(bd)[1]
        for a, (what, v, wm) in zip(refs[f"ii_{bd}"], info):
            ok = (what != "mode" or (a[0] == v and a[1] == (wm == 1 or (wm == 2 and a[1])))) and (what != "wedge" or (a[1] == 1 and a[2] == v)) and \
                (what != "equal" or a[1] == 0)
            if not ok:
                missing.append(f"ii_{bd}: {what} {v} wedge mode {wm}: {a.tolist()}")
        t = refs[f"ties_{bd}"]
        if not all(tuple(t[3 * k][1:3]) == (0, 0) and t[3 * k + 1][3] == 0 and t[3 * k + 2][0] == 0 for k in range(3)):
            missing.append(f"ties_{bd}: {t.tolist()}")
        for mult in (0, 1, 4):
            if [bool(a[0]) for a in refs[f"gate_{bd}_{mult}"]] != mc.gate_batch(bd, mult)[1]:
                missing.append(f"gate_{bd}_{mult}")
    if missing:
        raise RuntimeError(f"conditions the reference's results do not meet: {missing[:10]}")
    return n_jobs


def generate(L):
    out = {}
    prim, flip, contig = np.zeros((2, 6, 64, 64), np.uint8), np.zeros((9, 16), np.uint8), np.zeros(len(mc.contiguous_masks()), np.uint8)
    rc = L.harness_tables(prim.ctypes.data, flip.ctypes.data, contig.ctypes.data, np.array(mc.WEDGE_SIZES, np.int32).ctypes.data)
    if rc:
        raise RuntimeError(f"harness_tables: {rc}: the sizes with wedges are not the nine")
    if not (np.array_equal(prim, mc.primaries()) and np.array_equal(flip, mc.signflip()) and np.array_equal(contig, mc.contiguous_masks())):
        raise RuntimeError("the primaries, the sign-flip table or the contiguous masks differ from the reference's")
    out["primaries_crc"], out["signflip_crc"], out["contiguous_crc"] = (np.array([mc.crc8(a)], np.uint32) for a in (prim, flip, contig))
    n = (generate_pred(L, out), generate_blend(L, out), generate_search(L, out))
    print(f"{n[0]} prediction jobs, {n[1]} blend jobs (each in place and out of place) and {n[2]} search jobs, the restatement equal to the reference on all of them")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {mc.GOLDEN: generate})
