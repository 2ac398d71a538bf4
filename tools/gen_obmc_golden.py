#!/usr/bin/env python3
"""Writes tests/golden/obmc.npz: the reference encoder's own OBMC results on the cases of tests/obmc_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or bench.py.
It compiles a harness of its own into a temporary directory outside the tree (gcc, -O2).  The harness #includes Codec/enc_inter_prediction.c where
it lies, because build_prediction_by_above_preds / _left_preds, av1_build_obmc_inter_prediction and calc_target_weighted_pred are static, and links
Codec/inter_prediction.c, Codec/blend_a64_mask.c, C_DEFAULT/inter_prediction_c.c, C_DEFAULT/blend_a64_mask_c.c, C_DEFAULT/pack_unpack_c.c and the two
rtcd files where they lie, with the _c kernels installed in the rtcd pointers.  Whatever else the link still wants gets a stand-in that aborts.

Per block the harness scripts a mode-info grid of the picture (47 x 31 mode-info units and a margin of one): every entry is an intra 8x8 block but
the first entry of each span of the record, which is an inter block of the span's size (twice the block's size for some spans over a whole side: a
neighbour wider than the block) with the span's mv[0], ref_frame[0] (LAST_FRAME / LAST2_FRAME for reference 0 / 1) and interp_filters.  All three
statics run their own foreach_overlappable_nb_above / _left on that grid: no loop of theirs is restated.  The reference pictures are
EbPictureBufferDesc's whose buffers point at the picture's sample (0, 0) of the padded planes (org_x = org_y = 0, no 2-bit planes: the packed 16-bit
path at 10 bits).  The harness then runs, in the reference's order: the above strips, the left strips (all three planes each), at 10 bits
svt_enc_msb_un_pack2_d on the two luma strips (what svt_aom_un_pack2d, Codec/pic_operators.c:294-303, calls for these sizes; that file is not linked),
calc_target_weighted_pred, and av1_build_obmc_inter_prediction on copies of the three prediction blocks.  xd->up_available / left_available are
n_above > 0 / n_left > 0: build_prediction_by_above_preds resets mb_to_left_edge to the block's natural value when it runs, which a record with an
edge of its own (the plane-edge batches) must not see.

A second unit #includes Codec/mode_decision.c where it lies and drives single_motion_search (OBMC_CAUSAL) at all five refine levels on the cases of
tests/obmc_search_cases.py, with Codec/av1me.c, Codec/rd_cost.c, Codec/convolve.c, C_DEFAULT/sad_av1.c and C_DEFAULT/variance.c linked where they lie
and svt_aom_mefn_ptr's osdf / ovf, svt_aom_upsampled_pred and svt_aom_convolve8_horiz / _vert set to the _c functions.  x->sadperbit16 is what the
case asks for: the unit writes it into sad_per_bit_lut_8[0], which svt_aom_get_sad_per_bit(base_q_idx = 0) returns, and full_lambda_md is
error_per_bit << RD_EPB_SHIFT; the harness checks that the function used both.  It then calls svt_av1_obmc_full_pixel_search and
svt_av1_find_best_obmc_sub_pixel_tree_up as single_motion_search calls them, for their return values, *distortion and *sse1, and checks that both
paths end at the same MV.  No loop of theirs is restated.  The conditions of the planted inputs are asserted on the restatement's events after the
restatement was found equal to the reference on every output of every job.

The fixture holds numbers only: every output of every search job; the CRC-32 of the reference's mask rows in the library's packing; per batch a CRC-32 per block and plane of the two
strip areas and of the blended block and a CRC-32 per block of wsrc and of mask; per size and depth the whole luma results of one block.  --check
recomputes everything and compares it with the committed file instead of writing it; either way the restatement of tests/obmc_cases.py is compared
with the reference on every block and plane a batch runs, every prediction's reads are checked to lie inside its padded plane, and the conditions
of the case list are asserted."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import inter_pred_cases as ip  # noqa: E402
import obmc_cases as oc  # noqa: E402
import obmc_search_cases as sc  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include "enc_inter_prediction.c"
#include <stdlib.h>
#include <string.h>
#include "sequence_control_set.h"
#include "pcs.h"
#include "md_process.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "pack_unpack_c.h"

#define PIC_W 192
#define PIC_H 128
#define GRID_STRIDE (PIC_W / 4 + 1)
#define GRID_ROWS (PIC_H / 4 + 1)

static SequenceControlSet *g_scs;

static BlockSize bsize_of(int w, int h) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h) return (BlockSize)b;
    return BLOCK_INVALID;
}

static void plain_memcpy(void *dst, void const *src, size_t size) { memcpy(dst, src, size); }

int harness_init(void) {
    svt_memcpy = plain_memcpy;
    svt_aom_convolve[0][0][0] = svt_av1_convolve_2d_copy_sr_c; svt_aom_convolve[1][0][0] = svt_av1_convolve_x_sr_c;
    svt_aom_convolve[0][1][0] = svt_av1_convolve_y_sr_c; svt_aom_convolve[1][1][0] = svt_av1_convolve_2d_sr_c;
    svt_aom_convolveHbd[0][0][0] = svt_av1_highbd_convolve_2d_copy_sr_c; svt_aom_convolveHbd[1][0][0] = svt_av1_highbd_convolve_x_sr_c;
    svt_aom_convolveHbd[0][1][0] = svt_av1_highbd_convolve_y_sr_c; svt_aom_convolveHbd[1][1][0] = svt_av1_highbd_convolve_2d_sr_c;
    svt_aom_blend_a64_vmask = svt_aom_blend_a64_vmask_c; svt_aom_blend_a64_hmask = svt_aom_blend_a64_hmask_c;
    svt_aom_highbd_blend_a64_vmask_16bit = svt_aom_highbd_blend_a64_vmask_16bit_c;
    svt_aom_highbd_blend_a64_hmask_16bit = svt_aom_highbd_blend_a64_hmask_16bit_c;
    svt_av1_calc_target_weighted_pred_above = svt_av1_calc_target_weighted_pred_above_c;
    svt_av1_calc_target_weighted_pred_left = svt_av1_calc_target_weighted_pred_left_c;
    if (!g_scs) g_scs = calloc(1, sizeof(*g_scs));
    return g_scs ? 0 : 1;
}

/* rows: 64 bytes, the row of length n at [n, 2n) */
void harness_masks(uint8_t *rows) {
    memset(rows, 0, 64);
    for (int n = 1; n <= 32; n *= 2) memcpy(rows + n, svt_av1_get_obmc_mask(n), n);
}

/* p: bit_depth, width, height, org_x, org_y, the four edges (left, right, top, bottom), n_above, n_left, then 4 + 4 spans of 8: rel, size, ref,
 *    filter_x, filter_y, mv row, mv col, the neighbour's own size in 4-sample units.
 * refs: [2][3] the picture's sample (0, 0) of every plane of the two references, ref_stride[3] in samples; above / left: 3 * w * h samples each,
 * pre-filled; pred[3] / pred_stride[3]: the block's own prediction per plane, blended in place; src: the block's first source sample. */
int harness_obmc_block(const int *p, uint8_t **refs, const int *ref_stride, uint8_t *above, uint8_t *left, uint8_t **pred, const int *pred_stride,
                       uint8_t *src, int src_stride, int32_t *wsrc, int32_t *mask) {
    const int bd = p[0], is16 = bd > 8, w = p[1], h = p[2], mi_col = p[3] >> 2, mi_row = p[4] >> 2, n[2] = {p[9], p[10]};
    const BlockSize bsize = bsize_of(w, h);
    PictureControlSet       *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    Av1Common               *cm   = (Av1Common *)calloc(1, sizeof(*cm));
    EbPictureBufferDesc     *pic  = (EbPictureBufferDesc *)calloc(3, sizeof(*pic));
    EbObjectWrapper         *wrap = (EbObjectWrapper *)calloc(2, sizeof(*wrap));
    EbReferenceObject       *ref  = (EbReferenceObject *)calloc(2, sizeof(*ref));
    ModeInfo                *mis  = (ModeInfo *)calloc(9, sizeof(*mis)); /* [0] the intra filler, then the spans */
    ModeInfo               **grid = (ModeInfo **)calloc(GRID_STRIDE * GRID_ROWS, sizeof(*grid));
    MacroBlockD              xd;
    BlockGeom                geo;
    if (!pcs || !ppcs || !ctx || !cm || !pic || !wrap || !ref || !mis || !grid) return 2;
    if (bsize == BLOCK_INVALID) return 3;
    memset(&xd, 0, sizeof(xd));
    memset(&geo, 0, sizeof(geo));
    cm->mi_cols = PIC_W / 4; cm->mi_rows = PIC_H / 4; cm->subsampling_x = 1; cm->subsampling_y = 1;
    pcs->ppcs = ppcs; pcs->scs = g_scs; ppcs->av1_cm = cm;
    for (int r = 0; r < 2; r++) {
        EbPictureBufferDesc *d = &pic[r];
        d->buffer_y = refs[3 * r]; d->buffer_cb = refs[3 * r + 1]; d->buffer_cr = refs[3 * r + 2];
        d->stride_y = (uint16_t)ref_stride[0]; d->stride_cb = (uint16_t)ref_stride[1]; d->stride_cr = (uint16_t)ref_stride[2];
        d->width = PIC_W; d->height = PIC_H; d->bit_depth = (EbBitDepth)bd;
        ref[r].reference_picture = d;
        wrap[r].object_ptr = &ref[r];
        pcs->ref_pic_ptr_array[0][r] = &wrap[r];
    }
    pic[2].buffer_y = src; pic[2].stride_y = (uint16_t)src_stride; pic[2].width = PIC_W; pic[2].height = PIC_H; /* the source, from the block on */
    ppcs->enhanced_pic = &pic[2];
    mis[0].mbmi.block_mi.ref_frame[0] = INTRA_FRAME; mis[0].mbmi.block_mi.bsize = BLOCK_8X8;
    for (int i = 0; i < GRID_STRIDE * GRID_ROWS; i++) grid[i] = &mis[0];
    for (int dir = 0; dir < 2; dir++)
        for (int k = 0; k < n[dir]; k++) {
            const int *s = p + 11 + 32 * dir + 8 * k;
            ModeInfo  *m = &mis[1 + 4 * dir + k];
            m->mbmi.block_mi.bsize = bsize_of(s[7] * 4, s[7] * 4);
            if (m->mbmi.block_mi.bsize == BLOCK_INVALID) return 4;
            m->mbmi.block_mi.ref_frame[0] = (MvReferenceFrame)(LAST_FRAME + s[2]); m->mbmi.block_mi.ref_frame[1] = NONE_FRAME;
            m->mbmi.block_mi.mv[0].as_mv.row = (int16_t)s[5]; m->mbmi.block_mi.mv[0].as_mv.col = (int16_t)s[6];
            m->mbmi.block_mi.interp_filters = av1_make_interp_filters((InterpFilter)s[4], (InterpFilter)s[3]);
            if (dir == 0) grid[mi_row * GRID_STRIDE + 1 + mi_col + s[0]] = m; /* the row above the block, one column of margin */
            else grid[(mi_row + 1 + s[0]) * GRID_STRIDE + mi_col] = m;
        }
    xd.mi = grid + (mi_row + 1) * GRID_STRIDE + mi_col + 1; xd.mi_stride = GRID_STRIDE;
    xd.n4_w = (uint8_t)(w >> 2); xd.n4_h = (uint8_t)(h >> 2); xd.bsize = bsize;
    xd.up_available = n[0] > 0; xd.left_available = n[1] > 0;
    xd.mb_to_left_edge = p[5]; xd.mb_to_right_edge = p[6]; xd.mb_to_top_edge = p[7]; xd.mb_to_bottom_edge = p[8];

    const int sz = is16 ? 2 : 1;
    uint8_t  *buf1[3] = {above, above + w * h * sz, above + 2 * w * h * sz}, *buf2[3] = {left, left + w * h * sz, left + 2 * w * h * sz};
    int       stride[3] = {w, w, w};
    build_prediction_by_above_preds(1, bsize, pcs, &xd, mi_row, mi_col, buf1, stride, (uint8_t)is16);
    build_prediction_by_left_preds(1, bsize, pcs, &xd, mi_row, mi_col, buf2, stride, (uint8_t)is16);
    if (xd.mb_to_right_edge != p[6] || xd.mb_to_bottom_edge != p[8]) return 5;

    uint8_t *a8 = above, *l8 = left, *un = NULL;
    if (is16) { /* svt_aom_precompute_obmc_data's un_pack of the luma strips */
        un = (uint8_t *)malloc(2 * w * h);
        if (!un) return 2;
        a8 = un; l8 = un + w * h;
        svt_enc_msb_un_pack2_d((uint16_t *)above, w, a8, NULL, w, w, w, h);
        svt_enc_msb_un_pack2_d((uint16_t *)left, w, l8, NULL, w, w, w, h);
    }
    geo.bsize = bsize; geo.bwidth = (uint8_t)w; geo.bheight = (uint8_t)h;
    ctx->blk_geom = &geo; ctx->obmc_ctrls.max_blk_size_to_refine = 64; ctx->wsrc_buf = wsrc; ctx->mask_buf = mask;
    ctx->blk_org_x = 0; ctx->blk_org_y = 0; /* enhanced_pic starts at the block */
    calc_target_weighted_pred(pcs, ctx, cm, &xd, mi_row, mi_col, a8, w, l8, w);

    av1_build_obmc_inter_prediction(pred[0], (uint16_t)pred_stride[0], pred[1], (uint16_t)pred_stride[1], pred[2], (uint16_t)pred_stride[2],
                                    PICTURE_BUFFER_DESC_LUMA_MASK | PICTURE_BUFFER_DESC_CHROMA_MASK, bsize, pcs, &xd, mi_row, mi_col, buf1, stride, buf2, stride,
                                    (uint8_t)is16);
    free(un); free(pcs); free(ppcs); free(ctx); free(cm); free(pic); free(wrap); free(ref); free(mis); free(grid);
    return 0;
}
"""

HARNESS_SEARCH = r"""
#include "mode_decision.c"
#include <stdlib.h>
#include <string.h>

static BlockSize bsize_of2(int w, int h) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h) return (BlockSize)b;
    return BLOCK_INVALID;
}

#define OBFN(W, H) svt_aom_mefn_ptr[BLOCK_##W##X##H].osdf = svt_aom_obmc_sad##W##x##H##_c; svt_aom_mefn_ptr[BLOCK_##W##X##H].ovf = svt_aom_obmc_variance##W##x##H##_c;
int harness_search_init(void) {
    OBFN(8, 8) OBFN(16, 8) OBFN(32, 32) OBFN(64, 64) OBFN(16, 16)
    svt_aom_upsampled_pred = svt_aom_upsampled_pred_c;
    svt_aom_convolve8_horiz = svt_aom_convolve8_horiz_c; svt_aom_convolve8_vert = svt_aom_convolve8_vert_c;
    return 0;
}

/* p: width, height, org_x, org_y, start row, start col, ref row, ref col, refine_level, fpel_search_diag, fpel_search_range, approx_inter_rate, allow_hp,
 *    sadpb, error_per_bit.  ref: the co-located block's first sample.  out: single_motion_search's best row, col and rate_mv; then, from the two
 * av1me.c functions called as single_motion_search calls them: the full-pel return value, besterr, distortion, sse1, best row, col. */
int harness_obmc_search(const int *p, uint8_t *ref, int ref_stride, int32_t *wsrc, int32_t *mask, int *mvjcost, int *mvrow, int *mvcol, int *out) {
    PictureControlSet       *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    ModeDecisionCandidate   *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    MdRateEstimationContext *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    Av1Common               *cm   = (Av1Common *)calloc(1, sizeof(*cm));
    BlkStruct               *blk  = (BlkStruct *)calloc(1, sizeof(*blk));
    IntraBcContext          *x    = (IntraBcContext *)calloc(1, sizeof(*x));
    MacroBlockD              xd;
    BlockGeom                geo;
    const BlockSize          bsize = bsize_of2(p[0], p[1]);
    if (!pcs || !ppcs || !ctx || !cand || !rate || !cm || !blk || !x) return 2;
    if (bsize == BLOCK_INVALID) return 3;
    memset(&xd, 0, sizeof(xd));
    memset(&geo, 0, sizeof(geo));
    cm->mi_cols = 192 / 4; cm->mi_rows = 128 / 4;
    pcs->ppcs = ppcs; ppcs->av1_cm = cm;
    ppcs->frm_hdr.quantization_params.base_q_idx = 0; ppcs->frm_hdr.allow_high_precision_mv = (uint8_t)p[12];
    sad_per_bit_lut_8[0] = p[13]; /* what svt_aom_get_sad_per_bit(0, 0) returns: x->sadperbit16 */
    ctx->full_lambda_md[EB_8_BIT_MD] = (uint32_t)p[14] << RD_EPB_SHIFT; /* x->errorperbit */
    xd.mb_to_left_edge = -p[2] * 8; xd.mb_to_top_edge = -p[3] * 8;
    blk->av1xd = &xd; ctx->blk_ptr = blk;
    memcpy(rate->nmv_vec_cost, mvjcost, sizeof(rate->nmv_vec_cost));
    rate->nmvcoststack[0] = mvrow; rate->nmvcoststack[1] = mvcol;
    ctx->md_rate_est_ctx = rate;
    geo.bsize = bsize; geo.bwidth = (uint8_t)p[0]; geo.bheight = (uint8_t)p[1];
    ctx->blk_geom = &geo;
    ctx->obmc_ctrls.fpel_search_range = (uint8_t)p[10]; ctx->obmc_ctrls.fpel_search_diag = (uint8_t)p[9];
    ctx->approx_inter_rate = (uint8_t)p[11];
    ctx->wsrc_buf = wsrc; ctx->mask_buf = mask;
    cand->motion_mode = OBMC_CAUSAL;
    x->xdplane[0].pre[0].buf = ref; x->xdplane[0].pre[0].stride = ref_stride;
    IntMv start; MV ref_mv; int rate_mv = 0;
    start.as_mv.row = (int16_t)p[4]; start.as_mv.col = (int16_t)p[5]; ref_mv.row = (int16_t)p[6]; ref_mv.col = (int16_t)p[7];
    single_motion_search(pcs, ctx, cand, start, x, bsize, &ref_mv, &rate_mv, p[8]);
    out[0] = x->best_mv.as_mv.row; out[1] = x->best_mv.as_mv.col; out[2] = rate_mv;
    /* the same two calls once more, for what they return */
    const MvLimits lim = x->mv_limits;
    MV best;
    out[3] = 0;
    if (p[8] == 0 || p[8] == 1 || p[8] == 3) {
        MV mvp_full = {(int16_t)(start.as_mv.row >> 3), (int16_t)(start.as_mv.col >> 3)};
        svt_av1_set_mv_search_range(&x->mv_limits, &ref_mv);
        out[3] = svt_av1_obmc_full_pixel_search(ctx, x, &mvp_full, x->sadperbit16, &svt_aom_mefn_ptr[bsize], &ref_mv, &best, 0);
        x->mv_limits = lim;
    } else {
        best.row = (int16_t)(start.as_mv.row >> 3); best.col = (int16_t)(start.as_mv.col >> 3);
    }
    int dis = 0; unsigned int sse1 = 0;
    out[4] = svt_av1_find_best_obmc_sub_pixel_tree_up(ctx, x, cm, p[3] >> 2, p[2] >> 2, &best, &ref_mv, p[12], x->errorperbit, &svt_aom_mefn_ptr[bsize], 0, 2,
                                                      x->nmv_vec_cost, x->mv_cost_stack, &dis, &sse1, 0, USE_8_TAPS);
    out[5] = dis; out[6] = (int)sse1; out[7] = best.row; out[8] = best.col;
    out[9] = x->sadperbit16; out[10] = x->errorperbit;
    free(pcs); free(ppcs); free(ctx); free(cand); free(rate); free(cm); free(blk); free(x);
    return 0;
}
"""

SOURCES = ["Codec/inter_prediction.c", "Codec/blend_a64_mask.c", "C_DEFAULT/inter_prediction_c.c", "C_DEFAULT/blend_a64_mask_c.c", "C_DEFAULT/pack_unpack_c.c",
           "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c", "Codec/av1me.c", "C_DEFAULT/sad_av1.c", "C_DEFAULT/variance.c", "Codec/convolve.c", "Codec/rd_cost.c"]
MARGIN = 16  # samples around every padded plane handed to the reference: the plane-edge batches run all three planes there, only some of them on purpose


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    L = refbuild.build(ref, tmp, "obmcref", SOURCES, [("harness", HARNESS), ("harness_search", HARNESS_SEARCH)], standins=True)
    P = C.c_void_p
    L.harness_masks.argtypes = [P]
    L.harness_obmc_block.argtypes = [P, P, P, P, P, P, P, P, C.c_int, P, P]
    L.harness_obmc_search.argtypes = [P, P, C.c_int, P, P, P, P, P, P]
    if L.harness_init() or L.harness_search_init():
        raise RuntimeError("harness_init failed")
    return L


def reference_batch(L, name):
    """the reference's results of a batch, laid out as obmc_cases.restated()'s"""
    b = oc.batch(name)
    bd = b["bit_depth"]
    dt = np.uint16 if bd > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    padded, ptrs, strides = [], (C.c_void_p * 6)(), (C.c_int * 3)()
    for plane in range(3):
        for r, (pl, ox, oy) in enumerate(oc.ref_planes(b, plane)):
            assert pl.dtype == dt and r < 2
            big = np.pad(pl, MARGIN, mode="edge")
            padded.append(big)
            ptrs[3 * r + plane] = big.ctypes.data + ((oy + MARGIN) * big.shape[1] + ox + MARGIN) * isz
            strides[plane] = big.shape[1]
    if len(b["planes"]) == 1:
        for plane in range(3):
            ptrs[3 + plane] = ptrs[plane]
    res = {"above": oc.fill_array(b["strip_samples"], dt), "left": oc.fill_array(b["strip_samples"], dt),
           "blend": {p: oc.pred_plane(name, p).copy() for p in range(3)}}
    off, n_out = oc.target_offsets(b)
    res["wsrc"], res["mask"] = oc.fill_i32(n_out), oc.fill_i32(n_out)
    src = oc.src_plane(b["src"])
    for i, blk in enumerate(b["blocks"]):
        W, H, x, y, so = int(blk["width"]), int(blk["height"]), int(blk["org_x"]), int(blk["org_y"]), int(blk["strip_offset"])
        p = [bd, W, H, x, y, blk["mb_to_left_edge"], blk["mb_to_right_edge"], blk["mb_to_top_edge"], blk["mb_to_bottom_edge"], blk["n_above"], blk["n_left"]]
        for d, (nbs, n4) in enumerate(((blk["above"], W >> 2), (blk["left"], H >> 2))):
            for k in range(4):
                r = nbs[k]
                mv = b["mv_array"][int(r["mv_index"])] if r["flags"] & oc.MV_FROM_ARRAY else r["mv"]
                size = int(r["size"])
                own = size * 2 if size == n4 and size * 4 < 64 and (i + d) & 1 else size  # a neighbour wider (higher) than the block
                p += [r["rel_pos"], size, r["ref"], r["filter_x"], r["filter_y"], mv[0], mv[1], own]
        a = np.array([int(v) for v in p], np.int32)
        above, left = (np.ascontiguousarray(res[k][so:so + 3 * W * H]) for k in ("above", "left"))
        preds = [np.ascontiguousarray(oc.block_of(res["blend"][pl], oc.pred_layout(name, pl)[0][i], W >> oc.SS[pl], H >> oc.SS[pl])) for pl in range(3)]
        pp, ps = (C.c_void_p * 3)(*[q.ctypes.data for q in preds]), (C.c_int * 3)(*[q.shape[1] for q in preds])
        wsrc, mask = np.zeros(W * H, np.int32), np.zeros(W * H, np.int32)
        rc = L.harness_obmc_block(a.ctypes.data, ptrs, strides, above.ctypes.data, left.ctypes.data, pp, ps, src.ctypes.data + y * src.shape[1] + x, src.shape[1],
                                  wsrc.ctypes.data, mask.ctypes.data)
        if rc:
            raise RuntimeError(f"{name} block {i}: the harness returned {rc}")
        res["above"][so:so + 3 * W * H], res["left"][so:so + 3 * W * H] = above, left
        for pl in range(3):
            oc.block_of(res["blend"][pl], oc.pred_layout(name, pl)[0][i], W >> oc.SS[pl], H >> oc.SS[pl])[:] = preds[pl]
        res["wsrc"][int(off[i]):int(off[i]) + W * H], res["mask"][int(off[i]):int(off[i]) + W * H] = wsrc, mask
    return res


def reference_search(L, name):
    """(best_mv [n][2] int16, results) of a search batch from single_motion_search, checked against the two av1me.c functions called directly"""
    b = sc.batches()[name]
    ref, p = sc.ref_plane(b["ref"]), b["params"]
    tables = [np.ascontiguousarray(t, dtype=np.int32) for t in sc.cost_tables()]
    mvs, res = np.zeros((len(b["jobs"]), 2), np.int16), np.zeros(len(b["jobs"]), sc.RESULT_DTYPE)
    for i, j in enumerate(b["jobs"]):
        w, h = int(j["width"]), int(j["height"])
        y0, x0 = divmod(int(j["ref_offset"]), ref.shape[1])
        org = (x0 - sc.PAD, y0 - sc.PAD)
        if tuple(int(j[k]) for k in ("col_min", "col_max", "row_min", "row_max")) != sc.mv_limits(org, w, h):
            raise RuntimeError(f"{name} job {i}: the job's limits are not single_motion_search's")
        a = np.array([w, h, org[0], org[1], j["start_mv"][0], j["start_mv"][1], j["ref_mv"][0], j["ref_mv"][1], p["refine_level"], p["fpel_search_diag"],
                      p["fpel_search_range"], p["approx_inter_rate"], p["allow_hp"], p["sadpb"], p["error_per_bit"]], np.int32)
        o = int(j["target_offset"])
        wsrc, mask = np.ascontiguousarray(b["wsrc"][o:o + w * h]), np.ascontiguousarray(b["mask"][o:o + w * h])
        out = np.zeros(11, np.int32)
        rc = L.harness_obmc_search(a.ctypes.data, ref.ctypes.data + int(j["ref_offset"]), ref.shape[1], wsrc.ctypes.data, mask.ctypes.data, tables[0].ctypes.data,
                                   tables[1].ctypes.data + 4 * sc.MV_CENTRE, tables[2].ctypes.data + 4 * sc.MV_CENTRE, out.ctypes.data)
        if rc:
            raise RuntimeError(f"{name} job {i}: the harness returned {rc}")
        if (out[0], out[1]) != (out[7], out[8]) or (out[9], out[10]) != (p["sadpb"], p["error_per_bit"]):
            raise RuntimeError(f"{name} job {i}: single_motion_search and the direct calls disagree: {out.tolist()}")
        mvs[i] = out[0], out[1]
        res[i]["rate_mv"], res[i]["fullpel_value"], res[i]["besterr"], res[i]["distortion"], res[i]["sse1"] = out[2], out[3], np.uint32(out[4]), out[5], np.uint32(out[6])
    return mvs, res


def generate_search(L, out):
    bad, n = [], 0
    for name in sc.batches():
        mvs, res = reference_search(L, name)
        want_mv, want, events = sc.restated(name)
        shape = sc.ref_plane(sc.batches()[name]["ref"]).shape
        for i, e in enumerate(events):  # what a job read (restate_job tracks every candidate's floor and taps) lies inside its padded plane
            if not (e["reads"][0] >= 0 and e["reads"][1] >= 0 and e["reads"][2] < shape[0] and e["reads"][3] < shape[1]):
                raise RuntimeError(f"{name} job {i}: a search read leaves the padded plane: {e['reads']}")
        bad += [(name, i, mvs[i].tolist(), want_mv[i].tolist(), res[i].tolist(), want[i].tolist()) for i in range(len(res))
                if not np.array_equal(mvs[i], want_mv[i]) or res[i].tobytes() != want[i].tobytes()]
        out[f"searchmv_{name}"] = mvs
        out[f"search_{name}"] = np.array([[r[k] for k in ("fullpel_value", "besterr", "distortion", "sse1", "rate_mv")] for r in res], np.int64)
        n += len(res)
    if bad:
        raise RuntimeError(f"the search restatement differs from the reference on {len(bad)} jobs, first: {bad[:4]}")
    missing = sc.planted_missing()  # on the restatement, which equals the reference on every output of every job (above)
    if missing:
        raise RuntimeError(f"conditions of the planted search inputs that are not met: {missing}")
    print(f"{n} search jobs in {len(sc.batches())} batches: every output of the restatement equal to the reference's")


def generate(L):
    out = {}
    generate_search(L, out)
    rows = np.zeros(64, np.uint8)
    L.harness_masks(rows.ctypes.data)
    if not np.array_equal(rows, oc.MASKS):
        raise RuntimeError("the mask rows differ from the reference's")
    out["masks_crc"] = np.array([oc.crc(rows, "u1")], np.uint32)
    samples = {(name, i): key for key, name, i in oc.sample_blocks()}
    mismatch, n_blocks = [], 0
    for name in oc.batch_names():
        b = oc.batch(name)
        ref, want = reference_batch(L, name), oc.restated(name)
        for (plane, i), evs in want["events"].items():
            if not all(e["inside"] for _, e in evs):
                raise RuntimeError(f"{name} block {i} plane {plane}: a prediction's reads leave the padded plane")
        got, mine = oc.fixture_arrays(name, ref), oc.fixture_arrays(name, want)
        for k in got:
            if not np.array_equal(got[k], mine[k]):
                mismatch.append((k, np.argwhere(got[k] != mine[k])[:4].tolist()))
        out.update(got)
        for i in range(len(b["blocks"])):
            if (name, i) in samples:
                out[samples[(name, i)]] = oc.sample_arrays(name, i, ref)
        n_blocks += len(b["blocks"])
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference in {len(mismatch)} arrays, first: {mismatch[:8]}")
    missing = oc.coverage_missing()
    if missing:
        raise RuntimeError(f"conditions of the case list that are not met: {missing[:10]}")
    print(f"{n_blocks} blocks in {len(oc.batch_names())} batches: strips, blends, wsrc and mask of the restatement equal to the reference on all of them")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {oc.GOLDEN: generate})
