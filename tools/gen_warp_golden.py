#!/usr/bin/env python3
"""Writes tests/golden/warp.npz and tests/golden/warp_edges.npz: the reference encoder's own warped-motion results on the cases of tests/warp_cases.py
and of tests/warp_edge_cases.py (the same harness; per refinement the best MV, tot_checked_pos and the warp count, a CRC-32 per fit and per
predicted block).

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree) and a built libsvthip.so (the restatement takes
the filter table from it; no GPU is needed); never by the tests, build(), smoke() or bench.py.  It compiles a harness of its own into a temporary
directory outside the tree (gcc, -O2).  The harness #includes the reference's Codec/warped_motion.c where it lies, because the divisor table is
static, defines the run-time dispatch pointers itself (RTCD_C) and installs the _c kernels in them, and calls
  svt_av1_warp_plane            once per reference of a job, with the ConvolveParams plane_warped_motion_prediction builds (get_conv_params_no_round,
                                do_average 0 then 1, use_jnt_comp_avg and the offset pair); the picture alone is handed over, with no padding, so a
                                read outside it is a read outside the allocation; at 10 bits the packed plane is split into the 8-bit and the 2-bit
                                plane the reference reads
  svt_aom_select_samples, svt_find_projection (find_affine_int + svt_get_shear_params) and the band tests in the order
                                svt_aom_warped_motion_parameters runs them (Codec/adaptive_mv_pred.c:1736-1754)
A second translation unit #includes Codec/mode_decision.c where it lies and defines four callees that reach into encoder state itself:
svt_aom_warped_motion_parameters runs the real selection and fit on the scripted samples, svt_aom_warped_motion_prediction runs the real
svt_av1_warp_plane on the scripted picture into ctx->scratch_prediction_ptr, svt_aom_wm_count_samples and svt_aom_get_ref_pic_buffer do nothing;
svt_aom_choose_best_av1_mv_pred, which that file defines, returns at once because ctx->shut_fast_rate is set.  svt_aom_wm_motion_refinement itself
then runs with corrupted_mv_check = 0, the variance functions of C_DEFAULT/variance.c installed in svt_aom_mefn_ptr, and the rate of Codec/av1me.c.
It returns the MV alone, so the fixture holds per refinement the best MV, the calls of the fit (= tot_checked_pos) and the calls of the warp.
Whatever else the link still wants gets a stand-in that aborts.  The fixture holds numbers only: the CRC-32 of the reference's filter table and of
its divisor table, a CRC-32 per prediction job over the block, one whole block per size and depth, and a CRC-32 per fit over valid, num_samples
and -- for a valid fit -- the matrix and the four shear parameters, and the three numbers per refinement.  --check recomputes everything and compares it with the committed file
instead of writing it; either way the restatements are compared with the reference on every job, and the coverage conditions are asserted.

Two of the issue's conditions on the fit cannot be met by any input, and are therefore not asserted:
  wmmat[2] <= 0      get_mult_shift_diag clamps wmmat[2] to [2^16 - 2^13 + 1, 2^16 + 2^13 - 1], so is_affine_valid never fails behind find_affine_int
  shift < 0          in find_affine_int needs 0 < |det| < 4.  One sample gives A = [[S(sx), P(sx, sy)], [P(sx, sy), S(sy)]] with S >= 4 and
                     det >= 15 (searched exhaustively below for |sx|, |sy| <= 300, the range LS_MV_MAX and the block sizes allow for a kept sample
                     is wider, but S grows quadratically); further samples add positive semi-definite terms up to the rounding of the three
                     shifts, and a random search over two to eight samples (below) finds no determinant under 15 either."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import warp_cases as wc  # noqa: E402
import warp_edge_cases as ec  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#define RTCD_C
#include "warped_motion.c"
#include "common_dsp_rtcd.h"
#include <string.h>

void harness_tables(int16_t *filter, uint16_t *lut) {
    memcpy(filter, svt_aom_warped_filter, sizeof(int16_t) * 193 * 8);
    memcpy(lut, div_lut, sizeof(uint16_t) * 257);
}

static void set_model(EbWarpedMotionParams *wm, const int32_t *m) { /* m: wmmat[6], alpha, beta, gamma, delta, wmtype */
    memset(wm, 0, sizeof(*wm));
    for (int i = 0; i < 6; i++) wm->wmmat[i] = m[i];
    wm->alpha = (int16_t)m[6]; wm->beta = (int16_t)m[7]; wm->gamma = (int16_t)m[8]; wm->delta = (int16_t)m[9];
    wm->wmtype = (TransformationType)m[10];
}

/* pic0 / pic1: the pictures alone, width x height samples, packed; comp: 0 single, 1 average, 2 distance-weighted; out: [h][w] */
int harness_warp(int hbd, const int32_t *m0, const int32_t *m1, int comp, int fwd, int bck, const uint16_t *pic0, const uint16_t *pic1, int width, int height,
                 int p_col, int p_row, int w, int h, int ss_x, int ss_y, uint16_t *out) {
    const int       bd = hbd ? 10 : 8, n = width * height;
    const uint16_t *pics[2] = {pic0, pic1};
    uint8_t        *hi[2] = {NULL, NULL}, *lo[2] = {NULL, NULL};
    uint16_t       *tmp = (uint16_t *)malloc(sizeof(uint16_t) * 128 * 128);
    uint8_t        *dst = (uint8_t *)malloc(2 * 128 * 128);
    svt_av1_warp_affine        = svt_av1_warp_affine_c;
    svt_av1_highbd_warp_affine = svt_av1_highbd_warp_affine_c;
    for (int r = 0; r < (comp ? 2 : 1); r++) {
        hi[r] = (uint8_t *)malloc(n); lo[r] = (uint8_t *)malloc(n);
        for (int i = 0; i < n; i++) {
            if (hbd) { hi[r][i] = (uint8_t)(pics[r][i] >> 2); lo[r][i] = (uint8_t)((pics[r][i] & 3) << 6); }
            else { hi[r][i] = (uint8_t)pics[r][i]; lo[r][i] = 0; }
        }
    }
    memset(dst, 0xEE, 2 * 128 * 128);
    EbWarpedMotionParams wm;
    if (!comp) {
        ConvolveParams cp = get_conv_params_no_round(0, 0, 0, NULL, 128, 0, bd);
        set_model(&wm, m0);
        svt_av1_warp_plane(&wm, hbd, bd, hi[0], lo[0], width, height, width, dst, p_col, p_row, w, h, w, ss_x, ss_y, &cp);
    } else {
        ConvolveParams cp = get_conv_params_no_round(0, 0, 0, tmp, 128, 1, bd);
        cp.use_dist_wtd_comp_avg = comp == 2; cp.fwd_offset = fwd; cp.bck_offset = bck;
        cp.use_jnt_comp_avg = cp.use_dist_wtd_comp_avg;
        cp.do_average = 0;
        set_model(&wm, m0);
        svt_av1_warp_plane(&wm, hbd, bd, hi[0], lo[0], width, height, width, dst, p_col, p_row, w, h, w, ss_x, ss_y, &cp);
        cp.do_average = 1;
        set_model(&wm, m1);
        svt_av1_warp_plane(&wm, hbd, bd, hi[1], lo[1], width, height, width, dst, p_col, p_row, w, h, w, ss_x, ss_y, &cp);
    }
    for (int i = 0; i < w * h; i++) out[i] = hbd ? ((uint16_t *)dst)[i] : dst[i];
    for (int r = 0; r < 2; r++) { free(hi[r]); free(lo[r]); }
    free(tmp); free(dst);
    return 0;
}

/* the MV-dependent half of svt_aom_warped_motion_parameters.  out: valid, num_samples, wmmat[6], alpha, beta, gamma, delta */
int harness_fit(const int32_t *pts_in, const int32_t *ref_in, int n, int bw, int bh, int mv_row, int mv_col, int org_x, int org_y, int shut_approx, int lower,
                int upper, int32_t *out) {
    int pts[SAMPLES_ARRAY_SIZE], pts_inref[SAMPLES_ARRAY_SIZE];
    BlockSize bsize = BLOCK_INVALID;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == bw && block_size_high[b] == bh) bsize = (BlockSize)b;
    if (bsize == BLOCK_INVALID) return 1;
    for (int i = 0; i < SAMPLES_ARRAY_SIZE; i++) { pts[i] = pts_in[i]; pts_inref[i] = ref_in[i]; }
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof(wm));
    MV mv;
    mv.col = (int16_t)mv_col; mv.row = (int16_t)mv_row;
    uint16_t nsamples = (uint16_t)n;
    if (nsamples > 1) nsamples = svt_aom_select_samples(&mv, pts, pts_inref, nsamples, bsize);
    bool apply_wm = !svt_find_projection((int)nsamples, pts, pts_inref, bsize, mv.row, mv.col, &wm, org_y >> MI_SIZE_LOG2, org_x >> MI_SIZE_LOG2);
    if (apply_wm && !shut_approx) {
        if ((abs(wm.alpha) + abs(wm.beta)) < lower && (abs(wm.gamma) + abs(wm.delta)) < lower) apply_wm = 0;
        if ((4 * abs(wm.alpha) + 7 * abs(wm.beta) > upper) && (4 * abs(wm.gamma) + 4 * abs(wm.delta) > upper)) apply_wm = 0;
    }
    out[0] = apply_wm; out[1] = nsamples;
    for (int i = 0; i < 6; i++) out[2 + i] = wm.wmmat[i];
    out[8] = wm.alpha; out[9] = wm.beta; out[10] = wm.gamma; out[11] = wm.delta;
    return 0;
}
"""

HARNESS_REFINE = r"""
#include "mode_decision.c"
#include <string.h>

/* the scripted block: what the five callees that reach into encoder state are given instead */
static const int32_t *g_pts, *g_pts_inref;
static int            g_n, g_width, g_height;
static const uint8_t *g_ref; /* the reference picture alone, g_width x g_height */
static uint32_t       g_fits, g_warps;

bool svt_aom_warped_motion_parameters(PictureControlSet *pcs, BlkStruct *blk_ptr, MvUnit *mv_unit, const BlockGeom *blk_geom, uint16_t blk_org_x,
                                      uint16_t blk_org_y, uint8_t ref_frame_type, EbWarpedMotionParams *wm_params, uint16_t *num_samples,
                                      uint8_t min_neighbour_perc, uint8_t corner_perc_bias, uint16_t lower_band_th, uint16_t upper_band_th, bool shut_approx) {
    (void)pcs; (void)blk_ptr; (void)ref_frame_type; (void)min_neighbour_perc; (void)corner_perc_bias;
    int pts[SAMPLES_ARRAY_SIZE], pts_inref[SAMPLES_ARRAY_SIZE];
    g_fits++;
    *num_samples = 0;
    if (g_n == 0) return false; /* wm_find_samples found none */
    for (int i = 0; i < SAMPLES_ARRAY_SIZE; i++) { pts[i] = g_pts[i]; pts_inref[i] = g_pts_inref[i]; }
    MV mv;
    mv.col = mv_unit->mv[mv_unit->pred_direction % BI_PRED].x;
    mv.row = mv_unit->mv[mv_unit->pred_direction % BI_PRED].y;
    uint16_t nsamples = (uint16_t)g_n;
    if (nsamples > 1) nsamples = svt_aom_select_samples(&mv, pts, pts_inref, nsamples, blk_geom->bsize);
    *num_samples  = nsamples;
    bool apply_wm = !svt_find_projection((int)nsamples, pts, pts_inref, blk_geom->bsize, mv.row, mv.col, wm_params, blk_org_y >> MI_SIZE_LOG2, blk_org_x >> MI_SIZE_LOG2);
    if (apply_wm && !shut_approx) {
        if ((abs(wm_params->alpha) + abs(wm_params->beta)) < lower_band_th && (abs(wm_params->gamma) + abs(wm_params->delta)) < lower_band_th) apply_wm = 0;
        if ((4 * abs(wm_params->alpha) + 7 * abs(wm_params->beta) > upper_band_th) && (4 * abs(wm_params->gamma) + 4 * abs(wm_params->delta) > upper_band_th)) apply_wm = 0;
    }
    return apply_wm;
}

EbErrorType svt_aom_warped_motion_prediction(PictureControlSet *pcs, MvUnit *mv_unit, uint8_t ref_frame_type, uint8_t compound_idx,
                                             InterInterCompoundData *interinter_comp, uint16_t pu_origin_x, uint16_t pu_origin_y, BlkStruct *blk_ptr,
                                             const BlockGeom *blk_geom, EbPictureBufferDesc *ref_pic_list0, EbPictureBufferDesc *ref_pic_list1,
                                             EbPictureBufferDesc *prediction_ptr, uint16_t dst_origin_x, uint16_t dst_origin_y, NeighborArrayUnit *recon_neigh_y,
                                             NeighborArrayUnit *recon_neigh_cb, NeighborArrayUnit *recon_neigh_cr, ModeDecisionCandidate *cand,
                                             EbWarpedMotionParams *wm_params_l0, EbWarpedMotionParams *wm_params_l1, uint8_t bit_depth, uint32_t component_mask,
                                             bool is_encode_pass) {
    (void)pcs; (void)mv_unit; (void)ref_frame_type; (void)compound_idx; (void)interinter_comp; (void)blk_ptr; (void)ref_pic_list0; (void)ref_pic_list1;
    (void)recon_neigh_y; (void)recon_neigh_cb; (void)recon_neigh_cr; (void)cand; (void)wm_params_l1; (void)is_encode_pass;
    if (bit_depth != 8 || component_mask != PICTURE_BUFFER_DESC_LUMA_MASK) abort();
    g_warps++;
    ConvolveParams conv_params = get_conv_params_no_round(0, 0, 0, NULL, 128, 0, bit_depth);
    uint8_t *dst = prediction_ptr->buffer_y + (prediction_ptr->org_x + dst_origin_x + (prediction_ptr->org_y + dst_origin_y) * prediction_ptr->stride_y);
    svt_av1_warp_plane(wm_params_l0, 0, bit_depth, (uint8_t *)g_ref, NULL, g_width, g_height, g_width, dst, pu_origin_x, pu_origin_y, blk_geom->bwidth,
                       blk_geom->bheight, prediction_ptr->stride_y, 0, 0, &conv_params);
    return EB_ErrorNone;
}

void svt_aom_wm_count_samples(BlkStruct *blk_ptr, const BlockSize sb_size, const BlockGeom *blk_geom, uint16_t blk_org_x, uint16_t blk_org_y,
                              uint8_t ref_frame_type, PictureControlSet *pcs, uint16_t *num_samples) {
    (void)blk_ptr; (void)sb_size; (void)blk_geom; (void)blk_org_x; (void)blk_org_y; (void)ref_frame_type; (void)pcs; (void)num_samples;
}
EbPictureBufferDesc *svt_aom_get_ref_pic_buffer(PictureControlSet *pcs, uint8_t is_highbd, uint8_t list_idx, uint8_t ref_idx) {
    (void)pcs; (void)is_highbd; (void)list_idx; (void)ref_idx;
    return NULL;
}

#define SET_VF(W, H) svt_aom_mefn_ptr[BLOCK_##W##X##H].vf = svt_aom_variance##W##x##H##_c
/* settings: iterations, refine_diag, mv_prec_shift, shut_approx, lower_band_th, upper_band_th, approx_inter_rate, error_per_bit; geom: blk_org_x, blk_org_y, bw,
 * bh, n_samples, start row, col, pred row, col; src: the source block's first sample; out: best row, col, the calls of the fit and of the warp, the return */
int harness_refine(const int32_t *settings, const int32_t *geom, const int32_t *pts, const int32_t *pts_inref, const uint8_t *src, int src_stride,
                   const uint8_t *ref, int width, int height, const int32_t *mvjcost, int32_t *mvcost_row, int32_t *mvcost_col, int32_t *out) {
    PictureControlSet           *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet     *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    SequenceControlSet          *scs  = (SequenceControlSet *)calloc(1, sizeof(*scs));
    ModeDecisionContext         *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    MdRateEstimationContext     *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    ModeDecisionCandidateBuffer *cbf  = (ModeDecisionCandidateBuffer *)calloc(1, sizeof(*cbf));
    ModeDecisionCandidate       *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    EbPictureBufferDesc         *pic  = (EbPictureBufferDesc *)calloc(2, sizeof(*pic));
    BlkStruct                   *blk  = (BlkStruct *)calloc(1, sizeof(*blk));
    uint8_t                     *pred = (uint8_t *)calloc(128, 128);
    BlockGeom                    geo;
    if (!pcs || !ppcs || !scs || !ctx || !rate || !cbf || !cand || !pic || !blk || !pred) return 2;
    memset(&geo, 0, sizeof(geo));
    geo.bwidth = (uint8_t)geom[2]; geo.bheight = (uint8_t)geom[3]; geo.bsize = BLOCK_INVALID;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == geom[2] && block_size_high[b] == geom[3]) geo.bsize = (BlockSize)b;
    if (geo.bsize == BLOCK_INVALID) return 3;
    SET_VF(8, 8); SET_VF(8, 16); SET_VF(16, 8); SET_VF(16, 16); SET_VF(16, 32); SET_VF(32, 16); SET_VF(32, 32); SET_VF(32, 64); SET_VF(64, 32); SET_VF(64, 64);
    SET_VF(64, 128); SET_VF(128, 64); SET_VF(128, 128); SET_VF(8, 32); SET_VF(32, 8); SET_VF(16, 64); SET_VF(64, 16);
    svt_av1_warp_affine = svt_av1_warp_affine_c;
    g_pts = pts; g_pts_inref = pts_inref; g_n = geom[4]; g_ref = ref; g_width = width; g_height = height; g_fits = g_warps = 0;
    pcs->ppcs = ppcs; pcs->scs = scs;
    ppcs->frm_hdr.allow_high_precision_mv = settings[2] ? 0 : 1;
    pic[0].buffer_y = (uint8_t *)src - (geom[0] + geom[1] * src_stride); pic[0].stride_y = (uint16_t)src_stride; /* enhanced_pic: origin 0, the block at blk_org */
    ppcs->enhanced_pic = &pic[0];
    pic[1].buffer_y = pred; pic[1].stride_y = 128;
    ctx->scratch_prediction_ptr = &pic[1]; ctx->sb_size = 128;
    ctx->blk_geom = &geo; ctx->blk_org_x = (uint16_t)geom[0]; ctx->blk_org_y = (uint16_t)geom[1]; ctx->blk_ptr = blk;
    ctx->md_rate_est_ctx = rate;
    memcpy(rate->nmv_vec_cost, mvjcost, sizeof(rate->nmv_vec_cost));
    rate->nmvcoststack[0] = mvcost_row + (1 << 14); rate->nmvcoststack[1] = mvcost_col + (1 << 14);
    ctx->full_lambda_md[EB_8_BIT_MD] = (uint32_t)settings[7] << RD_EPB_SHIFT;
    ctx->wm_ctrls.refinement_iterations = (uint8_t)settings[0]; ctx->wm_ctrls.refine_diag = (uint8_t)settings[1];
    ctx->wm_ctrls.lower_band_th = (uint16_t)settings[4]; ctx->wm_ctrls.upper_band_th = (uint16_t)settings[5];
    ctx->approx_inter_rate = (uint8_t)settings[6];
    ctx->corrupted_mv_check = 0;
    ctx->shut_fast_rate = 1; /* svt_aom_choose_best_av1_mv_pred, which is defined in the included file, returns at once */
    cand->ref_frame_type = LAST_FRAME; cand->pred_mode = NEWMV;
    cand->mv[0].x = (int16_t)geom[6]; cand->mv[0].y = (int16_t)geom[5];
    cand->pred_mv[0].x = (int16_t)geom[8]; cand->pred_mv[0].y = (int16_t)geom[7];
    const uint8_t rc = svt_aom_wm_motion_refinement(pcs, ctx, cbf, cand, 0, settings[3]);
    out[0] = cand->mv[0].y; out[1] = cand->mv[0].x; out[2] = (int32_t)g_fits; out[3] = (int32_t)g_warps; out[4] = rc;
    free(pcs); free(ppcs); free(scs); free(ctx); free(rate); free(cbf); free(cand); free(pic); free(blk); free(pred);
    return 0;
}
"""

SOURCES = ["Codec/av1me.c", "Codec/rd_cost.c", "C_DEFAULT/variance.c"]


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    L = refbuild.build(ref, tmp, "warpref", SOURCES, [("harness", HARNESS), ("harness_refine", HARNESS_REFINE)], standins=True)
    P = C.c_void_p
    L.harness_warp.argtypes = [C.c_int, P, P, C.c_int, C.c_int, C.c_int, P, P] + [C.c_int] * 8 + [P]
    L.harness_fit.argtypes = [P, P] + [C.c_int] * 10 + [P]
    L.harness_tables.argtypes = [P, P]
    L.harness_refine.argtypes = [P, P, P, P, P, C.c_int, P, C.c_int, C.c_int, P, P, P, P]
    return L


def model_words(rec):
    return np.array([int(v) for v in rec["wmmat"]] + [int(rec[k]) for k in ("alpha", "beta", "gamma", "delta")] + [int(rec["wmtype"])], np.int32)


def reference_block(L, b, j):
    bd, w, h = b["bit_depth"], int(j["width"]), int(j["height"])
    comp = int(j["ref"][1]) != wc.NO_REF
    pics = []
    for r in range(2 if comp else 1):
        plane, ox, oy, pw, ph = b["planes"][int(j["ref"][r])]
        pics.append(np.ascontiguousarray(plane[oy:oy + ph, ox:ox + pw], dtype=np.uint16))
    from_array = (wc.MODEL0_FROM_ARRAY, wc.MODEL1_FROM_ARRAY)
    m = [model_words(b["models"][int(j["model_index"][r])] if int(j["flags"]) & from_array[r] else j["model"][r]) for r in range(2)]
    out = np.full((h, w), 0xEEEE, np.uint16)
    pw, ph = pics[0].shape[1], pics[0].shape[0]
    rc = L.harness_warp(int(bd > 8), m[0].ctypes.data, m[1].ctypes.data, (1 + int(j["comp_mode"])) if comp else 0, int(j["fwd_offset"]), int(j["bck_offset"]),
                        pics[0].ctypes.data, pics[-1].ctypes.data, pw, ph, int(j["p_col"]), int(j["p_row"]), w, h, b["ss_x"], b["ss_y"], out.ctypes.data)
    assert rc == 0
    return out


def search_small_determinant():
    """the least |det| of find_affine_int's system: exhaustively for one sample, at random for two to eight"""
    sq = lambda a: (a * a * 4 + a * 32 + 128) >> 4
    p1 = lambda a, b: (a * b * 4 + (a + b) * 16 + 64) >> 4
    v = np.arange(-300, 301)
    sx, sy = np.meshgrid(v, v)
    best = int(np.abs(sq(sx) * sq(sy) - p1(sx, sy) ** 2).min())
    rng = np.random.default_rng(5)
    for n in range(2, 9):
        s = rng.integers(-24, 25, (200000, n, 2))
        a00, a11, a01 = sq(s[..., 0]).sum(1), sq(s[..., 1]).sum(1), p1(s[..., 0], s[..., 1]).sum(1)
        best = min(best, int(np.abs(a00 * a11 - a01 * a01).min()))
    return best


def reference_fits(L, b, models, status, bad):
    """MODEL_DTYPE records of the reference's fit on the batch; the jobs on which the restatement (models, status) differs are added to `bad`"""
    name = b["name"]
    ref = np.zeros(len(models), wc.MODEL_DTYPE)
    for i, j in enumerate(b["jobs"]):
        mv = b["mv_array"][int(j["mv_index"])] if int(j["flags"]) & wc.MV_FROM_ARRAY else j["mv"]
        o = np.zeros(12, np.int32)
        pts, inref = np.ascontiguousarray(j["pts"], np.int32), np.ascontiguousarray(j["pts_inref"], np.int32)
        ref[i]["wmtype"] = wc.AFFINE
        if int(j["n_samples"]):  # the host half returns before the fit without samples
            rc = L.harness_fit(pts.ctypes.data, inref.ctypes.data, int(j["n_samples"]), int(j["bwidth"]), int(j["bheight"]), int(mv[0]), int(mv[1]),
                               int(j["blk_org_x"]), int(j["blk_org_y"]), b["shut_approx"], b["lower_band_th"], b["upper_band_th"], o.ctypes.data)
            assert rc == 0
            ref[i]["valid"], ref[i]["num_samples"] = o[0], o[1]
            if o[0]:
                ref[i]["wmmat"] = o[2:8]
                ref[i]["alpha"], ref[i]["beta"], ref[i]["gamma"], ref[i]["delta"] = o[8:12]
        if status[i] != wc.ST_OK or ref[i].tobytes() != models[i].tobytes():
            bad.append((name, i))
    return ref


def reference_refinements(L, b, want, bad):
    """[n][4] of svt_aom_wm_motion_refinement on the batch: best row, col, the positions tested, the positions warped; the jobs on which the
    restatement (want) differs are added to `bad`"""
    name = b["name"]
    ref = np.zeros((len(b["jobs"]), 4), np.int32)
    settings = np.array([b["settings"][k] for k in wc.SETTING_KEYS], np.int32)
    jc, tr, tc = (np.ascontiguousarray(t, np.int32) for t in b["cost_tables"])
    for i, j in enumerate(b["jobs"]):
        if want["status"][i] != wc.ST_OK:
            raise RuntimeError(f"refine {name} job {i} is not defined")
        start = b["mv_array"][int(j["mv_index"])] if int(j["flags"]) & wc.WM_START_FROM_ARRAY else j["start_mv"]
        geom = np.array([j["blk_org_x"], j["blk_org_y"], j["bwidth"], j["bheight"], j["n_samples"], start[0], start[1], j["pred_mv"][0], j["pred_mv"][1]], np.int32)
        plane, ox, oy, pw, ph = b["planes"][int(j["ref"])]
        pic = np.ascontiguousarray(plane[oy:oy + ph, ox:ox + pw], np.uint8)
        src = np.ascontiguousarray(b["src"], np.uint8)
        pts, inref = np.ascontiguousarray(j["pts"], np.int32), np.ascontiguousarray(j["pts_inref"], np.int32)
        o = np.zeros(5, np.int32)
        rc = L.harness_refine(settings.ctypes.data, geom.ctypes.data, pts.ctypes.data, inref.ctypes.data, src.ctypes.data + int(j["src_offset"]), src.shape[1],
                              pic.ctypes.data, pw, ph, jc.ctypes.data, tr.ctypes.data, tc.ctypes.data, o.ctypes.data)
        if rc or o[4] != 1:
            raise RuntimeError(f"harness_refine: {rc}, returned {o[4]}")
        ref[i] = o[:4]
        got = (int(want["best_mv"][i][0]), int(want["best_mv"][i][1]), int(want["n_checked"][i]), int(want["n_valid"][i]))
        if tuple(int(v) for v in o[:4]) != got:
            bad.append((name, i, tuple(int(v) for v in o[:4]), got))
    return ref


def generate_edges(L):
    """the arrays of golden/warp_edges.npz: the cases of tests/warp_edge_cases.py through the same harness"""
    out, bad = {}, []
    for name in ec.REFINE_EDGE_BATCHES:
        out[f"refine_{name}"] = reference_refinements(L, ec.refine_edge_batch(name), ec.restated_refine_edge(name)[0], bad)
    if bad:
        raise RuntimeError(f"the refinement restatement differs from the reference on {len(bad)} edge jobs, first: {bad[:6]}")
    models, status, _ = ec.restated_far()
    out["fit_far"] = wc.models_crc(reference_fits(L, ec.far_batch(), models, status, bad), status)
    if bad:
        raise RuntimeError(f"the fit restatement differs from the reference on {len(bad)} jobs of the far batch, first: {bad[:8]}")
    for name in ec.pred_edge_names():
        b = ec.pred_edge_batch(name)
        _, status, blocks = ec.restated_pred_edge(name)
        crcs = np.zeros(len(b["jobs"]), np.uint32)
        for i, j in enumerate(b["jobs"]):
            if status[i] != wc.ST_OK:
                raise RuntimeError(f"{name} job {i} is not defined")
            ref = reference_block(L, b, j)
            if not np.array_equal(ref, blocks[i]):
                bad.append((name, i, int(np.count_nonzero(ref != blocks[i]))))
            crcs[i] = wc.block_crc(ref)
        out[f"crc_{name}"] = crcs
    if bad:
        raise RuntimeError(f"the prediction restatement differs from the reference on {len(bad)} edge jobs, first: {bad[:8]}")
    missing = ec.edge_coverage_missing()
    if missing:
        raise RuntimeError(f"edge coverage conditions not met: {missing}")
    print(f"edges: {sum(len(out[k]) for k in out if k.startswith('refine_'))} refinements (the wrap batches included: the reference's own function takes them), "
          f"{len(out['fit_far'])} fits and {sum(len(out[k]) for k in out if k.startswith('crc_'))} prediction jobs, the restatements equal to the reference on all of them")
    return out


def generate(L):
    out = {}
    filt, lut = np.zeros((193, 8), np.int16), np.zeros(257, np.uint16)
    L.harness_tables(filt.ctypes.data, lut.ctypes.data)
    if not (np.array_equal(filt, wc.filter_table()) and np.array_equal(lut, wc.div_lut())):
        rows = np.flatnonzero((filt != wc.filter_table()).any(1)).tolist()
        raise RuntimeError(f"the filter table (rows {rows}) or the divisor table ({np.flatnonzero(lut != wc.div_lut()).tolist()}) differs from the reference's")
    out["filter_crc"] = np.array([wc.table_crc(filt, "<i2")], np.uint32)
    out["div_lut_crc"] = np.array([wc.table_crc(lut, "<u2")], np.uint32)
    samples = {(name, i): key for key, name, i in wc.sample_jobs()}
    n_jobs, mismatch = 0, []
    for name in wc.batch_names():
        b = wc.batch(name)
        _, status, blocks, _ = wc.restated(name)
        crcs = np.zeros(len(b["jobs"]), np.uint32)
        for i, j in enumerate(b["jobs"]):
            if status[i] != wc.ST_OK:
                raise RuntimeError(f"{name} job {i} is not defined")
            ref = reference_block(L, b, j)
            if not np.array_equal(ref, blocks[i]):
                mismatch.append((name, i, int(np.count_nonzero(ref != blocks[i]))))
            crcs[i] = wc.block_crc(ref)
            if (name, i) in samples:
                out[samples[(name, i)]] = ref
        out[f"crc_{name}"] = crcs
        n_jobs += len(crcs)
    if mismatch:
        raise RuntimeError(f"the prediction restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    n_fits, bad = 0, []
    for name in wc.MODEL_BATCHES:
        models, status, _ = wc.restated_models(name)
        ref = reference_fits(L, wc.model_batch(name), models, status, bad)
        out[f"fit_{name}"] = wc.models_crc(ref, status)
        n_fits += len(ref)
    if bad:
        raise RuntimeError(f"the fit restatement differs from the reference on {len(bad)} jobs, first: {bad[:8]}")
    n_refine, bad = 0, []
    for name in wc.REFINE_BATCHES:
        ref = reference_refinements(L, wc.refine_batch(name), wc.restated_refine(name)[0], bad)
        out[f"refine_{name}"] = ref
        n_refine += len(ref)
    if bad:
        raise RuntimeError(f"the refinement restatement differs from the reference on {len(bad)} jobs, first: {bad[:6]}")
    missing = wc.pred_coverage_missing() + wc.model_coverage_missing() + wc.refine_coverage_missing()
    if missing:
        raise RuntimeError(f"coverage conditions not met: {missing}")
    least = search_small_determinant()
    if least < 4:
        raise RuntimeError(f"a determinant of {least}: the shift < 0 branch of find_affine_int is reachable after all")
    print(f"{n_jobs} prediction jobs, {n_fits} fits and {n_refine} refinements, the restatements equal to the reference on all of them; least |det| found {least}")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {wc.GOLDEN: generate, ec.GOLDEN: generate_edges})
