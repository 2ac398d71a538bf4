#!/usr/bin/env python3
"""Writes tests/golden/ifs.npz: the reference encoder's own interpolation-filter search on the cases of tests/ifs_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or bench.py.
It compiles a harness of its own into a temporary directory outside the tree (gcc, -O2).  The harness #includes Codec/enc_inter_prediction.c where
it lies, because interpolation_filter_search, model_rd_for_sb and svt_av1_get_switchable_rate are static, and links Codec/inter_prediction.c,
Codec/psy_rd.c, Codec/entropy_coding.c (for svt_aom_get_pred_context_switchable_interp), Codec/pic_operators.c, C_DEFAULT/inter_prediction_c.c,
C_DEFAULT/picture_operators_c.c and the two rtcd files where they lie, with the _c kernels installed in the rtcd pointers.  Whatever else the link
still wants gets a stand-in that aborts.

Per job the harness scripts a PictureControlSet, a ModeDecisionContext and a candidate: reference pictures that are EbPictureBufferDesc's over the
padded planes, a source picture whose sample at the block's origin is the block's first source sample, a scratch prediction picture of the block's size, the frame's order hints (which
give svt_av1_dist_wtd_comp_weight_assign the job's fwd_offset / bck_offset), the Dequants entry, full_lambda_md, psy_rd, spy_rd, the sharpness
switch with picture_qp, ifs_ctrls, the rate table, and a MacroBlockD whose left and above mode infos are the scripted neighbour pair, so that
svt_aom_get_pred_context_switchable_interp computes the contexts itself.  It then
  1  calls interpolation_filter_search and takes cand->interp_filters and what it added to fast_luma_rate,
  2  predicts the winner once more with svt_aom_inter_prediction, as the caller at :5127 does, for the winner's samples,
  3  for each pair the search visits calls svt_aom_inter_prediction, model_rd_for_sb (once as configured, once with skip_sse_rd_model for the SSE it
     hides) and svt_av1_get_switchable_rate, and evaluates the reference's own RDCOST macro and the two bias statements on them.
The first minimum of 3 must be 1's winner, or the harness fails: the per-pair numbers are the ones the search compared.

The fixture holds numbers only.  --check recomputes everything and compares it with the committed file instead of writing it; either way the
restatement of tests/ifs_cases.py is compared with the reference on every output of every job, every prediction's reads are checked to lie inside
the plane handed to the reference, and the conditions of the case list are asserted."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ifs_cases as ic  # noqa: E402
import inter_pred_cases as ip  # noqa: E402
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
#include "utility.h"

BlockGeom svt_aom_blk_geom_mds[MAX_NUM_BLOCKS_ALLOC];

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
    svt_aom_convolve[0][0][1] = svt_av1_jnt_convolve_2d_copy_c; svt_aom_convolve[1][0][1] = svt_av1_jnt_convolve_x_c;
    svt_aom_convolve[0][1][1] = svt_av1_jnt_convolve_y_c; svt_aom_convolve[1][1][1] = svt_av1_jnt_convolve_2d_c;
    svt_aom_convolveHbd[0][0][0] = svt_av1_highbd_convolve_2d_copy_sr_c; svt_aom_convolveHbd[1][0][0] = svt_av1_highbd_convolve_x_sr_c;
    svt_aom_convolveHbd[0][1][0] = svt_av1_highbd_convolve_y_sr_c; svt_aom_convolveHbd[1][1][0] = svt_av1_highbd_convolve_2d_sr_c;
    svt_aom_convolveHbd[0][0][1] = svt_av1_highbd_jnt_convolve_2d_copy_c; svt_aom_convolveHbd[1][0][1] = svt_av1_highbd_jnt_convolve_x_c;
    svt_aom_convolveHbd[0][1][1] = svt_av1_highbd_jnt_convolve_y_c; svt_aom_convolveHbd[1][1][1] = svt_av1_highbd_jnt_convolve_2d_c;
    svt_spatial_full_distortion_kernel = svt_spatial_full_distortion_kernel_c;
    svt_full_distortion_kernel16_bits = svt_full_distortion_kernel16_bits_c;
    return 0;
}

/* p: 0 bit_depth, 1 width, 2 height, 3 org_x, 4 org_y, 5-8 the four edges (left, right, top, bottom), 9 compound, 10 comp_mode, 11-14 mv row / col of
 *    the two references, 15 / 16 the order hints of the two references (the current picture's is 64), 17 enable_dual_filter, 18 subsampled_distortion,
 *    19 skip_sse_rd_model, 20 spy_rd, 21 quantizer, 22 lambda, 23 smooth bias on, 24 picture_qp, 25-27 the left neighbour (available, y filter, x filter), 28-30 the above one,
 *    31 / 32 padded width / height of the reference planes, 33 / 34 their origin
 * refs[2]: the padded planes' first samples; out: 0 interp_filters, 1 switchable rate; rd / sse: [9]; pred: width x height samples of the winner */
int harness_ifs(const int *p, double psy_rd, uint8_t **refs, int ref_stride, uint8_t *src, int src_stride, const int32_t *fac_bits, int64_t *out,
                uint64_t *rd, uint64_t *sse, uint8_t *pred) {
    const int bd = p[0], is16 = bd > 8, w = p[1], h = p[2], comp = p[9];
    const BlockSize bsize = bsize_of(w, h);
    SequenceControlSet      *scs  = (SequenceControlSet *)calloc(1, sizeof(*scs));
    EncodeContext           *enc  = (EncodeContext *)calloc(1, sizeof(*enc));
    PictureControlSet       *pcs  = (PictureControlSet *)calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = (PictureParentControlSet *)calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    ModeDecisionCandidateBuffer *cb = (ModeDecisionCandidateBuffer *)calloc(1, sizeof(*cb));
    ModeDecisionCandidate   *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    MdRateEstimationContext *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    BlkStruct               *blk  = (BlkStruct *)calloc(1, sizeof(*blk));
    EbPictureBufferDesc     *pic  = (EbPictureBufferDesc *)calloc(4, sizeof(*pic)); /* two references, the source, the scratch prediction */
    ModeInfo                *mis  = (ModeInfo *)calloc(3, sizeof(*mis));
    ModeInfo               **grid = (ModeInfo **)calloc(16, sizeof(*grid));
    uint8_t                 *scratch = (uint8_t *)calloc((size_t)w * h, 2);
    MacroBlockD              xd;
    BlockGeom               *geo = &svt_aom_blk_geom_mds[0];
    if (!scs || !enc || !pcs || !ppcs || !ctx || !cb || !cand || !rate || !blk || !pic || !mis || !grid || !scratch) return 2;
    if (bsize == BLOCK_INVALID) return 3;
    memset(&xd, 0, sizeof(xd));
    memset(geo, 0, sizeof(*geo));
    svt_av1_setup_scale_factors_for_frame(&scs->sf_identity, 192, 128, 192, 128);
    scs->enc_ctx = enc;
    scs->seq_header.enable_dual_filter = (uint8_t)p[17];
    scs->seq_header.order_hint_info.enable_order_hint = 1; scs->seq_header.order_hint_info.order_hint_bits = 8;
    scs->static_config.encoder_bit_depth = (uint32_t)bd;
    scs->static_config.psy_rd = psy_rd; scs->static_config.spy_rd = (uint8_t)p[20];
    scs->vq_ctrls.sharpness_ctrls.ifs = (uint8_t)p[23];
    (is16 ? &enc->deq_bd : &enc->deq_8bit)->y_dequant_qtx[0][1] = (int16_t)p[21];
    pcs->scs = scs; pcs->ppcs = ppcs; ppcs->scs = scs;
    pcs->picture_qp = (uint8_t)p[24]; pcs->slice_type = B_SLICE; pcs->temporal_layer_index = 4; /* get_hvs_modulation_factor: psy_rd itself */
    ppcs->is_noise_level = (uint8_t)p[23]; ppcs->is_not_scaled = 1;
    ppcs->frm_hdr.interpolation_filter = SWITCHABLE; ppcs->frm_hdr.quantization_params.base_q_idx = 0;
    ppcs->cur_order_hint = 64; ppcs->ref_order_hint[LAST_FRAME - 1] = (uint32_t)p[15]; ppcs->ref_order_hint[BWDREF_FRAME - 1] = (uint32_t)p[16];
    for (int r = 0; r < 2; r++) {
        EbPictureBufferDesc *d = &pic[r];
        d->buffer_y = refs[r]; d->stride_y = (uint16_t)ref_stride; d->org_x = (uint16_t)p[33]; d->org_y = (uint16_t)p[34];
        d->width = 192; d->height = 128; d->bit_depth = (EbBitDepth)bd;
    }
    pic[2].buffer_y = src; pic[2].stride_y = (uint16_t)src_stride; pic[2].width = 192; pic[2].height = 128; /* the source: its (org_x, org_y) is the block's first sample */
    ppcs->enhanced_pic = &pic[2]; pcs->input_frame16bit = &pic[2];
    pic[3].buffer_y = scratch; pic[3].stride_y = (uint16_t)w; pic[3].width = (uint16_t)w; pic[3].height = (uint16_t)h;
    ctx->scratch_prediction_ptr = &pic[3];
    geo->bsize = bsize; geo->bwidth = (uint8_t)w; geo->bheight = (uint8_t)h;
    ctx->blk_geom = geo; ctx->blk_ptr = blk; blk->av1xd = &xd; blk->mds_idx = 0;
    ctx->blk_org_x = (uint32_t)p[3]; ctx->blk_org_y = (uint32_t)p[4]; /* the source picture's pointer is moved back by as much */
    ctx->hbd_md = (uint8_t)is16; ctx->md_stage = MD_STAGE_0;
    ctx->full_lambda_md[EB_8_BIT_MD] = (uint32_t)p[22]; ctx->full_lambda_md[EB_10_BIT_MD] = (uint32_t)p[22] << (2 * (bd - 8));
    ctx->ifs_ctrls.subsampled_distortion = (uint8_t)p[18]; ctx->ifs_ctrls.skip_sse_rd_model = (uint8_t)p[19];
    memcpy(rate->switchable_interp_fac_bitss, fac_bits, sizeof(rate->switchable_interp_fac_bitss));
    if (sizeof(rate->switchable_interp_fac_bitss) != 16 * 3 * sizeof(int32_t)) return 4;
    ctx->md_rate_est_ctx = rate;
    /* the neighbours: [0] the block itself, [1] left, [2] above; an unavailable one is a block of another reference frame */
    for (int i = 0; i < 16; i++) grid[i] = &mis[0];
    for (int k = 0; k < 2; k++) {
        const int *n = p + 25 + 3 * k;
        mis[1 + k].mbmi.block_mi.ref_frame[0] = n[0] ? LAST_FRAME : ALTREF_FRAME; mis[1 + k].mbmi.block_mi.ref_frame[1] = NONE_FRAME;
        mis[1 + k].mbmi.block_mi.interp_filters = av1_make_interp_filters((InterpFilter)n[1], (InterpFilter)n[2]);
    }
    xd.mi_stride = 4; xd.mi = grid + 5; grid[4] = &mis[1]; grid[1] = &mis[2];
    xd.left_available = 1; xd.up_available = 1;
    xd.mb_to_left_edge = p[5]; xd.mb_to_right_edge = p[6]; xd.mb_to_top_edge = p[7]; xd.mb_to_bottom_edge = p[8];
    xd.n4_w = (uint8_t)(w >> 2); xd.n4_h = (uint8_t)(h >> 2); xd.bsize = bsize;

    cb->cand = cand;
    cand->ref_frame_type = comp ? 8 : LAST_FRAME; /* {LAST_FRAME, BWDREF_FRAME} is the first pair of the compound types */
    MvReferenceFrame rf[2];
    av1_set_ref_frame(rf, cand->ref_frame_type);
    if (rf[0] != LAST_FRAME || rf[1] != (comp ? BWDREF_FRAME : NONE_FRAME)) return 5;
    cand->pred_mode = comp ? NEW_NEWMV : NEWMV; cand->motion_mode = SIMPLE_TRANSLATION;
    cand->compound_idx = comp && p[10] ? 0 : 1; /* 0: distance-weighted */
    cand->interinter_comp.type = comp && p[10] ? COMPOUND_DISTWTD : COMPOUND_AVERAGE;
    MvUnit mv_unit;
    memset(&mv_unit, 0, sizeof(mv_unit));
    mv_unit.pred_direction = comp ? BI_PRED : UNI_PRED_LIST_0;
    mv_unit.mv[REF_LIST_0].y = (int16_t)p[11]; mv_unit.mv[REF_LIST_0].x = (int16_t)p[12];
    mv_unit.mv[REF_LIST_1].y = (int16_t)p[13]; mv_unit.mv[REF_LIST_1].x = (int16_t)p[14];

    cb->fast_luma_rate = 1000;
    interpolation_filter_search(pcs, ctx, cb, mv_unit, &pic[0], comp ? &pic[1] : NULL, (uint8_t)is16, (uint8_t)bd);
    out[0] = cand->interp_filters; out[1] = (int64_t)cb->fast_luma_rate - 1000;
    const uint32_t best = cand->interp_filters;

    /* every pair once more, with the functions the search called */
    const uint32_t lambda = is16 ? ctx->full_lambda_md[EB_10_BIT_MD] >> (2 * (bd - 8)) : ctx->full_lambda_md[EB_8_BIT_MD];
    static const uint64_t smooth_bias[4] = {130, 120, 110, 100};
    uint64_t first = (uint64_t)~0;
    uint32_t first_filters = 0;
    for (int i = 0; i < 9; i++) {
        rd[i] = sse[i] = (uint64_t)~0;
        if (!p[17] && filter_sets[i][0] != filter_sets[i][1]) continue;
        cand->interp_filters = av1_make_interp_filters((InterpFilter)filter_sets[i][0], (InterpFilter)filter_sets[i][1]);
        const int32_t rs = svt_av1_get_switchable_rate(cb, &ppcs->frm_hdr, ctx, (bool)p[17]);
        svt_aom_inter_prediction(scs, pcs, cand->interp_filters, blk, cand->ref_frame_type, &mv_unit, 0, SIMPLE_TRANSLATION, 1, ctx, cand->compound_idx,
                                 &cand->interinter_comp, NULL, NULL, NULL, 0, 0, 0, 0, (uint16_t)p[3], (uint16_t)p[4], (uint8_t)w, (uint8_t)h, &pic[0], comp ? &pic[1] : NULL, &pic[3], 0, 0,
                                 PICTURE_BUFFER_DESC_LUMA_MASK, (uint8_t)bd, 0);
        int32_t r_; int64_t d_;
        model_rd_for_sb(pcs, &pic[3], ctx, 0, 0, &r_, &d_, (uint8_t)bd);
        uint64_t v = RDCOST(lambda, rs + r_, d_);
        if (p[23] && (filter_sets[i][0] == 1 || filter_sets[i][1] == 1)) v = (v * smooth_bias[p[24] >> 4]) / 100;
        if (p[20]) {
            if (filter_sets[i][0] == 2 || filter_sets[i][1] == 2) v = (v * 75) / 100;
            if (filter_sets[i][0] == 0 || filter_sets[i][1] == 0) v = (v * 80) / 100;
        }
        rd[i] = v;
        if (v < first) { first = v; first_filters = cand->interp_filters; }
        ctx->ifs_ctrls.skip_sse_rd_model = 1;
        model_rd_for_sb(pcs, &pic[3], ctx, 0, 0, &r_, &d_, (uint8_t)bd);
        ctx->ifs_ctrls.skip_sse_rd_model = (uint8_t)p[19];
        if (d_ % 10) return 6;
        sse[i] = (uint64_t)d_ / 10;
    }
    if (first_filters != best) return 7;
    out[2] = (int64_t)first;
    svt_aom_inter_prediction(scs, pcs, best, blk, cand->ref_frame_type, &mv_unit, 0, SIMPLE_TRANSLATION, 1, ctx, cand->compound_idx, &cand->interinter_comp, NULL,
                             NULL, NULL, 0, 0, 0, 0, (uint16_t)p[3], (uint16_t)p[4], (uint8_t)w, (uint8_t)h, &pic[0], comp ? &pic[1] : NULL, &pic[3], 0, 0, PICTURE_BUFFER_DESC_LUMA_MASK,
                             (uint8_t)bd, 0);
    memcpy(pred, scratch, (size_t)w * h << is16);
    free(scs); free(enc); free(pcs); free(ppcs); free(ctx); free(cb); free(cand); free(rate); free(blk); free(pic); free(mis); free(grid); free(scratch);
    return 0;
}
"""

SOURCES = ["Codec/inter_prediction.c", "Codec/psy_rd.c", "Codec/entropy_coding.c", "Codec/pic_operators.c", "C_DEFAULT/inter_prediction_c.c", "C_DEFAULT/picture_operators_c.c",
           "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]
MARGIN = 32  # samples of edge replication around an edge batch's planes: what the kernel's coordinate clamp stands for


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    L = refbuild.build(ref, tmp, "ifsref", SOURCES, [("harness", HARNESS)], standins=True)
    P = C.c_void_p
    L.harness_ifs.argtypes = [P, C.c_double, P, C.c_int, P, C.c_int, P, P, P, P, P]
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def order_hints(fwd, bck):
    """order hints of the two references (the current picture's is 64) for which svt_av1_dist_wtd_comp_weight_assign gives (fwd_offset, bck_offset):
    found by trying every pair of distances on the function's own statement (Codec/inter_prediction.c:273-309, order_idx = 0)"""
    weight, table = [(2, 3), (2, 5), (2, 7)], [(9, 7), (11, 5), (12, 4), (13, 3)]
    for d0 in range(1, 32):
        for d1 in range(1, 32):
            order = int(d0 <= d1)
            i = 0
            while i < 3:
                c0, c1 = weight[i][order], weight[i][1 - order]
                if (d0 > d1 and d0 * c0 < d1 * c1) or (d0 <= d1 and d0 * c0 > d1 * c1):
                    break
                i += 1
            if (table[i][order], table[i][1 - order]) == (fwd, bck):
                return 64 - d1, 64 + d0  # bck_frame_index is the first reference's hint, fwd_frame_index the second's
    raise RuntimeError(f"no distances give the offsets ({fwd}, {bck})")


def reference_batch(L, name):
    """the reference's results of a batch, laid out as ifs_cases.restated()'s"""
    b = ic.batch(name)
    bd, prm = b["bit_depth"], b["params"]
    dt = np.uint16 if bd > 8 else np.uint8
    isz = np.dtype(dt).itemsize
    planes = []
    for pl, ox, oy in ic.batch_planes(b):
        m = MARGIN if b["edge_planes"] else 0
        planes.append((np.ascontiguousarray(np.pad(pl, m, mode="edge")), ox + m, oy + m))
    ptrs = (C.c_void_p * 2)()
    fac = np.ascontiguousarray(b["fac_bits"], np.int32)
    src = np.ascontiguousarray(b["src"])
    qp = {0: 0, 130: 0, 120: 16, 110: 32, 100: 48}[prm["smooth_bias_pct"]]
    res = []
    for i, (job, nbr) in enumerate(zip(b["jobs"], b["nbrs"])):
        j = job["pred"]
        w, h, comp = int(j["width"]), int(j["height"]), int(j["ref"][1]) != ip.NO_REF
        for k in range(2):
            pl = planes[int(j["ref"][k]) if k == 0 or comp else 0][0]
            ptrs[k] = pl.ctypes.data
        mvs = [ip.job_mv(j, k, b["mv_array"]) for k in range(2)]
        hints = order_hints(int(j["fwd_offset"]), int(j["bck_offset"])) if comp and j["comp_mode"] else (60, 68)
        p = [bd, w, h, j["org_x"], j["org_y"], j["mb_to_left_edge"], j["mb_to_right_edge"], j["mb_to_top_edge"], j["mb_to_bottom_edge"], comp, j["comp_mode"],
             mvs[0][0], mvs[0][1], mvs[1][0], mvs[1][1], hints[0], hints[1], prm["enable_dual_filter"], prm["subsampled_distortion"], prm["skip_sse_rd_model"],
             prm["spy_rd"], prm["quantizer"], prm["lambda_"], int(prm["smooth_bias_pct"] != 0), qp]
        for n in nbr:
            p += [0, 0, 0] if n is None else [1, n[0], n[1]]
        p += [planes[0][0].shape[1], planes[0][0].shape[0], planes[0][1], planes[0][2]]
        a = np.array([int(v) for v in p], np.int32)
        out, rd, sse, pred = np.zeros(3, np.int64), np.zeros(9, np.uint64), np.zeros(9, np.uint64), np.zeros((h, w), dt)
        y0, x0 = divmod(int(job["src_offset"]), src.shape[1])
        rc = L.harness_ifs(a.ctypes.data, float(prm["psy_rd"]), ptrs, planes[0][0].shape[1], src.ctypes.data + ((y0 - int(j["org_y"])) * src.shape[1] + x0 - int(j["org_x"])) * isz, src.shape[1],
                           fac.ctypes.data, out.ctypes.data, rd.ctypes.data, sse.ctypes.data, pred.ctypes.data)
        if rc:
            raise RuntimeError(f"{name} job {i}: the harness returned {rc}")
        yf, xf = int(out[0]) & 0xFFFF, int(out[0]) >> 16
        res.append({"rd": rd, "sse": sse, "winner": ic.FILTER_SETS.index((yf, xf)), "switchable_rate": int(out[1]), "interp_filters": int(out[0]),
                    "best_rd": int(np.uint64(out[2])), "pred": pred.astype(np.uint16)})
    return res


def generate(L):
    out, mismatch, n_jobs = {}, [], 0
    for name in ic.batch_names():
        b = ic.batch(name)
        ref, want = reference_batch(L, name), ic.restated(name)
        for i, r in enumerate(want):
            if not b["edge_planes"] and not r["events"]["inside"]:
                raise RuntimeError(f"{name} job {i}: a prediction's reads leave the padded plane")
        got, mine = ic.fixture_arrays(name, ref), ic.fixture_arrays(name, want)
        for k in got:
            if not (got[k].dtype == mine[k].dtype and np.array_equal(got[k], mine[k])):
                mismatch.append((k, np.argwhere(got[k] != mine[k])[:4].tolist() if got[k].shape == mine[k].shape else "shape"))
        out.update(got)
        n_jobs += len(ref)
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference in {len(mismatch)} arrays, first: {mismatch[:8]}")
    missing = ic.coverage_missing()
    if missing:
        raise RuntimeError(f"conditions of the case list that are not met: {missing[:10]}")
    print(f"{n_jobs} jobs in {len(ic.batch_names())} batches: the nine costs and SSEs, the winner, its rate, cost and prediction of the restatement equal to the "
          "reference's on all of them")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {ic.GOLDEN: generate})
