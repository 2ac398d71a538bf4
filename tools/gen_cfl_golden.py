#!/usr/bin/env python3
"""Writes tests/golden/cfl.npz: the reference encoder's own chroma-from-luma results on the cases of tests/cfl_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles a harness of its own into a temporary directory outside the tree (gcc, -O2), in two translation units:
  the leaves   calls the reference's svt_cfl_luma_subsampling_420_{lbd,hbd}_c, svt_subtract_average_c (Codec/intra_prediction.c) and
               svt_cfl_predict_{lbd,hbd}_c (C_DEFAULT/cfl_c.c) in the order compute_cfl_ac_components and av1_cost_calc_cfl call them, on the
               reference's own CFL_BUF_LINE buffer.  The luma is handed over as the job's 2W x 2H extent alone, in a band of a poison value, so a
               read beyond the extent shows as a mismatch
  the pick     #includes the reference's Codec/product_coding_loop.c where it lies, because md_cfl_rd_pick_alpha is static, and links stand-ins
               of its own: svt_aom_full_loop_uv returns the scripted (bits, distortion) of the alpha that cand_bf->cand->cfl_alpha_idx /
               cfl_alpha_signs and the component name, and notes the slot; svt_cfl_predict_* and the residual kernel do nothing.
               md_cfl_rd_pick_alpha itself then runs on the tables of tests/cfl_cases.py
and is linked with the rtcd files, with --gc-sections and a version script that exports the harness alone; whatever else the link still wants
gets a stand-in that aborts.  The fixture holds numbers only: per batch a CRC-32 per job over the predictions of both planes for the batch's
alpha list and over the AC; one whole block per size and depth (three alphas and the AC); per alpha-search case the reference's best_rd,
cfl_alpha_idx, cfl_alpha_signs and the slots it evaluated.  Where the reference finds no pair it leaves its two outputs untouched (the harness
checks that) and the fixture holds 0, 0, as include/svt_hip_cfl.h defines.  --check recomputes everything and compares it with the committed
file instead of writing it; either way the restatement is compared with the reference on every job and every case, and the coverage conditions
are asserted."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cfl_cases as cc  # noqa: E402
import refbuild  # noqa: E402

HARNESS_LEAVES = r"""
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "intra_prediction.h"
#include "common_dsp_rtcd.h"
#include "aom_dsp_rtcd.h"

static int ilog2(int v) { int n = 0; while (v > 1) { v >>= 1; n++; } return n; }
/* luma: the first sample of the 2W x 2H extent; dc: [2] blocks of W x H with the stride dc_stride; out: [2][n_alpha][H][W]; ac: [H][W] */
void harness_cfl_job(int hbd, const void *luma, int luma_stride, int w, int h, void *dc_cb, void *dc_cr, int dc_stride, const int8_t *alphas, int n_alpha,
                     uint16_t *out, int16_t *ac) {
    int16_t *q3 = (int16_t *)malloc(sizeof(int16_t) * CFL_BUF_SQUARE);
    memset(q3, 0x55, sizeof(int16_t) * CFL_BUF_SQUARE);
    if (hbd) svt_cfl_luma_subsampling_420_hbd_c((const uint16_t *)luma, luma_stride, q3, 2 * w, 2 * h);
    else svt_cfl_luma_subsampling_420_lbd_c((const uint8_t *)luma, luma_stride, q3, 2 * w, 2 * h);
    svt_subtract_average_c(q3, w, h, (w * h) >> 1, ilog2(w) + ilog2(h));
    for (int r = 0; r < h; r++) memcpy(ac + r * w, q3 + r * CFL_BUF_LINE, sizeof(int16_t) * w);
    void *dc[2] = {dc_cb, dc_cr};
    for (int p = 0; p < 2; p++)
        for (int k = 0; k < n_alpha; k++) {
            uint16_t *o = out + ((size_t)p * n_alpha + k) * w * h;
            if (hbd) svt_cfl_predict_hbd_c(q3, (uint16_t *)dc[p], dc_stride, o, w, alphas[k], 10, w, h);
            else {
                uint8_t tmp[32 * 32];
                svt_cfl_predict_lbd_c(q3, (uint8_t *)dc[p], dc_stride, tmp, w, alphas[k], 8, w, h);
                for (int i = 0; i < w * h; i++) o[i] = tmp[i];
            }
        }
    free(q3);
}
"""

HARNESS_PICK = r"""
#include "product_coding_loop.c"

static const uint64_t *g_bits, *g_dist;
static uint64_t        g_evals[2];
static uint32_t        g_calls, g_noops;

/* stand-ins: the evaluation md_cfl_rd_pick_alpha interleaves with its search, scripted */
void svt_aom_full_loop_uv(PictureControlSet *pcs, ModeDecisionContext *ctx, ModeDecisionCandidateBuffer *cand_bf, EbPictureBufferDesc *input_pic,
                          COMPONENT_TYPE component_type, uint32_t chroma_qindex, uint64_t cb_full_distortion[DIST_TOTAL][DIST_CALC_TOTAL],
                          uint64_t cr_full_distortion[DIST_TOTAL][DIST_CALC_TOTAL], uint64_t *cb_coeff_bits, uint64_t *cr_coeff_bits, bool is_full_loop) {
    (void)pcs; (void)ctx; (void)input_pic; (void)chroma_qindex; (void)is_full_loop;
    const int plane = component_type == COMPONENT_CHROMA_CR;
    const int k     = 16 + cfl_idx_to_alpha(cand_bf->cand->cfl_alpha_idx, cand_bf->cand->cfl_alpha_signs, plane ? CFL_PRED_V : CFL_PRED_U);
    g_evals[plane] |= 1ull << k;
    g_calls++;
    if (plane) { cr_full_distortion[DIST_SSD][DIST_CALC_RESIDUAL] += g_dist[33 + k]; *cr_coeff_bits += g_bits[33 + k]; }
    else { cb_full_distortion[DIST_SSD][DIST_CALC_RESIDUAL] += g_dist[k]; *cb_coeff_bits += g_bits[k]; }
}
void svt_aom_residual_kernel(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *pred, uint32_t pred_offset, uint32_t pred_stride,
                             int16_t *residual, uint32_t residual_offset, uint32_t residual_stride, bool hbd, uint32_t area_width, uint32_t area_height) {
    (void)input; (void)input_offset; (void)input_stride; (void)pred; (void)pred_offset; (void)pred_stride; (void)residual; (void)residual_offset;
    (void)residual_stride; (void)hbd; (void)area_width; (void)area_height;
    g_noops++;
}
static void noop_lbd(const int16_t *q3, uint8_t *pred, int32_t ps, uint8_t *dst, int32_t ds, int32_t alpha, int32_t bd, int32_t w, int32_t h) {
    (void)q3; (void)pred; (void)ps; (void)dst; (void)ds; (void)alpha; (void)bd; (void)w; (void)h; g_noops++; }
static void noop_hbd(const int16_t *q3, uint16_t *pred, int32_t ps, uint16_t *dst, int32_t ds, int32_t alpha, int32_t bd, int32_t w, int32_t h) {
    (void)q3; (void)pred; (void)ps; (void)dst; (void)ds; (void)alpha; (void)bd; (void)w; (void)h; g_noops++; }

/* bits / dist: [2][33], slot k = alpha_q3 + 16; fac: [8][2][16]; out: best_rd, cfl_alpha_idx, cfl_alpha_signs (both preset to 0xEE), the slots
 * evaluated per plane, the evaluations, the calls of the no-ops */
int harness_pick(const uint64_t *bits, const uint64_t *dist, const int32_t *fac, int32_t mode_bits, uint32_t lambda, int itr_th, int hbd, uint64_t *out) {
    ModeDecisionContext         *ctx  = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
    MdRateEstimationContext     *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    ModeDecisionCandidateBuffer *cbf  = (ModeDecisionCandidateBuffer *)calloc(1, sizeof(*cbf));
    ModeDecisionCandidate       *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    EbPictureBufferDesc         *pic  = (EbPictureBufferDesc *)calloc(4, sizeof(*pic));
    uint8_t                     *mem  = (uint8_t *)calloc(4, 4096);
    BlockGeom                    geom;
    if (!ctx || !rate || !cbf || !cand || !pic || !mem) return 2;
    memset(&geom, 0, sizeof(geom));
    geom.bwidth = geom.bheight = 16; geom.bwidth_uv = geom.bheight_uv = 8;
    for (int i = 0; i < 4; i++) { pic[i].buffer_cb = mem + i * 4096; pic[i].buffer_cr = mem + i * 4096 + 2048; pic[i].stride_cb = pic[i].stride_cr = 16; }
    svt_cfl_predict_lbd = noop_lbd; svt_cfl_predict_hbd = noop_hbd;
    g_bits = bits; g_dist = dist; g_evals[0] = g_evals[1] = 0; g_calls = g_noops = 0;
    ctx->blk_geom = &geom; ctx->hbd_md = (uint8_t)hbd; ctx->full_lambda_md[0] = ctx->full_lambda_md[1] = lambda; ctx->md_rate_est_ctx = rate;
    ctx->cfl_ctrls.itr_th = (uint8_t)itr_th; ctx->scratch_prediction_ptr = &pic[2];
    cand->pred_mode = DC_PRED;
    rate->intra_uv_mode_fac_bits[CFL_ALLOWED][DC_PRED][UV_CFL_PRED] = mode_bits;
    memcpy(rate->cfl_alpha_fac_bits, fac, sizeof(rate->cfl_alpha_fac_bits));
    if (sizeof(rate->cfl_alpha_fac_bits) != 8 * 2 * 16 * sizeof(int32_t)) return 3;
    cbf->cand = cand; cbf->pred = &pic[0]; cbf->residual = &pic[1];
    uint8_t idx = 0xEE, signs = 0xEE;
    out[0] = md_cfl_rd_pick_alpha(NULL, cbf, ctx, &pic[3], 0, 0, &idx, &signs);
    out[1] = idx; out[2] = signs; out[3] = g_evals[0]; out[4] = g_evals[1]; out[5] = g_calls; out[6] = g_noops; out[7] = MAX_MODE_COST;
    free(ctx); free(rate); free(cbf); free(cand); free(pic); free(mem);
    return 0;
}
"""

SOURCES = ["Codec/intra_prediction.c", "C_DEFAULT/cfl_c.c", "C_DEFAULT/intra_prediction_c.c", "C_DEFAULT/filterintra_c.c", "C_DEFAULT/picture_operators_c.c",
           "Codec/cdef.c", "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]


def build(ref, tmp):
    """The stand-ins are the SIMD bodies the rtcd files name and what the rest of product_coding_loop.c calls."""
    L = refbuild.build(ref, tmp, "cflref", SOURCES, [("harness_leaves", HARNESS_LEAVES), ("harness_pick", HARNESS_PICK)], standins=True)
    L.harness_cfl_job.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.harness_cfl_job.restype = None
    L.harness_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    return L


def reference_job(L, b, j):
    bd, w, h = b["bit_depth"], b["width"], b["height"]
    dt = np.uint16 if bd > 8 else np.uint8
    lx, ly = int(j["luma_x"]), int(j["luma_y"])
    band = np.full((2 * h + 2, 2 * w + 16), 0x2C5 if bd > 8 else 0xC5, dt)  # the extent alone, in poison
    band[1:1 + 2 * h, 8:8 + 2 * w] = b["luma"][ly:ly + 2 * h, lx:lx + 2 * w]
    dc = [np.ascontiguousarray(cc.dc_block(b, j, p)) for p in range(2)]
    alphas = np.array(b["alphas"], np.int8)
    out, ac = np.full((2, len(alphas), h, w), 0xA5A5, np.uint16), np.full((h, w), 0x5A5A, np.int16)
    L.harness_cfl_job(int(bd > 8), band.ctypes.data + (band.shape[1] + 8) * band.itemsize, band.shape[1], w, h, dc[0].ctypes.data, dc[1].ctypes.data, w,
                      alphas.ctypes.data, len(alphas), out.ctypes.data, ac.ctypes.data)
    return out, ac


def generate(L):
    out, mismatch = {}, []
    samples = {(name, i): (kp, ka) for kp, ka, name, i in cc.sample_jobs()}
    n_jobs = 0
    for name in cc.batch_names():
        b = cc.batch(name)
        want_p, want_a, _ = cc.restated(name)
        got_p, got_a = [], []
        for i, j in enumerate(b["jobs"]):
            if not cc.job_defined(b, j):
                raise RuntimeError(f"{name} job {i} is not defined")
            p, a = reference_job(L, b, j)
            if not (np.array_equal(p, want_p[i]) and np.array_equal(a, want_a[i])):
                mismatch.append((name, i, int(np.count_nonzero(p != want_p[i])), int(np.count_nonzero(a != want_a[i]))))
            got_p.append(p)
            got_a.append(a)
            if (name, i) in samples:
                kp, ka = samples[(name, i)]
                out[kp], out[ka] = p[:, cc.sample_slots()], a
        out[f"crc_{name}"] = cc.batch_crcs(got_p, got_a)
        n_jobs += len(got_p)
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    missing = cc.coverage_missing(cc.all_records())
    # the alpha search
    cases, results = cc.pick_cases(), cc.pick_results()
    ref = np.zeros((len(cases), 5), np.uint64)  # best_rd, idx, signs, the slots evaluated in Cb, in Cr
    bad = []
    for n, (c, r) in enumerate(zip(cases, results)):
        o = np.zeros(8, np.uint64)
        bits, dist, fac = (np.ascontiguousarray(c[k]) for k in ("bits", "dist", "fac"))
        for hbd in (0, 1):  # the depth only chooses the lambda and the no-op
            rc = L.harness_pick(bits.ctypes.data, dist.ctypes.data, fac.ctypes.data, c["mode_bits"], c["lam"], c["itr_th"], hbd, o.ctypes.data)
            if rc or int(o[7]) != cc.MAX_MODE_COST:
                raise RuntimeError(f"harness_pick: {rc}, MAX_MODE_COST {int(o[7])}")
            if int(o[6]) != 2 * int(o[5]):
                raise RuntimeError(f"{c['name']}: {int(o[5])} evaluations, {int(o[6])} calls of the prediction and residual stand-ins")
            if int(o[0]) == cc.MAX_MODE_COST:
                if (int(o[1]), int(o[2])) != (0xEE, 0xEE):
                    raise RuntimeError(f"{c['name']}: no pair, but the reference wrote its outputs")
                o[1] = o[2] = 0
            if hbd and not np.array_equal(o[:5], ref[n]):
                raise RuntimeError(f"{c['name']}: the two depths differ")
            ref[n] = o[:5]
        got = (r["best_rd"], r["idx"], r["signs"], r["evals"][0], r["evals"][1])
        if c["n_mag"] == 16 or r["status"] == 0:  # a truncated replay may differ: that is what its bit says
            if tuple(int(v) for v in ref[n]) != got:
                bad.append((c["name"], tuple(int(v) for v in ref[n]), got))
        elif r["status"] != cc.PICK_TRUNCATED:
            bad.append((c["name"], "status", r["status"]))
    if bad:
        raise RuntimeError(f"the alpha-search restatement differs from the reference on {len(bad)} cases, first: {bad[:4]}")
    missing += cc.pick_coverage_missing(cases, results)
    if missing:
        raise RuntimeError(f"coverage conditions not met: {missing}")
    out["pick_ref"] = ref
    print(f"{n_jobs} prediction jobs and {len(cases)} alpha-search cases, the restatement equal to the reference on all of them")
    return out


def wrote(path, out):
    largest = max(os.path.getsize(os.path.join(os.path.dirname(path), f)) for f in os.listdir(os.path.dirname(path)) if f != os.path.basename(path))
    line = f"wrote {path} ({os.path.getsize(path)} bytes; the largest other fixture has {largest}), {len(out)} arrays"
    if os.path.getsize(path) > largest:
        sys.exit(line + "\nthe fixture is larger than the largest fixture already there")
    return line


if __name__ == "__main__":
    refbuild.main(__doc__, build, {cc.GOLDEN: generate}, wrote=wrote)
