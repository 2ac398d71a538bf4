#!/usr/bin/env python3
"""Writes tests/golden/inter_pred.npz: the reference encoder's own svt_aom_enc_make_inter_predictor results on the cases of tests/inter_pred_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles the reference's Codec/inter_prediction.c and Codec/enc_inter_prediction.c (and Codec/aom_dsp_rtcd.c,
Codec/common_dsp_rtcd.c for the rtcd pointers) where they lie, together with a small harness of its own, into a temporary directory outside
the tree (gcc, -O2), links with --gc-sections and a version script that exports the harness alone, and
  fills svt_aom_convolve[][][] / svt_aom_convolveHbd[][][] with the sixteen _c bodies, each behind a wrapper that counts its calls,
  calls svt_aom_enc_make_inter_predictor itself for every reference of every job: identity ScaleFactors (svt_av1_setup_scale_factors_for_frame
  on equal sizes), a zero-filled SequenceControlSet, a MacroBlockD carrying the job's four edges, src_ptr_2b = NULL, is_masked_compound = 0,
  ConvolveParams from get_conv_params_no_round with the 128-wide CONV_BUF_TYPE buffer; before a compound's second reference do_average = 1,
  fwd_offset / bck_offset and use_dist_wtd_comp_avg = use_jnt_comp_avg = comp_mode, as svt_aom_inter_prediction does.  Clamp, position, filter
  choice, dispatch and the 16-bit path are then the reference's own.
Whatever else the link still wants gets a stand-in that aborts (svt_aom_pack2d_src, which only the split 8 + 2-bit layout reaches).  The fixture holds numbers only: per
batch a CRC-32 per job of the predicted block (per filter pair for the exhaustive sweeps) and the full block of a sample of jobs.  --check
recomputes everything and compares it with the committed file instead of writing it; either way the restatement of tests/inter_pred_cases.py
is compared with the reference on every job, every job's reads are checked to lie inside its padded plane, and the coverage conditions are
asserted on the reference's results (the call counts of the sixteen functions are the harness's own)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import inter_pred_cases as ip  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "sequence_control_set.h"
#include "enc_inter_prediction.h"
#include "inter_prediction.h"
#include "convolve.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"

static uint32_t g_count[16]; /* [hbd][compound][variant = (sx != 0) + 2 * (sy != 0)] */
#define W8(idx, fn)                                                                                                                         \
    static void w8_##idx(const uint8_t *src, int32_t ss, uint8_t *dst, int32_t ds, int32_t w, int32_t h, InterpFilterParams *fx,           \
                         InterpFilterParams *fy, const int32_t sx, const int32_t sy, ConvolveParams *cp) {                                  \
        g_count[idx]++;                                                                                                                     \
        fn(src, ss, dst, ds, w, h, fx, fy, sx, sy, cp);                                                                                     \
    }
#define W16(idx, fn)                                                                                                                        \
    static void w16_##idx(const uint16_t *src, int32_t ss, uint16_t *dst, int32_t ds, int32_t w, int32_t h, const InterpFilterParams *fx,  \
                          const InterpFilterParams *fy, const int32_t sx, const int32_t sy, ConvolveParams *cp, int32_t bd) {               \
        g_count[8 + idx]++;                                                                                                                 \
        fn(src, ss, dst, ds, w, h, fx, fy, sx, sy, cp, bd);                                                                                 \
    }
W8(0, svt_av1_convolve_2d_copy_sr_c) W8(1, svt_av1_convolve_x_sr_c) W8(2, svt_av1_convolve_y_sr_c) W8(3, svt_av1_convolve_2d_sr_c)
W8(4, svt_av1_jnt_convolve_2d_copy_c) W8(5, svt_av1_jnt_convolve_x_c) W8(6, svt_av1_jnt_convolve_y_c) W8(7, svt_av1_jnt_convolve_2d_c)
W16(0, svt_av1_highbd_convolve_2d_copy_sr_c) W16(1, svt_av1_highbd_convolve_x_sr_c) W16(2, svt_av1_highbd_convolve_y_sr_c)
W16(3, svt_av1_highbd_convolve_2d_sr_c) W16(4, svt_av1_highbd_jnt_convolve_2d_copy_c) W16(5, svt_av1_highbd_jnt_convolve_x_c)
W16(6, svt_av1_highbd_jnt_convolve_y_c) W16(7, svt_av1_highbd_jnt_convolve_2d_c)

static SequenceControlSet *g_scs;
static ScaleFactors        g_sf;
static ConvBufType         g_tmp[128 * 128] __attribute__((aligned(32)));

int harness_init(void) {
    svt_aom_convolve[0][0][0] = w8_0; svt_aom_convolve[1][0][0] = w8_1; svt_aom_convolve[0][1][0] = w8_2; svt_aom_convolve[1][1][0] = w8_3;
    svt_aom_convolve[0][0][1] = w8_4; svt_aom_convolve[1][0][1] = w8_5; svt_aom_convolve[0][1][1] = w8_6; svt_aom_convolve[1][1][1] = w8_7;
    svt_aom_convolveHbd[0][0][0] = w16_0; svt_aom_convolveHbd[1][0][0] = w16_1; svt_aom_convolveHbd[0][1][0] = w16_2; svt_aom_convolveHbd[1][1][0] = w16_3;
    svt_aom_convolveHbd[0][0][1] = w16_4; svt_aom_convolveHbd[1][0][1] = w16_5; svt_aom_convolveHbd[0][1][1] = w16_6; svt_aom_convolveHbd[1][1][1] = w16_7;
    memset(g_count, 0, sizeof(g_count));
    if (!g_scs) g_scs = calloc(1, sizeof(*g_scs));
    if (!g_scs) return 1;
    svt_av1_setup_scale_factors_for_frame(&g_sf, 192, 128, 192, 128);
    return av1_is_scaled(&g_sf) ? 2 : 0;
}
void harness_counts(uint32_t *out) { memcpy(out, g_count, sizeof(g_count)); }
/* p: width, height, org_x, org_y, filter_x, filter_y, n_refs, comp_mode, fwd_offset, bck_offset, mv0 row, mv0 col, mv1 row, mv1 col,
 *    the four edges (left, right, top, bottom), ss_x, ss_y, bit_depth, visible width, visible height.
 * src0 / src1: the picture's sample (0, 0) in the (padded) reference planes; strides in samples. */
void harness_predict(const int *p, uint8_t *src0, uint8_t *src1, int src_stride, uint8_t *dst, int dst_stride) {
    const int      bd = p[20], is16 = bd > 8, comp = p[6] == 2;
    MacroBlockD    xd;
    ConvolveParams cp = get_conv_params_no_round(0, 0, 0, g_tmp, 128, comp, bd);
    InterpFilters  filters = av1_make_interp_filters((InterpFilter)p[5], (InterpFilter)p[4]);
    memset(&xd, 0, sizeof(xd));
    xd.mb_to_left_edge = p[14]; xd.mb_to_right_edge = p[15]; xd.mb_to_top_edge = p[16]; xd.mb_to_bottom_edge = p[17];
    for (int k = 0; k < p[6]; k++) {
        MV mv;
        mv.row = (int16_t)p[10 + 2 * k]; mv.col = (int16_t)p[11 + 2 * k];
        if (k) {
            cp.do_average = 1; cp.fwd_offset = p[8]; cp.bck_offset = p[9];
            cp.use_dist_wtd_comp_avg = p[7]; cp.use_jnt_comp_avg = p[7];
        }
        svt_aom_enc_make_inter_predictor(g_scs, k ? src1 : src0, NULL, dst, (int16_t)p[3], (int16_t)p[2], mv, &g_sf, &cp, filters, NULL, NULL,
                                         (uint16_t)p[21], (uint16_t)p[22], (uint8_t)p[0], (uint8_t)p[1], BLOCK_8X8, &xd, src_stride, dst_stride,
                                         p[18] ? 1 : 0, (uint32_t)p[19], (uint32_t)p[18], (uint8_t)bd, 0, 0, (uint8_t)is16);
    }
}
"""
SOURCES = ["Codec/inter_prediction.c", "Codec/enc_inter_prediction.c", "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]


def build(ref, tmp):
    """Symbols the link still wants get stand-ins: the SIMD bodies the rtcd files name and what the rest of the compiled sources calls."""
    L = refbuild.build(ref, tmp, "interpredref", SOURCES, [("harness", HARNESS)], standins=True)
    L.harness_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.harness_predict.restype = None
    L.harness_counts.argtypes = [C.c_void_p]
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def reference_block(L, b, planes, j):
    bd, ss = b["bit_depth"], b["ss"]
    dt = np.uint16 if bd > 8 else np.uint8
    w, h = int(j["width"]), int(j["height"])
    comp = int(j["ref"][1]) != ip.NO_REF
    pw, ph, _ = ip.plane_dims(ss)
    mvs = [ip.job_mv(j, k, b["mv_array"]) for k in range(2)]
    p = np.array([w, h, j["org_x"], j["org_y"], j["filter_x"], j["filter_y"], 2 if comp else 1, j["comp_mode"], j["fwd_offset"], j["bck_offset"],
                  mvs[0][0], mvs[0][1], mvs[1][0], mvs[1][1], j["mb_to_left_edge"], j["mb_to_right_edge"], j["mb_to_top_edge"], j["mb_to_bottom_edge"],
                  ss, ss, bd, pw, ph], np.int32)
    srcs = []
    for k in range(2):
        pl, ox, oy = planes[int(j["ref"][k]) if (k == 0 or comp) else int(j["ref"][0])]
        assert pl.dtype == dt
        srcs.append(pl.ctypes.data + (oy * pl.shape[1] + ox) * pl.itemsize)
    stride = planes[0][0].shape[1]
    assert all(pl.shape[1] == stride for pl, _, _ in planes)
    out = np.full((h, w), 0xA5A5 if bd > 8 else 0xA5, dt)
    L.harness_predict(p.ctypes.data, srcs[0], srcs[1], stride, out.ctypes.data, w)
    return out.astype(np.uint16)


def generate(L):
    out, records, mismatch = {}, [], []
    samples = {(name, i): key for key, name, i in ip.sample_jobs()}
    n_jobs = 0
    for name in ip.batch_names():
        b = ip.batch(name)
        planes = ip.batch_planes(b)
        want, events = ip.restated(name)
        got = []
        for i, j in enumerate(b["jobs"]):
            if not events[i]["inside"]:
                raise RuntimeError(f"{name} job {i}: the block plus the filter reach leaves the padded plane")
            blk = reference_block(L, b, planes, j)
            if not np.array_equal(blk, want[i]):
                mismatch.append((name, i, int(np.count_nonzero(blk != want[i]))))
            got.append(blk)
            records.append((b["bit_depth"], j, events[i]))
            if (name, i) in samples:
                out[samples[(name, i)]] = blk
        out[f"crc_{name}"] = ip.batch_crcs(name, got)
        n_jobs += len(got)
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    missing = ip.coverage_missing(records)
    counts = np.zeros(16, np.uint32)
    L.harness_counts(counts.ctypes.data)
    missing += [f"the reference never called convolve function {k} ([hbd][compound][variant])" for k in range(16) if counts[k] == 0]
    if missing:
        raise RuntimeError(f"coverage conditions the reference's results do not meet: {missing}")
    print(f"{n_jobs} jobs, none left out; calls per convolve function [hbd][compound][variant]: {counts.tolist()}")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {ip.GOLDEN: generate}, save=refbuild.savez)
