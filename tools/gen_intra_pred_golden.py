#!/usr/bin/env python3
"""Writes tests/golden/intra_pred.npz: the reference encoder's own build_intra_predictors / build_intra_predictors_high results on the cases of
tests/intra_pred_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles a small harness of its own into a temporary directory outside the tree (gcc, -O2).  The harness #includes the
reference's Codec/enc_intra_prediction.c where it lies, because the two functions are static, and is linked with Codec/intra_prediction.c,
C_DEFAULT/intra_prediction_c.c, C_DEFAULT/filterintra_c.c, the files that hold svt_memcpy_c and svt_aom_memset16, and the rtcd files, with --gc-sections and a version script that exports the harness
alone; whatever else the link still wants gets a stand-in that aborts.  The harness
  sets every rtcd pointer to its _c body (svt_aom_setup_common_rtcd_internal and svt_aom_setup_rtcd_internal without a CPU flag) and lets the
  reference's svt_aom_init_intra_predictors_internal fill svt_aom_dc_pred / svt_aom_eb_pred and their 16-bit tables from them,
  puts every entry of those tables and the pointer-level entries (edge filter, upsampling, the three zones, filter-intra; both depths) behind
  wrappers that count their calls (the harness generates one wrapper per table entry),
  calls the two static functions themselves, with a MacroBlockD whose above_mbmi is a SMOOTH_PRED block (filt_type 1) or absent (0).
The neighbours are handed over as the reference takes them -- a row whose index -1 is the corner and a contiguous left column -- holding exactly
the samples tests/intra_pred_cases.py's job_reads names and a poison value everywhere else, so a read beyond them shows as a mismatch.  The
fixture holds numbers only: per batch a CRC-32 per job of the predicted block, and the full block of a sample of jobs.  --check recomputes
everything and compares it with the committed file instead of writing it; either way the restatement is compared with the reference on every
job, every job's reads are checked to lie inside the neighbour plane, and the coverage conditions are asserted on the reference's results."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import intra_pred_cases as ic  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include <stdlib.h>
#include <string.h>
#include "enc_intra_prediction.c"
#include "aom_dsp_rtcd.h"

void svt_aom_init_intra_predictors_internal(void);
void svt_aom_init_intra_dc_predictors_c_internal(void);

/* 0 filter edge, 1 upsample, 2 z1, 3 z2, 4 z3, 5 filter-intra; + 6 for the 16-bit forms, of which the upsampling (7) and filter-intra (11)
 * are called by name, not through a pointer, and are not counted */
static uint32_t g_count[12];
static void w_fe(uint8_t *p, int32_t sz, int32_t s) { g_count[0]++; svt_av1_filter_intra_edge_c(p, sz, s); }
static void w_up(uint8_t *p, int32_t sz) { g_count[1]++; svt_av1_upsample_intra_edge_c(p, sz); }
static void w_z1(uint8_t *d, ptrdiff_t s, int32_t bw, int32_t bh, const uint8_t *a, const uint8_t *l, int32_t ua, int32_t dx, int32_t dy) {
    g_count[2]++; svt_av1_dr_prediction_z1_c(d, s, bw, bh, a, l, ua, dx, dy); }
static void w_z2(uint8_t *d, ptrdiff_t s, int32_t bw, int32_t bh, const uint8_t *a, const uint8_t *l, int32_t ua, int32_t ul, int32_t dx, int32_t dy) {
    g_count[3]++; svt_av1_dr_prediction_z2_c(d, s, bw, bh, a, l, ua, ul, dx, dy); }
static void w_z3(uint8_t *d, ptrdiff_t s, int32_t bw, int32_t bh, const uint8_t *a, const uint8_t *l, int32_t ul, int32_t dx, int32_t dy) {
    g_count[4]++; svt_av1_dr_prediction_z3_c(d, s, bw, bh, a, l, ul, dx, dy); }
static void w_fi(uint8_t *d, ptrdiff_t s, TxSize tx, const uint8_t *a, const uint8_t *l, int32_t m) {
    g_count[5]++; svt_av1_filter_intra_predictor_c(d, s, tx, a, l, m); }
static void h_fe(uint16_t *p, int32_t sz, int32_t s) { g_count[6]++; svt_av1_filter_intra_edge_high_c(p, sz, s); }
static void h_z1(uint16_t *d, ptrdiff_t s, int32_t bw, int32_t bh, const uint16_t *a, const uint16_t *l, int32_t ua, int32_t dx, int32_t dy, int32_t bd) {
    g_count[8]++; svt_av1_highbd_dr_prediction_z1_c(d, s, bw, bh, a, l, ua, dx, dy, bd); }
static void h_z2(uint16_t *d, ptrdiff_t s, int32_t bw, int32_t bh, const uint16_t *a, const uint16_t *l, int32_t ua, int32_t ul, int32_t dx, int32_t dy,
                 int32_t bd) { g_count[9]++; svt_av1_highbd_dr_prediction_z2_c(d, s, bw, bh, a, l, ua, ul, dx, dy, bd); }
static void h_z3(uint16_t *d, ptrdiff_t s, int32_t bw, int32_t bh, const uint16_t *a, const uint16_t *l, int32_t ul, int32_t dx, int32_t dy, int32_t bd) {
    g_count[10]++; svt_av1_highbd_dr_prediction_z3_c(d, s, bw, bh, a, l, ul, dx, dy, bd); }

/* the predictor tables: every entry the reference's init has set goes behind a wrapper that counts by [16-bit][DC variant left * 2 + top | 4 + mode] */
static uint32_t        g_tab[2][4 + INTRA_MODES];
static IntraPredFn     o_dc[2][2][TX_SIZES_ALL], o_eb[INTRA_MODES][TX_SIZES_ALL];
static IntraHighPredFn oh_dc[2][2][TX_SIZES_ALL], oh_eb[INTRA_MODES][TX_SIZES_ALL];
@TABLE_WRAPPERS@
static MbModeInfo g_smooth;

int harness_init(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0);
    svt_aom_init_intra_dc_predictors_c_internal();
    svt_aom_init_intra_predictors_internal();
    svt_av1_filter_intra_edge = w_fe; svt_av1_upsample_intra_edge = w_up; svt_av1_dr_prediction_z1 = w_z1; svt_av1_dr_prediction_z2 = w_z2;
    svt_av1_dr_prediction_z3 = w_z3; svt_av1_filter_intra_predictor = w_fi; svt_av1_filter_intra_edge_high = h_fe;
    svt_av1_highbd_dr_prediction_z1 = h_z1; svt_av1_highbd_dr_prediction_z2 = h_z2; svt_av1_highbd_dr_prediction_z3 = h_z3;
    for (int tx = 0; tx < TX_SIZES_ALL; tx++) {
        for (int v = 0; v < 4; v++) {
            o_dc[v >> 1][v & 1][tx] = svt_aom_dc_pred[v >> 1][v & 1][tx]; oh_dc[v >> 1][v & 1][tx] = svt_aom_dc_pred_high[v >> 1][v & 1][tx];
            if (!o_dc[v >> 1][v & 1][tx] || !oh_dc[v >> 1][v & 1][tx]) return 3;
            svt_aom_dc_pred[v >> 1][v & 1][tx] = w_dc[v][tx]; svt_aom_dc_pred_high[v >> 1][v & 1][tx] = wh_dc[v][tx];
        }
        for (int m = 0; m < INTRA_MODES; m++) {
            o_eb[m][tx] = svt_aom_eb_pred[m][tx]; oh_eb[m][tx] = svt_aom_pred_high[m][tx];
            if (o_eb[m][tx]) svt_aom_eb_pred[m][tx] = w_eb[m][tx];
            if (oh_eb[m][tx]) svt_aom_pred_high[m][tx] = wh_eb[m][tx];
        }
    }
    memset(g_count, 0, sizeof(g_count));
    memset(g_tab, 0, sizeof(g_tab));
    memset(&g_smooth, 0, sizeof(g_smooth));
    g_smooth.block_mi.mode = SMOOTH_PRED;
    return 0;
}
void harness_counts(uint32_t *out) { memcpy(out, g_count, sizeof(g_count)); memcpy(out + 12, g_tab, sizeof(g_tab)); }
/* p: bit_depth, mode, angle_delta, filter_intra_mode, tx_size, disable_edge_filter, n_top_px, n_topright_px, n_left_px, n_bottomleft_px, filt_type.
 * top: above_ref (top[-1] the corner); left: left_ref, contiguous. */
void harness_predict(const int *p, void *top, void *left, void *dst, int dst_stride) {
    MacroBlockD xd;
    memset(&xd, 0, sizeof(xd));
    xd.above_mbmi = p[10] ? &g_smooth : NULL;
    if (p[0] > 8) {
        build_intra_predictors_high(&xd, (uint16_t *)top, (uint16_t *)left, (uint16_t *)dst, dst_stride, (PredictionMode)p[1], p[2], (FilterIntraMode)p[3],
                                    (TxSize)p[4], p[5], p[6], p[7], p[8], p[9], 0, p[0]);
    } else
        build_intra_predictors(&xd, (uint8_t *)top, (uint8_t *)left, (uint8_t *)dst, dst_stride, (PredictionMode)p[1], p[2], (FilterIntraMode)p[3], (TxSize)p[4],
                               p[5], p[6], p[7], p[8], p[9], 0);
}
"""


def table_wrappers():
    """the C text of one counting wrapper per entry of svt_aom_dc_pred / svt_aom_eb_pred and their 16-bit tables, and the tables of the wrappers"""
    out = []
    for hbd, (px, fn, extra_p, extra_a) in enumerate((("uint8_t", "", "", ""), ("uint16_t", "h", ", int32_t bd", ", bd"))):
        sig = f"({px} *d, ptrdiff_t s, const {px} *a, const {px} *l{extra_p})"
        for v in range(4):
            for tx in range(ic.N_TX):
                out.append(f"static void w{fn}_dc_{v}_{tx}{sig} {{ g_tab[{hbd}][{v}]++; o{fn}_dc[{v >> 1}][{v & 1}][{tx}](d, s, a, l{extra_a}); }}")
        for m in range(13):
            for tx in range(ic.N_TX):
                out.append(f"static void w{fn}_eb_{m}_{tx}{sig} {{ g_tab[{hbd}][{4 + m}]++; o{fn}_eb[{m}][{tx}](d, s, a, l{extra_a}); }}")
        typ = "IntraHighPredFn" if hbd else "IntraPredFn"
        out.append(f"static const {typ} w{fn}_dc[4][TX_SIZES_ALL] = {{" + ", ".join("{" + ", ".join(f"w{fn}_dc_{v}_{tx}" for tx in range(ic.N_TX)) + "}" for v in range(4)) + "};")
        out.append(f"static const {typ} w{fn}_eb[INTRA_MODES][TX_SIZES_ALL] = {{" + ", ".join("{" + ", ".join(f"w{fn}_eb_{m}_{tx}" for tx in range(ic.N_TX)) + "}" for m in range(13)) + "};")
    return "\n".join(out)


SOURCES = ["Codec/intra_prediction.c", "C_DEFAULT/intra_prediction_c.c", "C_DEFAULT/filterintra_c.c", "C_DEFAULT/picture_operators_c.c",
           "Codec/cdef.c", "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]


def build(ref, tmp):
    """The stand-ins are the SIMD bodies the rtcd files name, never chosen without a CPU flag, and what the rest of enc_intra_prediction.c calls."""
    L = refbuild.build(ref, tmp, "intrapredref", SOURCES, [("harness", HARNESS.replace("@TABLE_WRAPPERS@", table_wrappers()))], standins=True)
    L.harness_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.harness_predict.restype = None
    L.harness_counts.argtypes = [C.c_void_p]
    if L.harness_init():
        raise RuntimeError("harness_init failed")
    return L


def reference_block(L, b, nbr, j):
    bd = b["bit_depth"]
    dt = np.uint16 if bd > 8 else np.uint8
    poison = 0x2C5 if bd > 8 else 0xC5
    w, h = ic.TX_W[int(j["tx_size"])], ic.TX_H[int(j["tx_size"])]
    a_n, l_n, corner = ic.job_reads(j)
    x0, y0 = int(j["nbr_x"]), int(j["nbr_y"])
    top, left = np.full(32 + 160, poison, dt), np.full(32 + 160, poison, dt)
    if a_n:
        top[32:32 + a_n] = nbr[y0 - 1, x0:x0 + a_n]
    if corner:
        top[31] = nbr[y0 - 1, x0 - 1]
    if l_n:
        left[32:32 + l_n] = nbr[y0:y0 + l_n, x0 - 1]
    p = np.array([bd, j["mode"], j["angle_delta"], j["filter_intra_mode"], j["tx_size"], b["disable_edge_filter"], j["n_top_px"], j["n_topright_px"],
                  j["n_left_px"], j["n_bottomleft_px"], j["filt_type"]], np.int32)
    out = np.full((h, w), 0xA5A5 if bd > 8 else 0xA5, dt)
    L.harness_predict(p.ctypes.data, top.ctypes.data + 32 * top.itemsize, left.ctypes.data + 32 * left.itemsize, out.ctypes.data, w)
    return out.astype(np.uint16)


def generate(L):
    out, records, mismatch = {}, [], []
    samples = {(name, i): key for key, name, i in ic.sample_jobs()}
    n_jobs = 0
    for name in ic.batch_names():
        b = ic.batch(name)
        nbr = ic.plane(b["plane"], b["bit_depth"])
        want, events = ic.restated(name)
        got = []
        for i, j in enumerate(b["jobs"]):
            if not ic.reads_inside(j, nbr.shape[1], nbr.shape[0]):
                raise RuntimeError(f"{name} job {i}: a read leaves the neighbour plane")
            blk = reference_block(L, b, nbr, j)
            if not np.array_equal(blk, want[i]):
                mismatch.append((name, i, int(np.count_nonzero(blk != want[i]))))
            got.append(blk)
            records.append((b["bit_depth"], j, events[i]))
            if (name, i) in samples:
                out[samples[(name, i)]] = blk
        out[f"crc_{name}"] = ic.batch_crcs(got)
        n_jobs += len(got)
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    missing = ic.coverage_missing(records)
    counts = np.zeros(12 + 2 * 17, np.uint32)
    L.harness_counts(counts.ctypes.data)
    counts, tab = counts[:12], counts[12:].reshape(2, 17)
    table_modes = (ic.V_PRED, ic.H_PRED, ic.SMOOTH_PRED, ic.SMOOTH_V_PRED, ic.SMOOTH_H_PRED, ic.PAETH_PRED)
    missing += [f"the reference never called DC variant {v} (left * 2 + top) at {8 + 8 * h} bits" for h in range(2) for v in range(4) if tab[h][v] == 0]
    missing += [f"the reference never called the table predictor of mode {m} at {8 + 8 * h} bits" for h in range(2) for m in table_modes if tab[h][4 + m] == 0]
    missing += [f"the reference never called entry {k} (filter edge, upsample, z1, z2, z3, filter-intra; + 6 at 16 bits)" for k in range(12) if counts[k] == 0 and k not in (7, 11)]
    if missing:
        raise RuntimeError(f"coverage conditions the reference's results do not meet: {missing}")
    print(f"{n_jobs} jobs, none left out; calls per entry (filter edge, upsample, z1, z2, z3, filter-intra; 8-bit then 16-bit): {counts.tolist()}; per table entry (the four DC variants, then the 13 modes; 8-bit, 16-bit): {tab.tolist()}")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {ic.GOLDEN: generate}, save=refbuild.savez)
