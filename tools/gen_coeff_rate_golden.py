#!/usr/bin/env python3
"""Writes tests/golden/coeff_rate.npz: the reference encoder's own rate tables and svt_av1_cost_coeffs_txb results on the cases of tests/coeff_rate_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles the reference's Codec/rd_cost.c, Codec/md_rate_estimation.c, Codec/cabac_context_model.c, Codec/aom_dsp_rtcd.c and
C_DEFAULT/encode_txb_ref_c.c where they lie, together with a small harness of its own, into a temporary directory outside the tree (gcc, -O2),
links with --gc-sections and a version script that exports the harness alone, and
  sets svt_av1_txb_init_levels / svt_av1_get_nz_map_contexts to their _c bodies,
  fills a FRAME_CONTEXT with svt_av1_default_coef_probs(fc, qindex) + svt_aom_init_mode_probs, for every qindex of QINDEXES,
  derives the tables with svt_aom_estimate_syntax_rate + svt_aom_estimate_coefficients_rate,
  calls svt_av1_cost_coeffs_txb (allow_update_cdf = 0) on a zeroed ModeDecisionContext that carries md_rate_est_ctx, mds_fast_coeff_est_level
  and mds_subres_step, for every job of every case and every (level, step) of RATE_VARIANTS.
The four symbols the link still wants (svt_memcpy, svt_memcpy_c, svt_aom_filter_intra_allowed_bsize, svt_aom_get_wedge_params_bits) are stand-ins
in the harness: they feed syntax tables this fixture does not hold.  The fixture holds numbers only: the four table members the function reads,
the jobs, their qcoeff and eob, and the reference's costs.  --check recomputes everything and compares it with the committed file instead of
writing it; either way the restatement of tests/coeff_rate_cases.py is compared with the reference on every job."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import coeff_rate_cases as cr  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "md_process.h"
#include "mode_decision.h"
#include "rd_cost.h"
#include "md_rate_estimation.h"
#include "cabac_context_model.h"
#include "aom_dsp_rtcd.h"

void (*svt_memcpy)(void *dst_ptr, void const *src_ptr, size_t size);
void svt_memcpy_c(void *dst_ptr, void const *src_ptr, size_t size) { memcpy(dst_ptr, src_ptr, size); }
int  svt_aom_filter_intra_allowed_bsize(BlockSize bs) { (void)bs; return 0; }
int  svt_aom_get_wedge_params_bits(BlockSize bsize) { (void)bsize; return 0; }

static MdRateEstimationContext     g_rate;
static FRAME_CONTEXT               g_fc;
static ModeDecisionContext        *g_ctx;
static ModeDecisionCandidateBuffer g_bf;
static ModeDecisionCandidate       g_cand;

int harness_init(int qindex) {
    svt_memcpy                  = svt_memcpy_c;
    svt_av1_txb_init_levels     = svt_av1_txb_init_levels_c;
    svt_av1_get_nz_map_contexts = svt_av1_get_nz_map_contexts_c;
    memset(&g_rate, 0, sizeof(g_rate));
    memset(&g_fc, 0, sizeof(g_fc));
    svt_av1_default_coef_probs(&g_fc, qindex);
    svt_aom_init_mode_probs(&g_fc);
    svt_aom_estimate_syntax_rate(&g_rate, false, 0, 0, 0, 0, &g_fc);
    svt_aom_estimate_coefficients_rate(&g_rate, &g_fc);
    if (!g_ctx) g_ctx = calloc(1, sizeof(*g_ctx));
    if (!g_ctx) return 1;
    g_ctx->md_rate_est_ctx = &g_rate;
    g_bf.cand              = &g_cand;
    return 0;
}
/* member: 0 coeff_fac_bits, 1 eob_frac_bits, 2 intra_tx_type_fac_bits, 3 inter_tx_type_fac_bits; returns the byte count */
size_t harness_table(int member, void *out) {
    const void *src;
    size_t      n;
    switch (member) {
    case 0: src = g_rate.coeff_fac_bits; n = sizeof(g_rate.coeff_fac_bits); break;
    case 1: src = g_rate.eob_frac_bits; n = sizeof(g_rate.eob_frac_bits); break;
    case 2: src = g_rate.intra_tx_type_fac_bits; n = sizeof(g_rate.intra_tx_type_fac_bits); break;
    default: src = g_rate.inter_tx_type_fac_bits; n = sizeof(g_rate.inter_tx_type_fac_bits); break;
    }
    if (out) memcpy(out, src, n);
    return n;
}
uint64_t harness_cost(const int32_t *qcoeff, int eob, int plane, int tx_size, int tx_type, int txb_skip_ctx, int dc_sign_ctx, int is_inter,
                      int intra_dir, int reduced, int fast_level, int subres_step) {
    g_ctx->mds_fast_coeff_est_level = (uint8_t)fast_level;
    g_ctx->mds_subres_step          = (uint8_t)subres_step;
    g_cand.pred_mode                = is_inter ? NEARESTMV : (PredictionMode)intra_dir;
    g_cand.filter_intra_mode        = FILTER_INTRA_MODES;
    return svt_av1_cost_coeffs_txb(g_ctx, 0, NULL, &g_bf, qcoeff, (uint16_t)eob, (PlaneType)plane, (TxSize)tx_size, (TxType)tx_type, (int16_t)txb_skip_ctx,
                                   (int16_t)dc_sign_ctx, reduced != 0);
}
"""
SOURCES = ["Codec/rd_cost.c", "Codec/md_rate_estimation.c", "Codec/cabac_context_model.c", "Codec/aom_dsp_rtcd.c", "C_DEFAULT/encode_txb_ref_c.c"]
MEMBERS = list(cr.TABLE_SHAPES)


def build(ref, tmp):
    L = refbuild.build(ref, tmp, "coeffrateref", SOURCES, [("harness", HARNESS)])
    L.harness_table.restype = C.c_size_t
    L.harness_table.argtypes = [C.c_int, C.c_void_p]
    L.harness_cost.restype = C.c_uint64
    L.harness_cost.argtypes = [C.c_void_p] + [C.c_int] * 11
    return L


def generate(L):
    cases = cr.build_cases()
    out = cr.cases_to_arrays(cases)
    out["qindex"] = np.array(cr.QINDEXES, np.int32)
    n_jobs = len(out["eob"])
    bits = np.zeros((len(cr.RATE_VARIANTS), n_jobs), np.uint64)
    mismatch = []
    for k, qindex in enumerate(cr.QINDEXES):
        if L.harness_init(int(qindex)):
            raise RuntimeError("harness_init failed")
        members = {}
        for m, name in enumerate(MEMBERS):
            a = np.zeros(cr.TABLE_SHAPES[name], np.int32)
            if L.harness_table(m, None) != a.nbytes:
                raise RuntimeError(f"{name}: the reference holds {L.harness_table(m, None)} bytes, the restatement expects {a.nbytes}")
            L.harness_table(m, a.ctypes.data)
            members[name] = out[f"{name}_{k}"] = a
        T = cr.Tables(**members)
        j0 = 0
        for c in cases:
            n = len(c["jobs"])
            if c["table"] == k:
                q = np.ascontiguousarray(c["qcoeff"], np.int32)
                for i, (j, e) in enumerate(zip(c["jobs"], c["eob"])):
                    if e == 0:
                        continue  # the reference's function is not called with eob 0 (rd_cost.c:433)
                    for v, (fast, sub) in enumerate(cr.RATE_VARIANTS):
                        bits[v, j0 + i] = L.harness_cost(q[i].ctypes.data, int(e), c["plane"], c["tx_size"], int(j["tx_type"]), int(j["txb_skip_ctx"]),
                                                         int(j["dc_sign_ctx"]), int(j["is_inter"]), int(j["intra_dir"]), c["reduced"], fast, sub)
                raw, _ = cr.run_case(T, c)
                for v in range(len(cr.RATE_VARIANTS)):
                    for i in range(n):
                        if c["eob"][i] and raw[v][i] != int(bits[v, j0 + i]):
                            mismatch.append((c["tx_size"], c["plane"], c["reduced"], i, cr.RATE_VARIANTS[v], raw[v][i], int(bits[v, j0 + i])))
            j0 += n
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference on {len(mismatch)} results, first: {mismatch[:5]}")
    out["bits"] = bits
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {cr.GOLDEN: generate}, save=refbuild.savez, wrote=refbuild.wrote_shapes)
