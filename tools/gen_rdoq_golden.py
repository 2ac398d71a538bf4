#!/usr/bin/env python3
"""Writes tests/golden/rdoq.npz: the reference encoder's own svt_aom_quantize_inv_quantize results (RDOQ on) on the cases of tests/rdoq_cases.py.

Run by hand on a machine that has the reference's sources (--ref: the root of its source tree); never by the tests, build(), smoke() or
bench.py.  It compiles the reference's Codec/rd_cost.c, Codec/md_rate_estimation.c, Codec/cabac_context_model.c, Codec/aom_dsp_rtcd.c and
Codec/common_dsp_rtcd.c where they lie, together with a small harness of its own that reaches the static functions by #include-ing
Codec/full_loop.c, into a temporary directory outside the tree (gcc, -O2), links with --gc-sections and a version script that exports the harness
alone, and
  sets the quantizer, svt_av1_txb_init_levels and svt_av1_compute_cul_level pointers to their _c bodies,
  derives the rate tables as tools/gen_coeff_rate_golden.py does (qindex 40 and 200) and compares them with golden/coeff_rate.npz,
  zero-fills PictureControlSet / SequenceControlSet / PictureParentControlSet / EncodeContext / ModeDecisionContext and sets the fields the
  function reads: the quantizer rows of tests/rd_cases.py:quant_rows() at q_index 0..2 (delta_q_present = 1, so the qindex argument selects the
  row), rdoq_level = 1, fp_q_y = fp_q_uv = 1, satd_factor = 255, early_exit_th = 0, the case's rdoq_ctrls, static_config.sharpness, the
  quantization matrix pointers; a job's `sharp` flag is passed as static_config.sharp_tx with sharpness_ctrls.rdoq = 1,
  calls svt_aom_quantize_inv_quantize itself (is_encode_pass = 0) for every job: the fp quantizer, both gates, the fast trim,
  svt_av1_optimize_b, the re-quantization behind the eob_th gate and the cul_level are the reference's own; and the two quantizer facades
  alone, to compare the CPU oracle's quantizations (the inputs the tests regenerate) with the reference's.
The four symbols the link still wants (svt_memcpy_c, svt_aom_filter_intra_allowed_bsize, svt_aom_get_wedge_params_bits,
svt_av1_is_lossless_segment = false: lossless segments are not listed as jobs) are stand-ins in the harness.  The fixture holds numbers only: per
case the controls, per job the reference's qcoeff (int16), eob, cul_level and the status the restatement assigns, per case a CRC of the
reference's dqcoeff.  --check recomputes everything and compares it with the committed file instead of writing it; either way the restatement
of tests/rdoq_cases.py is compared with the reference on every job, and the coverage conditions are asserted on the reference's results."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import coeff_rate_cases as cr  # noqa: E402
import rdoq_cases as rq  # noqa: E402
import refbuild  # noqa: E402

HARNESS = r"""
#include <stdlib.h>
#include <string.h>
#include "full_loop.c"
#include "md_rate_estimation.h"
#include "cabac_context_model.h"

void svt_memcpy_c(void *dst_ptr, void const *src_ptr, size_t size) { memcpy(dst_ptr, src_ptr, size); }
int  svt_aom_filter_intra_allowed_bsize(BlockSize bs) { (void)bs; return 0; }
int  svt_aom_get_wedge_params_bits(BlockSize bsize) { (void)bsize; return 0; }
bool svt_av1_is_lossless_segment(PictureControlSet *pcs, int8_t segment_id) { (void)pcs; (void)segment_id; return false; }
static uint32_t h_log2f(uint32_t x) { uint32_t l = 0; while (x >>= 1) l++; return l; }

static MdRateEstimationContext  g_rate;
static FRAME_CONTEXT            g_fc;
static PictureControlSet       *g_pcs;
static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_ppcs;
static EncodeContext           *g_enc;
static ModeDecisionContext     *g_ctx;

int harness_init(int qindex) {
    svt_memcpy                    = svt_memcpy_c;
    svt_av1_txb_init_levels       = svt_av1_txb_init_levels_c;
    svt_av1_compute_cul_level     = svt_av1_compute_cul_level_c;
    svt_log2f                     = h_log2f;
    svt_aom_quantize_b            = svt_aom_quantize_b_c_ii;
    svt_aom_highbd_quantize_b     = svt_aom_highbd_quantize_b_c;
    svt_av1_quantize_b_qm         = svt_aom_quantize_b_c_ii;
    svt_av1_highbd_quantize_b_qm  = svt_aom_highbd_quantize_b_c;
    svt_av1_quantize_fp           = svt_av1_quantize_fp_c;
    svt_av1_quantize_fp_32x32     = svt_av1_quantize_fp_32x32_c;
    svt_av1_quantize_fp_64x64     = svt_av1_quantize_fp_64x64_c;
    svt_av1_quantize_fp_qm        = svt_av1_quantize_fp_qm_c;
    svt_av1_highbd_quantize_fp    = svt_av1_highbd_quantize_fp_c;
    svt_av1_highbd_quantize_fp_qm = svt_av1_highbd_quantize_fp_qm_c;
    memset(&g_rate, 0, sizeof(g_rate));
    memset(&g_fc, 0, sizeof(g_fc));
    svt_av1_default_coef_probs(&g_fc, qindex);
    svt_aom_init_mode_probs(&g_fc);
    svt_aom_estimate_syntax_rate(&g_rate, false, 0, 0, 0, 0, &g_fc);
    svt_aom_estimate_coefficients_rate(&g_rate, &g_fc);
    if (!g_pcs) {
        g_pcs = calloc(1, sizeof(*g_pcs)); g_scs = calloc(1, sizeof(*g_scs)); g_ppcs = calloc(1, sizeof(*g_ppcs));
        g_enc = calloc(1, sizeof(*g_enc)); g_ctx = calloc(1, sizeof(*g_ctx));
        if (!g_pcs || !g_scs || !g_ppcs || !g_enc || !g_ctx) return 1;
        g_ctx->blk_ptr  = calloc(1, sizeof(*g_ctx->blk_ptr));
        g_ctx->sb_ptr   = calloc(1, sizeof(*g_ctx->sb_ptr));
        BlockGeom *geom = calloc(1, sizeof(*geom));
        if (!g_ctx->blk_ptr || !g_ctx->sb_ptr || !geom) return 1;
        geom->sq_size     = 64;
        g_ctx->blk_geom   = geom;
        g_ctx->sb_ptr->qindex = 255; /* never below quantizer_to_qindex[picture_qp = 0]: `sharp` comes from sharp_tx alone */
    }
    g_pcs->scs = g_scs; g_pcs->ppcs = g_ppcs; g_scs->enc_ctx = g_enc;
    g_ctx->md_rate_est_ctx = &g_rate;
    return 0;
}
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
int harness_plane_rd_mult(int is_inter, int plane_type) { return plane_rd_mult[is_inter][plane_type]; }
/* rows: [n][7][2] int16 in the order zbin, round, quant, quant_shift, round_fp, quant_fp, dequant ([0] DC, [1] AC) */
void harness_rows(const int16_t *rows, int n) {
    for (int q = 0; q < n; q++)
        for (int k = 0; k < 8; k++) {
            const int16_t *r = rows + q * 14;
            const int      i = k ? 1 : 0;
            Quants   *qs[2] = {&g_enc->quants_8bit, &g_enc->quants_bd};
            Dequants *ds[2] = {&g_enc->deq_8bit, &g_enc->deq_bd};
            for (int b = 0; b < 2; b++) {
                qs[b]->y_zbin[q][k] = qs[b]->u_zbin[q][k] = r[0 + i];
                qs[b]->y_round[q][k] = qs[b]->u_round[q][k] = r[2 + i];
                qs[b]->y_quant[q][k] = qs[b]->u_quant[q][k] = r[4 + i];
                qs[b]->y_quant_shift[q][k] = qs[b]->u_quant_shift[q][k] = r[6 + i];
                qs[b]->y_round_fp[q][k] = qs[b]->u_round_fp[q][k] = r[8 + i];
                qs[b]->y_quant_fp[q][k] = qs[b]->u_quant_fp[q][k] = r[10 + i];
                ds[b]->y_dequant_qtx[q][k] = ds[b]->u_dequant_qtx[q][k] = r[12 + i];
            }
        }
}
/* ctl: sharpness, eob_fast_inter, eob_fast_intra, eob_th, eob_fast_th, plane_type, bit_depth */
static void set_controls(const int *ctl, int tx_size, const uint8_t *qm, const uint8_t *iqm) {
    const int plane = ctl[5];
    memset(&g_ctx->rdoq_ctrls, 0, sizeof(g_ctx->rdoq_ctrls));
    g_ctx->rdoq_level = 1;
    g_ctx->rdoq_ctrls.enabled = 1;
    g_ctx->rdoq_ctrls.fp_q_y = g_ctx->rdoq_ctrls.fp_q_uv = 1;
    g_ctx->rdoq_ctrls.satd_factor   = (uint8_t)~0;
    g_ctx->rdoq_ctrls.early_exit_th = 0;
    if (plane) { g_ctx->rdoq_ctrls.eob_fast_uv_inter = (uint8_t)ctl[1]; g_ctx->rdoq_ctrls.eob_fast_uv_intra = (uint8_t)ctl[2]; }
    else { g_ctx->rdoq_ctrls.eob_fast_y_inter = (uint8_t)ctl[1]; g_ctx->rdoq_ctrls.eob_fast_y_intra = (uint8_t)ctl[2]; }
    g_ctx->rdoq_ctrls.eob_th      = (uint8_t)ctl[3];
    g_ctx->rdoq_ctrls.eob_fast_th = (uint8_t)ctl[4];
    g_ctx->mds_skip_rdoq = 0;
    g_ctx->hbd_md        = 0;
    g_ctx->rate_est_ctrls.update_skip_ctx_dc_sign_ctx = 1;
    g_scs->static_config.sharpness        = (int8_t)ctl[0];
    g_scs->vq_ctrls.sharpness_ctrls.rdoq  = 1;
    g_pcs->picture_qp                     = 0;
    g_ppcs->frm_hdr.delta_q_params.delta_q_present = 1;
    memset(g_ppcs->gqmatrix, 0, sizeof(g_ppcs->gqmatrix));
    memset(g_ppcs->giqmatrix, 0, sizeof(g_ppcs->giqmatrix));
    g_ppcs->frm_hdr.quantization_params.using_qmatrix = qm != NULL;
    for (int p = 0; p < 3; p++) g_ppcs->frm_hdr.quantization_params.qm[p] = 5;
    if (qm)
        for (int p = 0; p < 3; p++) {
            g_ppcs->gqmatrix[5][p][aom_av1_get_adjusted_tx_size((TxSize)tx_size)]  = qm;
            g_ppcs->giqmatrix[5][p][aom_av1_get_adjusted_tx_size((TxSize)tx_size)] = iqm;
        }
}
/* job: tx_type, txb_skip_ctx, dc_sign_ctx, is_inter, quant_row, sharp */
int harness_run(const int *ctl, int tx_size, const int *job, uint32_t lambda, const uint8_t *qm, const uint8_t *iqm, const int32_t *coeff,
                int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob) {
    set_controls(ctl, tx_size, qm, iqm);
    g_scs->static_config.sharp_tx = (uint8_t)job[5];
    return svt_aom_quantize_inv_quantize(g_pcs, g_ctx, (int32_t *)coeff, qcoeff, dqcoeff, (uint32_t)job[4], 0, (TxSize)tx_size, eob,
                                         ctl[5] ? COMPONENT_CHROMA_CB : COMPONENT_LUMA, (uint32_t)ctl[6], (TxType)job[0], (int16_t)job[1],
                                         (int16_t)job[2], job[3] ? NEARESTMV : DC_PRED, lambda, false);
}
/* the quantizer alone: rdoq_level 0 takes the "b" quantizer; fp != 0 takes the "fp" one with every later stage gated off */
void harness_quantize(const int *ctl, int tx_size, const int *job, int fp, const uint8_t *qm, const uint8_t *iqm, const int32_t *coeff, int32_t *qcoeff,
                      int32_t *dqcoeff, uint16_t *eob) {
    set_controls(ctl, tx_size, qm, iqm);
    if (!fp) g_ctx->rdoq_level = 0;
    if (fp) {
        MacroblockPlane p;
        QuantParam      qp;
        const int       hbd = ctl[6] > 8, q = job[4];
        Quants         *qs  = hbd ? &g_enc->quants_bd : &g_enc->quants_8bit;
        p.quant_fp_qtx = qs->y_quant_fp[q]; p.round_fp_qtx = qs->y_round_fp[q]; p.zbin_qtx = qs->y_zbin[q]; p.quant_shift_qtx = qs->y_quant_shift[q];
        p.quant_qtx = qs->y_quant[q]; p.round_qtx = qs->y_round[q];
        p.dequant_qtx = hbd ? g_enc->deq_bd.y_dequant_qtx[q] : g_enc->deq_8bit.y_dequant_qtx[q];
        qp.log_scale = av1_get_tx_scale_tab[tx_size]; qp.tx_size = (TxSize)tx_size;
        qp.qmatrix = job[0] < IDTX ? qm : NULL; qp.iqmatrix = job[0] < IDTX ? iqm : NULL;
        if (hbd) svt_av1_highbd_quantize_fp_facade(coeff, av1_get_max_eob((TxSize)tx_size), &p, qcoeff, dqcoeff, eob, &av1_scan_orders[tx_size][job[0]], &qp);
        else svt_av1_quantize_fp_facade(coeff, av1_get_max_eob((TxSize)tx_size), &p, qcoeff, dqcoeff, eob, &av1_scan_orders[tx_size][job[0]], &qp);
        return;
    }
    svt_aom_quantize_inv_quantize(g_pcs, g_ctx, (int32_t *)coeff, qcoeff, dqcoeff, (uint32_t)job[4], 0, (TxSize)tx_size, eob,
                                  ctl[5] ? COMPONENT_CHROMA_CB : COMPONENT_LUMA, (uint32_t)ctl[6], (TxType)job[0], (int16_t)job[1], (int16_t)job[2],
                                  job[3] ? NEARESTMV : DC_PRED, 0, false);
}
"""
SOURCES = ["Codec/rd_cost.c", "Codec/md_rate_estimation.c", "Codec/cabac_context_model.c", "Codec/aom_dsp_rtcd.c", "Codec/common_dsp_rtcd.c"]
MEMBERS = list(cr.TABLE_SHAPES)


def build(ref, tmp):
    L = refbuild.build(ref, tmp, "rdoqref", SOURCES, [("harness", HARNESS)])
    L.harness_table.restype = C.c_size_t
    L.harness_table.argtypes = [C.c_int, C.c_void_p]
    L.harness_rows.argtypes = [C.c_void_p, C.c_int]
    L.harness_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
    L.harness_quantize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.harness_quantize.restype = None
    return L


def reference_tables(L):
    """the reference's tables per qindex, compared with the ones golden/coeff_rate.npz holds (the tests read those)"""
    z = np.load(cr.GOLDEN)
    tables = []
    for k, qindex in enumerate(cr.QINDEXES):
        if L.harness_init(int(qindex)):
            raise RuntimeError("harness_init failed")
        members = {}
        for m, name in enumerate(MEMBERS):
            a = np.zeros(cr.TABLE_SHAPES[name], np.int32)
            L.harness_table(m, a.ctypes.data)
            if not np.array_equal(a, z[f"{name}_{k}"]):
                raise RuntimeError(f"{name} at qindex {qindex} differs from golden/coeff_rate.npz")
            members[name] = a
        tables.append(cr.Tables(**members))
    return tables


def generate(L):
    if [[L.harness_plane_rd_mult(i, p) for p in (0, 1)] for i in (0, 1)] != rq.PLANE_RD_MULT:
        raise RuntimeError("plane_rd_mult differs: TUNE_CHROMA_SSIM is not 1 in this tree")
    tables = reference_tables(L)
    cases = rq.build_cases()
    p = lambda a: a.ctypes.data if a is not None else None
    out = {"case_meta": np.array([rq.case_meta(c) for c in cases], np.int64)}
    qs, eobs, culs, sts, crcs = [], [], [], [], []
    mismatch, events = [], []
    for k in range(len(cr.QINDEXES)):
        L.harness_init(int(cr.QINDEXES[k]))
        rows = np.ascontiguousarray(rq.quant_rows()).view(np.int16).reshape(-1)
        L.harness_rows(rows.ctypes.data, 3)
        for ci, c in enumerate(cases):
            if c["table"] != k:
                continue
            ts = c["tx_size"]
            n, npk = c["coeff"].shape
            ctl = np.array([c["sharpness"], c["eob_fast_inter"], c["eob_fast_intra"], c["eob_th"], c["eob_fast_th"], c["plane"], c["bit_depth"]], np.int32)
            inp = rq.quantized(c)
            q, dq = np.zeros((n, npk), np.int32), np.zeros((n, npk), np.int32)
            eob, cul = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
            for i, j in enumerate(c["jobs"]):
                job = np.array([j["tx_type"], j["txb_skip_ctx"], j["dc_sign_ctx"], j["is_inter"], j["quant_row"], j["flags"] & 1], np.int32)
                co = np.ascontiguousarray(c["coeff"][i])
                for fp, names in ((1, ("qcoeff", "dqcoeff", "eob")), (0, ("qcoeff_b", "dqcoeff_b", "eob_b"))):  # the oracle's quantizers
                    tq, tdq, te = np.zeros(npk, np.int32), np.zeros(npk, np.int32), np.zeros(1, np.uint16)
                    L.harness_quantize(p(ctl), ts, p(job), fp, p(c["qmatrix"]), p(c["iqmatrix"]), p(co), p(tq), p(tdq), p(te))
                    if not (np.array_equal(tq, inp[names[0]][i]) and np.array_equal(tdq, inp[names[1]][i]) and te[0] == inp[names[2]][i]):
                        raise RuntimeError(f"the oracle's {'fp' if fp else 'b'} quantizer differs from the reference: case {ci} ({ts}, {c['variant']}) job {i}")
                cul[i] = L.harness_run(p(ctl), ts, p(job), c["lam"], p(c["qmatrix"]), p(c["iqmatrix"]), p(co), p(q[i]), p(dq[i]), p(eob[i:]))
            ev = []
            want = rq.run_case(tables[k], c, inp, True, ev)
            for i in range(n):
                if not (np.array_equal(want["qcoeff"][i], q[i]) and np.array_equal(want["dqcoeff"][i], dq[i]) and want["eob"][i] == eob[i]
                        and want["cul_level"][i] == cul[i]):
                    mismatch.append((ci, ts, rq.VARIANTS[c["variant"]][0], i, int(want["eob"][i]), int(eob[i]), int(np.count_nonzero(want["qcoeff"][i] != q[i]))))
            if np.abs(q).max() > 32767:
                raise RuntimeError("a level does not fit the fixture's int16")
            qs.append((ci, q.astype(np.int16).reshape(-1)))
            eobs.append((ci, eob)); culs.append((ci, cul)); sts.append((ci, want["status"])); crcs.append((ci, rq.crc(dq)))
            events.append((ci, ev, inp, want))
    if mismatch:
        raise RuntimeError(f"the restatement differs from the reference on {len(mismatch)} jobs, first: {mismatch[:8]}")
    order = lambda lst: [v for _, v in sorted(lst, key=lambda t: t[0])]
    out["qcoeff"], out["eob"], out["cul_level"], out["status"] = (np.concatenate(order(x)) for x in (qs, eobs, culs, sts))
    out["dqcoeff_crc"] = np.array(order(crcs), np.uint32)
    missing = rq.coverage_missing([(cases[ci], ev, inp, want) for ci, ev, inp, want in sorted(events, key=lambda t: t[0])])
    if missing:
        raise RuntimeError(f"coverage conditions the reference's results do not meet: {missing}")
    return out


if __name__ == "__main__":
    refbuild.main(__doc__, build, {rq.GOLDEN: generate}, save=refbuild.savez, wrote=refbuild.wrote_shapes)
