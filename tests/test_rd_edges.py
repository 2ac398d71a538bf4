"""CPU: the fast-path edge cases of tests/rd_edge_cases.py.  The oracle agrees with the reference on exactly these inputs (so the GPU
comparisons of tests/test_rd_edges_gpu.py rest on a pinned checker), the cases reach the regimes they are named after (so an edit to a
generator cannot quietly drop a branch), and the forward / inverse batch descriptors keep their compiled layout."""
import ctypes as C

import numpy as np
import pyoracle
import pytest

import rd_edge_cases as E
from svt_av1_psyex_amd import abi
from txfm_cases import TX_H, TX_W, ref_fwd, ref_inv, valid_types


def _waves(values, bpw):
    return [values[i:i + bpw] for i in range(0, len(values) - bpw + 1, bpw)]


def _job_blocks(ts, f, src, pred, jobs):
    """the residual block of every job, int64"""
    w, h, stride = TX_W[ts], TX_H[ts], f["src_stride"]
    r = src.astype(np.int64).reshape(-1) - pred.astype(np.int64).reshape(-1)
    return [r[int(o) + np.add.outer(np.arange(h) * stride, np.arange(w))] for o in jobs["src_offset"]]


def _mixed(flags, bpw):
    """the waves (full ones) reach: all below, one beyond first, one beyond last"""
    kinds = set()
    for wv in _waves(flags, bpw):
        if not any(wv):
            kinds.add("below")
        if bpw > 1 and wv[0] and not any(wv[1:]):
            kinds.add("first")
        if bpw > 1 and wv[-1] and not any(wv[:-1]):
            kinds.add("last")
    return kinds


@pytest.mark.parametrize("ts", range(19))
def test_rd_cases_reach_fast_col_and_q24_bounds(oracle, ts):
    """10-bit: per size, waves entirely below the fast_col bound and the q24 bound, and waves with one block beyond it first / last"""
    f, src, pred, jobs = E.rd_edge_case(ts, 10)
    bpw = E.blocks_per_wave(ts)
    blocks = _job_blocks(ts, f, src, pred, jobs)
    rmax = [int(np.abs(b).max()) for b in blocks]
    col = [(m << E.FWD_SHIFT0[ts]) * TX_H[ts] >= (1 << 17) for m in rmax]
    cmax = [int(np.abs(E.fwd_full(oracle, ts, int(tt), b)).max()) for b, tt in zip(blocks, jobs["tx_type"])]
    q = [c >= (1 << 16) for c in cmax]
    want = {"below", "first", "last"} if bpw > 1 else {"below"}
    assert _mixed(col, bpw) >= want and any(col), ts
    assert _mixed(q, bpw) >= want and any(q), ts
    assert any(m == E.fast_col_limit(ts) for m in rmax) and any(m == E.fast_col_limit(ts) + 1 for m in rmax)
    # q24 straddled tightly: a block within 2 residual steps of the crossing on either side, with coefficients just below / at 2^16
    assert any((1 << 16) - 200 < c < (1 << 16) for c in cmax) and any((1 << 16) <= c < (1 << 16) + 200 for c in cmax), ts
    # the residuals realised exactly, with samples beyond 10 bits where the magnitude needs them
    assert max(rmax) > 1023 and int(src.max()) > 1023


def test_rd_cases_reach_the_8bit_quantizer_clamp():
    """8-bit: flat +-255 blocks whose |coeff| + round exceeds 32767, at a step where the int16 clamp changes the quantized level -- and the
    oracle quantizes them with the clamp"""
    cases = E.clamp_cases()
    sizes = sorted({ts for ts, _ in cases})
    assert {2, 3, 15, 16, 17, 18} <= set(sizes), sizes
    rows = E.quant_rows()
    for ts in sizes:
        f, src, pred, jobs = E.rd_edge_case(ts, 8)
        blocks = _job_blocks(ts, f, src, pred, jobs)
        flat = [i for i, b in enumerate(blocks) if np.abs(b).min() == 255 and len(np.unique(b)) == 1 and jobs["tx_type"][i] == 0]
        assert flat, ts
        qi = [q for t, q in cases if t == ts][0]
        i = flat[0]
        one = jobs[i:i + 1].copy()
        one["quant_row"] = qi
        out = pyoracle.rd_batch(dict(f, quant_kind=0), src, pred, one, rows)
        a = abs(int(out["coeff"][0, 0]))
        rnd = (int(rows[qi]["round"][0]) + ((1 << E.LOG_SCALE[ts]) >> 1)) >> E.LOG_SCALE[ts]
        assert a + rnd > 32767, (ts, a, rnd)
        lv = abs(int(out["qcoeff"][0, 0]))
        assert lv == E.quantize_b_level(a, rows[qi], 0, E.LOG_SCALE[ts], True) != E.quantize_b_level(a, rows[qi], 0, E.LOG_SCALE[ts], False), ts
        # a rotation of the quantizer rows in the GPU test gives every flat block this row
        assert len(rows) == len(E.QUANT_STEPS)


@pytest.mark.parametrize("ts", range(19))
def test_inverse_cases_straddle_the_fast_pass_bounds(oracle, ts):
    """the inverse cases, decided per wave as the kernel decides fast_irow / fast_icol: waves entirely below 2^18 / W (2^18 / H) and waves
    with one block at the bound first / last, wherever the clamps let an input reach it; blocks beyond the bd + 8 clamp and at the int32
    extremes"""
    rng = np.random.default_rng(ts)
    w, h = TX_W[ts], TX_H[ts]
    bpw = E.blocks_per_wave(ts)
    want = {"below", "first", "last"} if bpw > 1 else {"below"}
    for bd in (8, 10):
        types, co = E.inverse_case(rng, ts, bd)
        assert bpw == 1 or len(types) % bpw == bpw - 1  # a partial last wave
        row_max = E.inv_row_input_max(ts, bd, co)
        row = [int(m) * w >= (1 << 18) for m in row_max]
        col = [E.inv_col_input_max(oracle, ts, bd, tt, b) * h >= (1 << 18) for tt, b in zip(types, co)]
        assert "below" in _mixed(row, bpw) and "below" in _mixed(col, bpw), (ts, bd)
        if ((1 << (bd + 7)) - 1) * w >= (1 << 18):
            assert _mixed(row, bpw) >= want and any(row), (ts, bd)
            assert (row_max == E.inv_fast_limit(w)).any() and (row_max == E.inv_fast_limit(w) + 1).any(), (ts, bd)
        if any(E.inv_col_crossing(ts, bd, tt) for tt in E.inv_col_pair_types(ts)):
            assert _mixed(col, bpw) >= want and any(col), (ts, bd)
        else:  # no pattern reaches the column bound: then no block of the cases may either (else the search missed a way)
            assert not any(col), (ts, bd)
            assert bd == 8 and ts in (14, 18), ts  # 16x4, 64x16: the 8-bit stage clamps keep every column input below 2^18 / H
        lim = 1 << (bd + 7)
        co = co.astype(np.int64)
        assert (np.abs(co) > lim).any() and (co == -(1 << 31)).any() and (co == (1 << 31) - 1).any()


def test_fwd_and_inv_batch_descriptor_layout(oracle):
    oracle.orc_sizeof_dsp.restype = C.c_size_t
    assert oracle.orc_sizeof_dsp(0) == C.sizeof(abi.RdBatchDesc)
    assert oracle.orc_sizeof_dsp(1) == C.sizeof(abi.TxJob) == np.dtype(abi.JOB_DTYPE).itemsize
    assert oracle.orc_sizeof_dsp(2) == C.sizeof(abi.QuantRow) == np.dtype(abi.QUANT_ROW_DTYPE).itemsize
    assert oracle.orc_sizeof_dsp(3) == C.sizeof(abi.FwdTxBatchDesc)
    assert oracle.orc_sizeof_dsp(4) == C.sizeof(abi.InvTxBatchDesc)


# ---- the oracle against the reference on these inputs (build container: needs the reference build) -----------------------------
@pytest.mark.parametrize("ts", range(19))
def test_rd_edge_cases_oracle_equals_reference(ref, ts):
    rows = E.quant_rows()
    for bd in (8, 10):
        f0, src, pred, jobs = E.rd_edge_case(ts, bd)
        for quant_kind in (0, 1):
            for rot in range(len(rows)) if quant_kind == 0 else (0,):
                jobs["quant_row"] = (np.arange(len(jobs)) + rot) % len(rows)
                f = dict(f0, quant_kind=quant_kind)
                a = pyoracle.rd_batch(f, src, pred, jobs, rows)
                b = pyoracle.rd_batch(f, src, pred, jobs, rows, impl="ref")
                for k in a:
                    assert np.array_equal(a[k], b[k]), (ts, bd, quant_kind, rot, k, np.argwhere(a[k] != b[k])[:3].tolist())


@pytest.mark.parametrize("ts", range(19))
def test_fwd_and_inv_edge_inputs_oracle_equals_reference(ref, oracle, ts):
    """orc_fwd_txfm2d against the reference's forward entries on the separable worst cases at the fast_col magnitudes and the int16 extremes;
    orc_inv_txfm2d_add against its inverse entries on the inverse edge coefficients"""
    rng = np.random.default_rng(600 + ts)
    w, h = TX_W[ts], TX_H[ts]
    mags = [E.fast_col_limit(ts), E.fast_col_limit(ts) + 1, E.fast_col_limit_unshifted(ts), 32767]
    for tt in valid_types(ts):
        for m in mags:
            for pattern in E.PATTERNS:
                r = np.ascontiguousarray(E.residual_block(ts, tt, m, pattern, k=1 + tt % 3, sign=-1 if m % 2 else 1).astype(np.int16))
                got = np.zeros(w * h, np.int32)
                oracle.orc_fwd_txfm2d(r.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), C.c_uint32(w), tt, ts)
                assert np.array_equal(ref_fwd(ref, ts, tt, r, w, 10), got), (tt, m, pattern)
        r = np.ascontiguousarray(np.full((h, w), -32768, np.int16))
        got = np.zeros(w * h, np.int32)
        oracle.orc_fwd_txfm2d(r.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), C.c_uint32(w), tt, ts)
        assert np.array_equal(ref_fwd(ref, ts, tt, r, w, 10), got), (tt, "-32768")
    for bd in (8, 10):
        types, co = E.inverse_case(rng, ts, bd)
        for j in range(len(co)):
            tt = int(types[j])
            c = np.ascontiguousarray(co[j])
            pred = rng.integers(0, 1 << bd, (h, w)).astype(np.uint16)
            want = pred.copy()
            oracle.orc_inv_txfm2d_add(c.ctypes.data_as(C.c_void_p), pred.ctypes.data_as(C.c_void_p), C.c_int32(w), want.ctypes.data_as(C.c_void_p),
                                      C.c_int32(w), tt, ts, bd)
            assert np.array_equal(ref_inv(ref, ts, tt, c, pred, w, bd), want), (bd, j, tt)


def _ref_quantize(ref, quant_kind, highbd, co, row, qm, iqm, scan, iscan, log_scale):
    """the reference's own quantizer `_c` functions on one block of coefficients: (qcoeff, dqcoeff, eob)"""
    P = C.c_void_p
    p = lambda a: a.ctypes.data_as(P)
    n = len(co)
    qa, da, ea = np.full(n, 7, np.int32), np.full(n, 7, np.int32), C.c_uint16(999)
    q = {k: np.ascontiguousarray(row[k]) for k in ("zbin", "round", "quant", "quant_shift", "round_fp", "quant_fp", "dequant")}
    pq, pi = (p(qm), p(iqm)) if qm is not None else (None, None)
    if quant_kind == 0:
        fn = ref.svt_aom_highbd_quantize_b_c if highbd else ref.svt_aom_quantize_b_c_ii
        fn(p(co), C.c_ssize_t(n), p(q["zbin"]), p(q["round"]), p(q["quant"]), p(q["quant_shift"]), p(qa), p(da), p(q["dequant"]), C.byref(ea), p(scan),
           p(iscan), pq, pi, C.c_int32(log_scale))
    else:
        args = (p(co), C.c_ssize_t(n), p(q["zbin"]), p(q["round_fp"]), p(q["quant_fp"]), p(q["quant_shift"]), p(qa), p(da), p(q["dequant"]), C.byref(ea),
                p(scan), p(iscan))
        if qm is not None:
            (ref.svt_av1_highbd_quantize_fp_qm_c if highbd else ref.svt_av1_quantize_fp_qm_c)(*args, pq, pi, C.c_int16(log_scale))
        elif highbd:
            ref.svt_av1_highbd_quantize_fp_c(*args, C.c_int16(log_scale))
        else:
            [ref.svt_av1_quantize_fp_c, ref.svt_av1_quantize_fp_32x32_c, ref.svt_av1_quantize_fp_64x64_c][log_scale](*args)
    return qa, da, ea.value


@pytest.mark.parametrize("ts", range(19))
def test_matrix_and_tpl_quantizers_oracle_equals_reference(ref, ts):
    """What the reference chain (ref_rd_batch) does not take -- quantization matrices and quant_kind 2 (plain svt_av1_quantize_fp at every
    size) -- pinned at the quantizer: on the coefficients of the magnitude edges and of the output-set pictures, the oracle's qcoeff /
    dqcoeff / eob equal the reference's quantizer functions with the same matrices (applied to the 2-D types only, like the chain)."""
    rows = E.quant_rows()
    qm, iqm = E.qmatrices(ts)
    for bd in (8, 10):
        for f0, src, pred, jobs in (E.rd_edge_case(ts, bd), E.output_set_case(ts, bd)):
            jobs = jobs.copy()
            jobs["pf_shape"] = 0
            jobs["quant_row"] = np.arange(len(jobs)) % len(rows)
            for quant_kind, use_qm in ((0, True), (1, True), (2, False), (2, True)):
                f = dict(f0, quant_kind=quant_kind)
                out = pyoracle.rd_batch(f, src, pred, jobs, rows, qmatrix=qm if use_qm else None, iqmatrix=iqm if use_qm else None, want_recon=False)
                log_scale = 0 if quant_kind == 2 else E.LOG_SCALE[ts]
                for j, jb in enumerate(jobs):
                    tt = int(jb["tx_type"])
                    n = out["coeff"].shape[1]
                    scan, iscan = np.zeros(n, np.int16), np.zeros(n, np.int16)
                    ref.ref_scan_order(ts, tt, scan.ctypes.data_as(C.c_void_p), iscan.ctypes.data_as(C.c_void_p))
                    m = (qm, iqm) if use_qm and tt < 9 else (None, None)
                    qa, da, eob = _ref_quantize(ref, quant_kind, bd != 8, np.ascontiguousarray(out["coeff"][j]), rows[int(jb["quant_row"])], *m, scan, iscan,
                                                log_scale)
                    assert np.array_equal(qa, out["qcoeff"][j]) and np.array_equal(da, out["dqcoeff"][j]) and eob == out["eob"][j, 0], \
                        (ts, bd, quant_kind, use_qm, j, tt)
