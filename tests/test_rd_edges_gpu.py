"""GPU: svt_hip_rd_batch, svt_hip_fwd_txfm_batch and svt_hip_inv_txfm_batch at the bounds of their fast paths (tests/rd_edge_cases.py),
bit for bit against the oracle: every output set the RD batch accepts (which picks the quantizer loop), magnitudes on both sides of
every bound in mixed waves, partial last waves and output slots past n_jobs."""
import ctypes as C

import numpy as np
import pyoracle
import pytest

import rd_edge_cases as E
from svt_av1_psyex_amd import abi, rd
from txfm_cases import TX_H, TX_W, valid_types

pytestmark = pytest.mark.gpu

FILL = 0xA5  # canary byte of every output slot past n_jobs
ALL = ("coeff", "qcoeff", "dqcoeff", "cul_level", "recon")
OUTPUT_SETS = {  # optional outputs requested; eob .. sse always
    "all": ALL,
    "bench": ("qcoeff", "cul_level", "recon"),  # bench.py's RD launches: the fast quantizer loop with qcoeff stores
    "scalars": ("cul_level",),
    "coeff": ("coeff", "cul_level", "recon"),
    "dqcoeff": ("dqcoeff", "cul_level", "recon"),
    "no_cul_level": ("coeff", "qcoeff", "dqcoeff", "recon"),
}


def _compare(want, got, n, outputs, what):
    """got (n + spare slots per array) against the oracle's all-outputs run: the requested outputs equal, the spare slots untouched"""
    for name in got:
        if name == "recon":
            assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:3].tolist())
            continue
        a = got[name]
        assert np.array_equal(a[:n], want[name]), (what, name, np.argwhere(a[:n] != want[name])[:3].tolist())
        assert (a[n:].view(np.uint8) == FILL).all(), (what, name, "written past n_jobs")
    assert set(got) == {nm for nm, _, _ in abi.RD_OUT_FIELDS if nm != "cul_level"} | set(outputs), (what, sorted(got))


@pytest.mark.parametrize("tx_size", range(19))
def test_rd_batch_output_sets(hip_ctx, tx_size):
    """The same jobs with every output set: each returned output equals the oracle's all-outputs run, slots past n_jobs keep their canary
    and so do the recon samples outside every job."""
    rows = E.quant_rows()
    for bd in (8, 10):
        f0, src, pred, jobs = E.output_set_case(tx_size, bd)
        canary = np.full_like(pred, 0x5A)
        for quant_kind in (0, 1, 2):
            f = dict(f0, quant_kind=quant_kind)
            want = pyoracle.rd_batch(f, src, pred, jobs, rows, recon_init=canary)
            assert want["eob"].max() > 0 and (want["recon"] == 0x5A).any()
            for name, outputs in OUTPUT_SETS.items():
                got = rd.run_hip(hip_ctx, f, src, pred, jobs, rows, outputs=outputs, spare_jobs=E.blocks_per_wave(tx_size) + 1, fill=FILL, recon_init=canary)
                _compare(want, got, len(jobs), outputs, (tx_size, bd, quant_kind, name))


@pytest.mark.parametrize("tx_size", range(19))
def test_rd_batch_magnitude_edges(hip_ctx, tx_size):
    """Residuals on both sides of the fast_col, q24 and 8-bit clamp bounds, one block beyond a bound first / last among blocks below it,
    with and without a quantization matrix; each with bench.py's output set (the fast quantizer loop) and with all outputs."""
    rows = E.quant_rows()
    for bd in (8, 10):
        f0, src, pred, jobs = E.rd_edge_case(tx_size, bd)
        for quant_kind in (0, 1):
            for use_qm in (False, True):
                qm, iqm = E.qmatrices(tx_size) if use_qm else (None, None)
                for rot in range(len(rows)) if (quant_kind == 0 and not use_qm) else (0,):  # every block meets every "b" quantizer row
                    jobs["quant_row"] = (np.arange(len(jobs)) + rot) % len(rows)
                    f = dict(f0, quant_kind=quant_kind)
                    want = pyoracle.rd_batch(f, src, pred, jobs, rows, qmatrix=qm, iqmatrix=iqm)
                    for name in ("bench", "all"):
                        got = rd.run_hip(hip_ctx, f, src, pred, jobs, rows, qmatrix=qm, iqmatrix=iqm, outputs=OUTPUT_SETS[name], spare_jobs=1, fill=FILL)
                        _compare(want, got, len(jobs), OUTPUT_SETS[name], (tx_size, bd, quant_kind, use_qm, rot, name))


# ---- forward transform alone ----------------------------------------------------------------------------------------------------
def _fwd_want(oracle, ts, plane, jobs):
    w, h = TX_W[ts], TX_H[ts]
    flat = np.ascontiguousarray(plane, np.int16).reshape(-1)
    out = np.zeros((len(jobs), w * h), np.int32)
    for j, jb in enumerate(jobs):
        blk = np.zeros(w * h, np.int32)
        off = int(jb["src_offset"])
        oracle.orc_fwd_txfm2d(C.c_void_p(flat.ctypes.data + 2 * off), blk.ctypes.data_as(C.c_void_p), C.c_uint32(plane.shape[1]), C.c_int(int(jb["tx_type"])),
                              C.c_int(ts))
        m = blk.reshape(h, w)
        pf = int(jb["pf_shape"])
        keep = np.zeros((h, w), bool)
        if pf == 3:
            keep[0, 0] = True
        else:
            keep[:h >> pf, :w >> pf] = True
        out[j] = np.where(keep, m, 0).reshape(-1)
    return out


@pytest.mark.parametrize("tx_size", range(19))
def test_fwd_txfm_batch_matches_oracle(hip_ctx, oracle, tx_size):
    """svt_hip_fwd_txfm_batch: every allowed type, pf_shape 0..3 per job (3 = the DC coefficient alone), a residual stride wider than the
    blocks, odd offsets, partial waves, the full int16 range and the fast_col bound's magnitudes in mixed waves; slots past n_jobs untouched."""
    rng = np.random.default_rng(4300 + tx_size)
    w, h = TX_W[tx_size], TX_H[tx_size]
    bpw = E.blocks_per_wave(tx_size)
    types = valid_types(tx_size)
    mags = [E.fast_col_limit(tx_size), E.fast_col_limit(tx_size) + 1, E.fast_col_limit_unshifted(tx_size), 1023, 32767]
    specs = []
    for i, tt in enumerate(types):
        for m_below, m_beyond in ((mags[0], mags[1]), (mags[0], mags[2]), (1023, 32767)):
            for wave in ([m_below] * bpw, [m_beyond] + [m_below] * (bpw - 1), [m_below] * (bpw - 1) + [m_beyond]):
                specs += [(tt, ("flat", "basis", "checker")[(i + j) % 3], m, 1 if j % 2 else -1) for j, m in enumerate(wave)]
    n_rand = 3 * bpw + 1
    stride = 256 + 13
    per_row = (stride - 1) // w
    n = len(specs) + n_rand
    plane = np.zeros((((n + per_row - 1) // per_row) * h, stride), np.int64)
    jobs = np.zeros(n, abi.JOB_DTYPE)
    for j in range(n):
        y, x = (j // per_row) * h, 1 + (j % per_row) * w  # odd offsets
        if j < len(specs):
            tt, pattern, m, sign = specs[j]
            plane[y:y + h, x:x + w] = E.residual_block(tx_size, tt, m, pattern, k=1 + j % 3, sign=sign)
        else:
            tt = types[j % len(types)]
            plane[y:y + h, x:x + w] = rng.integers(-32768, 32768, (h, w))
        jobs[j]["src_offset"] = y * stride + x
        jobs[j]["tx_type"] = tt
    jobs["pf_shape"] = rng.integers(0, 4, n)
    jobs["pf_shape"][:len(specs)] = np.where(np.arange(len(specs)) % 4 == 1, jobs["pf_shape"][:len(specs)], 0)
    jobs["quant_row"] = rng.integers(0, 256, n)  # not read by the forward batch
    jobs = jobs[:n - bpw // 2] if bpw > 1 else jobs  # partial last wave
    plane16 = plane.astype(np.int16)
    want = _fwd_want(oracle, tx_size, plane16, jobs)
    got = rd.run_fwd_hip(hip_ctx, tx_size, plane16, jobs, spare_jobs=bpw + 1, fill=FILL)
    assert np.array_equal(got[:len(jobs)], want), (tx_size, np.argwhere(got[:len(jobs)] != want)[:3].tolist())
    assert (got[len(jobs):].view(np.uint8) == FILL).all(), "written past n_jobs"


def test_fwd_txfm_batch_rejects_bad_descriptors(hip_ctx):
    from svt_av1_psyex_amd import api
    L = api.lib()
    d = abi.FwdTxBatchDesc(tx_size=19, n_jobs=1, residual_stride=4, residual=1, jobs=1, coeff=1)
    assert L.svt_hip_fwd_txfm_batch(hip_ctx._h, C.byref(d)) == 2
    d = abi.FwdTxBatchDesc(tx_size=0, n_jobs=1, residual_stride=4)
    assert L.svt_hip_fwd_txfm_batch(hip_ctx._h, C.byref(d)) == 2
    d = abi.FwdTxBatchDesc(tx_size=0, n_jobs=0)
    assert L.svt_hip_fwd_txfm_batch(hip_ctx._h, C.byref(d)) == 0


# ---- inverse transform alone --------------------------------------------------------------------------------------------------
def _inv_want(oracle, ts, bd, pred, recon, jobs, co):
    """orc_inv_txfm2d_add per job: pred block at pred_offset, recon block at src_offset (planes as uint16 copies)"""
    p16, r16 = np.ascontiguousarray(pred, np.uint16), np.ascontiguousarray(recon, np.uint16).copy()
    for j, jb in enumerate(jobs):
        po, ro = int(jb["pred_offset"]), int(jb["src_offset"])
        oracle.orc_inv_txfm2d_add(C.c_void_p(co[j].ctypes.data), C.c_void_p(p16.ctypes.data + 2 * po), C.c_int32(pred.shape[1]),
                                  C.c_void_p(r16.ctypes.data + 2 * ro), C.c_int32(recon.shape[1]), int(jb["tx_type"]), ts, bd)
    return r16


@pytest.mark.parametrize("tx_size", range(19))
def test_inverse_batch_coefficient_edges(hip_ctx, oracle, tx_size):
    """svt_hip_inv_txfm_batch on the waves of rd_edge_cases.inverse_case: blocks just below / at the 2^18 bound of the fast row pass and of
    the fast column pass (the bound's block first / last among blocks below it), beyond the bd + 8 input clamp and at the int32 extremes;
    separate planes with their own strides, and in place (recon == pred, same offsets); uint8 and uint16 storage."""
    rng = np.random.default_rng(4400 + tx_size)
    w, h = TX_W[tx_size], TX_H[tx_size]
    for bd, dt in ((8, np.uint8), (8, np.uint16), (10, np.uint16)):
        types, co = E.inverse_case(rng, tx_size, bd)
        PW = 192
        PH = -(-len(types) // (PW // w)) * h
        jobs = rd.grid_jobs(PW, PH, PW, tx_size)[:len(types)].copy()
        jobs["tx_type"] = types
        pred = rng.integers(0, 1 << bd, (PH, PW)).astype(dt)
        # separate planes: recon has a wider stride and its blocks one row down
        RW = PW + 24
        recon0 = np.full((PH + h, RW), 0x5A, dt)
        sep = jobs.copy()
        ys, xs = jobs["pred_offset"] // PW, jobs["pred_offset"] % PW
        sep["src_offset"] = (ys + 1) * RW + xs
        want = _inv_want(oracle, tx_size, bd, pred, recon0, sep, co)
        got = rd.run_inv_hip(hip_ctx, bd, tx_size, pred, sep, co, recon=recon0)
        assert np.array_equal(got.astype(np.uint16), want), (tx_size, bd, dt.__name__, "separate")
        # in place
        want = _inv_want(oracle, tx_size, bd, pred, pred, jobs, co)
        got = rd.run_inv_hip(hip_ctx, bd, tx_size, pred, jobs, co)
        assert np.array_equal(got.astype(np.uint16), want), (tx_size, bd, dt.__name__, "in place")
