"""CPU: the restatement of RDOQ (tests/rdoq_cases.py) against the reference's own svt_aom_quantize_inv_quantize results (golden/rdoq.npz), the
coverage conditions on those results, the anti-diagonal property the kernel's simple phase relies on, and the C-ABI of svt_hip_rdoq_batch
(validation needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import coeff_rate_cases as cr
import rdoq_cases as rq
from batch_entry_cases import good_rdoq_desc
from svt_av1_psyex_amd import abi, api

BAD_PARAM = 2


@pytest.mark.parametrize("tx_size", range(cr.N_TX_SIZES))
def test_restatement_equals_the_reference_on_every_job(tx_size):
    """qcoeff, eob and cul_level job by job, dqcoeff by the case's CRC; every variant of the size"""
    cases = rq.shared()["cases"]
    ran = 0
    for k, c in enumerate(cases):
        if c["tx_size"] != tx_size:
            continue
        inp, want, _ = rq.restated(k)
        ref = c["ref"]
        bad = [i for i in range(len(c["jobs"])) if not np.array_equal(want["qcoeff"][i], ref["qcoeff"][i])]
        assert not bad, (rq.VARIANTS[c["variant"]][0], bad[:5])
        assert np.array_equal(want["eob"], ref["eob"]) and np.array_equal(want["cul_level"], ref["cul_level"]), rq.VARIANTS[c["variant"]][0]
        assert np.array_equal(want["status"], ref["status"])
        assert rq.crc(want["dqcoeff"]) == ref["dqcoeff_crc"]
        assert np.all(want["written"])  # with the fallback arrays every defined job is written
        gated = want["status"] == rq.ST_GATED
        assert np.array_equal(want["qcoeff"][gated], inp["qcoeff_b"][gated]) and np.array_equal(want["eob"][gated], inp["eob_b"][gated])
        ran += 1
    assert ran == len(rq.VARIANTS)


def test_the_cases_are_what_the_issue_lists():
    cases = rq.shared()["cases"]
    assert len(cases) == cr.N_TX_SIZES * len(rq.VARIANTS) and {c["tx_size"] for c in cases} == set(range(cr.N_TX_SIZES))
    for ts in range(cr.N_TX_SIZES):
        mine = [c for c in cases if c["tx_size"] == ts]
        assert {c["plane"] for c in mine} == {0, 1}
        assert {c["variant"] for c in mine} == set(range(len(rq.VARIANTS)))
        classes = {cr.tx_class(int(t)) for c in mine for t in c["jobs"]["tx_type"]}
        admitted = {cr.tx_class(t) for t in range(16) if cr.EXT_TX_USED[cr.ext_tx_set_type(ts, 1, 0)][t]}
        assert classes == admitted, ts
        assert all({0, 1} == set(c["jobs"]["is_inter"].tolist()) for c in mine)
        jpw = max(1, 64 // mine[0]["coeff"].shape[1])
        assert all(20 <= len(c["jobs"]) and (jpw == 1 or len(c["jobs"]) % jpw) for c in mine)
    assert {c["bit_depth"] for c in cases} == {8, 10} and {c["qmatrix"] is None for c in cases} == {True, False}
    assert len({c["lam"] for c in cases}) >= 3 and {c["table"] for c in cases} == {0, 1}
    by_name = {rq.VARIANTS[c["variant"]][0]: c for c in cases if c["tx_size"] == 2}
    assert by_name["sharpness4"]["sharpness"] == 4 and by_name["sharpness7"]["sharpness"] == 7
    assert by_name["eob_fast"]["eob_fast_inter"] == 1 and by_name["fast_th30"]["eob_fast_th"] == 30 and by_name["fast_th0"]["eob_fast_th"] == 0
    assert by_name["eob_th85"]["eob_th"] == 85 and by_name["plain_y"]["eob_th"] == 255 == by_name["plain_y"]["eob_fast_th"]
    sharp = by_name["sharp"]["jobs"]["flags"] & 1
    assert 0 < np.count_nonzero(sharp) < len(sharp)


def test_coverage_conditions_hold_on_the_reference_results():
    """the events are those of the restatement's walks, which the test above ties to the reference job by job"""
    cases = rq.shared()["cases"]
    records = [(c, rq.restated(k)[2]) for k, c in enumerate(cases)]
    assert rq.coverage_missing(records) == []
    # the lambdas span "changes nothing" to "zeroes most blocks"
    for lam, lo, hi in ((rq.LAMBDAS[0], 0.0, 0.35), (rq.LAMBDAS[-1], 0.6, 1.0)):
        ks = [k for k, c in enumerate(cases) if c["lam"] == lam and rq.VARIANTS[c["variant"]][0] == "plain_y"]
        inp_eob = np.concatenate([rq.restated(k)[0]["eob"] for k in ks])
        out_eob = np.concatenate([rq.restated(k)[1]["eob"] for k in ks])
        zeroed = np.count_nonzero((inp_eob > 0) & (out_eob == 0)) / max(1, np.count_nonzero(inp_eob > 0))
        assert lo <= zeroed <= hi, (lam, zeroed)


def test_sharp_jobs_never_shorten_eob_or_skip():
    cases = rq.shared()["cases"]
    seen = 0
    for k, c in enumerate(cases):
        if rq.VARIANTS[c["variant"]][0] != "sharp":
            continue
        inp, want, ev = rq.restated(k)
        for i, j in enumerate(c["jobs"]):
            if j["flags"] & 1 and want["status"][i] == rq.ST_OPTIMISED:
                assert not ev[i].get("head_shortens") and not ev[i].get("skip_zeroes") and want["eob"][i] == inp["eob"][i]
                seen += 1
    assert seen > 50


@pytest.mark.parametrize("tx_size", range(cr.N_TX_SIZES))
def test_context_neighbours_lie_on_later_antidiagonals_and_later_in_the_scan(tx_size):
    """Every level get_nz_mag / get_br_ctx read around a position has a larger row + column and a larger scan index than the position, for
    the diagonal scan, the row scan (V_*) and the column scan (H_*) of every size: the positions of one anti-diagonal are independent, and
    walking the anti-diagonals from the far corner visits a position after everything its decision reads."""
    w, h = cr.packed_dims(tx_size)
    for tx_type in (0, 10, 11):  # TX_CLASS_2D, TX_CLASS_VERT (rows), TX_CLASS_HORIZ (columns)
        assert rq.antidiagonal_violations(tx_size, tx_type) == []
        assert sorted(cr.scan_order(tx_size, tx_type).tolist()) == list(range(w * h))
    # the neighbour lists are the ones the contexts read: moving a level at any of them changes a context, at any other position it does not
    for cls, tx_type in ((0, 0), (2, 10), (1, 11)):
        if w * h < 64:
            continue
        T = rq.shared()["tables"][0]
        mk = lambda: rq.Walk(T, tx_size, 0, tx_type, None, None, None, None, None)
        centre = w + 1
        reads = set()
        for pos in range(w * h):
            W = mk()
            W.set_level(pos, 3)
            if (W.ctx(centre), W.br_ctx(centre)) != (mk().ctx(centre), mk().br_ctx(centre)):
                reads.add((pos // w - centre // w, pos % w - centre % w))
        want = {(dr, dc) for dr, dc in rq.context_neighbours(cls) if centre // w + dr < h and centre % w + dc < w}
        assert reads == want, (cls, reads)


def test_rdmult_and_rdcost_arithmetic():
    assert rq.rdmult_of(400, 0, 0, 0, 0) == (400 * 17 + 2) >> 2 and rq.rdmult_of(400, 1, 1, 0, 0) == (400 * 10 + 2) >> 2
    assert rq.rdmult_of(400, 0, 1, 0, 4) == (400 * 13 + 2) >> 4 and rq.rdmult_of(400, 1, 0, 0, 7) == (400 * 16 + 2) >> 7
    assert rq.rdmult_of(1 << 31, 0, 0, 1, 0) == 0 and rq.rdmult_of(400, 0, 0, 0, 1) == rq.rdmult_of(400, 0, 0, 0, 2)
    assert rq.rdcost(1000, 512, -3) == 1000 - 384 and rq.rdcost(7, 100, -1) == ((700 + 256) >> 9) - 128  # dist - dist0 is negative: * 128, no shift
    assert rq.GOLOMB_BITS_COST[:5] == [0, 512, 1536, 1536, 2560] and len(rq.GOLOMB_BITS_COST) == len(rq.GOLOMB_COST_DIFF) == 32
    assert [i for i, v in enumerate(rq.GOLOMB_COST_DIFF) if v] == [1, 2, 4, 8, 16]


def test_the_module_and_its_entries_are_exported():
    from svt_av1_psyex_amd import rdoq
    assert callable(rdoq.run_rdoq_device) and callable(rdoq.run_rdoq_hip)
    L = api.lib()
    for name in ("svt_hip_rdoq_batch", "svt_hip_rdoq_desc_size"):
        assert hasattr(L, name), name


def test_struct_sizes_match_ctypes():
    L = api.lib()
    L.svt_hip_rdoq_desc_size.restype = C.c_size_t
    assert L.svt_hip_rdoq_desc_size() == C.sizeof(abi.RdoqDesc)
    assert C.sizeof(abi.RdoqJob) == 8 == np.dtype(abi.RDOQ_JOB_DTYPE).itemsize == np.dtype(rq.RDOQ_JOB_DTYPE).itemsize
    assert abi.RDOQ_JOB_DTYPE == rq.RDOQ_JOB_DTYPE
    assert (abi.RDOQ_OPTIMISED, abi.RDOQ_EMPTY, abi.RDOQ_GATED, abi.RDOQ_UNDEFINED) == (rq.ST_OPTIMISED, rq.ST_EMPTY, rq.ST_GATED, rq.ST_UNDEFINED)


# (null arguments: tests/test_batch_entries.py)
BAD = ["tx_size_19", "tx_size_255", "plane_type_2", "sharpness_8", "no_jobs", "no_tables", "no_quant_rows", "no_coeff", "no_qcoeff",
       "no_dqcoeff", "no_eob", "zero_quant_rows", "fallback_without_qcoeff_b", "fallback_without_dqcoeff_b", "fallback_without_eob_b"]


@pytest.mark.parametrize("bad", BAD)
def test_bad_descriptor_is_rejected_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_rdoq_desc()
    p = C.c_void_p(0x1000)
    if bad.startswith("tx_size"):
        d.tx_size = int(bad.split("_")[-1])
    elif bad == "plane_type_2":
        d.plane_type = 2
    elif bad == "sharpness_8":
        d.sharpness = 8
    elif bad == "zero_quant_rows":
        d.n_quant_rows = 0
    elif bad.startswith("no_"):
        setattr(d, bad[3:], None)
    else:
        d.qcoeff_b, d.dqcoeff_b, d.eob_b = p, p, p
        setattr(d, bad[len("fallback_without_"):], None)
    assert L.svt_hip_rdoq_batch(ctx, C.byref(d)) == BAD_PARAM
    assert b"svt_hip_rdoq_batch" in L.svt_hip_last_error(None)
