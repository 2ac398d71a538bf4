"""GPU: svt_hip_rd_batch around the wave-uniform decision of the lean quantizer loop, in partial last waves and in waves that mix flipping
and non-flipping transform types (tests/rd_lean_cases.py), bit for bit against the oracle on every output of abi.RD_OUT_FIELDS, qcoeff and the recon plane."""
import numpy as np
import pyoracle
import pytest

import rd_edge_cases as E
import rd_lean_cases as L
from svt_av1_psyex_amd import abi, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5  # canary byte of every output slot past n_jobs
BENCH = ("qcoeff", "cul_level", "recon")  # bench.py's output set: the fast quantizer loops with qcoeff stores


def _check(hip_ctx, f, src, pred, jobs, rows, outputs, what):
    want = pyoracle.rd_batch(f, src, pred, jobs, rows, impl="oracle")
    got = rd.run_hip(hip_ctx, f, src, pred, jobs, rows, outputs=outputs, spare_jobs=E.blocks_per_wave(f["tx_size"]) + 1, fill=FILL)
    n = len(jobs)
    assert set(got) == {nm for nm, _, _ in abi.RD_OUT_FIELDS if nm != "cul_level"} | set(outputs), (what, sorted(got))
    for name, a in got.items():
        if name == "recon":
            assert np.array_equal(a, want[name]), (what, name, np.argwhere(a != want[name])[:3].tolist())
            continue
        assert np.array_equal(a[:n], want[name]), (what, name, np.argwhere(a[:n] != want[name])[:3].tolist())
        assert (a[n:].view(np.uint8) == FILL).all(), (what, name, "written past n_jobs")
    return want


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", L.SIZES)
def test_rd_batch_lean_bounds(hip_ctx, tx_size, bd):
    """Largest |coeff| at, one above and (32-bit product bound) one below the largest value the lean loop accepts, for every row of
    rd_edge_cases.QUANT_STEPS (the 32-bit sum bound) and the large-round row (the 32-bit product bound; at 8 bits the int16 clamp of
    |coeff| + round): the block beyond the bound first / last among blocks at it, all at it, all beyond it; both signs of DC and AC."""
    rows = L.lean_rows(tx_size, bd)
    waves, expect = L.bound_waves(tx_size, bd)
    ac, neg, pos = 0, False, False
    for i, (f0, src, pred, jobs) in enumerate(L.batches(tx_size, bd, waves)):
        want = _check(hip_ctx, dict(f0, quant_kind=0), src, pred, jobs, rows, BENCH, (tx_size, bd, i))
        ac += int((want["eob"] > 1).sum())
        neg, pos = neg or bool((want["qcoeff"][:, 0] < 0).any()), pos or bool((want["qcoeff"][:, 0] > 0).any())
    assert ac > 0 and neg and pos  # AC levels, and DC levels of both signs


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size,n_jobs", ((1, 13), (2, 5), (3, 3), (7, 7)))
def test_rd_batch_lean_partial_wave(hip_ctx, tx_size, n_jobs, bd):
    """n_jobs not a multiple of the blocks per wave: the full waves store qcoeff without a predicate, the last wave keeps it.  With coeff or
    dqcoeff also requested the real blocks take the general loop while the missing blocks' lanes take a fast one."""
    f0, src, pred, jobs = L.partial_wave_case(tx_size, bd, n_jobs)
    rows = L.lean_rows(tx_size, bd)
    for outputs in (BENCH, BENCH + ("coeff",), BENCH + ("dqcoeff",), ("qcoeff",)):
        _check(hip_ctx, dict(f0, quant_kind=0), src, pred, jobs, rows, outputs, (tx_size, bd, outputs))


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", L.FLIP_SIZES)
def test_rd_batch_flip_mixes(hip_ctx, tx_size, bd):
    """waves that mix a vertically flipping type with a non-flipping one (FLIPADST_DCT beside DCT_DCT, first and last block), all-flip and
    no-flip waves, both quantizers"""
    f0, src, pred, jobs = L.flip_case(tx_size, bd)
    rows = E.quant_rows()
    for quant_kind in (0, 1):
        for outputs in (BENCH, BENCH + ("coeff", "dqcoeff")):
            _check(hip_ctx, dict(f0, quant_kind=quant_kind), src, pred, jobs, rows, outputs, (tx_size, bd, quant_kind, outputs))
