"""GPU: svt_hip_rd_batch where the per-block fixed cost of rd_tx_kernel changed form -- the wave's magnitudes and the block's sums on DPP and
scalar registers, the runs of samples addressed from one base per plane -- at 16x16, 32x32 and 64x64, 8 and 10 bit, bit for bit against the
oracle on eob, satd, both dist_coeff, three_quad_energy, sse, cul_level, qcoeff and the recon plane.

Block sums past 2^32 (test_group_sums_past_32_bits).  Two kinds of block, both with a quantizer row whose quant_shift is 0, so every level is 0
and dist_coeff[0] == dist_coeff[1] == the sum of the squared coefficients:
  "checker"  source (1 << bd) - 1 / prediction 0 in a checkerboard.  At 10 bits its DC coefficient is outside the lean loop's bound at every size,
             so its sums take the 64-bit butterfly.
  "lean"     the largest field of random signs whose wave still takes the lean loop (rd_lean_cases.lane_is_lean): the 32-bit sums of a lane
             that are widened inside the block's reduction (on DPP at 16x16 and 64x64).  That the kernel takes the lean loop for it is
             inferred from that mirror of the kernel's test, as in tests/test_rd_lean_paths_gpu.py: were the two to drift apart, the block
             would pass through the 64-bit butterfly instead.
PAST_32_BITS says where the oracle's dist_coeff of such a block reaches 2^32 (computed on the CPU, asserted below).  At 10 bits the lean block
does at all three sizes (2^32.8 / 2^33.4 / 2^33.4 at 16x16 / 32x32 / 64x64) and the checkerboard at 16x16 and 32x32 (2^33.0); at 64x64 the
checkerboard gives 4,286,223,810, 0.2 % short of 2^32.  At 8 bits no block reaches it: a full-swing residual of any signs, the largest energy
8-bit samples have, gives 2^30.0 / 2^30.0 / 2^29.4 (the lean block is one), the checkerboard 2^29.0 / 2^29.0 / 2^28.0.  Those cases run with
the largest sums the size and bit depth allow."""
import functools

import numpy as np
import pyoracle
import pytest

import rd_edge_cases as E
import rd_lean_cases as L
from svt_av1_psyex_amd import abi, rd
from txfm_cases import TX_H, TX_W, valid_types

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4)  # TX_16X16, TX_32X32, TX_64X64
FILL = 0xA5        # canary byte of every output slot past n_jobs
BENCH = ("qcoeff", "cul_level", "recon")
COMPARED = ("eob", "satd", "dist_coeff", "three_quad_energy", "sse", "cul_level", "qcoeff", "recon")
ZERO_LEVELS = len(E.QUANT_STEPS)  # index of the row whose levels are all zero
PAST_32_BITS = {("checker", 2, 10): True, ("checker", 3, 10): True, ("checker", 4, 10): False, ("lean", 2, 10): True, ("lean", 3, 10): True, ("lean", 4, 10): True,
                ("checker", 2, 8): False, ("checker", 3, 8): False, ("checker", 4, 8): False, ("lean", 2, 8): False, ("lean", 3, 8): False, ("lean", 4, 8): False}


def quant_rows():
    """rd_edge_cases.QUANT_STEPS, then a row with quant_shift 0: every level is zero whatever the coefficient"""
    zero = rd.quant_row_from_step(4, 4).copy()
    zero["quant_shift"][:] = 0
    return np.concatenate([E.quant_rows(), np.stack([zero])])


def lim(bd):
    return (1 << bd) - 1


def noise(rng, ts, bd):
    a = 40 if bd == 8 else 160
    return rng.integers(-a, a + 1, (TX_H[ts], TX_W[ts])).astype(np.int64)


def lay(ts, bd, blocks, odd=False, seed=0):
    """blocks: (tx_type, quant row, pf_shape, H x W residual).  Three blocks per band of rows.  odd=False: one stride (a multiple of 8), blocks
    side by side, source and prediction offsets equal.  odd=True: source and prediction planes of different strides, neither a multiple of 8,
    odd offsets that differ between the planes, gaps between the blocks.  Samples outside the blocks are noise (the recon plane must keep them).
    Returns (desc fields without quant_kind, src, pred, jobs)."""
    w, h, per_row = TX_W[ts], TX_H[ts], 3
    rng = np.random.default_rng(6100 + seed)
    gap_s, gap_p, org_s, org_p = (2, 4, 1, 3) if odd else (0, 0, 0, 0)
    stride_s, stride_p = per_row * (w + gap_s) + org_s + (2 if odd else 0), per_row * (w + gap_p) + org_p + (6 if odd else 0)
    assert (stride_s % 8 != 0 and stride_p % 8 != 0 and stride_s != stride_p) if odd else (stride_s % 8 == 0 and stride_s == stride_p)
    bands = -(-len(blocks) // per_row)
    dt = np.uint8 if bd == 8 else np.uint16
    src = rng.integers(0, lim(bd) + 1, (bands * h + 1, stride_s)).astype(dt)
    pred = rng.integers(0, lim(bd) + 1, (bands * h + 1, stride_p)).astype(dt)
    jobs = np.zeros(len(blocks), abi.JOB_DTYPE)
    for i, (tt, qi, pf, res) in enumerate(blocks):
        assert np.abs(res).max() <= lim(bd)
        y, xs, xp = (i // per_row) * h, org_s + (i % per_row) * (w + gap_s), org_p + (i % per_row) * (w + gap_p)
        src[y:y + h, xs:xs + w] = np.maximum(res, 0)
        pred[y:y + h, xp:xp + w] = np.maximum(-res, 0)
        jobs[i] = (y * stride_s + xs, y * stride_p + xp, tt, qi, pf, 0)
        assert not odd or (jobs[i]["src_offset"] % 2 == 1 and jobs[i]["pred_offset"] % 2 == 1 and jobs[i]["src_offset"] != jobs[i]["pred_offset"])
    return dict(bit_depth=bd, tx_size=ts, src_stride=stride_s, pred_stride=stride_p), np.ascontiguousarray(src), np.ascontiguousarray(pred), jobs


def check(hip_ctx, case, outputs, what, rows=None):
    f0, src, pred, jobs = case
    f, rows = dict(f0, quant_kind=0), quant_rows() if rows is None else rows
    want = pyoracle.rd_batch(f, src, pred, jobs, rows, impl="oracle")
    got = rd.run_hip(hip_ctx, f, src, pred, jobs, rows, outputs=outputs, spare_jobs=E.blocks_per_wave(f["tx_size"]) + 1, fill=FILL)
    n = len(jobs)
    assert set(got) == (set(COMPARED) - set(rd.OPTIONAL_OUTPUTS)) | set(outputs), (what, sorted(got))
    for name, a in got.items():
        if name == "recon":
            assert np.array_equal(a, want[name]), (what, name, np.argwhere(a != want[name])[:3].tolist())
            continue
        assert np.array_equal(a[:n], want[name]), (what, name, np.argwhere(a[:n] != want[name])[:3].tolist())
        assert (a[n:].view(np.uint8) == FILL).all(), (what, name, "written past n_jobs")
    return want, got


def second_type(ts):
    t = valid_types(ts)
    return t[1] if len(t) > 1 else t[0]


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_job_counts(hip_ctx, tx_size, bd):
    """1, 3, 4 and 5 jobs (9 at 16x16): whole waves and a partial last wave, whose lanes of missing blocks run along on job 0"""
    rng = np.random.default_rng(6200 + tx_size + 100 * bd)
    for n in (1, 3, 4, 5) + ((9,) if tx_size == 2 else ()):
        blocks = [(0, 1, 0, noise(rng, tx_size, bd)) for _ in range(n)]
        check(hip_ctx, lay(tx_size, bd, blocks), BENCH, (tx_size, bd, n))


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_mixed_and_sorted_waves(hip_ctx, tx_size, bd):
    """Quantizer rows and transform types alternating job by job (no wave of several blocks is uniform), and the same jobs sorted so that
    every wave is: both orders agree with the oracle, hence with each other job by job"""
    rng = np.random.default_rng(6300 + tx_size + 100 * bd)
    n = 4 * max(E.blocks_per_wave(tx_size), 2)
    blocks = [((0, second_type(tx_size))[(i // 2) % 2], (1, 3)[i % 2], 0, noise(rng, tx_size, bd)) for i in range(n)]
    order = sorted(range(n), key=lambda i: (blocks[i][1], blocks[i][0]))
    mixed, _ = check(hip_ctx, lay(tx_size, bd, blocks), BENCH, (tx_size, bd, "mixed"))
    by_wave, _ = check(hip_ctx, lay(tx_size, bd, [blocks[i] for i in order]), BENCH, (tx_size, bd, "sorted"))
    for name in COMPARED[:-1]:
        assert np.array_equal(mixed[name][order], by_wave[name]), name


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_partial_frequency_job_per_wave(hip_ctx, tx_size, bd):
    """one job with pf_shape 1 in every wave, first, last or alone in it, among full ones"""
    rng = np.random.default_rng(6400 + tx_size + 100 * bd)
    bpw = E.blocks_per_wave(tx_size)
    n = 3 * max(bpw, 2)
    where = {0, bpw + bpw - 1, 2 * bpw + bpw // 2} if bpw > 1 else {0, 2, 5}
    blocks = [(0, 1, 1 if i in where else 0, noise(rng, tx_size, bd)) for i in range(n)]
    want, _ = check(hip_ctx, lay(tx_size, bd, blocks), BENCH, (tx_size, bd))
    assert (want["eob"] > 1).any()


@functools.lru_cache(maxsize=None)
def lean_noise(ts, bd):
    """the largest field of random signs (one field, scaled) whose block alone in a wave takes the lean loop with the zero-level row; at 64x64
    every sample twice in each direction, which puts the energy into the 32 x 32 coefficients the size keeps"""
    h, w = TX_H[ts], TX_W[ts]
    u = np.kron(np.random.default_rng(6500 + ts).choice((-1.0, 1.0), (min(h, 32), min(w, 32))), np.ones((h // min(h, 32), w // min(w, 32))))
    row = quant_rows()[ZERO_LEVELS]
    lean = lambda a: L.lane_is_lean(ts, bd, L.comax_of(ts, 0, np.rint(a * u).astype(np.int64)), row)
    lo, hi = 1, lim(bd) + 1  # lean(lo), not lean(hi) or hi beyond the samples' range
    assert lean(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lean(mid) else (lo, mid)
    return np.rint(lo * u).astype(np.int64)


def checker(ts, bd):
    yy, xx = np.mgrid[0:TX_H[ts], 0:TX_W[ts]]
    return np.where((yy + xx) % 2 == 0, lim(bd), 0).astype(np.int64)


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_group_sums_past_32_bits(hip_ctx, tx_size, bd):
    """a wave of lean-noise blocks (both signs), a wave of checkerboards, every level zero: see the module docstring"""
    bpw = E.blocks_per_wave(tx_size)
    ln, ck = lean_noise(tx_size, bd), checker(tx_size, bd)
    blocks = [(0, ZERO_LEVELS, 0, ln if i % 2 == 0 else -ln) for i in range(bpw)] + [(0, ZERO_LEVELS, 0, ck) for i in range(bpw)]
    want, _ = check(hip_ctx, lay(tx_size, bd, blocks), BENCH, (tx_size, bd))
    assert (want["eob"] == 0).all() and np.array_equal(want["dist_coeff"][:, 0], want["dist_coeff"][:, 1])
    rows = quant_rows()
    assert L.lane_is_lean(tx_size, bd, L.comax_of(tx_size, 0, ln), rows[ZERO_LEVELS])
    assert bd == 8 or not L.lane_is_lean(tx_size, bd, L.comax_of(tx_size, 0, ck), rows[ZERO_LEVELS])
    for kind, job in (("lean", 0), ("checker", bpw)):
        d = int(want["dist_coeff"][job, 0])
        print(f"tx_size {tx_size} bd {bd} {kind}: dist_coeff 2^{np.log2(max(d, 1)):.2f}")
        assert (d >= 1 << 32) == PAST_32_BITS[(kind, tx_size, bd)], (kind, d)


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_lean_beside_general(hip_ctx, tx_size, bd):
    """constant full-swing residuals of both signs (at 10 bits coefficients of 2^16 and more: the general loop) beside small ones, in one wave where
    a wave holds several blocks and in neighbouring waves"""
    rng = np.random.default_rng(6600 + tx_size + 100 * bd)
    n = 3 * max(E.blocks_per_wave(tx_size), 2)
    flat = np.full((TX_H[tx_size], TX_W[tx_size]), lim(bd), np.int64)
    blocks = [(0, 1, 0, (flat if i % 4 == 1 else -flat) if i % 2 == 1 and i < n - 2 else noise(rng, tx_size, bd)) for i in range(n)]
    if bd == 10:
        assert L.comax_of(tx_size, 0, flat) >= 1 << 16
    check(hip_ctx, lay(tx_size, bd, blocks), BENCH, (tx_size, bd))


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_null_outputs_in_turn(hip_ctx, tx_size, bd):
    """recon, cul_level and qcoeff null in turn (without qcoeff no wave takes the lean loop)"""
    rng = np.random.default_rng(6700 + tx_size + 100 * bd)
    blocks = [(0, 1 + i % 2, 0, noise(rng, tx_size, bd)) for i in range(2 * max(E.blocks_per_wave(tx_size), 2) + 1)]
    case = lay(tx_size, bd, blocks)
    for outputs in (("qcoeff", "cul_level"), ("qcoeff", "recon"), ("cul_level", "recon")):
        check(hip_ctx, case, outputs, (tx_size, bd, outputs))


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("tx_size", SIZES)
def test_odd_strides_and_offsets(hip_ctx, tx_size, bd):
    """source and prediction strides that are no multiples of 8 and differ, odd offsets that differ between the planes: the run addresses"""
    rng = np.random.default_rng(6800 + tx_size + 100 * bd)
    blocks = [((0, second_type(tx_size))[i % 2], 1, 0, noise(rng, tx_size, bd)) for i in range(2 * max(E.blocks_per_wave(tx_size), 2) + 1)]
    for outputs in (BENCH, ("qcoeff", "cul_level")):
        check(hip_ctx, lay(tx_size, bd, blocks, odd=True), outputs, (tx_size, bd, outputs))
