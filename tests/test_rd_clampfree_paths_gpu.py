"""GPU: svt_hip_inv_txfm_batch and svt_hip_rd_batch around the clamp-free tier of the inverse passes (ipass_clamp_free, txfm_core.h) and the
input clamps that run only where a wave needs them, bit for bit against the oracle.

An inverse pass drops its stage clamps when gain64(N) x the wave's largest raw |input| + 64 slack(N) < 64 x 2^(CLAMP - 1) (CLAMP 18 for the
10-bit row pass, else 16; tests/inv_flow_graph.py derives the constants, tests/test_inv_clamp_bounds.py checks them); the choice is one
per wave, so every case is a batch of 9 jobs -- at 16x16 two full waves and a partial one -- with the extreme block first in the first
wave and last in the second, among small blocks.  One block beyond a limit takes its whole wave to the clamped code.  The cases:
  row at / above     dense blocks whose largest row-pass input is exactly the limit / one above it
  col at / above     blocks whose row-pass outputs land at most at the column limit / above it (by bisection on the oracle's row pass)
  entry              inputs at and beyond the bd + 8 clamp of the row pass (2^(bd+7) and the int32 extremes) and row outputs beyond the
                     16-bit clamp of the column pass: the clamps still act
  stage              dense one-signed blocks at 2^18 / W - 1, whose last-stage sums pass the stage clamps while the pass is bounded
  quantizer bound    svt_hip_rd_batch: lean-quantizer waves whose bound M on |dqcoeff| is at / above the row limit
for the square 16 / 32 / 64-point sizes, TX_16X32 (a rectangular 32-lane layout) and TX_64X16, both bit depths, every transform type of
each size as the extreme block's.  Which sizes have the tier and which clamp on load is the kernels' choice (rd_clamp_free_tier,
rd_skip_entry_clamps in rd_kernel.hip: the tier at 64x64, a build switch gives it to 16x16 and 32x32 as well); the limits are those of
the pass lengths, and every size has to be exact on both sides of them either way."""
import ctypes as C
import functools

import numpy as np
import pyoracle
import pytest

import inv_flow_graph as F
import rd_edge_cases as E
import rd_lean_cases as L
from svt_av1_psyex_amd import abi, rd
from txfm_cases import TX_H, TX_W, valid_types

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 9, 18)  # TX_16X16, TX_32X32, TX_64X64, TX_16X32, TX_64X16
TIERED = (2, 3, 4)
N_JOBS = 9
PW = 192
FILL = 0xA5
BENCH = ("qcoeff", "cul_level", "recon")


def _row_clamp(bd):
    return 16 if bd == 8 else 18


def _tier(max_abs, n, clamp_bits):
    """the kernels' choice for an n-point pass: 2 clamp-free, 1 bounded, 0 general"""
    if max_abs <= F.clamp_free_limit(n, clamp_bits):
        return 2
    return 1 if max_abs * n < (1 << 18) else 0


def _raw_row_input_max(ts, block):
    v = np.asarray(block, np.int64)
    if TX_W[ts] == 2 * TX_H[ts] or TX_H[ts] == 2 * TX_W[ts]:
        v = (v * 2896 + 2048) >> 12
    return int(np.abs(v).max())


def _extreme_slots(ts):
    bpw = E.blocks_per_wave(ts)
    return (0, 2 * bpw - 1)  # first of the first wave, last of the second


def _small(rng, ts):
    n = min(TX_W[ts], 32) * min(TX_H[ts], 32)
    return rng.choice([-1, 1], n) * 100


def _batch(rng, ts, extreme):
    """[9, NP] int64: `extreme` in the two extreme slots, small dense blocks elsewhere"""
    co = np.stack([_small(rng, ts) for _ in range(N_JOBS)]).astype(np.int64)
    for s in _extreme_slots(ts):
        co[s] = extreme
    return co


def _inv_want(oracle, ts, bd, pred, jobs, co):
    p16, r16 = np.ascontiguousarray(pred, np.uint16), np.ascontiguousarray(pred, np.uint16).copy()
    for j, jb in enumerate(jobs):
        po = int(jb["pred_offset"])
        oracle.orc_inv_txfm2d_add(C.c_void_p(co[j].ctypes.data), C.c_void_p(p16.ctypes.data + 2 * po), C.c_int32(pred.shape[1]),
                                  C.c_void_p(r16.ctypes.data + 2 * po), C.c_int32(pred.shape[1]), int(jb["tx_type"]), ts, bd)
    return r16


def _run_inverse(hip_ctx, oracle, rng, ts, bd, tt, co, what):
    w, h = TX_W[ts], TX_H[ts]
    ph = -(-N_JOBS // (PW // w)) * h
    jobs = rd.grid_jobs(PW, ph, PW, ts)[:N_JOBS].copy()
    types = valid_types(ts)
    jobs["tx_type"] = [types[(j + tt) % len(types)] for j in range(N_JOBS)]
    for s in _extreme_slots(ts):
        jobs["tx_type"][s] = tt
    co = np.ascontiguousarray(co, np.int32)
    pred = rng.integers(0, 1 << bd, (ph, PW)).astype(np.uint16)
    want = _inv_want(oracle, ts, bd, pred, jobs, co)
    got = rd.run_inv_hip(hip_ctx, bd, ts, pred, jobs, co)
    assert np.array_equal(got, want), (what, ts, bd, tt, np.argwhere(got != want)[:3].tolist())
    return jobs


def _wave_tiers(oracle, ts, bd, jobs, co):
    """(row tier, column tier) per wave, as the kernels decide them from the raw magnitudes"""
    bpw = E.blocks_per_wave(ts)
    out = []
    for j0 in range(0, N_JOBS, bpw):
        sl = range(j0, min(j0 + bpw, N_JOBS))
        rmax = max(_raw_row_input_max(ts, co[j]) for j in sl)
        cmax = max(E.inv_col_input_max(oracle, ts, bd, jobs[j]["tx_type"], co[j]) for j in sl)
        out.append((_tier(rmax, TX_W[ts], _row_clamp(bd)), _tier(cmax, TX_H[ts], 16)))
    return out


@pytest.mark.parametrize("bd", (10, 8))
@pytest.mark.parametrize("tx_size", SIZES)
def test_inverse_batch_at_the_row_limit(hip_ctx, oracle, tx_size, bd):
    rng = np.random.default_rng(9100 + tx_size + 100 * bd)
    n = min(TX_W[tx_size], 32) * min(TX_H[tx_size], 32)
    limit = F.clamp_free_limit(TX_W[tx_size], _row_clamp(bd))
    assert limit + 1 < (1 << (bd + 7))  # both sides are inside the bd + 8 input clamp
    seen = set()
    for tt in valid_types(tx_size):
        for m in (limit, limit + 1):
            v = E._rect_pre(tx_size, m)
            for signs in (rng.choice([-1, 1], n), np.ones(n, np.int64), -np.ones(n, np.int64)):
                co = _batch(rng, tx_size, signs * v)
                assert _raw_row_input_max(tx_size, co[0]) == m
                jobs = _run_inverse(hip_ctx, oracle, rng, tx_size, bd, tt, co, ("row", m - limit))
            tiers = _wave_tiers(oracle, tx_size, bd, jobs, co)
            assert tiers[0][0] == tiers[1][0], (tt, m, tiers)  # the extreme block decides for its whole wave, first or last in it
            assert (tiers[0][0] == 2) == (m == limit), (tt, m, tiers)  # one above: bounded, or general where W x (limit + 1) >= 2^18 (64 points at 10 bits)
            seen.add(tiers[0][0] == 2)
            assert tiers[-1][0] == 2 or E.blocks_per_wave(tx_size) == 1  # the partial wave holds small blocks only
    assert seen == {True, False}


def _col_block(ts, pattern, v):
    """rd_edge_cases._col_block, and "col": the first coefficient of every row, so that every input of every column pass is large"""
    if pattern != "col":
        return E._col_block(ts, pattern, v)
    wp, hp = min(TX_W[ts], 32), min(TX_H[ts], 32)
    b = np.zeros(wp * hp, np.int64)
    b[::wp] = v
    return b


@functools.lru_cache(maxsize=None)
def _col_crossing(ts, bd, tt, bound):
    """(pattern, sign, v): the first stored value at which the block's largest |column-pass input| exceeds `bound`, as
    rd_edge_cases.inv_col_crossing finds it for the bounded butterflies' bound; None where the input clamp keeps every block at or below it"""
    orc = pyoracle.load_oracle()
    for pattern in ("col", "dc", "row", "dense"):
        for sign, top in ((1, E._rect_pre(ts, (1 << (bd + 7)) - 1)), (-1, E._rect_pre(ts, 1 << (bd + 7)))):
            f = lambda v: E.inv_col_input_max(orc, ts, bd, tt, sign * _col_block(ts, pattern, v))
            if f(top) <= bound:
                continue
            hi = 1
            while f(hi) <= bound:
                hi = min(2 * hi, top)
            lo = hi // 2
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if f(mid) > bound:
                    hi = mid
                else:
                    lo = mid
            if f(hi - 1) <= bound < f(hi):
                return pattern, sign, hi
    return None


@pytest.mark.parametrize("bd", (10, 8))
@pytest.mark.parametrize("tx_size", SIZES)
def test_inverse_batch_at_the_column_limit(hip_ctx, oracle, tx_size, bd):
    rng = np.random.default_rng(9200 + tx_size + 100 * bd)
    limit = F.clamp_free_limit(TX_H[tx_size], 16)
    seen = set()
    for tt in valid_types(tx_size):
        cross = _col_crossing(tx_size, bd, tt, limit)
        assert cross is not None, (tx_size, bd, tt)
        pattern, sign, v = cross
        for x in (v - 1, v):
            co = _batch(rng, tx_size, sign * _col_block(tx_size, pattern, x))
            jobs = _run_inverse(hip_ctx, oracle, rng, tx_size, bd, tt, co, ("col", x - v))
            tiers = _wave_tiers(oracle, tx_size, bd, jobs, co)
            assert (tiers[0][1] == 2) == (x < v), (tt, x, tiers)
            seen.add(tiers[0][1] == 2)
    assert seen == {True, False}


@pytest.mark.parametrize("bd", (10, 8))
@pytest.mark.parametrize("tx_size", SIZES)
def test_inverse_batch_where_the_clamps_act(hip_ctx, oracle, tx_size, bd):
    """the input clamps of both passes (values at and beyond 2^(bd+7), the int32 extremes; row outputs beyond 16 bits) and the stage clamps
    (dense one-signed blocks at the bounded butterflies' limit), each among blocks that take the clamp-free tier in the other waves"""
    rng = np.random.default_rng(9300 + tx_size + 100 * bd)
    n = min(TX_W[tx_size], 32) * min(TX_H[tx_size], 32)
    lim = 1 << (bd + 7)
    bound = E.inv_fast_limit(TX_W[tx_size])
    types = valid_types(tx_size)
    k = 0
    clamped_rows = clamped_cols = 0
    for v in (lim - 1, -lim, lim, -lim - 1, 4 * lim + 3, -(1 << 31), (1 << 31) - 1, bound, -bound, bound + 1):
        for pattern in ("dc", "row", "dense", "one"):
            if pattern == "one":  # a single value beyond the clamp in an otherwise small block: only the raw maximum tells
                blk = _small(rng, tx_size).astype(np.int64)
                blk[int(rng.integers(0, n))] = v
            else:
                pre = E._rect_pre(tx_size, abs(v)) if abs(v) < (1 << 30) else abs(v)
                blk = np.clip(np.sign(v) * E._col_block(tx_size, pattern, pre), -(1 << 31), (1 << 31) - 1)
            tt = types[k % len(types)]
            k += 1
            co = _batch(rng, tx_size, blk)
            jobs = _run_inverse(hip_ctx, oracle, rng, tx_size, bd, tt, co, ("clamps", v, pattern))
            clamped_rows += _raw_row_input_max(tx_size, co[0]) >= lim
            clamped_cols += E.inv_col_input_max(oracle, tx_size, bd, tt, co[0]) >= (1 << 15)
    # at 8 bits the row pass's 16-bit stage clamps and its round-shift keep every DCT / ADST row output inside the column pass's 16-bit input clamp
    assert clamped_rows >= 16 and (clamped_cols >= 4 or bd == 8), (clamped_rows, clamped_cols)


# ---- svt_hip_rd_batch: the row pass's bound from the quantizer ---------------------------------------------------------------------
def _m_of(ts, bd, comax, row):
    nonneg, tmax, m = L.lane_limits(ts, bd, comax, row)
    assert nonneg
    return m


def _largest_comax_with_m_within(ts, bd, row, limit):
    lo, hi = 0, 1 << 16  # M is monotonic in comax
    assert _m_of(ts, bd, lo, row) <= limit
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _m_of(ts, bd, mid, row) <= limit:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("bd", (10, 8))
@pytest.mark.parametrize("tx_size", TIERED)
def test_rd_batch_row_bound_from_the_quantizer(hip_ctx, tx_size, bd):
    """lean-quantizer waves whose M = max(comax, dqmax) is the largest within the row pass's clamp-free limit, and one coefficient step
    beyond it (there the wave measures its row input as before); the extreme block first in the first wave and last in the second"""
    rows = E.quant_rows()
    limit = F.clamp_free_limit(TX_W[tx_size], _row_clamp(bd))
    bpw = E.blocks_per_wave(tx_size)
    sides = set()
    for qi in (0, 1):  # steps 4 and 342
        c = _largest_comax_with_m_within(tx_size, bd, rows[qi], limit)
        for target in (c, c + 1):
            if not L.lane_is_lean(tx_size, bd, target, rows[qi]):
                continue
            big = [L.block_with_comax(tx_size, 0, bd, target, sign, seed=s) for s, sign in ((0, 1), (1, -1))]
            if any(b is None for b in big):
                continue
            rng = np.random.default_rng(9400 + tx_size + 100 * bd + qi)
            amp = 6 if bd == 8 else 24
            blocks = [rng.integers(-amp, amp + 1, (TX_H[tx_size], TX_W[tx_size])).astype(np.int64) for _ in range(N_JOBS)]
            for s, b in zip(_extreme_slots(tx_size), big):
                blocks[s] = b
            waves = [[(0, qi, b) for b in blocks[j:j + bpw]] for j in range(0, N_JOBS, bpw)]
            for f0, src, pred, jobs in L.batches(tx_size, bd, waves):
                f = dict(f0, quant_kind=0)
                want = pyoracle.rd_batch(f, src, pred, jobs, rows, impl="oracle")
                got = rd.run_hip(hip_ctx, f, src, pred, jobs, rows, outputs=BENCH, spare_jobs=bpw + 1, fill=FILL)
                n = len(jobs)
                for name, a in got.items():
                    if name == "recon":
                        assert np.array_equal(a, want[name]), (tx_size, bd, qi, target - c, name)
                        continue
                    assert np.array_equal(a[:n], want[name]), (tx_size, bd, qi, target - c, name, np.argwhere(a[:n] != want[name])[:3].tolist())
                    assert (a[n:].view(np.uint8) == FILL).all(), (tx_size, bd, qi, name, "written past n_jobs")
            cm = L.comax_of(tx_size, 0, big[0])
            assert cm == target
            sides.add(_m_of(tx_size, bd, cm, rows[qi]) <= limit)
    assert sides == {True, False}, (tx_size, bd, sides)
