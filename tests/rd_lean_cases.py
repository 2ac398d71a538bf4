"""Cases aimed at the lean form of the RD kernel's "b" quantizer loop (rd_kernel.hip, `lean_q`) and at waves that mix vertically flipping
and non-flipping transform types in the column passes, shared by the CPU test (tests/test_rd_lean_bounds.py: the arithmetic is exact
up to its bounds, and the cases land on the side of a bound they aim at) and the GPU test (tests/test_rd_lean_paths_gpu.py: the kernels
agree with the oracle on them).

The lean loop is taken by a wave when every lane passes (mirrored by lane_is_lean below):
  every block of the wave exists and stores qcoeff, round / quant_shift / dequant are not negative,
  tmax = comax + max(round) (8 bits: at most 32767) < 2^(18 - KT), KT = 4 at log-scale 2, else 3       (32-bit quantizer products)
  M = max(comax, dqmax) < 2^16 and (NP / LW) * M^2 < 2^32, dqmax = the quantizer applied to tmax     (32-bit distortion sums)
with comax the largest |coefficient| of the wave.  With rows built the AV1 way dqmax is about tmax, so the second bound is the one a
block meets first (at log-scale 2 the two nearly coincide); the first is met alone with a row whose round is large against its step
(big_round_row).  Every decision is per wave: the cases put one block beyond a bound among blocks below it, first and last in the wave."""
import functools

import numpy as np

import rd_edge_cases as E
from svt_av1_psyex_amd import abi, rd
from txfm_cases import TX_H, TX_W, valid_types

SIZES = (1, 2, 3, 4, 17)  # TX_8X8, TX_16X16, TX_32X32, TX_64X64 and TX_16X64 (rectangular, log-scale 1)
FLIP_SIZES = (1, 2, 7)    # sizes that allow FLIPADST: TX_8X8, TX_16X16, TX_8X16
PLANE_W, PLANE_H = 192, 128
FLIPADST_DCT, DCT_DCT = 4, 0


def log_scale(ts):
    return E.LOG_SCALE[ts]


def kt(ts):
    """bits the lean loop shifts tmp up by before its v_mul_hi_u32_u24"""
    return 4 if log_scale(ts) == 2 else 3


def per_lane(ts):
    """coefficients a lane walks: NP / LW"""
    return min(TX_W[ts], 32) * min(TX_H[ts], 32) // max(TX_W[ts], TX_H[ts])


def t_bound(ts):
    """the lean loop needs |coeff| + round <= this"""
    return (1 << (18 - kt(ts))) - 1


def _rs(v, ls):
    return (int(v) + (1 << (ls - 1))) >> ls if ls else int(v)


def lane_limits(ts, bd, comax, row):
    """(nonneg, tmax, M) as the kernel computes them for a lane whose block uses `row`, the wave's largest |coeff| being comax"""
    ls = log_scale(ts)
    rnd = [_rs(row["round"][i], ls) for i in (0, 1)]
    s, d, q = [int(x) for x in row["quant_shift"]], [int(x) for x in row["dequant"]], [int(x) for x in row["quant"]]
    nonneg = min(rnd + s + d) >= 0
    if not nonneg:
        return False, 0, 0
    tmax = comax + max(rnd)
    if bd == 8:
        tmax = min(tmax, 32767)
    qvmax = (((tmax * (max(q) + 65536)) >> 11) * max(s)) >> (21 - ls)
    dqmax = (qvmax * max(d)) >> ls
    return True, tmax, max(comax, dqmax)


def lane_is_lean(ts, bd, comax, row):
    nonneg, tmax, m = lane_limits(ts, bd, comax, row)
    return nonneg and tmax <= t_bound(ts) and m < (1 << 16) and per_lane(ts) * m * m < (1 << 32)


def largest_lean_comax(ts, bd, row):
    """the largest comax at which a wave of blocks using `row` takes the lean loop (lane_is_lean is monotonic in comax); -1 if none"""
    lo, hi = -1, 1 << 16
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lane_is_lean(ts, bd, mid, row):
            lo = mid
        else:
            hi = mid
    return lo


def binding_bound(ts, bd, comax, row):
    """which bound rejects comax: "t", "sum" or None"""
    nonneg, tmax, m = lane_limits(ts, bd, comax, row)
    if tmax > t_bound(ts):
        return "t"
    if m >= (1 << 16) or per_lane(ts) * m * m >= (1 << 32):
        return "sum"
    return None


def big_round_row(ts, bd, comax):
    """a row whose round puts |coeff| + round exactly at t_bound for |coeff| = comax while the distortion bound is far: unit dequantizer,
    quant = 0 (Q = 2^16), quant_shift = 2^10, zbin 1.  At bit depth 8 and KT = 3 the int16 clamp keeps every t within the bound: there the
    round is 32000, which (at log-scale 0) makes the clamp active from |coeff| = 768 on."""
    ls = log_scale(ts)
    row = rd.quant_row_from_step(4, 4).copy()
    target = t_bound(ts) - comax  # the round after the log-scale shift
    r = 32000 if (bd == 8 and kt(ts) == 3) else min((target << ls), 32767)
    for i in (0, 1):
        row["zbin"][i], row["round"][i], row["quant"][i], row["quant_shift"][i], row["dequant"][i] = 1, r, 0, 1 << 10, 1
    return row


# ---- blocks with a chosen largest |coefficient| -----------------------------------------------------------------------------------
def _noise(ts, bd, seed):
    rng = np.random.default_rng(5100 + seed)
    a = 6 if bd == 8 else 48
    return rng.integers(-a, a + 1, (TX_H[ts], TX_W[ts])).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _block_cached(ts, tt, bd, target, sign, seed):
    import pyoracle
    orc = pyoracle.load_oracle()
    lim = 255 if bd == 8 else 4095  # far enough for every bound here; larger int16 residuals wrap inside the passes
    noise = _noise(ts, bd, seed)
    h, w = TX_H[ts], TX_W[ts]
    n = h * w

    # level idx // n everywhere, one more on the first idx % n samples (raster order): the DC coefficient grows by about 1 or less per step
    def make(idx):
        lvl = np.full(n, idx // n, np.int64)
        lvl[:idx % n] += 1
        return sign * lvl.reshape(h, w) + noise

    f = lambda idx: int(np.abs(E.fwd_full(orc, ts, tt, make(idx))).max())
    top = (lim - int(np.abs(noise).max())) * n
    if f(top) < target or f(0) >= target:
        return None
    lo, hi = 0, top  # f(lo) < target <= f(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(mid) >= target:
            hi = mid
        else:
            lo = mid
    for idx in range(hi, min(hi + 16, top) + 1):  # rounding can make a step skip a value
        if f(idx) == target:
            b = make(idx)
            assert np.abs(b).max() <= lim
            return b
    return None


def block_with_comax(ts, tt, bd, target, sign=1, seed=0):
    """H x W int64 residual (a flat level of the given sign, its first samples one step higher, and low noise) whose largest |coefficient|
    under the oracle's forward transform is exactly `target`; None where the bit depth's residual range cannot reach it"""
    for retry in range(8):  # the passes' rounding makes some values unreachable with one noise field: try another
        b = _block_cached(ts, tt, bd, int(target), int(sign), int(seed) + 100 * retry)
        if b is not None:
            return b.copy()
    return None


def comax_of(ts, tt, block):
    import pyoracle
    return int(np.abs(E.fwd_full(pyoracle.load_oracle(), ts, tt, block)).max())


# ---- waves, planes, batches ---------------------------------------------------------------------------------------------------------
def capacity(ts):
    return (PLANE_W // TX_W[ts]) * (PLANE_H // TX_H[ts])


def batches(ts, bd, waves):
    """waves: lists of (tt, quant row index, residual block), each list at most one wave long.  Packs whole waves into planes of at most
    PLANE_H x PLANE_W; yields (desc fields without quant_kind, src, pred, jobs) per plane.  A short wave is padded only by the end of the
    batch (so it must be the last of `waves` to stay short)."""
    bpw, cap = E.blocks_per_wave(ts), capacity(ts)
    w, h = TX_W[ts], TX_H[ts]
    per_row = PLANE_W // w
    out, cur = [], []
    for wave in waves:
        assert len(wave) <= bpw
        if len(cur) + len(wave) > cap:
            out.append(cur)
            cur = []
        assert len(cur) % bpw == 0
        cur = cur + list(wave)
    if cur:
        out.append(cur)
    for blocks in out:
        rows_used = -(-len(blocks) // per_row)
        plane = np.zeros((rows_used * h, PLANE_W), np.int64)
        jobs = np.zeros(len(blocks), abi.JOB_DTYPE)
        for i, (tt, qi, b) in enumerate(blocks):
            y, x = (i // per_row) * h, (i % per_row) * w
            plane[y:y + h, x:x + w] = b
            jobs[i]["src_offset"] = jobs[i]["pred_offset"] = y * PLANE_W + x
            jobs[i]["tx_type"], jobs[i]["quant_row"] = tt, qi
        src, pred = E.planes_for_residual(plane, bd)
        yield dict(bit_depth=bd, tx_size=ts, src_stride=PLANE_W, pred_stride=PLANE_W), src, pred, jobs


def _waves_of(ts, tt, bd, qi, below, beyond, k):
    """the four waves of rd_edge_cases._pair_waves with largest |coeff| `below` / `beyond`; signs alternate from block to block (negative DC
    and AC at the bound) starting with k's parity.  None where a magnitude cannot be reached."""
    waves = []
    for j, wave in enumerate(E._pair_waves(E.blocks_per_wave(ts), below, beyond)):
        blocks = [block_with_comax(ts, tt, bd, c, 1 if (i + j + k) % 2 == 0 else -1, seed=i) for i, c in enumerate(wave)]
        if any(b is None for b in blocks):
            return None
        waves.append([(tt, qi, b) for b in blocks])
    return waves


def lean_rows(ts, bd):
    """the rows of rd_edge_cases.QUANT_STEPS, then big_round_row aimed at |coeff| = 1000"""
    return np.concatenate([E.quant_rows(), np.stack([big_round_row(ts, bd, 1000)])])


BIG_ROUND = len(E.QUANT_STEPS)  # index of big_round_row in lean_rows


def bound_waves(ts, bd):
    """(waves, expectations): for every row of lean_rows the waves of _waves_of around the row's largest lean comax c* (below = c*, beyond =
    c* + 1), where the bit depth reaches it; else one wave at the largest magnitude it does reach.  For big_round_row also one wave at
    c* - 1.  expectations: per wave (quant row index, wave comax, lean expected, bound that rejects it or None)."""
    rows = lean_rows(ts, bd)
    bpw = E.blocks_per_wave(ts)
    tt = DCT_DCT
    waves, expect = [], []
    for qi in range(len(rows)):
        c = largest_lean_comax(ts, bd, rows[qi])
        assert c > 0
        ws = _waves_of(ts, tt, bd, qi, c, c + 1, qi)
        if ws is None:  # the bound is out of the bit depth's reach: the largest flat residual, all lean
            lim = 255 if bd == 8 else 32767
            blocks = []
            for i in range(bpw):
                b = (1 if (i + qi) % 2 == 0 else -1) * np.full((TX_H[ts], TX_W[ts]), lim - 6, np.int64) + _noise(ts, 8, i)
                blocks.append((tt, qi, b))
            cm = max(comax_of(ts, tt, b[2]) for b in blocks)
            waves.append(blocks)
            expect.append((qi, cm, lane_is_lean(ts, bd, cm, rows[qi]), binding_bound(ts, bd, cm, rows[qi])))
            continue
        if qi == BIG_ROUND:
            extra = [block_with_comax(ts, tt, bd, c - 1, -1 if i % 2 == 0 else 1, seed=i) for i in range(bpw)]
            if all(b is not None for b in extra):
                ws.append([(tt, qi, b) for b in extra])
        for wave in ws:
            cm = max(comax_of(ts, tt, b[2]) for b in wave)
            waves.append(wave)
            expect.append((qi, cm, cm <= c, binding_bound(ts, bd, cm, rows[qi])))
    return waves, expect


def partial_wave_case(ts, bd, n_jobs):
    """n_jobs random blocks (not a multiple of the blocks per wave), every row of lean_rows in turn: (fields, src, pred, jobs)"""
    assert n_jobs % E.blocks_per_wave(ts) != 0 and n_jobs <= capacity(ts)
    rng = np.random.default_rng(5200 + ts + 100 * bd)
    amp = 40 if bd == 8 else 160
    types = valid_types(ts)
    wave = [(types[i % len(types)], i % (len(E.QUANT_STEPS) + 1), rng.integers(-amp, amp + 1, (TX_H[ts], TX_W[ts])).astype(np.int64)) for i in range(n_jobs)]
    bpw = E.blocks_per_wave(ts)
    (case,) = batches(ts, bd, [wave[i:i + bpw] for i in range(0, n_jobs, bpw)])
    return case


def flip_case(ts, bd):
    """waves that mix a flipping column type with a non-flipping one: FLIPADST_DCT first / last among DCT_DCT, all FLIPADST_DCT, all DCT_DCT,
    then every type whose column pass flips beside its unflipped partner: (fields, src, pred, jobs)"""
    rng = np.random.default_rng(5300 + ts + 100 * bd)
    bpw = E.blocks_per_wave(ts)
    amp = 40 if bd == 8 else 160
    blk = lambda: rng.integers(-amp, amp + 1, (TX_H[ts], TX_W[ts])).astype(np.int64)
    layouts = [[FLIPADST_DCT] + [DCT_DCT] * (bpw - 1), [DCT_DCT] * (bpw - 1) + [FLIPADST_DCT], [FLIPADST_DCT] * bpw, [DCT_DCT] * bpw]
    flips = [t for t in valid_types(ts) if E.VTX[t] == 2]
    plain = [t for t in valid_types(ts) if E.VTX[t] != 2]
    layouts.append([(flips + plain)[i % len(flips + plain)] for i in range(bpw)])
    layouts.append([(plain + flips)[(3 * i) % len(flips + plain)] for i in range(bpw)])
    waves = [[(t, (i + j) % len(E.QUANT_STEPS), blk()) for i, t in enumerate(lay)] for j, lay in enumerate(layouts)]
    (case,) = batches(ts, bd, waves)
    return case
