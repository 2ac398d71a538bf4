"""Cases aimed at the bounds behind the fast paths of the RD and transform kernels (rd_kernel.hip, txfm_core.h), shared by the CPU
tests (tests/test_rd_edges.py: the oracle agrees with the reference on them, and they reach their regimes) and the GPU tests
(tests/test_rd_edges_gpu.py: the kernels agree with the oracle on them).

The paths and the bounds they rest on:
  fast_col / fast_row  forward butterflies in 24-bit multiplies: N x (largest pass input, after the column pass's up-shift) < 2^17
  q24                  quantizer products in 24 bits: every |coeff| of the wave < 2^16
  fast_q               the separate "b" quantizer loop (flat matrix, pf_shape 0, neither coeff nor dqcoeff requested), whose 8-bit
                       path clamps |coeff| + round to int16
  fast_irow / fast_icol inverse butterflies: N x (largest pass input) < 2^18
Every decision is taken per wave (64 lanes = 64 / max(W, H) blocks), so the cases put one block beyond a bound among blocks below it,
first and last in the wave."""
import ctypes as C
import functools

import numpy as np

from svt_av1_psyex_amd import abi, rd
from txfm_cases import TX_H, TX_W, valid_types

VTX = [0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3]  # 1-D type of the column pass per TxType: 0 DCT, 1 ADST, 2 FLIPADST, 3 identity
HTX = [0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2]  # ... of the row pass
FWD_SHIFT0 = [2, 2, 2, 2, 0, 2, 2, 2, 2, 2, 2, 0, 2, 2, 2, 2, 2, 0, 2]  # fwd_txfm_shift_ls[ts][0]: the up-shift in front of the column pass
LOG_SCALE = [0, 0, 0, 1, 2, 0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0, 1, 1]
PATTERNS = ("basis", "flat", "checker")
# dequantizer steps (dc, ac) across AV1's range: the smallest, one where the 8-bit int16 clamp of |coeff| + round becomes active
# (round = 48/128 step > 32767 - 32640), the 8-bit AC maximum 1828 (also as the DC step: there the clamp changes a flat block's level),
# the 8-bit DC / AC maxima 1336 / 1828 and the 10-bit ones 5347 / 7312
QUANT_STEPS = [(4, 4), (342, 342), (1828, 1828), (1336, 1828), (5347, 7312)]


def quant_rows():
    return np.stack([rd.quant_row_from_step(dc, ac) for dc, ac in QUANT_STEPS])


def blocks_per_wave(ts):
    return 64 // max(TX_W[ts], TX_H[ts])


def fast_col_limit(ts):
    """largest |residual| M whose column pass takes the 24-bit butterflies: (M << up-shift) x H < 2^17"""
    return (1 << 17) // (TX_H[ts] << FWD_SHIFT0[ts]) - 1


def fast_col_limit_unshifted(ts):
    """the same bound with the up-shift left out: residuals in (fast_col_limit, this] overflow the butterflies if a pass accepts them"""
    return min((1 << 17) // TX_H[ts] - 1, 32767)


def inv_fast_limit(n):
    """largest |pass input| of an n-point inverse pass that takes the 18-bit butterflies: x n < 2^18"""
    return (1 << 18) // n - 1


# ---- separable worst-case residuals --------------------------------------------------------------------------------------
def sign_vector(kind, n, k=0):
    """+-1 vector of length n matching a 1-D kernel: 0 DCT (basis row k), 1 ADST (row k), 2 FLIPADST (row k reversed: the 2-D passes
    flip before the ADST), 3 identity (all ones), "checker" (alternating)."""
    i = np.arange(n)
    if kind == "checker":
        v = np.where(i % 2 == 0, 1.0, -1.0)
    elif kind == 0:
        v = np.cos(np.pi * (2 * i + 1) * k / (2 * n))
    elif kind in (1, 2):
        v = np.sin(np.pi * (2 * i + 1) * (2 * k + 1) / (4 * n))
        if kind == 2:
            v = v[::-1]
    else:
        v = np.ones(n)
    return np.where(v >= 0, 1, -1).astype(np.int64)


def residual_block(ts, tt, magnitude, pattern, k=1, sign=1):
    """H x W int64 residual of magnitude M: "basis" = outer product of the sign vectors of the block's own column / row kernels (DCT
    rows k), "flat" = +-M everywhere, "checker" = alternating signs."""
    w, h = TX_W[ts], TX_H[ts]
    if pattern == "flat":
        return np.full((h, w), sign * magnitude, np.int64)
    if pattern == "checker":
        return sign * magnitude * np.outer(sign_vector("checker", h), sign_vector("checker", w))
    return sign * magnitude * np.outer(sign_vector(VTX[tt], h, k), sign_vector(HTX[tt], w, k))


def fwd_full(oracle, ts, tt, block):
    """orc_fwd_txfm2d of an int16 block: the full W x H coefficients (int64 copy)"""
    w, h = TX_W[ts], TX_H[ts]
    r = np.ascontiguousarray(block, np.int16)
    out = np.zeros(w * h, np.int32)
    oracle.orc_fwd_txfm2d(r.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint32(w), C.c_int(tt), C.c_int(ts))
    return out.astype(np.int64)


@functools.lru_cache(maxsize=None)
def q24_crossing(ts, tt, pattern):
    """the first residual magnitude M (<= 32767) at which the oracle's largest |coeff| of the pattern reaches 2^16, by bisection over an
    interval whose ends stay on either side (so M - 1 is below 2^16 whatever the curve does in between); None if no power of two reaches it"""
    import pyoracle
    orc = pyoracle.load_oracle()
    f = lambda m: int(np.abs(fwd_full(orc, ts, tt, residual_block(ts, tt, m, pattern))).max())
    hi = 1  # the first power of two past the crossing (large int16 residuals wrap inside the passes: the curve is not monotonic there)
    while f(hi) < (1 << 16):
        if hi == 32767:
            return None
        hi = min(2 * hi, 32767)
    lo = hi // 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(mid) >= (1 << 16):
            hi = mid
        else:
            lo = mid
    return hi


# ---- magnitudes per size: both sides of every bound ------------------------------------------------------------------------
def edge_pairs(ts, bd):
    """(tt, pattern, below, beyond) magnitude pairs: the wave takes a fast path with `below` everywhere and leaves it with one `beyond`
    block.  Bit depth 8: the uint8 planes bound |residual| by 255, which every fast path accepts; the pairs there are 255 against small
    residuals (the int16 clamp regime of the quantizer).  Bit depth 10: magnitudes beyond 1023 come from uint16 samples beyond 10 bits."""
    pairs = []
    for tt in valid_types(ts):
        for pattern in PATTERNS if tt == 0 else PATTERNS[:2]:
            if bd == 8:
                pairs.append((tt, pattern, 60, 255))
                continue
            pairs.append((tt, pattern, fast_col_limit(ts), fast_col_limit(ts) + 1))
            m = q24_crossing(ts, tt, pattern)
            if m is not None:
                pairs.append((tt, pattern, m - 1, m))
                pairs.append((tt, pattern, m - 1, m + 1))
            if pattern == "flat" and FWD_SHIFT0[ts]:
                pairs.append((tt, pattern, fast_col_limit(ts), fast_col_limit_unshifted(ts)))
    return pairs


def wave_specs(ts, bd):
    """per block (tt, pattern, magnitude, sign), in job order: for every edge pair one wave of `below` blocks, one with a `beyond`
    block first, one with it last, and one wave of `beyond` blocks"""
    bpw = blocks_per_wave(ts)
    specs = []
    for i, (tt, pattern, below, beyond) in enumerate(edge_pairs(ts, bd)):
        waves = [[below] * bpw, [beyond] + [below] * (bpw - 1), [below] * (bpw - 1) + [beyond], [beyond] * bpw]
        if bpw == 1:
            waves = [[below], [beyond]]
        for w in waves:
            specs += [(tt, pattern, m, 1 if (i + j) % 2 == 0 else -1) for j, m in enumerate(w)]
    return specs


def residual_plane(ts, specs, width=256):
    """int64 residual plane holding the blocks of `specs` in raster order, and the block offsets (samples)"""
    w, h = TX_W[ts], TX_H[ts]
    per_row = width // w
    rows = (len(specs) + per_row - 1) // per_row
    plane = np.zeros((rows * h, width), np.int64)
    offsets = np.zeros(len(specs), np.uint32)
    for i, (tt, pattern, m, sign) in enumerate(specs):
        y, x = (i // per_row) * h, (i % per_row) * w
        plane[y:y + h, x:x + w] = residual_block(ts, tt, m, pattern, k=1 + i % 3, sign=sign)
        offsets[i] = y * width + x
    return plane, offsets


def planes_for_residual(residual, bd):
    """src, pred with src - pred == residual exactly: uint8 planes at bit depth 8, else uint16 (samples beyond 10 bits where |r| > 1023)"""
    assert np.abs(residual).max() <= (255 if bd == 8 else 32767)
    dt = np.uint8 if bd == 8 else np.uint16
    return np.ascontiguousarray(np.maximum(residual, 0).astype(dt)), np.ascontiguousarray(np.maximum(-residual, 0).astype(dt))


def rd_edge_case(ts, bd, n_drop=1):
    """(desc fields without quant_kind, src, pred, jobs) of the magnitude edges of one size and bit depth; the last wave is left
    `n_drop` blocks short where a wave holds several blocks"""
    specs = wave_specs(ts, bd)
    if blocks_per_wave(ts) > 1 and n_drop:
        specs = specs[:-n_drop]
    plane, offsets = residual_plane(ts, specs)
    src, pred = planes_for_residual(plane, bd)
    jobs = np.zeros(len(specs), abi.JOB_DTYPE)
    jobs["src_offset"] = offsets
    jobs["pred_offset"] = offsets
    jobs["tx_type"] = [s[0] for s in specs]
    jobs["quant_row"] = np.arange(len(specs)) % len(QUANT_STEPS)
    f = dict(bit_depth=bd, tx_size=ts, src_stride=plane.shape[1], pred_stride=plane.shape[1])
    return f, src, pred, jobs


# ---- ordinary pictures for the output sets, and quantization matrices -------------------------------------------------------
def _mixed_jobs(rng, ts, width, height):
    """jobs on a grid with gaps (recon samples outside every job), every type the size allows, one wave with a
    pf_shape != 0 job among pf_shape 0 jobs, and a partial last wave"""
    jobs = rd.grid_jobs(width, height, width, ts)
    jobs = jobs[np.arange(len(jobs)) % 5 != 3]
    bpw = blocks_per_wave(ts)
    n = len(jobs) - (len(jobs) % bpw) - bpw // 2 if bpw > 1 else len(jobs)
    jobs = jobs[:max(n, 1)].copy()
    types = valid_types(ts)
    jobs["tx_type"] = [types[i % len(types)] for i in range(len(jobs))]
    jobs["quant_row"] = rng.integers(0, len(QUANT_STEPS), len(jobs))
    jobs["pf_shape"][min(bpw, len(jobs) - 1)] = 1 + (ts % 3)  # first block of the second wave
    return jobs


def _planes(rng, bd, width, height):
    hi = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    base = np.kron(rng.integers(0, hi + 1, (height // 8 + 2, width // 8 + 2)).astype(np.float64), np.ones((8, 8)))[:height, :width]
    src = np.clip(base + rng.normal(0, 12 * (1 << (bd - 8)), base.shape), 0, hi).astype(dt)
    pred = np.clip(base + rng.normal(0, 4 * (1 << (bd - 8)), base.shape), 0, hi).astype(dt)
    src[:64, :64] = np.where(rng.integers(0, 2, (64, 64)) == 0, 0, hi)  # a corner of full-swing residuals
    pred[:64, :64] = hi - src[:64, :64]
    src[64:128, 64:192] = hi  # flat full-swing blocks: the largest coefficients a picture of this bit depth can give
    pred[64:128, 64:192] = 0
    return np.ascontiguousarray(src), np.ascontiguousarray(pred)


def output_set_case(ts, bd, width=256, height=192):
    """(desc fields without quant_kind, src, pred, jobs): smooth content with a corner of full-swing residuals and flat full-swing blocks,
    the jobs of _mixed_jobs"""
    rng = np.random.default_rng(4100 + ts + 100 * bd)
    src, pred = _planes(rng, bd, width, height)
    jobs = _mixed_jobs(rng, ts, width, height)
    return dict(bit_depth=bd, tx_size=ts, src_stride=width, pred_stride=width), src, pred, jobs


def qmatrices(ts):
    """a (qmatrix, iqmatrix) pair for the kept coefficients of size ts: weights drawn from [16, 255] (AOM_QM_BITS = 5: 32 = unit weight),
    a wider range than the AV1 tables' in both directions"""
    rng = np.random.default_rng(4200 + ts)
    npk = min(TX_W[ts], 32) * min(TX_H[ts], 32)
    return rng.integers(16, 256, npk).astype(np.uint8), rng.integers(16, 256, npk).astype(np.uint8)


# ---- the quantizer's 8-bit int16 clamp ----------------------------------------------------------------------------------------
def quantize_b_level(a, row, ac, log_scale, clamp):
    """|qcoeff| of svt_aom_quantize_b for |coeff| = a with a flat matrix, with or without the 8-bit int16 clamp of |coeff| + round"""
    r = lambda v: (int(v) + (1 << (log_scale - 1))) >> log_scale if log_scale else int(v)
    if a < r(row["zbin"][ac]):
        return 0
    t = a + r(row["round"][ac])
    if clamp:
        t = min(t, 32767)
    tmp = ((t * int(row["quant"][ac])) >> 16) + t
    return (tmp * int(row["quant_shift"][ac])) >> (16 - log_scale)


def clamp_cases():
    """(ts, quant row index) pairs where a flat +-255 8-bit block has |coeff| + round > 32767 and the clamp changes the level"""
    import pyoracle
    orc = pyoracle.load_oracle()
    rows = quant_rows()
    out = []
    for ts in range(19):
        a = int(np.abs(fwd_full(orc, ts, 0, residual_block(ts, 0, 255, "flat"))).max())
        for qi in range(len(rows)):
            if quantize_b_level(a, rows[qi], 0, LOG_SCALE[ts], True) != quantize_b_level(a, rows[qi], 0, LOG_SCALE[ts], False):
                out.append((ts, qi))
    return out


# ---- inverse transform inputs ---------------------------------------------------------------------------------------------
def inv_row_input_max(ts, bd, co):
    """per block of co [n, min(W,32) * min(H,32)]: the largest |row-pass input| (the rectangular sizes' 2896 / 4096 scaling, then the
    bd + 8 clamp), which decides fast_irow"""
    w, h = TX_W[ts], TX_H[ts]
    v = np.asarray(co, np.int64)
    if w == 2 * h or h == 2 * w:
        v = (v * 2896 + 2048) >> 12
    lim = 1 << (bd + 7)
    return np.abs(np.clip(v, -lim, lim - 1)).max(axis=1)


def inv_col_input_max(oracle, ts, bd, tt, block):
    """largest |column-pass input| of one block (the row pass's shifted outputs, before the column clamp), which decides fast_icol"""
    w, h = TX_W[ts], TX_H[ts]
    c = np.ascontiguousarray(block, np.int32)
    buf = np.zeros(w * h, np.int32)
    oracle.orc_inv_txfm2d_rows(c.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.c_int(int(tt)), C.c_int(ts), C.c_int(bd))
    return int(np.abs(buf.astype(np.int64)).max())


def _rect_pre(ts, v):
    """the smallest stored value whose row-pass input (after the rectangular sizes' 2896 / 4096 scaling) reaches v"""
    w, h = TX_W[ts], TX_H[ts]
    if not (w == 2 * h or h == 2 * w):
        return v
    x = (v * 4096) // 2896
    while (x * 2896 + 2048) >> 12 < v:
        x += 1
    while x > 0 and ((x - 1) * 2896 + 2048) >> 12 >= v:
        x -= 1
    return x


def _col_block(ts, pattern, v):
    n = min(TX_W[ts], 32) * min(TX_H[ts], 32)
    b = np.zeros(n, np.int64)
    if pattern == "dc":
        b[0] = v
    elif pattern == "row":  # every coefficient of the first row: a spike in the row pass's output
        b[:min(TX_W[ts], 32)] = v
    else:  # every coefficient
        b[:] = v
    return b


@functools.lru_cache(maxsize=None)
def inv_col_crossing(ts, bd, tt):
    """(pattern, sign, v): the first stored value sign * v at which the block's largest |column-pass input| reaches 2^18 / H, by doubling and
    bisection as q24_crossing; both signs, as the bd + 8 clamp reaches one step further on the negative side.  None where the clamps keep
    every such block below it."""
    import pyoracle
    orc = pyoracle.load_oracle()
    bound = (1 << 18) // TX_H[ts]
    for pattern in ("dc", "row", "dense"):
        for sign, top in ((1, _rect_pre(ts, (1 << (bd + 7)) - 1)), (-1, _rect_pre(ts, 1 << (bd + 7)))):
            f = lambda v: inv_col_input_max(orc, ts, bd, tt, sign * _col_block(ts, pattern, v))
            if f(top) < bound:
                continue
            hi = 1
            while f(hi) < bound:
                hi = min(2 * hi, top)
            lo = hi // 2
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if f(mid) >= bound:
                    hi = mid
                else:
                    lo = mid
            return pattern, sign, hi
    return None


def inv_col_pair_types(ts):
    """the types whose column-pass bound the inverse cases aim at: DCT_DCT, the last type the size allows, and the first with identity rows
    (unclamped by the row pass's stage ranges: the only way 8-bit inputs reach the bound at some sizes)"""
    types = valid_types(ts)
    identity_rows = [t for t in types if HTX[t] == 3]
    return sorted({types[0], types[-1]} | set(identity_rows[:1]))


def _pair_waves(bpw, below, beyond):
    """all below, beyond first, beyond last, all beyond (one wave each way where a wave holds one block)"""
    if bpw == 1:
        return [[below], [beyond]]
    return [[below] * bpw, [beyond] + [below] * (bpw - 1), [below] * (bpw - 1) + [beyond], [beyond] * bpw]


def inverse_case(rng, ts, bd):
    """(tx types [n], dequantized coefficients [n, min(W,32) * min(H,32)] int32) in job order, in waves of blocks_per_wave(ts) blocks:
      row pair   dense blocks whose largest row-pass input is 2^18 / W - 1 (fast_irow) against ones at 2^18 / W, in the four waves of
                 _pair_waves (where the bd + 8 clamp lets an input reach the bound; else one wave of dense blocks at the clamp)
      col pair   for each of inv_col_pair_types: blocks whose largest column-pass input is just below / at 2^18 / H (inv_col_crossing),
                 the same four waves (where reachable)
      clamp      dense blocks beyond the bd + 8 input clamp, two waves of their own
      extremes   int32 extremes, one wave
      sparse     random sparse blocks, the last wave one block short where a wave holds several"""
    w = TX_W[ts]
    n = min(w, 32) * min(TX_H[ts], 32)
    bpw = blocks_per_wave(ts)
    types = valid_types(ts)
    clamp = (1 << (bd + 7)) - 1
    blocks = []  # (tt, kind, value)
    row_lim = inv_fast_limit(w)
    if row_lim + 1 <= clamp:
        for wave in _pair_waves(bpw, _rect_pre(ts, row_lim), _rect_pre(ts, row_lim + 1)):
            blocks += [(types[len(blocks) % len(types)], "dense", v) for v in wave]
    else:
        blocks += [(types[(len(blocks) + j) % len(types)], "dense", _rect_pre(ts, clamp)) for j in range(bpw)]
    for tt in inv_col_pair_types(ts):
        cross = inv_col_crossing(ts, bd, tt)
        if cross is not None:
            pattern, sign, v = cross
            for wave in _pair_waves(bpw, v - 1, v):
                blocks += [(tt, ("col", pattern, sign), x) for x in wave]
    for kind, v in (("dense", clamp + 1), ("dense", clamp + 1000), ("extreme", 0), ("sparse", 0)):
        blocks += [(types[(len(blocks) + j) % len(types)], kind, v) for j in range(bpw)]
    if bpw > 1:
        blocks = blocks[:-1]
    co = np.zeros((len(blocks), n), np.int64)
    for j, (tt, kind, v) in enumerate(blocks):
        s = rng.choice([-1, 1], n)
        if kind == "dense":
            co[j] = s * v
        elif isinstance(kind, tuple):  # the sign the crossing was found for (rounding makes the magnitudes asymmetric)
            co[j] = kind[2] * _col_block(ts, kind[1], v)
        elif kind == "extreme":
            co[j] = rng.choice([-(1 << 31), (1 << 31) - 1, -(1 << 31) + 1, 0], n)
        else:
            co[j] = np.where(rng.random(n) < 0.1, rng.integers(-(1 << (bd + 6)), 1 << (bd + 6), n), 0)
    return np.array([b[0] for b in blocks], np.uint8), co.astype(np.int32)
