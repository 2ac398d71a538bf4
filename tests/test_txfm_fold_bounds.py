"""CPU: the two folds of the bounded transform passes (csrc/txfm_core.h), restated in numpy with wrapping int32 arithmetic, against the
reference forms in int64:
  forward   the butterfly that produces an output of a DCT / ADST pass, with the pass's round-shift in its rounding term and shift count
            (btf_folded), against half_btf followed by round_shift;
  inverse   the last butterfly stage of the DCT with the round-shift behind the stage clamp (idct_core, out_s), against clamp_value
            followed by round_shift.
Exhaustive over cos_bit 10..13, the shifts 1, 2 and 4 (and 0: nothing folded), and every cosine pair of the table with the signs the
networks use; node values at and next to the bounds pass_fits_17_bits / ipass_fits_18_bits establish, of both signs, and sums at and next
to the clamp limits +-2^15 / +-2^17.  No intermediate of the folded forms leaves int32 while the bounds hold."""
import numpy as np
import pytest

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SHIFTS = (0, 1, 2, 4)


def cospi(bit):
    """cospi_arr(bit): round(cos(j pi / 128) 2^bit), j = 0..63"""
    return np.array([int(np.cos(np.pi * j / 128.0) * (1 << bit) + 0.5) for j in range(64)], np.int64)


def pass_fits_17_bits(wave_max_abs_input, n):
    return wave_max_abs_input * n < (1 << 17)


def ipass_fits_18_bits(wave_max_abs_input, n):
    return wave_max_abs_input * n < (1 << 18)


def wrap32(v):
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def sext24(v):
    return ((np.asarray(v, np.int64) + (1 << 23)) & 0xFFFFFF) - (1 << 23)


def mad_i32_i24(w, a, acc):
    """v_mad_i32_i24: low 32 bits of sext24(w) * sext24(a) + acc"""
    return wrap32(sext24(w) * sext24(a) + acc)


def round_shift(v, s):
    return v if s == 0 else (v + (1 << (s - 1))) >> s


def half_btf(w0, a, w1, b, bit):
    """half_btf of the reference: two wrapping 32-bit products, summed and rounded in 64 bits, stored as int32"""
    return wrap32((wrap32(w0 * a) + wrap32(w1 * b) + (1 << (bit - 1))) >> bit)


def node_values(limit):
    """node values of a pass whose nodes stay below `limit` in magnitude: the extremes and their neighbours, small values of both signs, a
    seeded spread"""
    rng = np.random.default_rng(7700)
    edge = [limit - 1, limit - 2, limit - 3, limit // 2, limit // 2 + 1, 1, 2, 3, 0]
    v = np.array(edge + [-x for x in edge if x] + list(rng.integers(-limit + 1, limit, 24)), np.int64)
    assert np.abs(v).max() == limit - 1
    return v


@pytest.mark.parametrize("bit", (10, 11, 12, 13))
def test_folded_forward_butterfly_equals_half_btf_then_round_shift(bit):
    c = cospi(bit)
    # largest wave input 1 with n = 2^17 - 1 is the loosest case the test admits: every node of the pass is then below 2^17
    assert pass_fits_17_bits(1, (1 << 17) - 1) and not pass_fits_17_bits(1, 1 << 17)
    v = node_values(1 << 17)
    a, b = [x.reshape(-1) for x in np.meshgrid(v, v, indexing="ij")]
    j = np.arange(1, 64)
    # (w0, w1) of every butterfly of the networks: a cosine and the matching sine (c[A], c[64 - A]; A = 32 gives the equal pair), any signs
    w_pairs = [(s0 * c[j], s1 * c[64 - j]) for s0 in (1, -1) for s1 in (1, -1)]
    big_pos = big_neg = 0
    for s in SHIFTS:
        rnd = (1 << (bit - 1)) + ((1 << (s - 1 + bit)) if s else 0)
        for w0s, w1s in w_pairs:
            w0, w1 = w0s[:, None], w1s[:, None]
            want = round_shift(half_btf(w0, a[None, :], w1, b[None, :], bit), s)
            exact1 = w0 * a[None, :] + rnd            # the first multiply-add, unwrapped
            exact2 = exact1 + w1 * b[None, :]         # the second
            assert exact1.min() >= I32_MIN and exact1.max() <= I32_MAX, (bit, s, "first multiply-add leaves int32")
            assert exact2.min() >= I32_MIN and exact2.max() <= I32_MAX, (bit, s, "second multiply-add leaves int32")
            acc = mad_i32_i24(w1, b[None, :], mad_i32_i24(w0, a[None, :], np.int64(rnd)))
            got = acc >> (bit + s)
            assert np.array_equal(got, want), (bit, s, np.argwhere(got != want)[:3].tolist())
            big_pos, big_neg = max(big_pos, int(exact2.max())), min(big_neg, int(exact2.min()))
    # the cases reach the bound the overflow argument rests on: |w0 a + w1 b| up to about 2^bit sqrt(2) (2^17 - 1), both signs
    reach = int((1 << bit) * 1.41 * ((1 << 17) - 1))
    assert big_pos >= reach and big_neg <= -reach and big_pos < (1 << 31)


def test_folded_forward_butterfly_rounds_negative_sums_down():
    """floor semantics on the negative side, on hand-made sums: S = -(2^(bit+s-1)) - 1 rounds away from zero, S = -(2^(bit+s-1)) does not"""
    for bit in (10, 11, 12, 13):
        for s in (1, 2, 4):
            rnd = (1 << (bit - 1)) + (1 << (s - 1 + bit))
            for S, want in ((-(1 << (bit + s - 1)) - (1 << (bit - 1)) - 1, -1), (-(1 << (bit + s - 1)) - (1 << (bit - 1)), 0), (-1, 0), ((1 << (bit + s - 1)) - (1 << (bit - 1)), 1),
                            ((1 << (bit + s - 1)) - (1 << (bit - 1)) - 1, 0)):
                y = (S + (1 << (bit - 1))) >> bit
                assert round_shift(y, s) == (S + rnd) >> (bit + s) == want, (bit, s, S)


@pytest.mark.parametrize("clamp_bits", (16, 18))
def test_shifted_clamp_inverse_stage_equals_clamp_then_round_shift(clamp_bits):
    assert ipass_fits_18_bits(1, (1 << 18) - 1) and not ipass_fits_18_bits(1, 1 << 18)
    lo, hi = -(1 << (clamp_bits - 1)), (1 << (clamp_bits - 1)) - 1
    v = node_values(1 << 18)
    # pairs whose sum or difference sits at and next to either clamp limit
    extra_a, extra_b = [], []
    for lim in (lo, hi):
        for d in (-2, -1, 0, 1, 2):
            for a0 in (0, 1, -1, lim // 2, lim, (1 << 18) - 1 if lim > 0 else -(1 << 18) + 1):
                for sign in (1, -1):  # a + b == lim + d, a - b == lim + d
                    b0 = sign * (lim + d - a0)
                    if abs(b0) < (1 << 18):
                        extra_a.append(a0)
                        extra_b.append(b0)
    a, b = [x.reshape(-1) for x in np.meshgrid(v, v, indexing="ij")]
    a, b = np.concatenate([a, np.array(extra_a, np.int64)]), np.concatenate([b, np.array(extra_b, np.int64)])
    hit = {"lo": False, "hi": False}
    for s in (1, 2, 4):
        r = 1 << (s - 1)
        t = a + r
        for sgn in (1, -1):
            exact = t + sgn * b
            assert exact.min() >= I32_MIN and exact.max() <= I32_MAX
            got = np.clip(wrap32(exact), lo + r, hi + r) >> s
            want = round_shift(np.clip(a + sgn * b, lo, hi), s)  # clamp_value, then round_shift
            assert np.array_equal(got, want), (clamp_bits, s, sgn, np.argwhere(got != want)[:3].tolist())
            hit["lo"] = hit["lo"] or bool(((a + sgn * b) == lo).any() and ((a + sgn * b) == lo - 1).any() and ((a + sgn * b) == lo + 1).any())
            hit["hi"] = hit["hi"] or bool(((a + sgn * b) == hi).any() and ((a + sgn * b) == hi - 1).any() and ((a + sgn * b) == hi + 1).any())
    assert hit["lo"] and hit["hi"]
