"""CPU: the arithmetic of the RD kernel's lean quantizer loop (rd_kernel.hip, `lean_q`), restated in numpy with wrapping uint32 and 24-bit
multiplies, against the reference formula in int64 -- exhaustively up to the bounds the kernel tests, and past them; and the cases of
tests/rd_lean_cases.py land on the side of a bound they aim at."""
import math

import numpy as np
import pytest

import rd_edge_cases as E
import rd_lean_cases as L

U32 = np.uint32
M24 = np.uint64(0xFFFFFF)


def mul_u24(a, b):
    """v_mul_u32_u24: low 32 bits of the product of the operands' low 24 bits"""
    return ((a.astype(np.uint64) & M24) * (np.uint64(b) & M24)).astype(U32)


def mul_hi_u24(a, b):
    """v_mul_hi_u32_u24: bits 32..47 of the same product"""
    return (((a.astype(np.uint64) & M24) * (np.uint64(b) & M24)) >> np.uint64(32)).astype(U32)


def lean_level(t, quant, quant_shift, ls):
    """|qcoeff| as the lean loop computes it from t = |coeff| + round (uint32 array)"""
    kt = 4 if ls == 2 else 3
    tmp = mul_u24(t, int(quant) + 65536) >> U32(11)
    return mul_hi_u24(tmp << U32(kt), int(quant_shift) << (11 + ls - kt))


def ref_level(t, quant, quant_shift, ls):
    """svt_aom_quantize_b_c_ii / svt_aom_highbd_quantize_b_c with the flat matrix (wt = 32, AOM_QM_BITS = 5), in int64"""
    tw = t.astype(np.int64) * 32
    tmp = ((tw * int(quant)) >> 16) + tw
    return (tmp * int(quant_shift)) >> (16 - ls + 5)


def _rows():
    rows = list(E.quant_rows())
    extreme = rows[0].copy()  # the int16 extremes: the largest Q = quant + 65536 and quant_shift, and the most negative quant
    extreme["quant"][:] = (32767, -32768)
    extreme["quant_shift"][:] = (32767, 16384)
    return rows + [extreme]


@pytest.mark.parametrize("ls", (0, 1, 2))
def test_lean_quantizer_is_exact_up_to_its_bound(ls):
    """every t in [0, 2^(18 - KT)), every row (DC and AC entries), and the int16 extremes of quant / quant_shift"""
    kt = 4 if ls == 2 else 3
    t = np.arange(0, 1 << (18 - kt), dtype=U32)
    for row in _rows():
        for i in (0, 1):
            got, want = lean_level(t, row["quant"][i], row["quant_shift"][i], ls), ref_level(t, row["quant"][i], row["quant_shift"][i], ls)
            assert np.array_equal(got.astype(np.int64), want), (ls, row, i, int(np.argmax(got != want)))


@pytest.mark.parametrize("ls", (0, 1, 2))
def test_lean_quantizer_beyond_its_bound(ls):
    """Past the bound: with the rows' own Q < 2^17 the form stays exact until t * Q reaches 2^32 (KT = 3) or (t * Q >> 11) << KT reaches 2^24
    (KT = 4), so the bound is conservative for a given row; with the largest Q it fails within a factor 4/3 of the bound, and with any row at
    twice the bound at the latest -- the kernel's test may not be dropped."""
    kt = 4 if ls == 2 else 3
    bound = 1 << (18 - kt)
    t = np.arange(bound, 4 * bound, dtype=U32)
    for row in _rows():
        for i in (0, 1):
            q, s = int(row["quant"][i]), int(row["quant_shift"][i])
            got, want = lean_level(t, q, s, ls), ref_level(t, q, s, ls)
            exact_limit = ((1 << (35 - kt)) + q + 65535) // (q + 65536)  # first t with t * Q >= 2^(35 - KT)
            bad = np.nonzero(got.astype(np.int64) != want)[0]
            assert exact_limit >= bound
            assert bad.size == 0 or int(t[bad[0]]) >= exact_limit, (ls, row, i, int(t[bad[0]]), exact_limit)
            if s >= 1 << 9 and exact_limit < 4 * bound:  # a quant_shift large enough for the lost high bits to reach the level
                assert bad.size > 0 and int(t[bad[0]]) < 2 * exact_limit, (ls, row, i)
    # the bound + 1 and a few above it with the largest Q: 2^15 * 98303 < 2^32 still, 43691 * 98303 >= 2^32 wraps
    for tv, exact in ((bound, True), (bound + 1, True), (bound + 7, True), (((1 << (35 - kt)) + 98302) // 98303, False)):
        tt = np.array([tv], U32)
        assert (int(lean_level(tt, 32767, 16384, ls)[0]) == int(ref_level(tt, 32767, 16384, ls)[0])) == exact, (ls, tv)


@pytest.mark.parametrize("ls", (0, 1, 2))
def test_lean_signs_by_multiplication(ls):
    """qcoeff = qv * sg and dqcoeff (log-scale 0: qcoeff * dequant; else ((qv * dequant) >> ls) * sg) equal the reference's
    (x ^ sign) - sign forms for both signs: the shift stays on the magnitude."""
    rng = np.random.default_rng(7)
    qv = rng.integers(0, 1 << 14, 4096).astype(np.int64)
    for deq in (4, 342, 1336, 1828, 5347, 7312):
        keep = (qv * deq >> ls) < (1 << 16)
        for sign in (0, -1):
            sg = sign | 1
            want_q, want_dq = (qv ^ sign) - sign, ((qv * deq >> ls) ^ sign) - sign
            qs = qv * sg
            dqs = qs * deq if ls == 0 else (qv * deq >> ls) * sg
            assert np.array_equal(qs[keep], want_q[keep]) and np.array_equal(dqs[keep], want_dq[keep])
            if ls and deq % 2:  # the shift applied to the signed (here often odd) product rounds towards minus infinity: not the reference's value
                assert sign == 0 or not np.array_equal((qs * deq >> ls)[keep], want_dq[keep])


@pytest.mark.parametrize("tx_size", L.SIZES)
def test_lean_sums_are_exact_up_to_their_bound(tx_size):
    """NP / LW squares of magnitude M summed in wrapping uint32: exact while (NP / LW) * M^2 < 2^32, wrong one step beyond"""
    n = L.per_lane(tx_size)
    m = math.isqrt(((1 << 32) - 1) // n)
    assert n * m * m < (1 << 32) <= n * (m + 1) * (m + 1)
    for mv, exact in ((m, True), (m - 1, True), (m + 1, False), (m + 2, False)):
        acc = U32(0)
        sq = mul_u24(np.full(n, mv, U32), mv)  # M < 2^16: a 24-bit multiply
        for v in sq:
            acc = U32((int(acc) + int(v)) & 0xFFFFFFFF)
        assert (int(acc) == n * mv * mv) == exact, (tx_size, mv)


def test_lean_bound_mirror_is_monotonic_and_av1_rows_meet_the_sum_bound_first():
    for ts in L.SIZES:
        for bd in (8, 10):
            rows = L.lean_rows(ts, bd)
            for qi, row in enumerate(rows):
                c = L.largest_lean_comax(ts, bd, row)
                assert c > 0 and L.lane_is_lean(ts, bd, c, row) and not L.lane_is_lean(ts, bd, c + 1, row)
                assert all(L.lane_is_lean(ts, bd, v, row) for v in range(0, c, max(c // 97, 1)))
                if qi < L.BIG_ROUND:
                    assert L.binding_bound(ts, bd, c + 1, row) in (("sum",) if L.kt(ts) == 3 else ("sum", "t")), (ts, bd, qi)  # KT = 4: both at 2^14
    # the row with the large round meets the 32-bit product bound first where the sum bound leaves room (not at 32x32: 32 sums per lane)
    assert L.binding_bound(2, 10, 1001, L.lean_rows(2, 10)[L.BIG_ROUND]) == "t"
    assert L.binding_bound(4, 10, L.largest_lean_comax(4, 10, L.lean_rows(4, 10)[L.BIG_ROUND]) + 1, L.lean_rows(4, 10)[L.BIG_ROUND]) == "t"
    assert L.binding_bound(4, 8, L.largest_lean_comax(4, 8, L.lean_rows(4, 8)[L.BIG_ROUND]) + 1, L.lean_rows(4, 8)[L.BIG_ROUND]) == "t"
    assert L.binding_bound(17, 10, L.largest_lean_comax(17, 10, L.lean_rows(17, 10)[L.BIG_ROUND]) + 1, L.lean_rows(17, 10)[L.BIG_ROUND]) == "t"


@pytest.mark.parametrize("tx_size", L.SIZES)
def test_lean_cases_reach_both_sides(oracle, tx_size):
    """the waves of bound_waves: at bit depth 10 every row has lean waves and rejected waves, the rejected ones by the bound meant; the
    oracle's coefficients are what the search aimed at; at the clamped 8-bit row the clamp is active"""
    for bd in (8, 10):
        waves, expect = L.bound_waves(tx_size, bd)
        assert len(waves) == len(expect)
        by_row = {}
        for qi, cm, lean, bound in expect:
            assert lean == (bound is None)
            by_row.setdefault(qi, set()).add(lean)
        if bd == 10:
            assert all(v == {True, False} for v in by_row.values()), (tx_size, by_row)
        else:
            assert all(True in v for v in by_row.values()), (tx_size, by_row)
    row = L.lean_rows(1, 8)[L.BIG_ROUND]
    c = [cm for qi, cm, lean, _ in L.bound_waves(1, 8)[1] if qi == L.BIG_ROUND]
    assert max(c) + int(row["round"][1]) > 32767 and L.lane_is_lean(1, 8, max(c), row)
