"""CPU: the bound behind the clamp-free tier of the inverse passes (ipass_clamp_free, csrc/txfm_core.h).

An inverse pass of AV1 clamps every sum and difference of every stage to the stage range (clamp_value).  The kernels drop those clamps
in a wave whose largest |pass input| m satisfies G_n m + slack_n < 2^(CLAMP - 1).  Here the inverse DCT (4 .. 64 points, the 64-point
one over its 32 live inputs) and the inverse ADST (8, 16) are restated as flow graphs in integer arithmetic (tests/inv_flow_graph.py),
pinned to the oracle's inverse transform, and from the graphs
  G_n      the largest L1 gain of any node over the pass inputs (exact, in fractions; below n, as txfm_core.h always said), and
  slack_n  the largest accumulated rounding of the half_btfs upstream of any node
are computed, the kernel's constants are compared with them, and at the tier's limit every sign pattern that maximises a node (and its
negation: the rounding is not symmetric) is fed through the network with and without the clamps.

The margin.  The kernel holds G_n in 64ths rounded up and slack_n rounded up, and slack_n is a bound that no single input reaches at
every half_btf at once.  So the limit is not tight: the first magnitude at which one of the patterns drives a node out of the clamp
range lies above it, by at most 1 / (64 G_n) of the limit for the gain's rounding plus 2 slack_n / G_n + 1 for the rounding bound
(the true node is within slack_n of G_n m on either side).  The last test measures that distance and holds it to this figure."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import inv_flow_graph as F

SIZES = (4, 8, 16, 32, 64)
TX_SQUARE = {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}
INV_SHIFT0 = {4: 0, 8: -1, 16: -2, 32: -2, 64: -2}
CLAMPS = (16, 18)  # columns and 8-bit rows / 10-bit rows
CASES = [(k, n) for n in SIZES for k in F.kinds(n)]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svt-av1-psyex_amd", "csrc", "txfm_core.h")


@pytest.mark.parametrize("kind,n", CASES)
@pytest.mark.parametrize("bd", (8, 10))
def test_flow_graph_is_the_oracles_inverse_pass(oracle, kind, n, bd):
    """the row pass of the square n x n inverse transform (bd + 8 input clamp, stage clamps, round-shift) on random rows of all magnitudes"""
    g = F.graph(kind, n)
    rng = np.random.default_rng(1300 + n + bd)
    lim, clamp_bits, rows = 1 << (bd + 7), 16 if bd == 8 else 18, min(n, 32)
    mags = [3, 100, 5000, lim // 4, lim, 4 * lim]
    for rep in range(4):
        co = np.stack([rng.integers(-mags[(r + rep) % len(mags)], mags[(r + rep) % len(mags)] + 1, g.live) for r in range(rows)]).astype(np.int32)
        buf = np.zeros(n * n, np.int32)
        oracle.orc_inv_txfm2d_rows(co.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.c_int(0 if kind == "dct" else 2), C.c_int(TX_SQUARE[n]), C.c_int(bd))
        out = F.evaluate(g, np.clip(co.astype(np.int64), -lim, lim - 1), clamp_bits)[g.outputs].T
        s = -INV_SHIFT0[n]
        if s:
            out = (out + (1 << (s - 1))) >> s
        assert np.array_equal(out, buf.reshape(n, n)[:rows]), (kind, n, bd, rep)


def test_gain_is_below_the_number_of_live_inputs():
    for kind, n in CASES:
        assert max(F.analysis(kind, n)[1]) < min(n, 32), (kind, n)


def test_kernel_constants_are_the_derived_ones():
    text = open(HEADER).read()
    for name, idx in (("inv_gain64", 0), ("inv_slack", 1)):
        m = re.search(r"constexpr int " + name + r"\(int n\) \{ return n == 4 \? (\d+) : n == 8 \? (\d+) : n == 16 \? (\d+) : n == 32 \? (\d+) : (\d+); \}", text)
        assert m, name
        assert [int(v) for v in m.groups()] == [F.kernel_constants(n)[idx] for n in SIZES], name
    m = re.search(r"return \(u64\)wave_max_abs_input \* \(unsigned\)inv_gain64\(n\) \+ (\d+)u \* \(unsigned\)inv_slack\(n\) < \(\(u64\)(\d+) << \(clamp_bits - 1\)\);", text)
    assert m and int(m.group(1)) == F.GAIN_UNIT and int(m.group(2)) == F.GAIN_UNIT


def _leaves_range(kind, n, m, clamp_bits):
    """does any node of the clamp-free network leave the clamp range with one of the extreme patterns at magnitude m?"""
    v = F.evaluate(F.graph(kind, n), m * F.extreme_patterns(kind, n), None)
    return bool((v < -(1 << (clamp_bits - 1))).any() or (v > (1 << (clamp_bits - 1)) - 1).any())


@pytest.mark.parametrize("kind,n", CASES)
@pytest.mark.parametrize("clamp_bits", CLAMPS)
def test_no_node_leaves_the_clamp_range_at_the_limit(kind, n, clamp_bits):
    g = F.graph(kind, n)
    m = F.clamp_free_limit(n, clamp_bits)
    g64, slack = F.kernel_constants(n)
    assert g64 * m + F.GAIN_UNIT * slack < (F.GAIN_UNIT << (clamp_bits - 1)) <= g64 * (m + 1) + F.GAIN_UNIT * slack  # m is the limit of the kernel's test
    pats = F.extreme_patterns(kind, n)
    rng = np.random.default_rng(1400 + n)
    inputs = np.concatenate([m * pats, rng.integers(-m, m + 1, (256, g.live))])  # every node's worst signs, and noise of the same magnitude
    free, clamped = F.evaluate(g, inputs, None), F.evaluate(g, inputs, clamp_bits)
    assert free.min() >= -(1 << (clamp_bits - 1)) and free.max() <= (1 << (clamp_bits - 1)) - 1, (kind, n, clamp_bits, int(free.min()), int(free.max()))
    assert np.array_equal(free, clamped)
    # the analytic bound itself: gain * m + error covers what the patterns reach, node by node
    _, gains, errs = F.analysis(kind, n)
    reach = np.abs(free[:, :len(pats)]).max(axis=1)
    for i in range(len(g.nodes)):
        assert int(reach[i]) <= gains[i] * m + errs[i], (kind, n, i)
        if g.nodes[i][0] != "zero":
            assert int(reach[i]) >= gains[i] * m - errs[i], (kind, n, i)  # ... and the node's own pattern reaches it, up to the rounding


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clamp_bits", CLAMPS)
def test_margin_of_the_limit(n, clamp_bits):
    """the first magnitude at which a pattern drives a node of some n-point graph out of the range: above the limit, and no further above
    it than the rounding of the constants explains"""
    limit = F.clamp_free_limit(n, clamp_bits)
    G, S = F.gain_and_slack(n)
    lo, hi = limit, 2 * limit + 64
    assert not any(_leaves_range(k, n, lo, clamp_bits) for k in F.kinds(n))
    assert any(_leaves_range(k, n, hi, clamp_bits) for k in F.kinds(n))
    while hi - lo > 1:  # the reach of a pattern grows with m up to the rounding; the ends of the interval stay on either side
        mid = (lo + hi) // 2
        if any(_leaves_range(k, n, mid, clamp_bits) for k in F.kinds(n)):
            hi = mid
        else:
            lo = mid
    margin = hi - limit
    allowed = math.ceil(limit / (F.GAIN_UNIT * G) + 2 * math.ceil(S) / G + 1) + 1
    print(f"n {n} clamp {clamp_bits}: G {float(G):.4f} slack {float(S):.2f} limit {limit} first magnitude out of range {hi} margin {margin} (allowed {allowed})")
    assert 1 <= margin <= allowed, (n, clamp_bits, limit, hi, allowed)
