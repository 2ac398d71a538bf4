"""The inverse DCT (4 .. 64 points) and inverse ADST (8, 16) of AV1 as explicit flow graphs in integer arithmetic, restated from the
structure the oracle and txfm_core.h share, with every node kept: what the clamp-free tier of the inverse passes (ipass_clamp_free,
txfm_core.h) rests on is computed from them.

A graph is a list of nodes in evaluation order:
  ("in", i) / ("zero",)                a pass input / a literal zero (inputs >= 32 of the 64-point passes)
  ("btf", w0, a, w1, b)                half_btf: (w0 * x[a] + w1 * x[b] + 2^11) >> 12
  ("add", a, b) / ("sub", a, b)        a sum / difference the reference passes through clamp_value(stage_range)
  ("neg", a)                           the sign changes behind the inverse ADST (not clamped)
and `outputs`, the node of every output.

For every node the exact linear map over the pass inputs (its weights, as fractions of 4096^depth) gives the L1 gain, and the rounding
of the half_btfs upstream of it gives an error bound e: with |input| <= m, |node| <= gain * m + e."""
import functools
import math
from fractions import Fraction

import numpy as np

COS_BIT = 12
COSPI = [int(math.cos(math.pi * j / 128.0) * (1 << COS_BIT) + 0.5) for j in range(64)]


def _brev(v, bits):
    r = 0
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def _ilog2(n):
    return n.bit_length() - 1


class Graph:
    def __init__(self, n, live):
        self.n, self.live = n, live
        self.nodes = [("in", i) if i < live else ("zero",) for i in range(n)]
        self.outputs = None

    def _is_zero(self, a):
        return self.nodes[a][0] == "zero"

    def _new(self, node):
        self.nodes.append(node)
        return len(self.nodes) - 1

    def btf(self, w0, a, w1, b):
        if self._is_zero(a) and self._is_zero(b):
            return a  # (0 + 2^11) >> 12 == 0
        return self._new(("btf", w0, a, w1, b))

    def add(self, a, b):
        return self._new(("add", a, b))

    def sub(self, a, b):
        return self._new(("sub", a, b))

    def neg(self, a):
        return self._new(("neg", a))


# ---- DCT: x[M .. 2M) is the odd part of a 2M-point DCT -----------------------------------------------------------------------------
def _odd_rot(g, x, M, k):
    c = COSPI
    t = M >> k
    if k == 1:
        for j in range(M // 4):
            p = M + M // 4 + j
            m = 3 * M - 1 - p
            a, b = x[p], x[m]
            x[p] = g.btf(-c[32], a, c[32], b)
            x[m] = g.btf(c[32], b, c[32], a)
        return
    for grp in range(1 << (k - 2)):
        A = (1 + 4 * _brev(grp, k - 2)) * (64 >> k)
        B = 64 - A
        base = M + grp * 2 * t
        for j in range(t // 2):
            p = base + t // 2 + j
            m = 3 * M - 1 - p
            a, b = x[p], x[m]
            x[p] = g.btf(-c[A], a, c[B], b)
            x[m] = g.btf(c[A], b, c[B], a)
        for j in range(t // 2):
            p = base + t + j
            m = 3 * M - 1 - p
            a, b = x[p], x[m]
            x[p] = g.btf(-c[B], a, -c[A], b)
            x[m] = g.btf(c[B], b, -c[A], a)


def _odd_bfly(g, x, M, k):
    t = M >> k
    for grp in range(M // t):
        b = M + grp * t
        for j in range(t // 2):
            lo, hi = x[b + j], x[b + t - 1 - j]
            s = g.add(lo, hi)
            d = g.sub(hi, lo) if grp & 1 else g.sub(lo, hi)
            if grp & 1:
                x[b + j], x[b + t - 1 - j] = d, s
            else:
                x[b + j], x[b + t - 1 - j] = s, d


def _odd_final_inv(g, x, M):
    c = COSPI
    L = _ilog2(M)
    for i in range(M // 2):
        A = 64 - (2 * _brev(i, L) + 1) * (32 // M)
        B = 64 - A
        p, m = M + i, 2 * M - 1 - i
        a, b = x[p], x[m]
        x[p] = g.btf(c[A], a, -c[B], b)
        x[m] = g.btf(c[B], a, c[A], b)


def _idct_core(g, x, N):
    c = COSPI
    if N == 2:
        a, b = x[0], x[1]
        x[0] = g.btf(c[32], a, c[32], b)
        x[1] = g.btf(c[32], a, -c[32], b)
        return
    M = N // 2
    _odd_final_inv(g, x, M)
    for k in range(_ilog2(M) - 1, 0, -1):
        _odd_bfly(g, x, M, k)
        _odd_rot(g, x, M, k)
    _idct_core(g, x, M)
    for i in range(M):
        a, b = x[i], x[N - 1 - i]
        x[i] = g.add(a, b)
        x[N - 1 - i] = g.sub(a, b)


def _adst_perm(n):
    if n == 2:
        return [0, 1]
    q = _adst_perm(n // 2)
    p = [0] * n
    for j in range(n // 2):
        p[2 * j], p[2 * j + 1] = q[j], n - 1 - q[j]
    return p


def _iadst(g, inp, N):
    c = COSPI
    x = [None] * N
    for j in range(N // 2):
        x[2 * j + 1] = inp[2 * j]
        x[N - 2 - 2 * j] = inp[2 * j + 1]
    for j in range(N // 2):  # adst_last
        A = (4 * j + 1) * (64 // (2 * N))
        B = 64 - A
        a, d = x[2 * j], x[2 * j + 1]
        x[2 * j] = g.btf(c[A], a, c[B], d)
        x[2 * j + 1] = g.btf(c[B], a, -c[A], d)
    h = N // 2
    while h >= 2:
        for b in range(0, N, 2 * h):  # adst_bfly
            for j in range(h):
                a, d = x[b + j], x[b + j + h]
                x[b + j] = g.add(a, d)
                x[b + j + h] = g.sub(a, d)
        for b in range(0, N, 2 * h):  # adst_rot
            if h == 2:
                a, d = x[b + 2], x[b + 3]
                x[b + 2] = g.btf(c[32], a, c[32], d)
                x[b + 3] = g.btf(c[32], a, -c[32], d)
                continue
            for j in range(h // 4):
                A = (4 * j + 1) * (64 // h)
                B = 64 - A
                p = b + h + 2 * j
                a, d = x[p], x[p + 1]
                x[p] = g.btf(c[A], a, c[B], d)
                x[p + 1] = g.btf(c[B], a, -c[A], d)
                p = b + h + h // 2 + 2 * j
                a, d = x[p], x[p + 1]
                x[p] = g.btf(-c[B], a, c[A], d)
                x[p + 1] = g.btf(c[A], a, c[B], d)
        h //= 2
    P = _adst_perm(N)
    out = [None] * N
    for k in range(N):
        out[P[k]] = g.neg(x[k]) if bin(k).count("1") & 1 else x[k]
    return out


@functools.lru_cache(maxsize=None)
def graph(kind, n):
    """kind "dct" (n = 4 .. 64; the 64-point graph has its inputs >= 32 zero, as every 64-point inverse pass of AV1) or "adst" (8, 16)"""
    g = Graph(n, min(n, 32))
    if kind == "dct":
        x = [None] * n
        for k in range(n):
            x[_brev(k, _ilog2(n))] = k
        _idct_core(g, x, n)
        g.outputs = x
    else:
        g.outputs = _iadst(g, list(range(n)), n)
    return g


def evaluate(g, inputs, clamp_bits):
    """all node values [n_nodes, P] (int64) for inputs [P, live]; clamp_bits None: no stage clamps"""
    inputs = np.asarray(inputs, np.int64)
    v = np.zeros((len(g.nodes), inputs.shape[0]), np.int64)
    for i, node in enumerate(g.nodes):
        op = node[0]
        if op == "in":
            v[i] = inputs[:, node[1]]
        elif op == "btf":
            v[i] = (node[1] * v[node[2]] + node[3] * v[node[4]] + (1 << (COS_BIT - 1))) >> COS_BIT
        elif op == "neg":
            v[i] = -v[node[1]]
        elif op in ("add", "sub"):
            s = v[node[1]] + v[node[2]] if op == "add" else v[node[1]] - v[node[2]]
            v[i] = s if clamp_bits is None else np.clip(s, -(1 << (clamp_bits - 1)), (1 << (clamp_bits - 1)) - 1)
    return v


@functools.lru_cache(maxsize=None)
def analysis(kind, n):
    """(weights [n_nodes][live] as Fractions, gains [n_nodes], errors [n_nodes]): the exact linear map of every node over the pass inputs,
    its L1 norm, and the bound of what the half_btfs' rounding upstream adds or takes: each rounds by at most 1/2 and passes on what its
    operands carry with its own weights' magnitudes"""
    g = graph(kind, n)
    live = g.live
    W, E = [], []
    for node in g.nodes:
        op = node[0]
        if op == "in":
            w, e = [Fraction(int(j == node[1])) for j in range(live)], Fraction(0)
        elif op == "zero":
            w, e = [Fraction(0)] * live, Fraction(0)
        elif op == "btf":
            f0, f1 = Fraction(node[1], 1 << COS_BIT), Fraction(node[3], 1 << COS_BIT)
            w = [f0 * p + f1 * q for p, q in zip(W[node[2]], W[node[4]])]
            e = abs(f0) * E[node[2]] + abs(f1) * E[node[4]] + Fraction(1, 2)
        elif op == "neg":
            w, e = [-p for p in W[node[1]]], E[node[1]]
        else:
            sg = 1 if op == "add" else -1
            w = [p + sg * q for p, q in zip(W[node[1]], W[node[2]])]
            e = E[node[1]] + E[node[2]]
        W.append(w)
        E.append(e)
    return W, [sum(abs(p) for p in w) for w in W], E


def kinds(n):
    return ("dct", "adst") if n in (8, 16) else ("dct",)


def gain_and_slack(n):
    """(G, slack) of the n-point inverse passes: the largest L1 gain of any node of the DCT and (8, 16 points) the ADST over the live
    inputs, and the largest rounding error bound of any node"""
    G = max(max(analysis(k, n)[1]) for k in kinds(n))
    S = max(max(analysis(k, n)[2]) for k in kinds(n))
    return G, S


GAIN_UNIT = 64  # the kernels hold the gain in 64ths, rounded up


def kernel_constants(n):
    G, S = gain_and_slack(n)
    return math.ceil(G * GAIN_UNIT), math.ceil(S)


def clamp_free_limit(n, clamp_bits):
    """largest max|input| with which an n-point pass takes the clamp-free tier: gain64 * m + 64 * slack < 64 * 2^(clamp_bits - 1)"""
    g64, s = kernel_constants(n)
    return ((GAIN_UNIT << (clamp_bits - 1)) - GAIN_UNIT * s - 1) // g64


def extreme_patterns(kind, n):
    """[2 * n_nodes', live] of +-1: for every node that depends on an input, the signs of its weights and their negation"""
    W, _, _ = analysis(kind, n)
    pats = {tuple(1 if p >= 0 else -1 for p in w) for w in W if any(w)}
    pats |= {tuple(-s for s in p) for p in pats}
    return np.array(sorted(pats), np.int64)
