"""Cases that take the warped-motion entries off the shapes they were written against, shared by tests/test_warp_edges.py (CPU: the restatements of
tests/warp_cases.py equal golden/warp_edges.npz on them, and they reach their conditions), tests/test_warp_edges_gpu.py (the kernels equal the
restatements and the fixture on them) and tools/gen_warp_golden.py (the reference's own functions on them).  The restatements are warp_cases's; this
module holds inputs and the conditions computed from the restatements' traces.

Refinement batches (refine_edge_batch; every batch runs with waves_per_job 0, 1 and 4):
  sizes_{diag}_{shift}  all 17 block sizes on a 160x136 picture, regimes calm and mild, two rounds, with and without diagonals, both MV precisions:
                        the tile loop and the cross-wave reduction at every size
  bias                  32x32, 64x64, 64x16, 128x64 and 128x128 blocks whose source is the reference plus noise plus a constant, so that the sum of
                        the differences leaves int32 when squared (|sum| >= 46341) and leaves uint32 (|sum| >= 65536), with either sign; and the
                        limits: 255 against 0 and 0 against 255 at 128x128 (variance exactly 0), a half-and-half source against a flat reference
                        (variance near N * 255^2 / 4).  Every job has a source picture of its own: they are stacked in one buffer, and src_offset
                        names the job's
  geometry              a 100x70 picture; the source plane is wider than the picture and the picture does not start at its first sample; eight
                        reference planes of different strides, origins and paddings; blocks flush with every edge and in every corner, MVs that
                        point outwards and wild models, so that tiles of costed warps lie outside and across every edge; one job whose src_offset
                        is not that of (blk_org_x, blk_org_y)
  walk_{shift}          flat planes and the light rate alone: the centre moves one diagonal step per round for 16 rounds, towards (40, 40) and
                        towards (-40, -40), so that the record passes 64 entries and a position is skipped because of an entry at index >= 64
  wrap_{shift}          start MVs from which one step leaves int16, in each component and direction.  Half of the jobs have samples that follow
                        the start MV (the wrapped positions are recorded but their fits are invalid); the other half have samples that follow the
                        MV one step past the limit, wrapped, so that a wrapped position is the one that wins.  approx_inter_rate = 1 only: the
                        entropy rate would index the cost tables with the reference's unclamped difference.
                        The reference's own svt_aom_wm_motion_refinement takes these inputs (with the light rate no table is indexed by an MV,
                        the fit is arithmetic alone and the warp clamps what it reads), so the fixture holds the reference's results for this
                        batch as for the others.
Fit batch "far": block origins over the whole uint16 range (65532 included), a third of the MVs next to the int16 limits, so that the clamp of the
translation to +-2^23 is the common case; the builder asserts that no 32-bit intermediate of find_affine_int wraps on these inputs.
Prediction batches: big2_{bd}, a 128x128 compound (averaged and distance-weighted, the models in the job and in the array) on a 160x136 picture;
refs8_{bd}, eight reference planes, every index used as first and as second reference."""
import functools
import os
import zlib

import numpy as np

import warp_cases as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_edges.npz")
WAVES = (0, 1, 4)
INT32_SQUARE, UINT32_SQUARE = 46341, 65536  # the least |sum| whose square leaves int32 / uint32
RECORD_SCAN = 64  # record entries scanned per trip of the kernel's loop over s_rec

# iterations, refine_diag, mv_prec_shift, shut_approx, lower_band_th, upper_band_th, approx_inter_rate, error_per_bit
REFINE_EDGE_BATCHES = {
    "sizes_0_0": (2, 0, 0, 0, 0, 65535, 0, 80), "sizes_0_1": (2, 0, 1, 0, 0, 65535, 1, 0), "sizes_1_0": (2, 1, 0, 0, 0, 65535, 1, 0),
    "sizes_1_1": (2, 1, 1, 0, 0, 65535, 0, 40), "bias": (2, 1, 0, 1, 0, 65535, 1, 0), "geometry": (3, 1, 1, 1, 0, 65535, 0, 100),
    "walk_0": (16, 1, 0, 1, 0, 65535, 1, 1), "walk_1": (16, 1, 1, 1, 0, 65535, 1, 1), "wrap_0": (2, 1, 0, 1, 0, 65535, 1, 0),
    "wrap_1": (2, 1, 1, 1, 0, 65535, 1, 0)}
BIAS_SIZES = [(32, 32), (64, 64), (64, 16), (128, 64), (128, 128)]
I16_MAX, I16_MIN = 32767, -32768


def embed(pic, org_x, org_y, right, below, fill=0x55):
    """the picture inside a plane with org_x columns to its left, `right` to its right, org_y rows above and `below` below, all holding `fill`"""
    ph, pw = pic.shape
    plane = np.full((org_y + ph + below, org_x + pw + right), fill, np.uint8)
    plane[org_y:org_y + ph, org_x:org_x + pw] = pic
    return (plane, org_x, org_y, pw, ph)


def field(rng, rows, cols, amp=(70, 50)):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return 128 + amp[0] * np.sin(xx / 4.3 + yy / 11.0) + amp[1] * np.cos(yy / 3.7 - xx / 13.0) + rng.normal(0, 6, xx.shape)


def edge_refine_job(rng, x, y, bw, bh, src_offset, n, regime, start, pred, ref=0, follow=None):
    """warp_cases.refine_job with the source offset given; follow: the MV the samples follow (default: the start MV)"""
    j = wc.refine_job(rng, x, y, bw, bh, 0, n, regime, start if follow is None else follow, pred, ref)
    j["start_mv"], j["src_offset"] = start, src_offset
    return j


def _finish(name, planes, src, jobs, rng, mvs=None):
    mvs = np.zeros((1, 2), np.int16) if mvs is None else mvs
    return dict(name=name, settings=dict(zip(wc.SETTING_KEYS, REFINE_EDGE_BATCHES[name])), planes=planes, src=np.ascontiguousarray(src, dtype=np.uint8),
                jobs=wc.pack_jobs(jobs, wc.REFINE_JOB_DTYPE), mv_array=mvs, cost_tables=wc.cost_tables(rng))


@functools.lru_cache(maxsize=None)
def refine_edge_batch(name):
    rng = np.random.default_rng(zlib.crc32(("refine_edge_" + name).encode()))
    kind = name.split("_")[0]
    if kind == "sizes":
        # the reference is the source moved by (1, -2) samples: the minimum is near the MV (8, -16), the search starts a step or two beside it
        pw, ph = 160, 136
        src, plane = wc.moving_planes(rng, pw, ph)
        planes = [plane, wc.moving_planes(rng, pw, ph)[1]]
        mvs = np.array([[8 + 2, -16 - 2], [8 - 2, -16 + 2], [8 + 2, -16 + 2]], np.int16)
        jobs = []
        for k, (bw, bh) in enumerate(wc.SIZES + wc.SIZES):
            x, y = int(rng.integers(0, (pw - bw) // 4 + 1)) * 4, int(rng.integers(0, (ph - bh) // 4 + 1)) * 4
            if (bw, bh) == (128, 128):
                x, y = (32, 8) if k < len(wc.SIZES) else (0, 4)
            start = (8 + (2, -2, 1, -3)[k % 4], -16 + (-2, 2, 3, 1)[k % 4])
            pred = (start[0] + int(rng.integers(-6, 7)), start[1] + int(rng.integers(-6, 7)))
            j = edge_refine_job(rng, x, y, bw, bh, y * pw + x, 4 + k % 5, ("calm", "mild")[(k // len(wc.SIZES) + k) % 2], start, pred)
            if k % 6 == 5:  # the start MV from the array; the samples follow that MV
                i = k % len(mvs)
                j = edge_refine_job(rng, x, y, bw, bh, y * pw + x, 4 + k % 5, "calm", (int(mvs[i][0]), int(mvs[i][1])), pred)
                j["flags"], j["mv_index"], j["start_mv"] = wc.WM_START_FROM_ARRAY, i, (-5, 11)
            jobs.append(j)
        return _finish(name, planes, src, jobs, rng, mvs)
    if kind == "bias":
        pw, ph, pad = 160, 136, 8
        base = field(rng, ph + 2 * pad, pw + 2 * pad + 3, amp=(25, 15))  # 70 .. 190: room for a constant of +-64 .. 80 without clipping much
        ref = np.clip(base, 0, 255).astype(np.uint8)
        flat = lambda v: (np.full_like(ref, v), pad, pad, pw, ph)
        planes = [(ref, pad, pad, pw, ph), flat(255), flat(0), flat(128)]
        jobs, layers = [], []

        def add(layer, x, y, bw, bh, ref_index, start, pred):
            layers.append(layer)
            jobs.append(edge_refine_job(rng, x, y, bw, bh, ((len(layers) - 1) * ph + y) * pw + x, 6, "calm", start, pred, ref=ref_index))
        for bw, bh in BIAS_SIZES:
            n = bw * bh
            beyond, between = -(-82000 // n), round(55500 / n)  # |sum| ~ 82000 (past uint32) and ~ 55500 (between the two limits)
            for offset in (beyond, -beyond, between, -between):
                x, y = int(rng.integers(0, (pw - bw) // 4 + 1)) * 4, int(rng.integers(0, (ph - bh) // 4 + 1)) * 4
                layer = np.clip(base[pad + 1:pad + 1 + ph, pad - 2:pad - 2 + pw] + rng.normal(0, 3, (ph, pw)) + offset, 0, 255)
                start = (8 + int(rng.integers(-2, 3)), -16 + int(rng.integers(-2, 3)))
                add(layer, x, y, bw, bh, 0, start, (start[0] + int(rng.integers(-4, 5)), start[1] + int(rng.integers(-4, 5))))
        # the limits: every position has the same variance, so the rate decides, and pred_mv two steps away gives a unique winner that is not the start
        half = np.zeros((ph, pw))
        half[:, pw // 2:] = 255
        add(np.zeros((ph, pw)), 16, 4, 128, 128, 1, (4, -4), (6, -4))       # reference 255, source 0
        add(np.full((ph, pw), 255), 32, 8, 128, 128, 2, (-8, 8), (-8, 10))  # reference 0, source 255
        add(half, pw // 2 - 64, 0, 128, 128, 3, (0, 0), (-2, -2))          # a half-and-half source, a flat reference
        add(half, pw // 2 - 32, 40, 64, 64, 3, (12, 4), (12, 2))
        return _finish(name, planes, np.concatenate(layers), jobs, rng)
    if kind == "geometry":
        pw, ph = 100, 70
        big = field(rng, ph + 40, pw + 40)
        src_org_x, src_org_y, src_stride = 5, 3, 117
        src = np.full((src_org_y + ph + 2, src_stride), 0x33, np.uint8)
        src[src_org_y:src_org_y + ph, src_org_x:src_org_x + pw] = np.clip(big[20:20 + ph, 20:20 + pw] + rng.normal(0, 3, (ph, pw)), 0, 255)
        planes = []
        for r, (ox, oy, right, below) in enumerate([(8, 8, 11, 8), (0, 0, 0, 0), (16, 2, 5, 9), (3, 12, 1, 0), (7, 5, 0, 3), (32, 0, 64, 1), (1, 1, 1, 1), (12, 9, 40, 2)]):
            dy, dx = ((1, -2), (0, 0), (-1, 1), (2, 2), (0, -3), (-2, 0), (1, 1), (3, -1))[r]
            planes.append(embed(np.clip(big[20 + dy:20 + dy + ph, 20 + dx:20 + dx + pw] + rng.normal(0, 2, (ph, pw)), 0, 255).astype(np.uint8), ox, oy, right, below))
        so = lambda x, y: (src_org_y + y) * src_stride + src_org_x + x
        jobs, k = [], 0
        # (x, y) of a block of each size flush with each edge and in each corner; the start MV points out of the picture there, 12 to 20 samples
        for bw, bh in ((16, 16), (8, 8), (32, 16), (64, 64), (8, 32), (16, 8)):
            xs, ys = {"l": 0, "m": (pw - bw) // 8 * 4, "r": pw - bw}, {"t": 0, "m": (ph - bh) // 8 * 4, "b": ph - bh}
            for hx, hy in ("lt", "rt", "lb", "rb", "lm", "rm", "mt", "mb"):
                if (bw, bh) in ((8, 32), (16, 8)) and hx + hy not in ("lt", "rb", "mb"):
                    continue
                out = int(rng.integers(12, 21)) * 8
                start = ({"t": -out, "m": int(rng.integers(-8, 9)), "b": out}[hy], {"l": -out, "m": int(rng.integers(-8, 9)), "r": out}[hx])
                pred = (start[0] + int(rng.integers(-10, 11)), start[1] + int(rng.integers(-10, 11)))
                regime = ("calm", "wild", "mild", "wild")[k % 4]
                jobs.append(edge_refine_job(rng, xs[hx], ys[hy], bw, bh, so(xs[hx], ys[hy]), 3 + k % 6, regime, start, pred, ref=k % 8))
                k += 1
        # src_offset and (blk_org_x, blk_org_y) are independent: the block at (40, 24) costed against the source samples at (12, 6)
        jobs.append(edge_refine_job(rng, 40, 24, 32, 32, so(12, 6), 6, "calm", (8, -16), (4, -10), ref=0))
        return _finish(name, planes, src, jobs, rng)
    if kind == "walk":
        pw, ph, shift = 64, 48, int(name.split("_")[1])
        plane = embed(np.full((ph, pw), 90, np.uint8), 8, 8, 11, 8, fill=90)
        jobs = []
        for k, (bw, bh, x, y, start) in enumerate([(8, 8, 24, 16, (8, -16)), (8, 8, 40, 8, (-24, 16)), (16, 8, 8, 32, (0, 0)), (32, 32, 16, 8, (16, 8)), (8, 8, 0, 40, (3, 5)),
                                                   (16, 16, 48, 32, (-9, -2))]):
            sign = -1 if k & 1 else 1
            jobs.append(edge_refine_job(rng, x, y, bw, bh, y * pw + x, 8 - k, "calm", start, (start[0] + 40 * sign, start[1] + 40 * sign)))
        return _finish(name, [plane], np.full((ph, pw), 90, np.uint8), jobs, rng)
    if kind == "wrap":
        pw, ph, shift = 96, 64, int(name.split("_")[1])
        src, plane = wc.moving_planes(rng, pw, ph)
        step = 1 << shift
        hi, lo = I16_MAX - (step - 1), I16_MIN + (step - 1)  # one step from here leaves int16: 32767 / -32768, or 32766 / -32767 in steps of 2
        jobs, k = [], 0
        for comp in (0, 1):
            for limit, past in ((hi, hi + step), (lo, lo - step)):
                for follows_wrapped in (False, True):
                    bw, bh = ((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (64, 32))[k % 8]
                    x, y = int(rng.integers(0, (pw - bw) // 4 + 1)) * 4, int(rng.integers(0, (ph - bh) // 4 + 1)) * 4
                    other = int(rng.integers(-40, 41))
                    start = (limit, other) if comp == 0 else (other, limit)
                    follow = None
                    if follows_wrapped:
                        follow = (wc.i16(past), other) if comp == 0 else (other, wc.i16(past))
                    inward = -3 if limit > 0 else 3
                    pred = (start[0] + inward, start[1] - 2) if comp == 0 else (start[0] + 2, start[1] + inward)
                    jobs.append(edge_refine_job(rng, x, y, bw, bh, y * pw + x, 5 + k % 4, "calm", start, pred, follow=follow))
                    k += 1
        return _finish(name, [plane], src, jobs, rng)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def restated_refine_edge(name):
    """(the outputs, the traces, the logs) of warp_cases.restate_refine on the batch"""
    traces, logs = [], []
    return wc.restate_refine(refine_edge_batch(name), traces, logs), traces, logs


def _tiles_where():
    return {"left": lambda x, y, w, h: x + 7 < 0, "right": lambda x, y, w, h: x - 7 > w - 1, "above": lambda x, y, w, h: y + 7 < 0,
            "below": lambda x, y, w, h: y - 7 > h - 1, "across the left edge": lambda x, y, w, h: x - 7 < 0 <= x + 7,
            "across the right edge": lambda x, y, w, h: x - 7 <= w - 1 < x + 7, "across the top edge": lambda x, y, w, h: y - 7 < 0 <= y + 7,
            "across the bottom edge": lambda x, y, w, h: y - 7 <= h - 1 < y + 7}


def refine_edge_stats():
    """the counts the conditions are judged on, per batch: what tests/test_warp_edges.py prints and the change's summary quotes"""
    st = {}
    sizes = {}
    for name in (n for n in REFINE_EDGE_BATCHES if n.startswith("sizes")):
        b = refine_edge_batch(name)
        out, _, logs = restated_refine_edge(name)
        for j, log, n_valid, mv in zip(b["jobs"], logs, out["n_valid"], out["best_mv"]):
            if n_valid >= 5 and (int(mv[0]), int(mv[1])) != log["start"]:
                sizes.setdefault(name, set()).add((int(j["bwidth"]), int(j["bheight"])))
    st["sizes"] = {n: len(s) for n, s in sizes.items()}
    st["sizes_missing"] = {n: sorted(set(wc.SIZES) - sizes.get(n, set())) for n in REFINE_EDGE_BATCHES if n.startswith("sizes")}
    b = refine_edge_batch("bias")
    _, _, logs = restated_refine_edge("bias")
    beyond_pos, beyond_neg, between = set(), set(), set()
    sums = [0]
    for j, log in zip(b["jobs"][:4 * len(BIAS_SIZES)], logs):
        size = (int(j["bwidth"]), int(j["bheight"]))
        for _, _, total, _ in log["costed"]:
            sums.append(total)
            if total >= UINT32_SQUARE:
                beyond_pos.add(size)
            if total <= -UINT32_SQUARE:
                beyond_neg.add(size)
            if INT32_SQUARE <= abs(total) < UINT32_SQUARE:
                between.add(size)
    # best_cost holds the variance of the winning position: where that position's |sum| is past the limit, a narrow square shows in best_cost
    winners = {(int(j["bwidth"]), int(j["bheight"])) for j, log in zip(b["jobs"][:4 * len(BIAS_SIZES)], logs)
               if abs(min(log["costed"], key=lambda c: c[1])[2]) >= INT32_SQUARE}
    st["bias"] = {"sizes with a winning position of |sum| >= 46341": len(winners), "sizes with sum >= 65536": len(beyond_pos), "sizes with sum <= -65536": len(beyond_neg), "sizes with 46341 <= |sum| < 65536": len(between),
                  "largest sum": max(sums), "least sum": min(sums)}
    limits = []
    for j, log in zip(b["jobs"][4 * len(BIAS_SIZES):], logs[4 * len(BIAS_SIZES):]):
        costs = [c for _, c, _, _ in log["costed"]]
        _, _, total, sse = log["costed"][0]
        limits.append(dict(sum=total, sse=sse, variance=sse - total * total // (int(j["bwidth"]) * int(j["bheight"])),
                           unique_winner_not_first=len(costs) > 1 and costs.count(min(costs)) == 1 and costs.index(min(costs)) != 0))
    st["bias_limits"] = limits
    b = refine_edge_batch("geometry")
    out, _, logs = restated_refine_edge("geometry")
    tiles = [t for log in logs for t in log["seen"]["tiles"]]
    st["geometry"] = {"tiles " + label: sum(1 for t in tiles if f(*t)) for label, f in _tiles_where().items()}
    st["geometry"]["reference indices with costed warps"] = sorted({int(j["ref"]) for j, n in zip(b["jobs"], out["n_valid"]) if n > 0})
    st["geometry"]["wild jobs with costed warps"] = int(sum(1 for k, n in enumerate(out["n_valid"][:-1]) if k % 2 == 1 and n > 0))
    for name in ("walk_0", "walk_1"):
        out, _, logs = restated_refine_edge(name)
        st[name] = {"longest record": int(out["n_checked"].max()), "largest record index of a skip": max(max(log["record_hits"], default=-1) for log in logs),
                    "jobs with more than 64 positions": int((out["n_checked"] > RECORD_SCAN).sum())}
    for name in ("wrap_0", "wrap_1"):
        out, _, logs = restated_refine_edge(name)
        wraps = {"row up": 0, "row down": 0, "col up": 0, "col down": 0}
        for log in logs:
            for comp, wide, got in log["wrapped"]:
                assert got == wc.i16(wide) and got != wide
                wraps[("row", "col")[comp] + (" up" if wide > I16_MAX else " down")] += 1
        won = sum(1 for log, mv in zip(logs, out["best_mv"]) if abs(int(mv[0]) - log["start"][0]) > 32768 or abs(int(mv[1]) - log["start"][1]) > 32768)
        st[name] = dict(wraps, **{"jobs won by a wrapped position": won})
    return st


def edge_coverage_missing():
    """the conditions the new batches exist for that the case lists do not meet"""
    missing = []
    st = refine_edge_stats()
    for name, left in st["sizes_missing"].items():
        if left:
            missing.append(f"{name}: no job with 5 costed warps and a best MV off its start for {left}")
    for label, n in st["bias"].items():
        if label.startswith("sizes with") and n < 3:
            missing.append(f"bias: {label} in {n} sizes")
    lim = st["bias_limits"]
    if not (lim[0]["variance"] == 0 and lim[0]["sse"] == 255 * 255 * 16384 and lim[0]["sum"] == 255 * 16384):
        missing.append(f"bias: reference 255 against source 0 at 128x128: {lim[0]}")
    if not (lim[1]["variance"] == 0 and lim[1]["sum"] == -255 * 16384):
        missing.append(f"bias: reference 0 against source 255 at 128x128: {lim[1]}")
    if not all(abs(l["variance"] - n * 255 * 255 // 4) < n for l, n in zip(lim[2:], (16384, 4096))):
        missing.append(f"bias: a half-and-half source with a variance near N * 255^2 / 4: {lim[2:]}")
    if not any(l["unique_winner_not_first"] for l in lim):
        missing.append("bias: a limit job with a unique winner that is not the first position")
    g = st["geometry"]
    missing += [f"geometry: {k}" for k, v in g.items() if k.startswith("tiles") and not v]
    if g["reference indices with costed warps"] != list(range(8)):
        missing.append(f"geometry: every reference index with costed warps: {g['reference indices with costed warps']}")
    if not g["wild jobs with costed warps"]:
        missing.append("geometry: a wild model with costed warps")
    b = refine_edge_batch("geometry")
    if not restated_refine_edge("geometry")[0]["n_valid"][-1] or int(b["jobs"][-1]["src_offset"]) == (3 + int(b["jobs"][-1]["blk_org_y"])) * 117 + 5 + int(b["jobs"][-1]["blk_org_x"]):
        missing.append("geometry: a costed job whose src_offset is not that of its block origin")
    for name in ("walk_0", "walk_1"):
        if st[name]["longest record"] <= RECORD_SCAN:
            missing.append(f"{name}: n_checked > 64")
        if st[name]["largest record index of a skip"] < RECORD_SCAN:
            missing.append(f"{name}: a skip because of a record entry at index >= 64")
    for name in ("wrap_0", "wrap_1"):
        missing += [f"{name}: a recorded wrap, {k}" for k in ("row up", "row down", "col up", "col down") if not st[name][k]]
        if not st[name]["jobs won by a wrapped position"]:
            missing.append(f"{name}: a job won by a wrapped position")
    missing += far_coverage_missing() + pred_edge_coverage_missing()
    return missing


# ---- the fit ----
FAR_SETTINGS = (0, 0, 65535)  # shut_approx, lower_band_th, upper_band_th: the bands refuse nothing, so that most fits stay valid
# trans_lo_k / trans_hi_k: the clamp of wmmat[k] to -2^23 / 2^23 - 1; valid_clamped: a valid fit with a clamped translation
FAR_CONDITIONS = [c for c in wc.MODEL_CONDITIONS if not c.startswith("band_")] + ["trans_lo_0", "trans_hi_0", "trans_lo_1", "trans_hi_1", "valid_clamped"]


def near_limit(rng):
    return int(rng.choice([I16_MAX - int(rng.integers(0, 200)), I16_MIN + int(rng.integers(0, 200))]))


@functools.lru_cache(maxsize=None)
def far_batch():
    rng = np.random.default_rng(zlib.crc32(b"model_far"))
    regimes = ("calm", "mild", "wild", "huge", "mixed", "lost", "same")
    org = [0, 4, 65532, 65528, 32768, 32764, 3840, 7680, 16384, 49152]
    mvs = np.array([[near_limit(rng), near_limit(rng)] if k % 2 else [int(v) for v in rng.integers(-300, 301, 2)] for k in range(16)], np.int16)
    mvs[0], mvs[1] = (I16_MAX, I16_MIN), (I16_MIN, I16_MAX)
    jobs = []
    for k in range(130):
        bw, bh = wc.SIZES[k % len(wc.SIZES)]
        mv = None
        if k % 3 == 0:  # next to the int16 limits, in one component or in both
            mv = ((near_limit(rng), near_limit(rng)), (near_limit(rng), int(rng.integers(-300, 301))), (int(rng.integers(-300, 301)), near_limit(rng)))[(k // 3) % 3]
        j = wc.model_job(rng, bw, bh, k % 9, regimes[(k // 3) % len(regimes)], mv=mv)
        j["blk_org_x"] = org[k % len(org)] if k % 4 == 0 else int(rng.integers(0, 16384)) * 4
        j["blk_org_y"] = org[(k // 4) % len(org)] if k % 5 == 0 else int(rng.integers(0, 16384)) * 4
        jobs.append(j)
    jobs[0]["blk_org_x"] = jobs[0]["blk_org_y"] = jobs[1]["blk_org_x"] = jobs[2]["blk_org_y"] = 65532
    for k in range(12):
        j = wc.model_job(rng, *wc.SIZES[(5 * k) % len(wc.SIZES)], 3 + k % 6, ("mild", "mixed", "calm")[k % 3], mv=(int(mvs[k][0]), int(mvs[k][1])))
        j["blk_org_x"], j["blk_org_y"] = int(rng.integers(0, 16384)) * 4, int(rng.integers(0, 16384)) * 4
        j["flags"], j["mv_index"], j["mv"] = wc.MV_FROM_ARRAY, k, (-7, 9)
        jobs.append(j)
    b = dict(name="far", shut_approx=FAR_SETTINGS[0], lower_band_th=FAR_SETTINGS[1], upper_band_th=FAR_SETTINGS[2], jobs=wc.pack_jobs(jobs, wc.MODEL_JOB_DTYPE),
             mv_array=mvs)
    traces = []
    wc.restate_models(b, traces)
    # the kernel's 32-bit arithmetic equals the reference's only while nothing wraps: positions and MVs of 16 bits and model terms of at most 8191
    # keep |mv * 2^13 - (isux * a + isuy * b)| under 2^28 + 2 * 65595 * 8191 = 1.34e9, and this holds the builder to it
    assert not any("int32_left" in t for t in traces), "a 32-bit intermediate of find_affine_int wraps on a job of the far batch"
    return b


@functools.lru_cache(maxsize=None)
def restated_far():
    traces = []
    models, status = wc.restate_models(far_batch(), traces)
    return models, status, traces


def far_stats():
    models, _, traces = restated_far()
    clamped = [t for t in traces if any(c.startswith("trans_") for c in t)]
    return {"fits": len(traces), "valid": int(models["valid"].sum()), "valid at a clamped translation": sum(1 for t in clamped if "valid" in t),
            **{c: sum(1 for t in traces if c in t) for c in ("trans_lo_0", "trans_hi_0", "trans_lo_1", "trans_hi_1")}}


def far_coverage_missing():
    b = far_batch()
    _, _, traces = restated_far()
    seen = set().union(*traces)
    if any("valid" in t and any(c.startswith("trans_") for c in t) for t in traces):
        seen.add("valid_clamped")
    missing = [f"far: {c}" for c in FAR_CONDITIONS if c not in seen] + [f"far: n_samples {n}" for n in range(1, 9) if n not in {int(j["n_samples"]) for j in b["jobs"]}]
    orgs = {int(v) for j in b["jobs"] for v in (j["blk_org_x"], j["blk_org_y"])}
    if not {0, 65532} <= orgs or any(v % 4 for v in orgs) or not any(32768 <= v < 65532 for v in orgs):
        missing.append("far: block origins over the whole uint16 range in multiples of 4")
    return missing


# ---- the prediction ----
def pred_edge_names():
    return [f"{kind}_{bd}" for kind in ("big2", "refs8") for bd in (8, 10)]


@functools.lru_cache(maxsize=None)
def pred_edge_batch(name):
    kind, bd = name.split("_")[0], int(name.split("_")[1])
    rng = np.random.default_rng(zlib.crc32(("pred_edge_" + name).encode()))
    if kind == "big2":
        # a 128x128 compound: 256 tiles, the first reference's result held in a register over the second's; the same three jobs with their models in
        # the array
        pw, ph = 160, 136
        planes = [wc.make_plane(rng, bd, pw, ph, kind="smooth"), wc.make_plane(rng, bd, pw, ph, kind="noise")]
        jobs, models, stride = [], [], 131
        for k, (comp_mode, offsets, refs) in enumerate([(0, (0, 0), [0, 1]), (1, wc.QUANT_DIST[2], [1, 0]), (1, wc.QUANT_DIST[5], [0, 1])]):
            ms = [wc.random_model(rng, pw, ph, 2500, wc.ROTZOOM if (k + r) % 3 == 0 else wc.AFFINE, span=10) for r in range(2)]
            p_col, p_row = ((0, 0), (32, 8), (18, 5))[k]
            jobs.append(wc.pred_job(k * 128 * stride + k, p_col, p_row, 128, 128, refs, ms, comp_mode, offsets))
            jobs.append(wc.pred_job((3 + k) * 128 * stride + 2, p_col, p_row, 128, 128, refs, [np.zeros((), wc.MODEL_DTYPE)] * 2, comp_mode, offsets,
                                    flags=wc.MODEL0_FROM_ARRAY | wc.MODEL1_FROM_ARRAY, model_index=(len(models) + 1, len(models))))
            models += [ms[1], ms[0]]
        return dict(name=name, bit_depth=bd, ss_x=0, ss_y=0, planes=planes, jobs=wc.pack_jobs(jobs, wc.PRED_JOB_DTYPE), dst_shape=(6 * 128 + 1, stride), dst_stride=stride,
                    models=wc.pack_jobs(models, wc.MODEL_DTYPE))
    if kind == "refs8":
        pw, ph = 56, 40
        planes = []
        for r in range(8):  # one picture size (a compound reads both references with it), eight strides and origins
            plane, _, _, _, _ = wc.make_plane(rng, bd, pw, ph, pad=0, kind=("noise", "smooth", "extreme")[r % 3])
            pic = plane[:ph, :pw]
            ox, oy, right, below = ((8, 8, 11, 8), (0, 0, 0, 0), (16, 2, 5, 9), (3, 12, 1, 0), (7, 5, 0, 3), (32, 0, 64, 1), (1, 1, 1, 1), (12, 9, 40, 2))[r]
            big = np.full((oy + ph + below, ox + pw + right), 0x155 if bd > 8 else 0x55, pic.dtype)
            big[oy:oy + ph, ox:ox + pw] = pic
            planes.append((big, ox, oy, pw, ph))
        jobs, stride, off = [], 37, 0
        for k in range(20):
            refs = [k % 8, (k + 3) % 8] if k < 16 else [(3 * k) % 8]  # every index first and second in 0 .. 7, again in 8 .. 15, then four single
            a = dict(comp_mode=0) if len(refs) == 1 or k % 2 == 0 else dict(comp_mode=1, offsets=wc.QUANT_DIST[k % 8])
            w, h = ((16, 16), (8, 8), (32, 16), (16, 8))[k % 4]
            ms = [wc.random_model(rng, pw, ph, 3000, wc.AFFINE if (k + r) & 1 else wc.ROTZOOM, span=8) for r in range(len(refs))]
            jobs.append(wc.pred_job(off, int(rng.integers(0, pw - w + 1)), int(rng.integers(0, ph - h + 1)), w, h, refs, ms, **a))
            off += h * stride + (k & 1)
        return dict(name=name, bit_depth=bd, ss_x=0, ss_y=0, planes=planes, jobs=wc.pack_jobs(jobs, wc.PRED_JOB_DTYPE), dst_shape=(off // stride + 2, stride),
                    dst_stride=stride)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def restated_pred_edge(name):
    return wc.restate_pred(pred_edge_batch(name))


def pred_edge_coverage_missing():
    missing = []
    for bd in (8, 10):
        b = pred_edge_batch(f"big2_{bd}")
        _, status, _ = restated_pred_edge(f"big2_{bd}")
        kinds = {(int(j["comp_mode"]), (int(j["fwd_offset"]), int(j["bck_offset"])), bool(int(j["flags"]))) for j, st in zip(b["jobs"], status)
                 if st == wc.ST_OK and (int(j["width"]), int(j["height"])) == (128, 128) and int(j["ref"][1]) != wc.NO_REF}
        if len({k[:2] for k in kinds if k[0] == 1}) < 2 or not any(k[0] == 0 for k in kinds) or {k[2] for k in kinds} != {False, True}:
            missing.append(f"big2_{bd}: a 128x128 compound averaged and weighted with two pairs, the models in the job and in the array")
        b = pred_edge_batch(f"refs8_{bd}")
        _, status, _ = restated_pred_edge(f"refs8_{bd}")
        first = {int(j["ref"][0]) for j, st in zip(b["jobs"], status) if st == wc.ST_OK}
        second = {int(j["ref"][1]) for j, st in zip(b["jobs"], status) if st == wc.ST_OK and int(j["ref"][1]) != wc.NO_REF}
        if len(b["planes"]) != 8 or first != set(range(8)) or second != set(range(8)):
            missing.append(f"refs8_{bd}: every reference index as first and as second reference")
    return missing
