"""The cases of the luma palette search and prediction (svt_hip_palette_search_batch, svt_hip_palette_pred_batch) and a numpy / pure-Python
restatement of what one job computes.

The reference's own results -- search_palette_luma, its three cost functions and its palette prediction driven job by job by
tools/gen_palette_golden.py -- are in golden/palette.npz as numbers only: the colour count of every job, the candidates it keeps (size, colours,
first index, the four rate terms and their sum with the mode bits), a CRC-32 of every kept candidate's colour map and prediction, and the most
candidates any job keeps.  The planes, caches, tables and jobs are regenerated from seeds here.

Restated (Source/Lib/Codec): search_palette_luma, palette_rd_y, optimize_palette_colors, av1_remove_duplicates, extend_palette_color_map,
svt_get_palette_cache_y, svt_av1_palette_color_cost_y, svt_av1_index_color_cache, delta_encode_cost, svt_av1_cost_color_map (palette.c);
svt_av1_k_means_dim1_c, svt_av1_calc_indices_dim1_c, calc_centroids (k_means_template.h) with lcg_rand16 (random.h); svt_av1_count_colors{,_highbd}
(pic_analysis_process.c:1809-1846); svt_aom_get_palette_color_index_context_optimized (cabac_context_model.c:2453-2560); the palette branch of the
luma rate (rd_cost.c:679-706) with svt_aom_write_uniform_cost (entropy_coding.c:4206-4215); the palette branch of svt_av1_predict_intra_block{,_16bit}
(enc_intra_prediction.c:501-510, :647-656).

A batch is one launch: one depth, one set of the per-batch parameters, one set of rate tables.  Every job has a block of its own in the batch's source
plane; the samples of a cropped block that lie outside rows x cols are noise that no output may depend on."""
import functools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "palette.npz")
MAX_CANDS, MAX_SIZE, MAX_CACHE, MAX_ITR = 14, 8, 16, 50
ST_OK, ST_UNDEFINED = 0, 0xFF
JOB_DTYPE = [("src_offset", "<u4"), ("map_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("rows", "u1"), ("cols", "u1"), ("n_cache", "u1"),
             ("bsize_ctx", "u1"), ("mode_ctx", "u1"), ("reserved", "u1"), ("color_cache", "<u2", (MAX_CACHE,))]
CAND_DTYPE = [("size", "u1"), ("first_index", "u1"), ("colors", "<u2", (MAX_SIZE,)), ("top_over", "u1"), ("reserved", "u1"), ("color_cost", "<i4"), ("map_cost", "<i4"),
              ("index0_cost", "<i4"), ("size_cost", "<i4"), ("rate", "<i4")]
RESULT_DTYPE = [("n_colors", "<u4"), ("n_cands", "<u4"), ("cands", CAND_DTYPE, (MAX_CANDS,))]
PRED_JOB_DTYPE = [("search_index", "<u4"), ("cand_index", "<u4"), ("dst_offset", "<u4"), ("map_offset", "<u4")]
COSTS = ("color_cost", "map_cost", "index0_cost", "size_cost", "rate")
# svt_av1_allow_palette: BLOCK_8X8 and every later entry of the BlockSize enum without a side of 128 -- so 4x16 and 16x4 too
SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
PARAMS = {"cost_bit_depth": 8, "dominant_color_step": 1, "reduce_palette_cost_precision": 0}
STRIDE = 288  # of every batch's source plane: four 64-sample columns of blocks and a margin


# ---------------------------------------------------------------------------------------------------------------- the restatement
def palette_cache(above, left):
    """svt_get_palette_cache_y: the merge of the two neighbours' sorted palettes (None: no such neighbour, or above across an SB row)"""
    above, left = list(above or []), list(left or [])
    cache = []

    def add(v):
        if not cache or cache[-1] != v:
            cache.append(v)
    a = b = 0
    if not above and not left:
        return cache
    while a < len(above) and b < len(left):
        va, vl = above[a], left[b]
        if vl < va:
            add(vl)
            b += 1
        else:
            add(va)
            a += 1
            if vl == va:
                b += 1
    for v in above[a:]:
        add(v)
    for v in left[b:]:
        add(v)
    return cache


def calc_indices(data, centroids):
    """svt_av1_calc_indices_dim1_c: strict <, so the first minimum"""
    d = (data[:, None] - np.asarray(centroids, np.int64)[None, :]) ** 2
    return d.argmin(axis=1), d


def k_means(data, centroids, ev):
    """svt_av1_k_means_dim1_c; returns the centroids (the indices are recomputed by palette_rd_y)"""
    n, k = len(data), len(centroids)
    centroids = list(centroids)
    idx, d = calc_indices(data, centroids)
    this_dist = int(d[np.arange(n), idx].sum())
    for _ in range(MAX_ITR):
        pre_dist, pre = this_dist, list(centroids)
        count, total = np.bincount(idx, minlength=k), np.bincount(idx, weights=data, minlength=k).astype(np.int64)
        state = int(data[0]) & 0xFFFFFFFF  # calc_centroids
        for j in range(k):
            if count[j] == 0:
                state = (state * 1103515245 + 12345) & 0xFFFFFFFF
                centroids[j] = int(data[((state // 65536) % 32768) % n])
                ev["empty_cluster"] = True
            else:
                centroids[j] = int((total[j] + (count[j] >> 1)) // count[j])
        idx, d = calc_indices(data, centroids)
        this_dist = int(d[np.arange(n), idx].sum())
        if this_dist > pre_dist:
            centroids = pre
            ev["restore"] = True
            break
        if centroids == pre:
            break
    return centroids


def color_index_context(cmap, r, c):
    """svt_aom_get_palette_color_index_context_optimized: (context, remapped index)"""
    nb = [int(cmap[r, c - 1]) if c >= 1 else -1, int(cmap[r - 1, c]) if r >= 1 else -1, int(cmap[r - 1, c - 1]) if c >= 1 and r >= 1 else -1]
    scores = [2, 2, 1]
    if nb[0] == nb[1]:
        scores[0] += scores[1]
        nb[1] = -1
        if nb[0] == nb[2]:
            scores[0] += scores[2]
            nb[2] = -1
    elif nb[0] == nb[2]:
        scores[0] += scores[2]
        nb[2] = -1
    elif nb[1] == nb[2]:
        scores[1] += scores[2]
        nb[2] = -1
    color_rank, score_rank, valid = [-1, -1, -1], [0, 0, 0], 0
    for i in range(3):
        if nb[i] != -1:
            score_rank[valid], color_rank[valid] = scores[i], nb[i]
            valid += 1

    def swap(a, b):
        score_rank[a], score_rank[b] = score_rank[b], score_rank[a]
        color_rank[a], color_rank[b] = color_rank[b], color_rank[a]
    if score_rank[0] < score_rank[1] or (score_rank[0] == score_rank[1] and color_rank[0] > color_rank[1]):
        swap(0, 1)
    if score_rank[0] < score_rank[2]:
        swap(0, 2)
    if score_rank[1] < score_rank[2]:
        swap(1, 2)
    cur = int(cmap[r, c])
    idx, same = cur, -1
    for i in range(3):
        if color_rank[i] > cur:
            idx += 1
        elif color_rank[i] == cur:
            same = i
    if same != -1:
        idx = same
    h = score_rank[0] + 2 * score_rank[1] + 2 * score_rank[2]
    return [-1, -1, 0, -1, -1, 4, 3, 2, 1][h], idx


def cost_color_map(cmap, rows, cols, n, ycolor):
    """svt_av1_cost_color_map: the reference walks the anti-diagonals; the sum does not depend on the order"""
    rate = 0
    for r in range(rows):
        for c in range(cols):
            if r or c:
                ctx, idx = color_index_context(cmap, r, c)
                rate += int(ycolor[n - 2][ctx][idx])
    return rate


def ceil_log2(n):
    return 0 if n < 2 else (n - 1).bit_length()


def delta_encode_cost(colors, bit_depth, min_val=1):
    num = len(colors)
    if num <= 0:
        return 0
    bits = bit_depth
    if num == 1:
        return bits
    bits += 2
    deltas = [colors[i] - colors[i - 1] for i in range(1, num)]
    per = max(ceil_log2(max(max(deltas), 0) + 1 - min_val), bit_depth - 3)
    rng = (1 << bit_depth) - colors[0] - min_val
    for d in deltas:
        bits += per
        rng -= d
        per = min(per, ceil_log2(rng))
    return bits


def color_cost_y(colors, cache, bit_depth, ev=None):
    """svt_av1_palette_color_cost_y with svt_av1_index_color_cache"""
    n = len(colors)
    if len(cache) <= 0:
        out = list(colors)
    else:
        flags, n_in = [0] * n, 0
        for cv in cache:
            if n_in >= n:
                break
            for j in range(n):
                if colors[j] == cv:
                    flags[j] = 1
                    n_in += 1
                    break
        out = [colors[i] for i in range(n) if not flags[i]]
        if ev is not None:
            ev["cache_found"] |= n_in > 0
            ev["cache_not_found"] |= len(out) > 0
    return (len(cache) + delta_encode_cost(out, bit_depth)) * 512


def write_uniform_cost(n, v):
    length = n.bit_length() if n > 0 else 0
    if length == 0:
        return 0
    return (length - 1 if v < (1 << length) - n else length) * 512


def job_cache(job):
    return [int(v) for v in job["color_cache"][:int(job["n_cache"])]]


def job_defined(job, bit_depth, src_stride, src_samples, map_bytes=None):
    """what the search kernel's refusal says; map_bytes None: no color_maps"""
    w, h, rows, cols = (int(job[k]) for k in ("width", "height", "rows", "cols"))
    if (w, h) not in SIZES or not (1 <= rows <= h and 1 <= cols <= w) or job["n_cache"] > MAX_CACHE or job["bsize_ctx"] >= 7 or job["mode_ctx"] >= 3:
        return False
    if int(job["src_offset"]) + (rows - 1) * src_stride + cols > src_samples:
        return False
    return map_bytes is None or int(job["map_offset"]) + MAX_CANDS * w * h <= map_bytes


def restate_job(src, bit_depth, job, params, tables):
    """One search job and the prediction of every candidate it keeps.  src: the source plane [H][W]; tables: {"ycolor" [7][5][8], "ysize" [7][8],
    "ymode" [7][3][3]}.  Returns {"n_colors", "n_cands", "cands": [{"size", "colors", "first_index", the five COSTS, "map" [h][w] uint8, "pred" [h][w]
    uint16}], "events"}."""
    w, h, rows, cols = (int(job[k]) for k in ("width", "height", "rows", "cols"))
    y0, x0 = divmod(int(job["src_offset"]), src.shape[1])
    block = src[y0:y0 + rows, x0:x0 + cols].astype(np.int64)
    data = block.reshape(-1)
    cache, max_val = job_cache(job), (1 << bit_depth) - 1
    ev = dict(empty_cluster=False, restore=False, snap=False, dedup=False, dropped=False, dom_differs=False, top_tie=False, equidistant=False,
              cache_found=False, cache_not_found=False, top_over=False)
    out = {"n_colors": 0, "n_cands": 0, "cands": [], "events": ev}
    if bit_depth > 8 and data.max() >= 1 << bit_depth:
        return out  # svt_av1_count_colors_highbd returns 0
    hist = np.bincount(data, minlength=1 << bit_depth)
    colors = int(np.count_nonzero(hist))
    out["n_colors"] = colors
    if not (1 < colors <= 64):
        return out
    lb, ub = int(data.min()), int(data.max())
    work, top = hist.copy(), []
    for _ in range(min(colors, MAX_SIZE)):
        t = int(work.argmax())  # the first maximum: the lower value among equal counts
        ev["top_tie"] |= int(np.count_nonzero(work == work[t])) > 1
        top.append(t)
        work[t] = 0
    bsize_ctx, mode_ctx = int(job["bsize_ctx"]), int(job["mode_ctx"])
    kept_by_n = {}

    def palette_rd_y(centroids, kind):
        n = len(centroids)
        cen = list(centroids)
        if cache:  # optimize_palette_colors
            for i in range(n):
                diffs = [abs(cen[i] - cv) for cv in cache]
                m = min(diffs)
                if m <= 1:
                    ev["snap"] |= cen[i] != cache[diffs.index(m)]
                    cen[i] = cache[diffs.index(m)]
        uniq = sorted(set(cen))
        k = len(uniq)
        ev["dedup"] |= 2 < k < n
        ev["dropped"] |= n > 2 and k <= 2
        if k <= 2:  # k < PALETTE_MIN_SIZE: size 0; k == 2: not counted
            return
        pal = [min(max(v, 0), max_val) for v in uniq]
        idx, d = calc_indices(data, uniq)
        two = np.sort(d, axis=1)[:, :2]
        ev["equidistant"] |= bool(np.any(two[:, 0] == two[:, 1]))
        cmap = np.pad(idx.reshape(rows, cols).astype(np.uint8), ((0, h - rows), (0, w - cols)), mode="edge")  # extend_palette_color_map
        c = {"size": k, "colors": pal, "first_index": int(cmap[0, 0]), "top_over": int(uniq[-1] > max_val)}
        ev["top_over"] |= uniq[-1] > max_val
        c["color_cost"] = color_cost_y(pal, cache, params["cost_bit_depth"], ev)
        c["map_cost"] = 0 if params["reduce_palette_cost_precision"] else cost_color_map(cmap, rows, cols, k, tables["ycolor"])
        c["index0_cost"] = write_uniform_cost(k, c["first_index"])
        c["size_cost"] = int(tables["ysize"][bsize_ctx][k - 2])
        c["rate"] = int(tables["ymode"][bsize_ctx][mode_ctx][1]) + c["size_cost"] + c["index0_cost"] + c["color_cost"] + c["map_cost"]
        c["map"] = cmap
        c["pred"] = np.minimum(np.asarray(pal, np.uint16)[cmap], 0xFF if bit_depth == 8 else 0xFFFF).astype(np.uint16)
        out["cands"].append(c)
        kept_by_n.setdefault(n, {})[kind] = pal

    for n in range(min(colors, MAX_SIZE), 1, -params["dominant_color_step"]):
        palette_rd_y(top[:n], "dominant")
    for n in range(min(colors, MAX_SIZE), 1, -1):
        if colors == 2:
            cen = [lb, ub]
        else:
            cen = k_means(data, [lb + (2 * i + 1) * (ub - lb) // n // 2 for i in range(n)], ev)
        palette_rd_y(cen, "kmeans")
    ev["dom_differs"] = any(len(v) == 2 and v["dominant"] != v["kmeans"] for v in kept_by_n.values())
    out["n_cands"] = len(out["cands"])
    assert out["n_cands"] <= MAX_CANDS
    return out


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- the case list
def cost_tables(seed):
    rng = np.random.default_rng(seed)
    return {"ycolor": rng.integers(20, 6000, (7, 5, 8)).astype(np.int32), "ysize": rng.integers(100, 3000, (7, 8)).astype(np.int32),
            "ymode": rng.integers(30, 2500, (7, 3, 3)).astype(np.int32)}


def spec(w, h, kind, k=0, rows=None, cols=None, above=None, left=None, mode_ctx=None, **kw):
    return dict(w=w, h=h, kind=kind, k=k, rows=h if rows is None else rows, cols=w if cols is None else cols, above=above, left=left, mode_ctx=mode_ctx, **kw)


def make_block(rng, s, bit_depth):
    """the rows x cols samples of a job, by kind:
    k        exactly k distinct values spread over the range, in patches with skewed frequencies
    near     k values in a few tight groups, so that rounded means collide and a cache colour one step away attracts several of them
    stripes  k values with equal counts
    values   the list `values` cycled with the frequencies `freq`
    noise    every sample random: far more than 64 colours
    oob      k values and one sample of 1 << bit_depth or above"""
    rows, cols, k, kind = s["rows"], s["cols"], s["k"], s["kind"]
    top = (1 << bit_depth) - 1
    n = rows * cols
    if kind == "noise":
        return rng.integers(0, top + 1, (rows, cols))
    if kind == "values":
        vals = np.asarray(s["values"])
        p = np.asarray(s.get("freq", [1] * len(vals)), float)
        a = rng.choice(len(vals), n, p=p / p.sum())
        a[:len(vals)] = np.arange(len(vals))  # each at least once, the first of them at (0, 0)
        return vals[a].reshape(rows, cols)
    if kind == "stripes":
        vals = np.sort(rng.choice(top + 1, k, replace=False))
        return vals[(np.arange(n) * k // n)].reshape(rows, cols)[:, ::-1]
    if kind == "near":
        centres = np.sort(rng.choice(np.arange(8, top - 8), max(2, k // 3), replace=False))
        vals = np.unique(np.clip(np.concatenate([centres + o for o in (-2, -1, 0, 1, 2, 3)]), 0, top))
        vals = rng.permutation(vals)[:k]
    else:
        vals = rng.choice(top + 1, k, replace=False)
        if s.get("extremes"):  # 0 and the largest value among them
            vals = np.concatenate([[0, top], rng.choice(np.arange(1, top), k - 2, replace=False)])
    k = len(vals)
    p = rng.dirichlet(np.full(k, 0.6)) + 0.02
    coarse = rng.choice(k, ((rows + 3) // 4, (cols + 3) // 4), p=p / p.sum())  # patches of 4 x 4, then single samples re-drawn
    a = np.kron(coarse, np.ones((4, 4), int))[:rows, :cols].reshape(-1)
    redraw = rng.random(n) < 0.25
    a[redraw] = rng.choice(k, int(redraw.sum()), p=p / p.sum())
    a[rng.permutation(n)[:k]] = np.arange(k)  # every value at least once
    blk = vals[a].reshape(rows, cols)
    if s.get("extremes"):
        blk[0, 0] = 0
    if kind == "oob":
        blk[rows // 2, cols // 3] = (1 << bit_depth) + int(rng.integers(0, 3000))
    return blk


def near_palette(rng, values, size, top, shift=(-1, 0, 1)):
    """a neighbour's palette: `size` sorted distinct colours, most of them a block value or one step from it"""
    vals = np.unique(values)
    picks = set()
    while len(picks) < size:
        v = int(rng.choice(vals)) + int(rng.choice(shift)) if rng.random() < 0.75 else int(rng.integers(0, top + 1))
        picks.add(min(max(v, 0), top))
    return sorted(picks)


def batch_specs(name):
    kind, bd = name.rsplit("_", 1)
    bd = int(bd)
    top = (1 << bd) - 1
    if kind == "sizes":  # every size, a handful of colours, caches of every length
        return [spec(w, h, "k" if i % 3 else "near", k=3 + (5 * i) % 11, nbr=("both", "left", "none", "above", "full")[i % 5], extremes=i % 4 == 1)
                for i, (w, h) in enumerate(SIZES)]
    if kind == "colors":  # the gate and the special cases around it
        out = [spec(8, 8, "values", values=[top // 3]), spec(8, 8, "values", values=[7, top - 9], nbr="both"), spec(8, 8, "k", k=3, nbr="left"),
               spec(8, 8, "k", k=8, nbr="both"), spec(16, 16, "k", k=9, nbr="above"), spec(8, 8, "k", k=64, nbr="full"), spec(16, 16, "k", k=64, nbr="both"),
               spec(16, 16, "k", k=65, nbr="both"), spec(16, 16, "noise"), spec(8, 16, "stripes", k=4, nbr="none"), spec(16, 8, "stripes", k=16, nbr="left"),
               spec(8, 8, "values", values=[0, 1, 2, 3, top], freq=[8, 4, 2, 1, 1], nbr="none"), spec(16, 16, "near", k=12, nbr="full"),
               spec(8, 8, "values", values=[10, 12, top - 40], freq=[3, 2, 2], above=[11, top - 100], left=None),  # 10 and 12 both become 11: two colours left
               spec(8, 8, "values", values=[20, 22, 90, top - 30], freq=[3, 3, 2, 2], above=[21], left=[21, top - 29]),  # four become three
               spec(16, 16, "values", values=[0, 4, 8, 100, 104, top - 4, top], freq=[5, 1, 5, 2, 2, 3, 3], nbr="both"),
               spec(8, 8, "values", values=[0, 2, 4, 6, 50], freq=[1, 1, 1, 1, 3], nbr="none")]
        if bd == 10:
            out += [spec(8, 8, "oob", k=5, nbr="both"), spec(16, 16, "oob", k=70)]
        return out
    if kind == "crop":  # rows only, columns only, both; 64 x 64 with 64 colours
        return [spec(16, 16, "k", k=7, rows=8, nbr="both"), spec(16, 16, "k", k=7, cols=8, nbr="left"), spec(16, 16, "near", k=9, rows=12, cols=4, nbr="full"),
                spec(8, 8, "k", k=5, rows=4, cols=4, nbr="none"), spec(4, 16, "k", k=6, rows=9, nbr="above"), spec(16, 4, "k", k=6, cols=11, nbr="both"),
                spec(64, 64, "k", k=64, nbr="full"), spec(64, 64, "k", k=40, rows=40, cols=52, nbr="both"), spec(32, 32, "near", k=20, rows=31, cols=1, nbr="left"),
                spec(8, 16, "k", k=4, rows=1, nbr="both"), spec(32, 8, "k", k=10, cols=20, rows=5, nbr="above")]
    if kind in ("step2", "lean"):  # dominant_color_step 2; no map cost; a 10-bit cost depth over 8-bit planes
        return [spec(w, h, "k" if i % 2 else "near", k=(4, 8, 13, 30, 5, 9)[i % 6], nbr=("both", "none", "full", "left")[i % 4], rows=h - (i % 3 == 2) * 3)
                for i, (w, h) in enumerate([(8, 8), (16, 16), (8, 16), (4, 16), (16, 4), (32, 16), (16, 8), (8, 32)])]
    if kind == "dual":  # a 10-bit encode searched at 8 bits: the neighbours' palettes are 10-bit colours (8-bit ones times 4), most above 255
        return [spec(8, 8, "values", values=[12, 90, top], freq=[2, 2, 5], above=[12, 256, 800], left=[88, 1020]),  # 255 becomes 256, clipped to 255
                spec(8, 8, "values", values=[40, 130, 254, top], freq=[2, 2, 3, 3], above=[256], left=None),  # 255 lies as far from 254 as from 256
                spec(16, 16, "values", values=[0, 60, 61, 200, 253, top], freq=[2, 2, 2, 2, 1, 4], above=[60, 256], left=[256, 400, 1020]),
                spec(8, 16, "values", values=[7, 100, 180, top], freq=[1, 1, 1, 2], above=[254], left=[256]),  # 254 comes first: 255 becomes 254
                spec(16, 8, "values", values=[7, 100, 180, top], freq=[1, 1, 1, 2], above=[255, 256], left=[256, 512]),  # 255 is in the cache: it stays
                spec(16, 16, "k", k=9, nbr="both", scale=4, extremes=True), spec(4, 16, "near", k=7, nbr="full", scale=4),
                spec(32, 32, "k", k=20, nbr="both", scale=4, extremes=True, add=256, rows=20, cols=28), spec(16, 4, "k", k=5, nbr="left", scale=4, add=256, extremes=True)]
    if kind == "over":  # the same one step above the maximum at 10 bits, which no encode produces but the arithmetic allows
        return [spec(8, 8, "values", values=[5, 500, top - 1, top], freq=[2, 2, 3, 3], above=[top + 1], left=[500]),
                spec(16, 16, "k", k=12, nbr="both", add=top + 1, extremes=True)]
    raise KeyError(name)


BATCH_PARAMS = {"sizes": {}, "colors": {}, "crop": {}, "step2": {"dominant_color_step": 2}, "lean": {"reduce_palette_cost_precision": 1, "cost_bit_depth": 10},
                "dual": {"cost_bit_depth": 10}, "over": {}}


def batch_names():
    return [f"{k}_{bd}" for k in ("sizes", "colors", "crop", "step2") for bd in (8, 10)] + ["lean_8", "dual_8", "over_10"]


@functools.lru_cache(maxsize=None)
def batch(name):
    """{"bit_depth", "params", "tables", "src" [H][STRIDE], "jobs", "nbrs" [(above, left)], "map_bytes", "specs"}"""
    kind, bd = name.rsplit("_", 1)
    bd = int(bd)
    top = (1 << bd) - 1
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    specs = batch_specs(name)
    n = len(specs)
    dt = np.uint16 if bd > 8 else np.uint8
    params = dict(PARAMS, cost_bit_depth=bd)
    params.update(BATCH_PARAMS[kind])
    src = rng.integers(0, top + 1, ((n + 3) // 4 * 64 + 3, STRIDE)).astype(dt)  # noise everywhere a job does not plant its samples
    jobs, nbrs, maps = np.zeros(n, JOB_DTYPE), [], 0
    for i, s in enumerate(specs):
        y0, x0 = (i // 4) * 64 + (i % 3), (i % 4) * 64 + 5 + (i % 5)
        blk = make_block(rng, s, bd)
        src[y0:y0 + s["rows"], x0:x0 + s["cols"]] = blk.astype(dt)
        nbr = s.get("nbr")
        above, left = s["above"], s["left"]
        ok = blk[blk <= top]
        if nbr == "both":
            above, left = near_palette(rng, ok, int(rng.integers(2, 6)), top), near_palette(rng, ok, int(rng.integers(2, 6)), top)
        elif nbr == "left":
            left = near_palette(rng, ok, int(rng.integers(1, 9)), top)
        elif nbr == "above":
            above = near_palette(rng, ok, int(rng.integers(1, 9)), top)
        elif nbr == "full":  # sixteen distinct colours
            both = near_palette(rng, ok, 16, top, shift=(-1, 1, 2))
            pick = rng.permutation(16)
            above, left = sorted(both[q] for q in pick[:8]), sorted(both[q] for q in pick[8:])
        if s.get("scale"):  # the neighbours' colours as a 10-bit encode keeps them
            above, left = ([v * s["scale"] for v in p] if p is not None else None for p in (above, left))
        if s.get("add") is not None:
            left = sorted({s["add"]} | set(sorted(set(left or []) - {s["add"]})[-7:]))
        cache = palette_cache(above, left)
        j = jobs[i]
        j["src_offset"], j["width"], j["height"], j["rows"], j["cols"] = y0 * STRIDE + x0, s["w"], s["h"], s["rows"], s["cols"]
        j["n_cache"], j["color_cache"][:len(cache)] = len(cache), cache
        j["color_cache"][len(cache):] = top  # never read
        j["bsize_ctx"] = (s["w"] * s["h"]).bit_length() - 1 - 6  # svt_aom_get_palette_bsize_ctx
        j["mode_ctx"] = (1 if above else 0) + (1 if left else 0) if s["mode_ctx"] is None else s["mode_ctx"]  # svt_aom_get_palette_mode_ctx
        maps += i % 3 == 1  # some maps start at an odd address
        j["map_offset"] = maps
        maps += MAX_CANDS * s["w"] * s["h"]
        nbrs.append((above, left))
    return {"bit_depth": bd, "params": params, "tables": cost_tables(zlib.crc32(name.encode()) + 1), "src": src, "jobs": jobs, "nbrs": nbrs, "map_bytes": maps + 7,
            "specs": specs}


@functools.lru_cache(maxsize=None)
def restated(name):
    b = batch(name)
    return [restate_job(b["src"], b["bit_depth"], j, b["params"], b["tables"]) for j in b["jobs"]]


def fixture_arrays(name, results):
    """what golden/palette.npz holds of a batch; `results` as restated()'s"""
    n = len(results)
    a = {"n_colors": np.zeros(n, np.uint32), "n_cands": np.zeros(n, np.uint32), "size": np.zeros((n, MAX_CANDS), np.uint8),
         "first_index": np.zeros((n, MAX_CANDS), np.uint8), "colors": np.zeros((n, MAX_CANDS, MAX_SIZE), np.uint16),
         "costs": np.zeros((n, MAX_CANDS, len(COSTS)), np.int32), "map_crc": np.zeros((n, MAX_CANDS), np.uint32), "pred_crc": np.zeros((n, MAX_CANDS), np.uint32)}
    for i, r in enumerate(results):
        a["n_colors"][i], a["n_cands"][i] = r["n_colors"], r["n_cands"]
        for q, c in enumerate(r["cands"]):
            a["size"][i, q], a["first_index"][i, q], a["colors"][i, q, :c["size"]] = c["size"], c["first_index"], c["colors"]
            a["costs"][i, q] = [c[k] for k in COSTS]
            a["map_crc"][i, q], a["pred_crc"][i, q] = crc(np.asarray(c["map"], np.uint8)), crc(np.asarray(c["pred"], np.uint16))
    a["max_cands"] = np.array([max(r["n_cands"] for r in results)], np.uint32)
    return {f"{name}_{k}": v for k, v in a.items()}


def result_records(results, fill, defined=None):
    """the result array as the kernel leaves it over bytes of `fill`: the records past n_cands, and all of an undefined job, untouched"""
    rec = np.frombuffer(bytes([fill]) * (np.dtype(RESULT_DTYPE).itemsize * len(results)), RESULT_DTYPE).copy()
    for i, r in enumerate(results):
        if defined is not None and not defined[i]:
            continue
        rec[i]["n_colors"], rec[i]["n_cands"] = r["n_colors"], r["n_cands"]
        for q, c in enumerate(r["cands"]):
            t = rec[i]["cands"][q]
            t["size"], t["first_index"], t["top_over"], t["reserved"] = c["size"], c["first_index"], c["top_over"], 0
            t["colors"] = 0
            t["colors"][:c["size"]] = c["colors"]
            for k in COSTS:
                t[k] = c[k]
    return rec


def expected_maps(jobs, results, map_bytes, fill, defined=None):
    """color_maps as the search leaves it"""
    buf = np.full(map_bytes, fill, np.uint8)
    for i, (j, r) in enumerate(zip(jobs, results)):
        if defined is not None and not defined[i]:
            continue
        wh = int(j["width"]) * int(j["height"])
        for q, c in enumerate(r["cands"]):
            o = int(j["map_offset"]) + q * wh
            buf[o:o + wh] = c["map"].reshape(-1)
    return buf


DST_STRIDE = 80  # of the prediction plane of the tests: wider than any block, a multiple of no block width above 16


def pred_jobs(jobs, results=None):
    """prediction jobs for the search jobs `jobs`: with `results` the kept candidates only, else every slot of every search job (so most name a
    candidate >= n_cands).  The blocks lie one below the other in a plane of DST_STRIDE samples, every other one 5 samples in; the maps are packed.
    Returns (jobs, dst_samples, map_bytes)."""
    out, y, maps = [], 0, 0
    for i, j in enumerate(jobs):
        w, h = int(j["width"]), int(j["height"])
        for q in range(MAX_CANDS if results is None else results[i]["n_cands"]):
            out.append((i, q, y * DST_STRIDE + 5 * (len(out) % 2), maps))
            y, maps = y + (h if 1 <= h <= 64 else 1), maps + (w * h if (w, h) in SIZES else 0)
    return np.array(out, PRED_JOB_DTYPE), max(1, y) * DST_STRIDE, max(1, maps)


def expected_pred(bit_depth, results, pjobs, dst_samples, map_bytes, fill, search_defined=None):
    """(dst [rows][DST_STRIDE], color_map, status) of svt_hip_palette_pred_batch; `results` as restated()'s, one per search job"""
    dt = np.uint16 if bit_depth > 8 else np.uint8
    dst = np.frombuffer(bytes([fill]) * (dst_samples * np.dtype(dt).itemsize), dt).copy().reshape(-1, DST_STRIDE)
    cmap, status = np.full(map_bytes, fill, np.uint8), np.zeros(len(pjobs), np.uint8)
    for i, p in enumerate(pjobs):
        si, q = int(p["search_index"]), int(p["cand_index"])
        if si >= len(results) or (search_defined is not None and not search_defined[si]) or q >= results[si]["n_cands"]:
            status[i] = ST_UNDEFINED
            continue
        c = results[si]["cands"][q]
        h, w = c["map"].shape
        y, x = divmod(int(p["dst_offset"]), DST_STRIDE)
        dst[y:y + h, x:x + w] = c["pred"].astype(dt)
        cmap[int(p["map_offset"]):int(p["map_offset"]) + w * h] = c["map"].reshape(-1)
    return dst, cmap, status


def coverage_missing():
    """the conditions a fixture must meet (listed in tests/test_palette.py) that the case list does not"""
    missing = []
    seen = {bd: set() for bd in (8, 10)}
    colors = {bd: set() for bd in (8, 10)}
    ev = {}
    caches, steps, precisions, crops = set(), set(), set(), set()
    flags = dict(oob=False, zero_top_8=False, zero_top_10=False, data0_zero=False, cache_above_255_at_8_bits=False, top_over_8=False, top_over_10=False)
    for name in batch_names():
        b = batch(name)
        bd, top = b["bit_depth"], (1 << b["bit_depth"]) - 1
        steps.add(b["params"]["dominant_color_step"])
        precisions.add(b["params"]["reduce_palette_cost_precision"])
        for j, r in zip(b["jobs"], restated(name)):
            w, h, rows, cols = (int(j[k]) for k in ("width", "height", "rows", "cols"))
            seen[bd].add((w, h))
            colors[bd].add(r["n_colors"])
            for k, v in r["events"].items():
                ev[k] = ev.get(k, False) or v
            if r["n_cands"]:
                caches.add(int(j["n_cache"]))
                crops.add((rows < h, cols < w))
            y0, x0 = divmod(int(j["src_offset"]), STRIDE)
            blk = b["src"][y0:y0 + rows, x0:x0 + cols]
            flags["oob"] |= bd == 10 and int(blk.max()) >= 1024
            if r["n_cands"]:
                flags[f"zero_top_{bd}"] |= int(blk.min()) == 0 and int(blk.max()) == top
                flags["data0_zero"] |= int(blk[0, 0]) == 0
                flags["cache_above_255_at_8_bits"] |= bd == 8 and b["params"]["cost_bit_depth"] == 10 and max(job_cache(j), default=0) > 256
                flags[f"top_over_{bd}"] |= any(c["top_over"] for c in r["cands"])
    for bd in (8, 10):
        missing += [f"size {s} at {bd} bits" for s in SIZES if s not in seen[bd]]
        missing += [f"{c} colours at {bd} bits" for c in (1, 2, 3, 8, 9, 64, 65) if c not in colors[bd]]
        missing += [f"far more than 64 colours at {bd} bits"] * (max(colors[bd]) < 150)
    missing += [k for k in ("empty_cluster", "snap", "dedup", "dropped", "dom_differs", "top_tie", "equidistant", "cache_found", "cache_not_found") if not ev.get(k)]
    missing += ["the restore fired"] * bool(ev.get("restore"))
    missing += [k for k, v in flags.items() if not v]
    missing += ["n_cache 0"] * (0 not in caches) + ["n_cache 16"] * (16 not in caches) + ["n_cache in between"] * (not any(0 < c < 16 for c in caches))
    missing += [f"step {s}" for s in (1, 2) if s not in steps] + [f"cost precision {p}" for p in (0, 1) if p not in precisions]
    missing += [f"crop {c}" for c in ((True, False), (False, True), (True, True), (False, False)) if c not in crops]
    return missing


def max_cands():
    return max(r["n_cands"] for name in batch_names() for r in restated(name))


def undefined_batch(bd):
    """the jobs of sizes_<bd> that fit 32 x 32 with one job of each refused kind among them: (batch, indices of the undefined ones)"""
    b = dict(batch(f"sizes_{bd}"))
    keep = [i for i, j in enumerate(b["jobs"]) if int(j["width"]) * int(j["height"]) <= 512]
    good = b["jobs"][keep]
    spoil = [("width", 4, "height", 8), ("width", 64, "height", 8), ("width", 12, "height", 12), ("rows", 0), ("cols", 0), ("rows", 200), ("cols", 65),
             ("n_cache", 17), ("bsize_ctx", 7), ("mode_ctx", 3), ("src_offset", b["src"].size - 3), ("map_offset", b["map_bytes"] - 100),
             ]
    jobs, bad = [], []
    for i, s in enumerate(spoil):
        jobs.append(good[i % len(good)].copy())
        j = good[(i + 1) % len(good)].copy()
        for k, v in zip(s[::2], s[1::2]):
            j[k] = v
        bad.append(len(jobs))
        jobs.append(j)
    b["jobs"] = np.array(jobs, JOB_DTYPE)
    return b, bad


def spoil_desc(d, bad):
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad == "bit_depth_12":
        d.bit_depth = 12
    elif bad == "bit_depth_0":
        d.bit_depth = 0
    elif bad == "cost_bit_depth_12":
        d.cost_bit_depth = 12
    elif bad == "step_0":
        d.dominant_color_step = 0
    elif bad == "step_3":
        d.dominant_color_step = 3
    elif bad == "zero_src_stride":
        d.src_stride = 0
    elif bad == "zero_src_samples":
        d.src_samples = 0
    elif bad == "maps_without_bytes":
        d.map_bytes = 0
    elif bad == "hbd_cost_8":
        d.bit_depth, d.cost_bit_depth = 10, 8
    else:
        raise KeyError(bad)
    return d


SPOILS = ["hbd_cost_8", "no_src", "no_jobs", "no_results", "no_status", "no_palette_ycolor_fac_bitss", "no_palette_ysize_fac_bits", "no_palette_ymode_fac_bits", "bit_depth_12",
          "bit_depth_0", "cost_bit_depth_12", "step_0", "step_3", "zero_src_stride", "zero_src_samples", "maps_without_bytes"]


def spoil_pred_desc(d, bad):
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad == "bit_depth_12":
        d.bit_depth = 12
    elif bad.startswith("zero_"):
        setattr(d, bad[5:], 0)
    elif bad == "map_without_bytes":
        d.map_bytes = 0
    else:
        raise KeyError(bad)
    return d


PRED_SPOILS = ["no_src", "no_dst", "no_search_jobs", "no_search_results", "no_search_status", "no_jobs", "no_status", "bit_depth_12", "zero_src_stride",
               "zero_src_samples", "zero_dst_stride", "zero_dst_samples", "zero_n_search_jobs", "map_without_bytes"]
