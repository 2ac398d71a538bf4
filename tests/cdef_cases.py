"""Numpy restatements of the three CDEF stages -- the strength search (cdef_seg_search), the joint strength selection (finish_cdef_search) and the
filter (svt_av1_cdef_frame) --, the case list the CPU and GPU tests and tools/gen_cdef_golden.py share, and the conditions the list has to meet.
The restatements follow the reference's own loops (cdef.c:84-430, enc_cdef.c:23-219, :284-965, cdef_process.c:106-349), not the kernels' lay-out;
the luma distortion is float64, whose square root numpy rounds correctly.  A plain helper module, not a conftest."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cdef.npz")
FILL = 0xA5
LARGE = 0x7F7F
NONE = 1 << 63
DEFAULT_MSE_UV = 1040400 * 64
MSB = np.array([max(v.bit_length() - 1, 0) for v in range(1 << 16)], np.int64)
DIRS = np.array([[[-1, 1], [-2, 2]], [[0, 1], [-1, 2]], [[0, 1], [0, 2]], [[0, 1], [1, 2]], [[1, 1], [2, 2]], [[1, 0], [2, 1]], [[1, 0], [2, 0]], [[1, 0], [2, -1]]], np.int64)
DIV_TABLE = [0, 840, 420, 280, 210, 168, 140, 120, 105]


def n_fb_of(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


# ---- pictures and masks, from seeds ----
def line_of(d, i, j):
    return [i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j][d]


def luma_pattern(kind, w, h, bd, rng):
    """(source, reconstruction) of the luma plane as int arrays"""
    top = (1 << bd) - 1
    cs = bd - 8
    if kind == "noise":
        src = rng.integers(0, top + 1, (h, w))
        rec = np.clip(src + rng.integers(-(6 << cs), (6 << cs) + 1, (h, w)), 0, top)
    elif kind == "flat":
        src = np.full((h, w), 100 << cs)
        rec = np.full((h, w), 101 << cs)
        rec[1::16, 2::16] += 2 << cs  # lone spikes: every neighbour lower by a little
        rec[6::16, 5::16] -= 2 << cs
    elif kind == "grating":  # every 8x8 block constant along the lines of one of the eight directions, the direction changing from block to block
        src = np.zeros((h, w), np.int64)
        for by in range(h // 8):
            for bx in range(w // 8):
                d = (by * 3 + bx) % 8
                amp = [60, 12, 3, 1][(by + bx // 8) % 4] << cs
                for i in range(8):
                    for j in range(8):
                        src[8 * by + i, 8 * bx + j] = (120 << cs) + (amp if line_of(d, i, j) % 4 < 2 else -amp)
        rec = np.clip(src + rng.integers(-(3 << cs), (3 << cs) + 1, (h, w)), 0, top)
    elif kind == "steps":  # saturated steps, vertical and horizontal and diagonal, with a little noise on one side
        yy, xx = np.mgrid[0:h, 0:w]
        src = np.where(((xx // 5) + (yy // 11)) % 2 == 0, 0, top)
        src = np.where((xx + yy) % 32 < 6, top - src, src)
        rec = np.clip(src + np.where(src == 0, rng.integers(0, (3 << cs) + 1, (h, w)), -rng.integers(0, (3 << cs) + 1, (h, w))), 0, top)
    else:
        raise ValueError(kind)
    return src.astype(np.int64), rec.astype(np.int64)


def picture(kind, w, h, bd, seed):
    """(recon, src): three planes each, uint8 or uint16, 4:2:0"""
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bd > 8 else np.uint8
    recon, src = [], []
    for pli, (pw, ph) in enumerate([(w, h), (w // 2, h // 2), (w // 2, h // 2)]):
        if pli == 0:
            s, r = luma_pattern(kind, pw, ph, bd, rng)
        else:  # chroma: the same kind at its own size, padded to a multiple of 8 for the generators that want it and cropped
            s, r = luma_pattern(kind, (pw + 7) // 8 * 8, (ph + 7) // 8 * 8, bd, rng)
            s, r = s[:ph, :pw], r[:ph, :pw]
        recon.append(r.astype(dt))
        src.append(s.astype(dt))
    return recon, src


def masks_of(kind, w, h, seed=0):
    """n_fb uint64: "full" (with stray bits outside the picture in every filter block), "empty", "one" (one block per filter block), "checker", "mixed"
    (the four in turn), "random" """
    n = n_fb_of(w, h)
    rng = np.random.default_rng(1000 + seed)
    full, checker = (1 << 64) - 1, 0xAA55AA55AA55AA55
    out = []
    for fb in range(n):
        k = ["full", "empty", "one", "checker"][fb % 4] if kind == "mixed" else kind
        out.append({"full": full, "empty": 0, "one": 1 << ((9 * fb) % 64 if w >= 64 and h >= 64 else 0), "checker": checker,
                    "random": int(rng.integers(0, 1 << 63)) | 1}[k])
    return np.array(out, np.uint64)


def valid_mask(hs, vs):
    m = 0
    for by in range(vs // 8):
        m |= ((1 << (hs // 8)) - 1) << (8 * by)
    return m


# ---- shared pieces ----
def window(plane, fbr, fbc, nvfb, nhfb, bs):
    """the reference's `in` of a filter block with its borders: [bs + 6][bs + 16] ints, sample (0, 0) of the block at [3][8]; and the block's size"""
    h, w = plane.shape
    x0, y0 = fbc * bs, fbr * bs
    hs, vs = min(bs, w - x0), min(bs, h - y0)
    win = np.full((bs + 6, bs + 16), LARGE, np.int64)
    xlo, xhi = x0 - (8 if fbc else 0), min(x0 + hs + (8 if fbc + 1 < nhfb else 0), w)  # taps reach 2 samples: what lies past the picture is never used
    ylo, yhi = y0 - (3 if fbr else 0), min(y0 + vs + (3 if fbr + 1 < nvfb else 0), h)
    win[ylo - (y0 - 3):yhi - (y0 - 3), xlo - (x0 - 8):xhi - (x0 - 8)] = plane[ylo:yhi, xlo:xhi]
    return win, hs, vs


def find_dir(img, cs):
    """svt_aom_cdef_find_dir_c on an 8x8 block: (dir, var)"""
    cost = [0] * 8
    partial = [[0] * 15 for _ in range(8)]
    for i in range(8):
        for j in range(8):
            x = (int(img[i, j]) >> cs) - 128
            for d in range(8):
                partial[d][line_of(d, i, j)] += x
    for i in range(8):
        cost[2] += partial[2][i] ** 2
        cost[6] += partial[6][i] ** 2
    cost[2] *= DIV_TABLE[8]
    cost[6] *= DIV_TABLE[8]
    for i in range(7):
        cost[0] += (partial[0][i] ** 2 + partial[0][14 - i] ** 2) * DIV_TABLE[i + 1]
        cost[4] += (partial[4][i] ** 2 + partial[4][14 - i] ** 2) * DIV_TABLE[i + 1]
    cost[0] += partial[0][7] ** 2 * DIV_TABLE[8]
    cost[4] += partial[4][7] ** 2 * DIV_TABLE[8]
    for i in range(1, 8, 2):
        for j in range(5):
            cost[i] += partial[i][3 + j] ** 2
        cost[i] *= DIV_TABLE[8]
        for j in range(3):
            cost[i] += (partial[i][j] ** 2 + partial[i][10 - j] ** 2) * DIV_TABLE[2 * j + 2]
    best_cost, best_dir = 0, 0
    for i in range(8):
        if cost[i] > best_cost:
            best_cost, best_dir = cost[i], i
    return best_dir, (best_cost - cost[(best_dir + 4) & 7]) >> 10


def adjust_strength(strength, var):
    i = min((var >> 6).bit_length() - 1, 12) if (var >> 6) else 0
    return (strength * (4 + i) + 8) >> 4 if var else 0


def constrain(diff, thr, damping):
    shift = np.where(thr > 0, np.maximum(0, damping - MSB[thr]), 0)
    a = np.abs(diff)
    m = np.minimum(a, np.maximum(0, thr - (a >> shift)))
    return np.where(thr > 0, np.sign(diff) * m, 0)


def filter_samples(win, rr, cc, d, pri, sec, damping, cs, seen=None, edges=None):
    """svt_cdef_filter_block_c on the samples win[rr, cc] (arrays of one shape): d the direction and pri the (adjusted) primary strength per sample, sec
    the secondary.  edges = (rows, cols) of the filter block inside the window, for the record of where a CDEF_VERY_LARGE tap lay."""
    x = win[rr, cc]
    pri = np.broadcast_to(pri, x.shape)
    sel = (pri >> cs) & 1
    taps_p = [np.where(sel == 1, 3, 4), np.where(sel == 1, 3, 2)]
    total, mn, mx = np.zeros_like(x), x.copy(), x.copy()
    for k in range(2):
        for sgn in (1, -1):
            for which, dd in (("pri", d), ("sec", (d + 2) & 7), ("sec", (d - 2) & 7)):
                r2, c2 = rr + sgn * DIRS[dd, k, 0], cc + sgn * DIRS[dd, k, 1]
                p = win[r2, c2]
                thr = pri if which == "pri" else np.broadcast_to(sec, x.shape)
                total = total + (taps_p[k] if which == "pri" else (2, 1)[k]) * constrain(p - x, thr, damping)
                mx = np.where(p != LARGE, np.maximum(mx, p), mx)
                mn = np.minimum(mn, p)
                if seen is not None and edges is not None:
                    big = (p == LARGE) & (thr > 0)
                    for side, hit in (("top", r2 < 3), ("bottom", r2 >= 3 + edges[0]), ("left", c2 < 8), ("right", c2 >= 8 + edges[1])):
                        if np.any(big & hit):
                            seen.add(f"large_{side}_{which}")
    y = x + ((8 + total - (total < 0)) >> 4)
    if seen is not None:
        if np.any(y < mn):
            seen.add("clamp_min")
        if np.any(y > mx):
            seen.add("clamp_max")
    return np.where(y < mn, mn, np.where(y > mx, mx, y))


def sec_of(v):
    s = v % 4
    return s + (s == 3)


def luma_dist(s, y, cs):
    """dist_8xn over [blocks][rows][8] arrays: uint64 per block"""
    s, y = s.astype(np.uint64), y.astype(np.uint64)
    ax = (1, 2)
    sum_s, sum_d, sum_s2, sum_d2, sum_sd = s.sum(ax), y.sum(ax), (s * s).sum(ax), (y * y).sum(ax), (s * y).sum(ax)
    svar = sum_s2 - ((sum_s * sum_s + np.uint64(32)) >> np.uint64(6))
    dvar = sum_d2 - ((sum_d * sum_d + np.uint64(32)) >> np.uint64(6))
    num = (sum_d2 + sum_s2 - np.uint64(2) * sum_sd).astype(np.float64) * .5 * (svar + dvar + np.uint64(400 << 2 * cs)).astype(np.float64)
    den = np.sqrt(np.float64(20000 << 4 * cs) + svar.astype(np.float64) * dvar.astype(np.float64))
    return np.floor(.5 + num / den).astype(np.uint64)


def listed(mask, hs, vs):
    m = int(mask) & valid_mask(hs, vs)
    return [b for b in range(64) if (m >> b) & 1]


def block_coords(blocks, n, rows=None):
    """window coordinates of the samples of the n x n blocks `blocks` (indices by * 8 + bx): [blocks][rows][n] each"""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    by, bx = np.array([b >> 3 for b in blocks]), np.array([b & 7 for b in blocks])
    rr = 3 + n * by[:, None, None] + rows[None, :, None] + np.zeros((1, 1, n), np.int64)
    cc = 8 + n * bx[:, None, None] + np.zeros((1, len(rows), 1), np.int64) + np.arange(n)[None, None, :]
    return rr, cc


def directions(win, blocks, cs):
    out = [find_dir(win[3 + 8 * (b >> 3):11 + 8 * (b >> 3), 8 + 8 * (b & 7):16 + 8 * (b & 7)], cs) for b in blocks]
    return np.array([o[0] for o in out], np.int64), [o[1] for o in out]


# ---- the search ----
def restate_search(recon, src, bd, base_q_idx, sf, sy, suv, masks, seen=None):
    """cdef_seg_search over a picture.  Returns mse [2][n_fb][64] uint64, dir [n_fb][64] uint8, var [n_fb][64] int32, block_dist [n_fb][n][64] uint64; what
    the device does not write holds the byte FILL."""
    h, w = recon[0].shape
    cs, n = bd - 8, len(sy)
    nhfb, nvfb = (w + 63) // 64, (h + 63) // 64
    n_fb = nhfb * nvfb
    fill8 = int.from_bytes(bytes([FILL]) * 8, "little")
    mse = np.full((2, n_fb, 64), fill8, np.uint64)
    dirs = np.full((n_fb, 64), FILL, np.uint8)
    var = np.frombuffer(bytes([FILL]) * (n_fb * 64 * 4), "<i4").reshape(n_fb, 64).copy()
    block_dist = np.full((n_fb, n, 64), fill8, np.uint64)
    damping = 3 + (base_q_idx >> 6)
    for fb in range(n_fb):
        fbr, fbc = fb // nhfb, fb % nhfb
        win, hs, vs = window(recon[0].astype(np.int64), fbr, fbc, nvfb, nhfb, 64)
        blocks = listed(masks[fb], hs, vs)
        if not blocks:
            continue
        bd_dir, bd_var = directions(win, blocks, cs)
        dirs[fb, blocks], var[fb, blocks] = bd_dir, bd_var
        if seen is not None:
            seen.update(f"dir_{d}" for d in bd_dir)
            seen.update(["var0"] if 0 in bd_var else [])
            seen.update(["var_cap12"] if any((v >> 6).bit_length() - 1 >= 12 for v in bd_var) else [])
            seen.update([f"damping_{damping}", f"sf_{sf}"])
        # luma
        lsf = min(sf, 4)
        rows = np.arange(0, 8, lsf)
        rr, cc = block_coords(blocks, 8, rows)
        s = src[0].astype(np.int64)[fbr * 64 + rr - 3, fbc * 64 + cc - 8]
        for gi in range(n):
            pri, sec = (sy[gi] // 4) << cs, sec_of(sy[gi] % 4) << cs
            t = np.array([adjust_strength(pri, v) for v in bd_var], np.int64)
            d = bd_dir if pri else np.zeros_like(bd_dir)
            if seen is not None:
                seen.update(f"tapset_{(int(v) >> cs) & 1}" for v in t if v)
                seen.update(["t0_with_pri"] if pri and (t == 0).any() else [])
                seen.update(["sec_only_dir_nonzero"] if not pri and sec and (bd_dir != 0).any() else [])
            y = filter_samples(win, rr, cc, d[:, None, None], t[:, None, None], sec, damping + cs, cs, seen, (vs, hs))
            dist = luma_dist(s, y, cs)
            block_dist[fb, gi, blocks] = dist
            mse[0, fb, gi] = (int(dist.sum()) >> 2 * cs) * lsf  # svt_aom_compute_cdef_dist_c shifts the sum of every plane
        # chroma: 4x4 blocks, the subsampling capped at 1
        if seen is not None:
            seen.add(f"chroma_damping_{damping + cs - 1}")
        rr, cc = block_coords(blocks, 4)
        acc = np.zeros(n, np.uint64)
        for pli in (1, 2):
            cwin, chs, cvs = window(recon[pli].astype(np.int64), fbr, fbc, nvfb, nhfb, 32)
            s = src[pli].astype(np.int64)[fbr * 32 + rr - 3, fbc * 32 + cc - 8]
            for gi in range(n):
                if suv[gi] == -1:
                    if seen is not None:
                        seen.add("uv_minus1")
                    continue
                pri, sec = (suv[gi] // 4) << cs, sec_of(suv[gi] % 4) << cs
                d = bd_dir if pri else np.zeros_like(bd_dir)
                y = filter_samples(cwin, rr, cc, d[:, None, None], np.int64(pri), sec, damping + cs - 1, cs, seen, (cvs, chs))
                acc[gi] += np.uint64(int(((y - s) ** 2).sum()) >> 2 * cs)
        for gi in range(n):
            mse[1, fb, gi] = DEFAULT_MSE_UV if suv[gi] == -1 else acc[gi]
    return {"mse": mse, "dir": dirs, "var": var, "block_dist": block_dist}


# ---- the pick ----
def rdcost(lam, rate, dist):
    return ((rate * lam + 256) >> 9) + dist * 128


def biased(v, bias, hbd, seen=None):
    f = bias
    if hbd:
        branch = "lt5000" if v < 5000 else "lt10000" if v < 10000 else "gt25000" if v > 25000 else "mid"
        f = {"lt5000": min(f - 10, 64), "lt10000": min(f - 5, 64), "gt25000": min(f + 1, 64), "mid": f}[branch]
    else:
        branch = "gt25000" if v > 25000 else "gt10000" if v > 10000 else "low"
        f = {"gt25000": min(f + 2, 64), "gt10000": min(f + 1, 64), "low": f}[branch]
    if seen is not None:
        seen.add(f"bias_{'hbd' if hbd else 'lbd'}_{branch}")
    return (f * v) >> 6


def search_one_dual(lev0, lev1, nb, m0, m1, seen=None):
    """svt_search_one_dual_c over the non-skipped filter blocks m0, m1 [count][n] (object arrays of Python ints would be slow: uint64 suffices, the sums
    stay far below 2^63)"""
    best = np.full(len(m0), NONE, np.uint64)
    for gi in range(nb):
        best = np.minimum(best, m0[:, lev0[gi]] + m1[:, lev1[gi]])
    tot = np.minimum(best[:, None, None], m0[:, :, None] + m1[:, None, :]).sum(0, dtype=np.uint64)
    flat = tot.ravel()
    at = int(np.argmin(flat))  # the first minimum in (j, k) raster order
    if int(flat[at]) >= NONE:
        at = 0
    if seen is not None and int((flat == flat[at]).sum()) > 1:
        seen.add("tie_in_tot")
    lev0[nb], lev1[nb] = at // tot.shape[1], at % tot.shape[1]
    return min(int(flat[at]), NONE)


def restate_pick(mse, masks, n, is_hbd, bias, lam, map_y, map_uv, seen=None):
    """finish_cdef_search without the mode-info writes.  Returns the result fields, fb_strength [n_fb] int8 (FILL where skipped) and mse as biased."""
    mse = mse.copy()
    n_fb = len(masks)
    live = [i for i in range(n_fb) if int(masks[i])]
    if bias:
        for i in live:
            for r in (0, 1):
                mse[r, i, 0] = biased(int(mse[r, i, 0]), bias, is_hbd, seen)
    m0, m1 = mse[0][live][:, :n], mse[1][live][:, :n]
    zero_dist = sum(int(m0[i, 0]) + int(m1[i, 0]) for i in range(len(live)))
    zero_cost = rdcost(lam, 512 * 12, zero_dist << 4)
    best_cost, best_bits, best0, best1 = NONE, 0, [0] * 8, [0] * 8
    for i in range(4):
        nb = 1 << i
        lev0, lev1 = [0] * 9, [0] * 9
        tot = NONE
        for k in range(nb):
            tot = search_one_dual(lev0, lev1, k, m0, m1, seen)
        for _ in range(4 * nb):
            for j in range(nb - 1):
                lev0[j], lev1[j] = lev0[j + 1], lev1[j + 1]
            tot = search_one_dual(lev0, lev1, nb - 1, m0, m1, seen)
        cost = rdcost(lam, 512 * (len(live) * i + nb * 12), tot * 16) & ((1 << 64) - 1)
        if cost < best_cost:
            best_cost, best_bits, best0, best1 = cost, i, lev0[:nb] + [0] * (8 - nb), lev1[:nb] + [0] * (8 - nb)
    if seen is not None:
        seen.add(f"bits_{best_bits}")
    nb = 1 << best_bits
    fb_strength = np.full(n_fb, FILL, np.uint8).view(np.int8)
    for q, i in enumerate(live):
        cur = [int(m0[q, best0[g]]) + int(m1[q, best1[g]]) for g in range(nb)]
        fb_strength[i] = cur.index(min(cur))
        if seen is not None and cur.count(min(cur)) > 1:
            seen.add("tie_in_block")
    dev = 0 if zero_cost == 0 else ((1000 - (1000 * best_cost) // zero_cost) & ((1 << 64) - 1))
    dev = ((dev & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    return {"cdef_bits": best_bits, "nb_strengths": nb, "y_strength": [map_y[best0[g]] if g < nb else 0 for g in range(8)],
            "uv_strength": [map_uv[best1[g]] if g < nb else 0 for g in range(8)], "best_cost": best_cost, "zero_cost": zero_cost, "cdef_dist_dev": dev,
            "fb_strength": fb_strength, "mse": mse}


# ---- the filter ----
def restate_apply(planes, bd, cdef_damping, n_planes, masks, fb_strength, y_strength, uv_strength, seen=None):
    """svt_av1_cdef_frame, out of place: the n_planes filtered planes.  Every tap reads the unfiltered input."""
    h, w = planes[0].shape
    cs = bd - 8
    nhfb, nvfb = (w + 63) // 64, (h + 63) // 64
    out = [p.copy() for p in planes[:n_planes]]
    for fb in range(nhfb * nvfb):
        fbr, fbc = fb // nhfb, fb % nhfb
        win, hs, vs = window(planes[0].astype(np.int64), fbr, fbc, nvfb, nhfb, 64)
        blocks = listed(masks[fb], hs, vs)
        if not blocks:
            if seen is not None:
                seen.add("apply_mask_empty")
            continue
        idx = int(fb_strength[fb]) & 7
        vy, vuv = int(y_strength[idx]), int(uv_strength[idx])
        if vy == 0 and vuv == 0:
            if seen is not None:
                seen.add("apply_fb_all_zero")
            continue
        if seen is not None and len(blocks) < (hs // 8) * (vs // 8):
            seen.add("apply_unlisted_block")
        bd_dir, bd_var = directions(win, blocks, cs)
        for pli in range(n_planes):
            v = vuv if pli else vy
            pri, sec = (v // 4) << cs, sec_of(v % 4) << cs
            if not (pri or sec):
                if seen is not None:
                    seen.add(f"apply_plane_zero_{'chroma' if pli else 'luma'}")
                continue
            n, bs = (4, 32) if pli else (8, 64)
            pw = win if pli == 0 else window(planes[pli].astype(np.int64), fbr, fbc, nvfb, nhfb, 32)[0]
            rr, cc = block_coords(blocks, n)
            t = np.array([pri if pli else adjust_strength(pri, x) for x in bd_var], np.int64)
            d = bd_dir if pri else np.zeros_like(bd_dir)
            y = filter_samples(pw, rr, cc, d[:, None, None], t[:, None, None], sec, cdef_damping + cs - (pli != 0), cs)
            out[pli][fbr * bs + rr - 3, fbc * bs + cc - 8] = y
    return out


# ---- the cases ----
ALL64 = list(range(64))
# name: (width, height, bit depth, picture, seed, masks, base_q_idx, subsampling_factor, strength_y, the indices whose strength_uv is -1,
#        zero_fs_cost_bias, full_lambda)
# The chroma strength of an index is the luma strength, or -1: the reference's chroma list only switches an index off.  The strength lists repeat a
# value here and there: equal columns of mse are how a tie comes about.
SEARCH_CASES = {
    "noise_8x8_8": (8, 8, 8, "noise", 1, "full", 0, 1, [0, 1, 4, 9, 15, 63, 2, 3, 9], [1], 0, 300),
    "grating_64x64_8": (64, 64, 8, "grating", 2, "full", 70, 2, ALL64, [7, 14, 21, 28, 35, 42, 49, 56, 63], 60, 50),
    "grating_72x40_10": (72, 40, 10, "grating", 3, "checker", 130, 4, [0, 5, 17, 32, 47, 61, 3, 1], [3], 58, 5000),
    "steps_136x72_8": (136, 72, 8, "steps", 4, "full", 255, 1, [0, 4, 8, 13, 30, 63, 2, 7], [], 62, 20000),
    "noise_136x72_10": (136, 72, 10, "noise", 5, "mixed", 140, 2, [0, 6, 21, 40, 59, 1, 2, 3, 21], [4], 59, 100),
    "flat_72x40_8": (72, 40, 8, "flat", 6, "full", 30, 1, [0, 8, 25, 62, 3], [], 61, 1000),
    "steps_64x64_10": (64, 64, 10, "steps", 7, "one", 200, 4, [0, 12, 36, 63, 2, 1], [], 0, 4000),
    "grating_136x72_8": (136, 72, 8, "grating", 8, "random", 100, 1, [0, 3, 10, 22, 45, 63], [5], 60, 10),
    "flat_64x64_10": (64, 64, 10, "flat", 9, "checker", 0, 1, [0, 9, 20, 63, 2], [], 64, 700),
}
# Synthetic mse for the pick: `clusters` groups of filter blocks, each cheapest at a pair of its own.
# name: (n_fb, n_strengths, clusters, is_hbd, zero_fs_cost_bias, full_lambda, every `skip`-th block skipped (0: none), seed)
PICK_CASES = {
    "one_cluster": (24, 6, 1, 0, 0, 400, 0, 11),
    "two_clusters": (40, 8, 2, 1, 58, 30, 5, 12),
    "four_clusters": (48, 10, 4, 0, 62, 20, 0, 13),
    "eight_clusters": (96, 12, 8, 1, 60, 10, 7, 14),
    "eight_clusters_dear_bits": (96, 12, 8, 0, 10, 4000000, 0, 15),
    "ranges_hbd": (64, 5, 2, 1, 59, 200, 0, 16),
    "ranges_lbd": (64, 5, 2, 0, 59, 200, 3, 17),
    "all_skipped": (6, 4, 1, 0, 60, 100, 1, 18),
}
# Apply on its own, with strengths the pick would not give: name: (search case for the picture, n_planes, masks or None for the case's, y_strength,
# uv_strength, fb_strength rule)
APPLY_CASES = {
    "luma_only_plane": ("noise_136x72_10", 1, None, [13, 0, 63, 2], [0, 0, 0, 0]),
    "chroma_zero": ("grating_136x72_8", 3, None, [13, 0, 63, 2], [0, 0, 5, 0]),
    "luma_zero": ("steps_136x72_8", 3, "mixed", [0, 0, 0, 7], [9, 0, 62, 3]),
    "all_pairs_8x8": ("noise_8x8_8", 3, None, [63], [63]),
    "sec_only_72x40": ("grating_72x40_10", 3, "full", [2, 1, 3, 0], [3, 1, 0, 2]),
}
CONDITIONS = ([f"dir_{d}" for d in range(8)] + ["var0", "var_cap12", "tapset_0", "tapset_1", "t0_with_pri"] + [f"damping_{d}" for d in (3, 4, 5, 6)] +
              ["chroma_damping_2", "clamp_min", "clamp_max"] + [f"large_{s}_{k}" for s in ("top", "bottom", "left", "right") for k in ("pri", "sec")] +
              ["sec_only_dir_nonzero", "uv_minus1", "sf_1", "sf_2", "sf_4"] + [f"bits_{i}" for i in range(4)] +
              [f"bias_hbd_{b}" for b in ("lt5000", "lt10000", "mid", "gt25000")] + [f"bias_lbd_{b}" for b in ("low", "gt10000", "gt25000")] +
              ["tie_in_tot", "tie_in_block", "apply_mask_empty", "apply_fb_all_zero", "apply_plane_zero_luma", "apply_plane_zero_chroma", "apply_unlisted_block"])


@functools.lru_cache(maxsize=None)
def search_case(name):
    w, h, bd, kind, seed, mk, q, sf, sy, off, bias, lam = SEARCH_CASES[name]
    suv = [-1 if i in off else v for i, v in enumerate(sy)]
    recon, src = picture(kind, w, h, bd, seed)
    return {"w": w, "h": h, "bd": bd, "recon": recon, "src": src, "masks": masks_of(mk, w, h, seed), "base_q_idx": q, "sf": sf, "sy": list(sy), "suv": list(suv),
            "bias": bias, "lam": lam, "damping": 3 + (q >> 6)}


@functools.lru_cache(maxsize=None)
def restated_search(name):
    """(outputs, the conditions met)"""
    c, seen = search_case(name), set()
    return restate_search(c["recon"], c["src"], c["bd"], c["base_q_idx"], c["sf"], c["sy"], c["suv"], c["masks"], seen), frozenset(seen)


def chain_pick_args(name):
    """the pick behind the search of a case: its arguments but mse and masks"""
    c = search_case(name)
    return {"n": len(c["sy"]), "is_hbd": int(c["bd"] > 8), "bias": c["bias"], "lam": c["lam"], "map_y": c["sy"], "map_uv": c["sy"]}


@functools.lru_cache(maxsize=None)
def restated_chain(name):
    """search, pick on its mse, apply with the pick's strengths: (search outputs, pick outputs, filtered planes, conditions)"""
    c = search_case(name)
    s, seen = restated_search(name)
    seen = set(seen)
    a = chain_pick_args(name)
    mse = np.where(np.arange(64)[None, None, :] < a["n"], s["mse"], 0)  # the pick reads the first n entries alone
    p = restate_pick(mse.astype(np.uint64), searched_masks(name), a["n"], a["is_hbd"], a["bias"], a["lam"],
                     a["map_y"], a["map_uv"], seen)
    p["mse"] = np.where(np.arange(64)[None, None, :] < 1, p["mse"], s["mse"])  # entry 0 biased, the rest as the search left them
    out = restate_apply(c["recon"], c["bd"], c["damping"], 3, c["masks"], p["fb_strength"], p["y_strength"], p["uv_strength"], seen)
    return s, p, out, frozenset(seen)


def searched_masks(name):
    """the masks with what lies outside the picture taken off: a filter block the search skips, the pick must skip too"""
    c = search_case(name)
    nhfb = (c["w"] + 63) // 64
    out = []
    for fb, m in enumerate(c["masks"]):
        hs, vs = min(64, c["w"] - 64 * (fb % nhfb)), min(64, c["h"] - 64 * (fb // nhfb))
        out.append(int(m) & valid_mask(hs, vs))
    return np.array(out, np.uint64)


@functools.lru_cache(maxsize=None)
def pick_case(name):
    n_fb, n, clusters, is_hbd, bias, lam, skip, seed = PICK_CASES[name]
    rng = np.random.default_rng(seed)
    mse = rng.integers(30000, 90000, (2, n_fb, 64)).astype(np.uint64)
    for i in range(n_fb):
        c = i % clusters
        mse[0, i, (c + 1) % n] = rng.integers(200, 900)
        mse[1, i, (2 * c + 1) % n] = rng.integers(200, 900)
    if name.startswith("ranges"):  # entry 0 through every range of the bias rules, and two equal columns for a tie
        mse[:, :, 0] = rng.choice([100, 4999, 5000, 9999, 10000, 10001, 25000, 25001, 400000], (2, n_fb))
        mse[:, :, 4] = mse[:, :, 3]
    masks = np.array([0 if skip and i % skip == 0 else (1 << (i % 64)) for i in range(n_fb)], np.uint64)
    maps = [(7 * g + 3) % 64 for g in range(n)]
    return {"w": 64 * n_fb, "h": 64, "mse": mse, "masks": masks, "n": n, "is_hbd": is_hbd, "bias": bias, "lam": lam, "map_y": maps, "map_uv": [(5 * g) % 64 for g in range(n)]}


@functools.lru_cache(maxsize=None)
def restated_pick(name):
    c, seen = pick_case(name), set()
    return restate_pick(c["mse"], c["masks"], c["n"], c["is_hbd"], c["bias"], c["lam"], c["map_y"], c["map_uv"], seen), frozenset(seen)


@functools.lru_cache(maxsize=None)
def apply_case(name):
    base, n_planes, mk, ys, uvs = APPLY_CASES[name]
    c = search_case(base)
    masks = c["masks"] if mk is None else masks_of(mk, c["w"], c["h"], 77)
    fbs = np.array([(3 * fb + 1) % len(ys) for fb in range(len(masks))], np.int8)
    return {"planes": c["recon"], "bd": c["bd"], "damping": c["damping"], "n_planes": n_planes, "masks": masks, "fb_strength": fbs, "y_strength": ys, "uv_strength": uvs,
            "w": c["w"], "h": c["h"]}


@functools.lru_cache(maxsize=None)
def restated_apply(name):
    c, seen = apply_case(name), set()
    return restate_apply(c["planes"], c["bd"], c["damping"], c["n_planes"], c["masks"], c["fb_strength"], c["y_strength"], c["uv_strength"], seen), frozenset(seen)


def pick_record(p, costs=True):
    """the pick's result as the comparisons hold it: int64 [22] = bits, count, y[8], uv[8], best_cost, zero_cost, dist_dev, 0.  The two costs are
    locals of the reference: the fixture has 0 in their place (costs=False)."""
    wrap = lambda v: v - (1 << 64) if v >= NONE else v
    return np.array([p["cdef_bits"], p["nb_strengths"]] + list(p["y_strength"]) + list(p["uv_strength"]) +
                    ([wrap(p["best_cost"]), wrap(p["zero_cost"])] if costs else [0, 0]) + [p["cdef_dist_dev"], 0], np.int64)


def fixture_arrays(search=None, pick=None, apply=None):
    """{fixture key: array} of what the reference computes itself: per search case the search's mse, dir and var, the pick behind it and the filtered
    planes; per pick case the result, the indices and the biased mse; per apply case the planes.  Each argument maps a case name to outputs laid out as
    the restatements'; None: the restatements themselves."""
    out = {}
    for name in SEARCH_CASES:
        s, p, planes, _ = restated_chain(name) if search is None else search[name]
        n = len(SEARCH_CASES[name][8])
        out[f"search_{name}_mse"], out[f"search_{name}_dir"], out[f"search_{name}_var"] = s["mse"][:, :, :n].copy(), s["dir"], s["var"]
        out[f"chain_{name}_pick"], out[f"chain_{name}_fb_strength"] = pick_record(p, False), p["fb_strength"]
        out[f"chain_{name}_mse0"] = p["mse"][:, :, 0].copy()
        for i, pl in enumerate(planes):
            out[f"chain_{name}_plane{i}"] = pl
    for name in PICK_CASES:
        p = restated_pick(name)[0] if pick is None else pick[name]
        out[f"pick_{name}_result"], out[f"pick_{name}_fb_strength"], out[f"pick_{name}_mse0"] = pick_record(p, False), p["fb_strength"], p["mse"][:, :, 0].copy()
    for name in APPLY_CASES:
        planes = restated_apply(name)[0] if apply is None else apply[name]
        for i, pl in enumerate(planes):
            out[f"apply_{name}_plane{i}"] = pl
    return out


def conditions_met(search=None, picks=None, applies=None):
    seen = set()
    for name in SEARCH_CASES if search is None else search:
        seen |= restated_chain(name)[3]
    for name in PICK_CASES if picks is None else picks:
        seen |= restated_pick(name)[1]
    for name in APPLY_CASES if applies is None else applies:
        seen |= restated_apply(name)[1]
    return seen


def coverage_missing(search=None, picks=None, applies=None):
    """the conditions of CONDITIONS that no case of the lists meets (None: the whole list), and the shapes and formats the issue names"""
    seen = conditions_met(search, picks, applies)
    missing = [c for c in CONDITIONS if c not in seen]
    if search is None:
        s = list(SEARCH_CASES.values())
        if not {(8, 8), (64, 64), (72, 40), (136, 72)} <= {(v[0], v[1]) for v in s}:
            missing.append("sizes")
        if {v[2] for v in s} != {8, 10} or not {"noise", "grating", "flat", "steps"} <= {v[3] for v in s}:
            missing.append("formats")
        if not {"full", "one", "checker", "mixed"} <= {v[5] for v in s}:
            missing.append("masks")
    return missing
