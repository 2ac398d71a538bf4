"""The intra prediction of the reference encoder restated in numpy, and the deterministic cases of its tests.

restate_job restates one call of build_intra_predictors / build_intra_predictors_high (Source/Lib/Codec/enc_intra_prediction.c:60-436) with
everything they call: the needed edges, the early constant fill, the edge extension, the corner, filter_intra_edge_corner,
svt_av1_filter_intra_edge with svt_aom_intra_edge_filter_strength, svt_av1_upsample_intra_edge with svt_aom_use_intra_edge_upsample, the three
directional zones, the DC / V / H / SMOOTH* / PAETH predictors (Codec/intra_prediction.c) and the filter-intra predictor
(C_DEFAULT/filterintra_c.c).  It returns the block and a record of what happened (zone, upsampling, strengths, fills, replication ...), from
which the coverage conditions are computed.  tools/gen_intra_pred_golden.py compares it with the reference's own functions on every job of
every batch below and writes golden/intra_pred.npz; the tests compare it with that fixture and the device with both."""
import functools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra_pred.npz")

TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]  # tx_size_wide
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]  # tx_size_high
N_TX = 19
DC_PRED, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED, D203_PRED, D67_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED = range(13)
NON_DIRECTIONAL = [DC_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED]
DIRECTIONAL = list(range(V_PRED, D67_PRED + 1))
MODE_TO_ANGLE = [0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0]
NO_FI = 5  # FILTER_INTRA_MODES
ST_OK, ST_UNDEFINED = 0, 0xFF
JOB_DTYPE = [("dst_offset", "<u4"), ("nbr_x", "<i4"), ("nbr_y", "<i4"), ("tx_size", "u1"), ("mode", "u1"), ("angle_delta", "i1"),
             ("filter_intra_mode", "u1"), ("n_top_px", "u1"), ("n_topright_px", "u1"), ("n_left_px", "u1"), ("n_bottomleft_px", "u1"),
             ("filt_type", "u1"), ("reserved", "u1", (3,))]
NBR_W, NBR_H = 208, 144  # the noise picture: a 64x64 block with 64 more samples to the right and below, and its edges, fits

SM_WEIGHTS = np.array([
    0, 0, 255, 128, 255, 149, 85, 64, 255, 197, 146, 105, 73, 50, 37, 32,
    255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16,
    255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8,
    255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
    65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4], np.int64)
DERIV = {3: 1023, 6: 547, 9: 372, 14: 273, 17: 215, 20: 178, 23: 151, 26: 132, 29: 116, 32: 102, 36: 90, 39: 80, 42: 71, 45: 64, 48: 57, 51: 51, 54: 45,
         58: 40, 61: 35, 64: 31, 67: 27, 70: 23, 73: 19, 76: 15, 81: 11, 84: 7, 87: 3}  # eb_dr_intra_derivative's non-zero entries
FI_TAPS = np.array([
    [[-6, 10, 0, 0, 0, 12, 0], [-5, 2, 10, 0, 0, 9, 0], [-3, 1, 1, 10, 0, 7, 0], [-3, 1, 1, 2, 10, 5, 0],
     [-4, 6, 0, 0, 0, 2, 12], [-3, 2, 6, 0, 0, 2, 9], [-3, 2, 2, 6, 0, 2, 7], [-3, 1, 2, 2, 6, 3, 5]],
    [[-10, 16, 0, 0, 0, 10, 0], [-6, 0, 16, 0, 0, 6, 0], [-4, 0, 0, 16, 0, 4, 0], [-2, 0, 0, 0, 16, 2, 0],
     [-10, 16, 0, 0, 0, 0, 10], [-6, 0, 16, 0, 0, 0, 6], [-4, 0, 0, 16, 0, 0, 4], [-2, 0, 0, 0, 16, 0, 2]],
    [[-8, 8, 0, 0, 0, 16, 0], [-8, 0, 8, 0, 0, 16, 0], [-8, 0, 0, 8, 0, 16, 0], [-8, 0, 0, 0, 8, 16, 0],
     [-4, 4, 0, 0, 0, 0, 16], [-4, 0, 4, 0, 0, 0, 16], [-4, 0, 0, 4, 0, 0, 16], [-4, 0, 0, 0, 4, 0, 16]],
    [[-2, 8, 0, 0, 0, 10, 0], [-1, 3, 8, 0, 0, 6, 0], [-1, 2, 3, 8, 0, 4, 0], [0, 1, 2, 3, 8, 2, 0],
     [-1, 4, 0, 0, 0, 3, 10], [-1, 3, 4, 0, 0, 4, 6], [-1, 2, 3, 4, 0, 4, 4], [-1, 2, 2, 3, 4, 3, 3]],
    [[-12, 14, 0, 0, 0, 14, 0], [-10, 0, 14, 0, 0, 12, 0], [-9, 0, 0, 14, 0, 11, 0], [-8, 0, 0, 0, 14, 10, 0],
     [-10, 12, 0, 0, 0, 0, 14], [-9, 1, 12, 0, 0, 0, 12], [-8, 0, 0, 12, 0, 1, 11], [-7, 0, 0, 1, 12, 1, 9]]], np.int64)  # eb_av1_filter_intra_taps[mode][k][0..6]
EDGE_KERNEL = np.array([[0, 4, 8, 4, 0], [0, 5, 6, 5, 0], [2, 4, 4, 4, 2]], np.int64)
OFF = 16  # of index 0 in an edge array


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def edge_filter_strength(bs0, bs1, delta, typ):  # svt_aom_intra_edge_filter_strength
    d, wh, s = abs(delta), bs0 + bs1, 0
    if typ == 0:
        if wh <= 8:
            s = 1 if d >= 56 else 0
        elif wh <= 16:
            s = 1 if d >= 40 else 0
        elif wh <= 24:
            s = 3 if d >= 32 else 2 if d >= 16 else 1 if d >= 8 else 0
        elif wh <= 32:
            s = 3 if d >= 32 else 2 if d >= 4 else 1 if d >= 1 else 0
        else:
            s = 3 if d >= 1 else 0
    else:
        if wh <= 8:
            s = 2 if d >= 64 else 1 if d >= 40 else 0
        elif wh <= 16:
            s = 2 if d >= 48 else 1 if d >= 20 else 0
        elif wh <= 24:
            s = 3 if d >= 4 else 0
        else:
            s = 3 if d >= 1 else 0
    return s


def use_upsample(bs0, bs1, delta, typ):  # svt_aom_use_intra_edge_upsample
    d = abs(delta)
    if d <= 0 or d >= 40:
        return 0
    return int(bs0 + bs1 <= 8) if typ else int(bs0 + bs1 <= 16)


def filter_edge(P, start, n, strength):  # svt_av1_filter_intra_edge on p = P[start:]
    if not strength:
        return
    e = P[start:start + n].copy()
    idx = np.clip(np.arange(1, n)[:, None] - 2 + np.arange(5)[None, :], 0, n - 1)
    P[start + 1:start + n] = ((e[idx] * EDGE_KERNEL[strength - 1]).sum(axis=1) + 8) >> 4


def upsample_edge(P, off, n, px_max):  # svt_av1_upsample_intra_edge on p = P[off:]
    inn = np.concatenate(([P[off - 1], P[off - 1]], P[off:off + n], [P[off + n - 1]]))
    i = np.arange(n)
    s = np.clip((-inn[i] + 9 * inn[i + 1] + 9 * inn[i + 2] - inn[i + 3] + 8) >> 4, 0, px_max)
    P[off - 2] = inn[0]
    P[off + 2 * i - 1] = s
    P[off + 2 * i] = inn[i + 2]


def needs(mode, angle_delta, fim):
    """(need_above, need_left, need_above_left, need_right, need_bottom, p_angle) as build_intra_predictors derives them"""
    na, nl, nal, nr, nb, p_angle = True, True, mode == PAETH_PRED, False, False, 0
    if V_PRED <= mode <= D67_PRED:
        p_angle = MODE_TO_ANGLE[mode] + 3 * angle_delta
        na, nl, nal, nr, nb = p_angle < 180, p_angle > 90, True, p_angle < 90, p_angle > 180
    if fim != NO_FI:
        na = nl = nal = True
        nr = nb = False
    return na, nl, nal, nr, nb, p_angle


def job_reads(j):
    """what the reference reads of the neighbour plane: (samples of the row above from nbr_x on, samples of the left column from nbr_y on, corner)"""
    na, nl_, nal, nr, nb, _ = needs(int(j["mode"]), int(j["angle_delta"]), int(j["filter_intra_mode"]))
    nt, ntr, nl, nbl = int(j["n_top_px"]), int(j["n_topright_px"]), int(j["n_left_px"]), int(j["n_bottomleft_px"])
    if (not na and nl == 0) or (not nl_ and nt == 0):  # the early constant fill
        return (1 if nl_ and nt > 0 else 0), (1 if not nl_ and nl > 0 else 0), False
    a = nt + (ntr if nr else 0) if na and nt > 0 else 0
    l = nl + (nbl if nb else 0) if nl_ and nl > 0 else 0
    return a, l, bool(nal and nt > 0 and nl > 0)


def reads_inside(j, width, height):
    a, l, corner = job_reads(j)
    x0, y0 = int(j["nbr_x"]), int(j["nbr_y"])
    ok = True
    if a:
        ok = ok and 1 <= y0 <= height and x0 >= 0 and x0 + a <= width
    if l:
        ok = ok and 1 <= x0 <= width and y0 >= 0 and y0 + l <= height
    if corner:
        ok = ok and 1 <= x0 <= width and 1 <= y0 <= height
    return ok


def job_defined(j, width, height, dst_samples, dst_stride):
    """the entry's own rules: False for a job that gets status 0xFF"""
    tx, mode, fim = int(j["tx_size"]), int(j["mode"]), int(j["filter_intra_mode"])
    if tx > 18 or mode > 12 or fim > NO_FI:
        return False
    w, h = TX_W[tx], TX_H[tx]
    if V_PRED <= mode <= D67_PRED and abs(int(j["angle_delta"])) > 3:
        return False
    if fim != NO_FI and (w > 32 or h > 32 or mode != DC_PRED):
        return False
    nt, ntr, nl, nbl = int(j["n_top_px"]), int(j["n_topright_px"]), int(j["n_left_px"]), int(j["n_bottomleft_px"])
    if nt > w or ntr > w or (ntr > 0 and nt != w) or nl > h or nbl > h or (nbl > 0 and nl != h):
        return False
    if not reads_inside(j, width, height):
        return False
    return int(j["dst_offset"]) + (h - 1) * dst_stride + w <= dst_samples


def filter_intra_block(above, left, corner, w, h, fim, px_max, by_diagonals=False):
    """svt_av1_filter_intra_predictor_c.  by_diagonals: every sub-block of an anti-diagonal R + C is computed from the buffer as it was before
    the diagonal began -- equal to the serial order exactly when those sub-blocks are independent.  Returns (block, clipped low, clipped high)"""
    buf = np.zeros((h + 1, w + 1), np.int64)
    buf[0, 0], buf[0, 1:], buf[1:, 0] = corner, above[:w], left[:h]
    n_r, n_c = h // 2, w // 4
    lo = hi = False

    def sub_block(src, R, C):
        r, c = 1 + 2 * R, 1 + 4 * C
        p = np.array([src[r - 1, c - 1], src[r - 1, c], src[r - 1, c + 1], src[r - 1, c + 2], src[r - 1, c + 3], src[r, c - 1], src[r + 1, c - 1]], np.int64)
        s = FI_TAPS[fim] @ p
        v = np.where(s < 0, -((-s + 8) >> 4), (s + 8) >> 4)  # ROUND_POWER_OF_TWO_SIGNED(s, 4)
        return r, c, v

    if by_diagonals:
        order = [[(d - C, C) for C in range(max(0, d - (n_r - 1)), min(n_c - 1, d) + 1)] for d in range(n_r + n_c - 1)]
    else:
        order = [[(R, C)] for R in range(n_r) for C in range(n_c)]
    for group in order:
        snap = buf.copy()
        for R, C in group:
            r, c, v = sub_block(snap, R, C)
            lo, hi = lo or bool((v < 0).any()), hi or bool((v > px_max).any())
            buf[r:r + 2, c:c + 4] = np.clip(v, 0, px_max).reshape(2, 4)
    return buf[1:, 1:], lo, hi


def restate_job(nbr, bd, disable_edge_filter, j):
    """(block [h][w] uint16, events) of one job on the neighbour plane `nbr`; reads only what job_reads names"""
    tx, mode, delta, fim = int(j["tx_size"]), int(j["mode"]), int(j["angle_delta"]), int(j["filter_intra_mode"])
    w, h = TX_W[tx], TX_H[tx]
    nt, ntr, nl, nbl = int(j["n_top_px"]), int(j["n_topright_px"]), int(j["n_left_px"]), int(j["n_bottomleft_px"])
    x0, y0 = int(j["nbr_x"]), int(j["nbr_y"])
    base, px_max = 128 << (bd - 8), (1 << bd) - 1
    need_above, need_left, need_al, need_right, need_bottom, p_angle = needs(mode, delta, fim)
    is_dr, use_fi = V_PRED <= mode <= D67_PRED, fim != NO_FI
    a_n, l_n, corner = job_reads(j)
    ev = {"tx": tx, "mode": mode, "fi": use_fi, "inside": reads_inside(j, nbr.shape[1], nbr.shape[0]), "early": None, "zone": 0, "rep": set(), "rep_over": set()}
    assert ev["inside"], "a read outside the neighbour plane"
    above_ref = nbr[y0 - 1, x0:x0 + a_n].astype(np.int64) if a_n else None
    left_ref = nbr[y0:y0 + l_n, x0 - 1].astype(np.int64) if l_n else None

    if (not need_above and nl == 0) or (not need_left and nt == 0):
        if need_left:
            val, ev["early"] = (int(above_ref[0]), "above") if nt > 0 else (base + 1, "base+1")
        else:
            val, ev["early"] = (int(left_ref[0]), "left") if nl > 0 else (base - 1, "base-1")
        return np.full((h, w), val, np.uint16), ev

    A, L = np.zeros(OFF + 128 + 16, np.int64), np.zeros(OFF + 128 + 16, np.int64)
    if need_left:
        n = h + (w if need_bottom else 0)
        if nl > 0:
            i = l_n
            L[OFF:OFF + i] = left_ref
            if i < n:
                L[OFF + i:OFF + n] = L[OFF + i - 1]
                ev["rep"].add("left" if nl < h else "bottomleft")
                if nl == h and need_bottom and nbl == h:
                    ev["rep_over"].add(("bottomleft", tx))
        else:
            L[OFF:OFF + n] = int(above_ref[0]) if nt > 0 else base + 1
    if need_above:
        n = w + (h if need_right else 0)
        if nt > 0:
            i = a_n
            A[OFF:OFF + i] = above_ref
            if i < n:
                A[OFF + i:OFF + n] = A[OFF + i - 1]
                ev["rep"].add("top" if nt < w else "topright")
                if nt == w and need_right and ntr == w:
                    ev["rep_over"].add(("topright", tx))
        else:
            A[OFF:OFF + n] = int(left_ref[0]) if nl > 0 else base - 1
    if need_al:
        if nt > 0 and nl > 0:
            cv = int(nbr[y0 - 1, x0 - 1])
        elif nt > 0:
            cv = int(above_ref[0])
        elif nl > 0:
            cv = int(left_ref[0])
        else:
            cv = base
        A[OFF - 1] = L[OFF - 1] = cv

    if use_fi:
        blk, lo, hi = filter_intra_block(A[OFF:], L[OFF:], A[OFF - 1], w, h, fim, px_max)
        ev["fi_clip"] = (lo, hi)
        return blk.astype(np.uint16), ev

    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    if is_dr:
        upa = upl = 0
        if not disable_edge_filter:
            ft = int(j["filt_type"] != 0)
            if p_angle != 90 and p_angle != 180:
                ev["corner_filter"] = bool(need_above and need_left and w + h >= 24)
                if ev["corner_filter"]:
                    A[OFF - 1] = L[OFF - 1] = (5 * L[OFF] + 6 * A[OFF - 1] + 5 * A[OFF] + 8) >> 4
                if need_above and nt > 0:
                    s = edge_filter_strength(w, h, p_angle - 90, ft)
                    ev.setdefault("strength", []).append((ft, s))
                    filter_edge(A, OFF - 1, nt + 1 + (h if need_right else 0), s)
                if need_left and nl > 0:
                    s = edge_filter_strength(h, w, p_angle - 180, ft)
                    ev.setdefault("strength", []).append((ft, s))
                    filter_edge(L, OFF - 1, nl + 1 + (w if need_bottom else 0), s)
            upa = use_upsample(w, h, p_angle - 90, ft)
            if need_above and upa:
                upsample_edge(A, OFF, w + (h if need_right else 0), px_max)
            upl = use_upsample(h, w, p_angle - 180, ft)
            if need_left and upl:
                upsample_edge(L, OFF, h + (w if need_bottom else 0), px_max)
        interp = lambda P, b, sh: np.clip((P[OFF + b] * (32 - sh) + P[OFF + b + 1] * sh + 16) >> 5, 0, px_max)
        if p_angle == 90:
            out = np.broadcast_to(A[OFF:OFF + w][None, :], (h, w))
        elif p_angle == 180:
            out = np.broadcast_to(L[OFF:OFF + h][:, None], (h, w))
        elif p_angle < 90:  # svt_av1_dr_prediction_z1
            dx = DERIV[p_angle]
            x = (r + 1) * dx
            b, sh, maxb = (x >> (6 - upa)) + (c << upa), ((x << upa) & 0x3F) >> 1, (w + h - 1) << upa
            out = np.where(b < maxb, interp(A, np.minimum(b, maxb - 1), sh), A[OFF + maxb])
            ev.update(zone=1, up=(upa,), past=bool((b >= maxb).any()))
        elif p_angle > 180:  # svt_av1_dr_prediction_z3
            dy = DERIV[270 - p_angle]
            y = (c + 1) * dy
            b, sh, maxb = (y >> (6 - upl)) + (r << upl), ((y << upl) & 0x3F) >> 1, (w + h - 1) << upl
            out = np.where(b < maxb, interp(L, np.minimum(b, maxb - 1), sh), L[OFF + maxb])
            ev.update(zone=3, up=(upl,), past=bool((b >= maxb).any()))
        else:  # svt_av1_dr_prediction_z2
            dx, dy = DERIV[180 - p_angle], DERIV[p_angle - 90]
            x = (c << 6) - (r + 1) * dx
            y = (r << 6) - (c + 1) * dy
            bx, by = x >> (6 - upa), y >> (6 - upl)
            from_above = bx >= -(1 << upa)
            assert np.all(by[~from_above] >= -(1 << upl))
            va = interp(A, np.where(from_above, bx, 0), ((x * (1 << upa)) & 0x3F) >> 1)
            vl = interp(L, np.where(from_above, 0, by), ((y * (1 << upl)) & 0x3F) >> 1)
            out = np.where(from_above, va, vl)
            ev.update(zone=2, up=(upa, upl), both_in_a_row=bool((from_above.any(axis=1) & (~from_above).any(axis=1)).any()))
        return np.asarray(out).astype(np.uint16), ev

    if mode == DC_PRED:  # svt_aom_dc_pred[n_left_px > 0][n_top_px > 0]
        ev["dc"] = (nl > 0, nt > 0)
        if nl == 0 and nt == 0:
            val = base
        else:
            s = (int(A[OFF:OFF + w].sum()) if nt > 0 else 0) + (int(L[OFF:OFF + h].sum()) if nl > 0 else 0)
            count = (w if nt > 0 else 0) + (h if nl > 0 else 0)
            val = (s + (count >> 1)) // count
        return np.full((h, w), val, np.uint16), ev
    above, left = A[OFF:OFF + w][None, :], L[OFF:OFF + h][:, None]
    sw, sh_ = SM_WEIGHTS[w:2 * w][None, :], SM_WEIGHTS[h:2 * h][:, None]
    below, right = L[OFF + h - 1], A[OFF + w - 1]
    if mode == SMOOTH_PRED:
        out = (sh_ * above + (256 - sh_) * below + sw * left + (256 - sw) * right + 256) >> 9
    elif mode == SMOOTH_V_PRED:
        out = (sh_ * above + (256 - sh_) * below + 128 + 0 * left) >> 8
    elif mode == SMOOTH_H_PRED:
        out = (sw * left + (256 - sw) * right + 128 + 0 * above) >> 8
    else:  # paeth_predictor_single: left, then top, then top-left
        tl = A[OFF - 1]
        b = above + left - tl
        pl, pt, ptl = np.abs(b - left), np.abs(b - above), np.abs(b - tl)
        pick_l, pick_t = (pl <= pt) & (pl <= ptl), pt <= ptl
        out = np.where(pick_l, left, np.where(pick_t, above, tl))
        ev["paeth"] = (bool(pick_l.any()), bool((~pick_l & pick_t).any()), bool((~pick_l & ~pick_t).any()))
    return out.astype(np.uint16), ev


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype="<u2").tobytes())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane(kind, bd):
    """the neighbour planes: NBR_H x NBR_W, uint8 / uint16"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:NBR_H, 0:NBR_W]
    if kind == "noise":
        p = np.random.default_rng([77, bd]).integers(0, mx + 1, (NBR_H, NBR_W))
    elif kind == "zero":
        p = np.zeros((NBR_H, NBR_W))
    elif kind == "max":
        p = np.full((NBR_H, NBR_W), mx)
    elif kind == "checker":
        p = ((xx + yy) & 1) * mx
    elif kind == "ramp":  # one sample per step
        p = (xx + yy) % (mx + 1)
    else:
        raise KeyError(kind)
    out = p.astype(np.uint16 if bd > 8 else np.uint8)
    out.setflags(write=False)
    return out


def make_job(tx, mode, pos, counts, angle_delta=0, fim=NO_FI, filt_type=0):
    j = np.zeros((), JOB_DTYPE)
    j["tx_size"], j["mode"], j["angle_delta"], j["filter_intra_mode"], j["filt_type"] = tx, mode, angle_delta, fim, filt_type
    j["nbr_x"], j["nbr_y"] = pos
    j["n_top_px"], j["n_topright_px"], j["n_left_px"], j["n_bottomleft_px"] = counts
    return j


def pack(jobs, stride, x_of=None, gap=4):
    """dst_offset of every job: shelves of blocks, left to right, `gap` untouched samples between two blocks and one row between two shelves"""
    x = y = shelf = 0
    out = np.array(jobs, JOB_DTYPE)
    for i in range(len(out)):
        w, h = TX_W[out[i]["tx_size"]], TX_H[out[i]["tx_size"]]
        x = x_of(i, x) if x_of else x
        if x + w > stride:
            x, y, shelf = (x_of(i, 0) if x_of else 0), y + shelf + 1, 0
        out[i]["dst_offset"] = y * stride + x
        x, shelf = x + w + gap, max(shelf, h)
    return out, y + shelf


def finish(name, bd, kind, disable, jobs, stride=None, x_of=None):
    if stride is None:
        stride = max(544, 8 * (4 + max(TX_W[int(j["tx_size"])] for j in jobs)))
    jobs, rows = pack(jobs, stride, x_of)
    return {"name": name, "bit_depth": bd, "plane": kind, "disable_edge_filter": disable, "jobs": jobs, "dst_shape": (rows, stride), "dst_stride": stride}


def random_pos(rng):
    """a block position whose every possible read (128 samples to the right and below, the row above, the column on the left) is inside"""
    return int(rng.integers(1, NBR_W - 128 + 1)), int(rng.integers(1, NBR_H - 128 + 1))


def availability_set(w, h):
    """group 1's counts: n_top_px in {0, w/2 if >= 4, w}, n_left_px likewise, the top-right / bottom-left counts {0, half, all} beside a full edge"""
    tops = [(0, 0)] + ([(w // 2, 0)] if w // 2 >= 4 else []) + [(w, 0), (w, w // 2), (w, w)]
    lefts = [(0, 0)] + ([(h // 2, 0)] if h // 2 >= 4 else []) + [(h, 0), (h, h // 2), (h, h)]
    return [(t, tr, l, bl) for t, tr in tops for l, bl in lefts]


def edge_missing_set(w, h):
    """group 2's counts: everything available, then each single edge missing"""
    return [(w, w, h, h), (0, 0, h, h), (w, 0, h, h), (w, w, 0, 0), (w, w, h, 0)]


def nondir_batch(bd):
    rng = np.random.default_rng([1, bd])
    jobs = [make_job(tx, mode, random_pos(rng), counts) for tx in range(N_TX) for mode in NON_DIRECTIONAL for counts in availability_set(TX_W[tx], TX_H[tx])]
    return finish(f"nondir_{bd}", bd, "noise", 0, jobs)


def dir_batch(tx, bd, disable):
    rng = np.random.default_rng([2, tx, bd, disable])
    jobs = [make_job(tx, mode, random_pos(rng), counts, delta, NO_FI, ft) for mode in DIRECTIONAL for delta in range(-3, 4) for ft in (0, 1)
            for counts in edge_missing_set(TX_W[tx], TX_H[tx])]
    return finish(f"dir_tx{tx}_{bd}_ef{1 - disable}", bd, "noise", disable, jobs)


FI_SIZES = [tx for tx in range(N_TX) if TX_W[tx] <= 32 and TX_H[tx] <= 32]


def fi_batch(bd):
    rng = np.random.default_rng([3, bd])
    jobs = []
    for fim in range(5):
        for tx in FI_SIZES:
            w, h = TX_W[tx], TX_H[tx]
            jobs += [make_job(tx, DC_PRED, random_pos(rng), counts, 0, fim) for counts in ((0, 0, 0, 0), (w, 0, 0, 0), (0, 0, h, 0), (w, 0, h, 0))]
    return finish(f"fi_{bd}", bd, "noise", 0, jobs)


EXTREME_KINDS = ["zero", "max", "checker", "ramp"]
EXTREME_SIZES = [0, 1, 2, 3, 4, 13, 14, 17, 18]  # 4x4 .. 64x64 and the 1:4 shapes


def extreme_batch(bd, kind):
    rng = np.random.default_rng([4, bd, EXTREME_KINDS.index(kind)])
    jobs = []
    for tx in EXTREME_SIZES:
        w, h = TX_W[tx], TX_H[tx]
        full = (w, w, h, h)
        jobs += [make_job(tx, mode, random_pos(rng), full) for mode in NON_DIRECTIONAL]
        jobs += [make_job(tx, mode, random_pos(rng), full, delta, NO_FI, ft) for mode in DIRECTIONAL for delta, ft in ((-3, 0), (0, 1), (2, 0), (3, 1))]
        if tx in FI_SIZES:
            jobs += [make_job(tx, DC_PRED, random_pos(rng), (w, 0, h, 0), 0, fim) for fim in range(5)]
    return finish(f"extreme_{kind}_{bd}", bd, kind, 0, jobs)


def geometry_batch(bd, stride):
    """blocks at the four corners of the neighbour plane (the counts of the sides that do not exist are 0), odd nbr_x, and destination offsets at
    every multiple of 4 within 16 on a pitch that is (204) or is not (203) a multiple of 4"""
    rng = np.random.default_rng([5, bd, stride])
    jobs = []
    families = [(DC_PRED, 0, NO_FI), (SMOOTH_PRED, 0, NO_FI), (PAETH_PRED, 0, NO_FI), (V_PRED, 0, NO_FI), (H_PRED, 0, NO_FI), (D45_PRED, -1, NO_FI),
                (D135_PRED, 2, NO_FI), (D113_PRED, -3, NO_FI), (D203_PRED, 1, NO_FI), (D67_PRED, 3, NO_FI), (DC_PRED, 0, 1), (DC_PRED, 0, 4)]
    for tx in (0, 1, 2, 3, 13, 14, 4):
        w, h = TX_W[tx], TX_H[tx]
        for mode, delta, fim in families:
            if fim != NO_FI and tx not in FI_SIZES:
                continue
            for cx, cy in ((0, 0), (NBR_W - w, 0), (0, NBR_H - h), (NBR_W - w, NBR_H - h)):
                t, l = (w if cy else 0), (h if cx else 0)
                jobs.append(make_job(tx, mode, (cx, cy), (t, 0, l, 0), delta, fim, (cx + cy) & 1))
            x, y = random_pos(rng)
            jobs.append(make_job(tx, mode, ((x - 1) | 1, y), (w, w, h, h), delta, fim, tx & 1))
    x_of = lambda i, x: x + ((4 * (i % 4)) - x) % 16  # the next x at or after x with x % 16 == 4 * (i % 4)
    return finish(f"geometry_{bd}_stride{stride}", bd, "noise", 0, jobs, stride, x_of)


@functools.lru_cache(maxsize=None)
def batch_names():
    names = []
    for bd in (8, 10):
        names.append(f"nondir_{bd}")
        names += [f"dir_tx{tx}_{bd}_ef{ef}" for tx in range(N_TX) for ef in (1, 0)]
        names.append(f"fi_{bd}")
        names += [f"extreme_{kind}_{bd}" for kind in EXTREME_KINDS]
        names += [f"geometry_{bd}_stride{s}" for s in (204, 203)]
    return tuple(names)


@functools.lru_cache(maxsize=None)
def batch(name):
    p = name.split("_")
    if p[0] == "nondir":
        return nondir_batch(int(p[1]))
    if p[0] == "dir":
        return dir_batch(int(p[1][2:]), int(p[2]), 1 - int(p[3][2:]))
    if p[0] == "fi":
        return fi_batch(int(p[1]))
    if p[0] == "extreme":
        return extreme_batch(int(p[2]), p[1])
    if p[0] == "geometry":
        return geometry_batch(int(p[1]), int(p[2][6:]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(blocks, events) of a batch, computed once and shared: do not change them"""
    b = batch(name)
    nbr = plane(b["plane"], b["bit_depth"])
    res = [restate_job(nbr, b["bit_depth"], b["disable_edge_filter"], j) for j in b["jobs"]]
    return [r[0] for r in res], [r[1] for r in res]


def batch_crcs(blocks):
    return np.array([crc(b) for b in blocks], np.uint32)


def sample_jobs():
    """(key, batch, job index): one full block per mode family x depth in the fixture"""
    out = []
    for bd in (8, 10):
        b = batch(f"nondir_{bd}")
        first = {}
        for i, j in enumerate(b["jobs"]):
            if int(j["tx_size"]) == 2 and int(j["n_top_px"]) == 16 and int(j["n_left_px"]) == 16:
                first.setdefault(int(j["mode"]), i)
        out += [(f"block_nondir_{bd}_mode{m}", b["name"], i) for m, i in sorted(first.items())]
        d = batch(f"dir_tx1_{bd}_ef1")
        first = {}
        for i, j in enumerate(d["jobs"]):
            if int(j["n_top_px"]) and int(j["n_left_px"]) and int(j["angle_delta"]) == -2:
                first.setdefault(int(j["mode"]), i)
        out += [(f"block_dir_{bd}_mode{m}", d["name"], i) for m, i in sorted(first.items())]
        f = batch(f"fi_{bd}")
        out += [(f"block_fi_{bd}_{int(j['filter_intra_mode'])}", f["name"], i) for i, j in enumerate(f["jobs"])
                if int(j["tx_size"]) == 1 and int(j["n_top_px"]) and int(j["n_left_px"]) and int(j["filter_intra_mode"]) in (0, 3)]
    return out


def block_of(b, img, j):
    y, x = divmod(int(j["dst_offset"]), b["dst_stride"])
    return img[y:y + TX_H[int(j["tx_size"])], x:x + TX_W[int(j["tx_size"])]].astype(np.uint16)


def expected_image(b, blocks, fill, defined=None):
    """the destination plane after the batch: `fill` bytes everywhere but in the blocks of the defined jobs"""
    dt = np.uint16 if b["bit_depth"] > 8 else np.uint8
    img = np.full(b["dst_shape"][0] * b["dst_stride"], fill * 0x0101 if b["bit_depth"] > 8 else fill, dt).reshape(b["dst_shape"][0], b["dst_stride"])
    for i, (j, blk) in enumerate(zip(b["jobs"], blocks)):
        if defined is None or defined[i]:
            y, x = divmod(int(j["dst_offset"]), b["dst_stride"])
            img[y:y + blk.shape[0], x:x + blk.shape[1]] = blk
    return img


def coverage_missing(records):
    """records: (bit_depth, job, events).  The coverage conditions the fixture must meet; returns the ones that are not met"""
    seen = set()
    for bd, j, e in records:
        if e["early"]:
            seen.add(("early", bd, e["early"]))
        for part in e["rep"]:
            seen.add(("rep", part))
        for part, tx in e["rep_over"]:
            seen.add(("rep_over", part, tx))
        if e["zone"]:
            for side, up in enumerate(e["up"]):
                seen.add(("zone", e["zone"], side, up))
            if e.get("past"):
                seen.add(("past", e["zone"]))
            if e.get("both_in_a_row"):
                seen.add(("z2_both",))
        for ft, s in e.get("strength", []):
            seen.add(("strength", ft, s))
        if "corner_filter" in e:
            seen.add(("corner_filter", e["corner_filter"]))
        if "dc" in e:
            seen.add(("dc",) + e["dc"])
        if "paeth" in e:
            seen |= {("paeth", k) for k in range(3) if e["paeth"][k]}
        if "fi_clip" in e:
            seen |= {("fi_clip", bd, k) for k in range(2) if e["fi_clip"][k]}
    want = [("early", bd, k) for bd in (8, 10) for k in ("above", "left", "base+1", "base-1")]
    want += [("rep", p) for p in ("top", "topright", "left", "bottomleft")]
    want += [("rep_over", "topright", 13), ("rep_over", "bottomleft", 14), ("rep_over", "topright", 17), ("rep_over", "bottomleft", 18)]
    want += [("zone", 1, 0, u) for u in (0, 1)] + [("zone", 3, 0, u) for u in (0, 1)] + [("zone", 2, s, u) for s in (0, 1) for u in (0, 1)]
    # zone 3's fill past max_base_y cannot occur: its steepest angle is 212 (D203 + 3), dy = 40 < 64, so base = ((c + 1) * dy >> 6) + r stays below
    # bw + bh - 1 for every sample (zone 1 reaches angle 36, dx = 90 > 64, and does fill)
    want += [("past", 1), ("z2_both",)]
    want += [("strength", ft, s) for ft in (0, 1) for s in range(4)]
    want += [("corner_filter", True), ("corner_filter", False)]
    want += [("dc", a, b) for a in (False, True) for b in (False, True)]
    want += [("paeth", k) for k in range(3)]
    want += [("fi_clip", bd, k) for bd in (8, 10) for k in range(2)]
    return [w for w in want if w not in seen]


def undefined_batch(bd):
    """ordinary 8x8 / 16x16 jobs with one of each kind of undefined job among them; returns (batch, indices of the undefined jobs)"""
    rng = np.random.default_rng([6, bd])
    good = lambda tx=1, mode=D135_PRED, counts=None, **kw: make_job(tx, mode, random_pos(rng), counts or (TX_W[tx], TX_W[tx], TX_H[tx], TX_H[tx]), **kw)
    spoiled = []

    def spoil(**fields):
        j = good(**{k: fields.pop(k) for k in list(fields) if k in ("tx", "mode", "counts", "angle_delta", "fim")})
        spoiled.append((j, fields))  # the fields are set after packing: the job keeps the place of the ordinary job it was

    spoil(tx_size=19)
    spoil(tx_size=255)
    spoil(mode=13)
    spoil(mode=D45_PRED, angle_delta=4)
    spoil(mode=D203_PRED, angle_delta=-4)
    spoil(filter_intra_mode=6)
    spoil(tx=4, mode=DC_PRED, fim=2)       # filter-intra on 64x64
    spoil(tx=11, mode=DC_PRED, fim=0)      # 32x64
    spoil(tx=1, mode=PAETH_PRED, fim=1)    # filter-intra with a mode other than DC
    spoil(counts=(9, 0, 8, 0))             # n_top_px > txw
    spoil(counts=(8, 9, 8, 0))             # n_topright_px > txw
    spoil(counts=(4, 4, 8, 0))             # top-right beside a partial top
    spoil(counts=(8, 0, 9, 0))
    spoil(counts=(8, 0, 8, 9))
    spoil(counts=(8, 0, 4, 4))
    spoil(mode=D45_PRED, nbr_x=NBR_W - 12)             # the top-right samples leave the plane on the right
    spoil(mode=D203_PRED, nbr_y=NBR_H - 12)            # the bottom-left samples leave it at the bottom
    spoil(mode=V_PRED, nbr_y=0)                        # the row above does not exist
    spoil(mode=H_PRED, nbr_x=0)                        # the column on the left does not exist
    spoil(mode=PAETH_PRED, nbr_x=-5)
    spoil(mode=SMOOTH_PRED, nbr_y=NBR_H + 1)
    spoil()                                            # its dst_offset is set below: the block ends past the destination
    n_good = 2 * len(spoiled) + 3
    jobs = [good(tx=1 + (i & 1), mode=(DC_PRED, D113_PRED, SMOOTH_H_PRED, PAETH_PRED, D67_PRED)[i % 5], angle_delta=(i % 7) - 3) for i in range(n_good)]
    bad = []
    for k, (j, _) in enumerate(spoiled):
        bad.append(3 * k + 1)
        jobs.insert(bad[-1], j)
    b = finish(f"undefined_{bd}", bd, "noise", 0, jobs, stride=300)
    for i, (_, fields) in zip(bad, spoiled):
        for k, v in fields.items():
            b["jobs"][i][k] = v
    b["jobs"][bad[-1]]["dst_offset"] = (b["dst_shape"][0] - 7) * b["dst_stride"] - 7  # an 8x8 block that ends one sample past the destination
    return b, bad


def spoil_desc(d, bad):
    """makes the descriptor one that svt_hip_intra_pred_check_desc refuses"""
    if bad == "no_nbr":
        d.nbr = None
    elif bad == "no_dst":
        d.dst = None
    elif bad == "no_jobs":
        d.jobs = None
    elif bad == "no_status":
        d.status = None
    elif bad.startswith("bit_depth_"):
        d.bit_depth = int(bad[10:])
    elif bad == "zero_stride":
        d.nbr_stride = 0
    elif bad == "stride_below_width":
        d.nbr_stride = d.nbr_width - 1
    elif bad == "zero_width":
        d.nbr_width = 0
    elif bad == "zero_height":
        d.nbr_height = 0
    elif bad == "zero_dst_stride":
        d.dst_stride = 0
    elif bad == "zero_dst_samples":
        d.dst_samples = 0
    elif bad == "dst_inside_nbr":
        d.dst = d.nbr + 64
    elif bad == "dst_ends_in_nbr":
        d.dst = d.nbr - 2 * d.dst_samples + 2
    elif bad == "nbr_ends_in_dst":
        d.dst = d.nbr + ((d.nbr_height - 1) * d.nbr_stride + d.nbr_width) * (2 if d.bit_depth > 8 else 1) - 1
    else:
        raise KeyError(bad)
    return d
