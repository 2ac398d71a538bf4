"""The cases of the inter prediction entry (svt_hip_inter_pred_batch) and a numpy restatement of what one job computes.

The reference's own results -- svt_aom_enc_make_inter_predictor called job by job by tools/gen_inter_pred_golden.py -- are in golden/inter_pred.npz
as numbers only: a CRC-32 of every predicted block (one CRC per size x filter pair x depth for the exhaustive sweep) and the full block of a sample
of jobs.  The planes and jobs are regenerated from seeds here.

Restated (Source/Lib): compute_subpel_params' unscaled branch and clamp_mv_to_umv_border_sb (Codec/enc_inter_prediction.c:3200-3211,30-50),
av1_get_convolve_filter_params (Codec/inter_prediction.h:137-153) with the six filter tables (Codec/inter_prediction.c:223-254,1065-1129), the
dispatch svt_aom_convolve[sx != 0][sy != 0][is_compound], svt_av1_convolve_{2d_copy,x,y,2d}_sr_c (:311-418), svt_av1_highbd_convolve_*_sr_c
(:670-777), svt_av1_jnt_convolve_*_c (:494-668), svt_av1_highbd_jnt_convolve_*_c (:852-1035) with get_conv_params_no_round's round_0 = 3 and
round_1 = 11 (single) / 7 (compound) (Codec/convolve.h:40-64).  Every InterpFilterParams has taps = 8, so fo_horiz = fo_vert = 3.

Geometry: the visible picture is 192x128 inside a padding of 160 (a 128x128 block at the clamp limit plus the filter reach stays inside the
plane); the sub-sampled planes are 96x64 inside a padding of 80.  A batch is one launch: one depth, one sub-sampling, up to 8 planes."""
import functools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_pred.npz")
PIC_W, PIC_H, PAD = 192, 128, 160
BLOCK_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128),
               (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]  # (width, height), BlockSize's order
DIST_PAIRS = [(9, 7), (11, 5), (12, 4), (13, 3), (7, 9), (5, 11), (4, 12), (3, 13)]  # quant_dist_lookup_table: (fwd_offset, bck_offset)
VARIANTS = ["copy", "x", "y", "2d"]  # index = (sx != 0) + 2 * (sy != 0)
MODES = ["single", "average", "dist_wtd"]
NO_REF = 0xFF
MV0_FROM_ARRAY, MV1_FROM_ARRAY = 1, 2
ST_OK, ST_UNDEFINED = 0, 0xFF
SWEEP_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (16, 16)]
JOB_DTYPE = [("dst_offset", "<u4"), ("org_x", "<i2"), ("org_y", "<i2"), ("width", "u1"), ("height", "u1"), ("filter_x", "u1"), ("filter_y", "u1"),
             ("ref", "u1", (2,)), ("flags", "u1"), ("comp_mode", "u1"), ("mv", "<i2", (2, 2)), ("mv_index", "<u4", (2,)),
             ("mb_to_left_edge", "<i4"), ("mb_to_right_edge", "<i4"), ("mb_to_top_edge", "<i4"), ("mb_to_bottom_edge", "<i4"),
             ("fwd_offset", "u1"), ("bck_offset", "u1"), ("reserved", "u1", (6,))]

# [0] sub_pel_filters_8, [1] sub_pel_filters_8smooth, [2] sub_pel_filters_8sharp, [3] bilinear_filters (InterpFilter's order), then the tables
# of a dimension <= 4: [4] sub_pel_filters_4, [5] sub_pel_filters_4smooth
FILTERS = np.array([
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -6, 126, 8, -2, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -12, 116, 28, -8, 2, 0],
     [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -14, 102, 48, -12, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 84, 66, -12, 2, 0],
     [0, 2, -14, 76, 76, -14, 2, 0], [0, 2, -12, 66, 84, -14, 2, 0], [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -12, 48, 102, -14, 2, 0],
     [0, 2, -10, 38, 110, -14, 2, 0], [0, 2, -8, 28, 116, -12, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0], [0, 0, -2, 8, 126, -6, 2, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, 28, 62, 34, 2, 0, 0], [0, 0, 26, 62, 36, 4, 0, 0], [0, 0, 22, 62, 40, 4, 0, 0],
     [0, 0, 20, 60, 42, 6, 0, 0], [0, 0, 18, 58, 44, 8, 0, 0], [0, 0, 16, 56, 46, 10, 0, 0], [0, -2, 16, 54, 48, 12, 0, 0],
     [0, -2, 14, 52, 52, 14, -2, 0], [0, 0, 12, 48, 54, 16, -2, 0], [0, 0, 10, 46, 56, 16, 0, 0], [0, 0, 8, 44, 58, 18, 0, 0],
     [0, 0, 6, 42, 60, 20, 0, 0], [0, 0, 4, 40, 62, 22, 0, 0], [0, 0, 4, 36, 62, 26, 0, 0], [0, 0, 2, 34, 62, 28, 2, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [-2, 2, -6, 126, 8, -2, 2, 0], [-2, 6, -12, 124, 16, -6, 4, -2], [-2, 8, -18, 120, 26, -10, 6, -2],
     [-4, 10, -22, 116, 38, -14, 6, -2], [-4, 10, -22, 108, 48, -18, 8, -2], [-4, 10, -24, 100, 60, -20, 8, -2], [-4, 10, -24, 90, 70, -22, 10, -2],
     [-4, 12, -24, 80, 80, -24, 12, -4], [-2, 10, -22, 70, 90, -24, 10, -4], [-2, 8, -20, 60, 100, -24, 10, -4], [-2, 8, -18, 48, 108, -22, 10, -4],
     [-2, 6, -14, 38, 116, -22, 10, -4], [-2, 6, -10, 26, 120, -18, 8, -2], [-2, 4, -6, 16, 124, -12, 6, -2], [0, 2, -2, 8, 126, -6, 2, -2]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, 0, 120, 8, 0, 0, 0], [0, 0, 0, 112, 16, 0, 0, 0], [0, 0, 0, 104, 24, 0, 0, 0],
     [0, 0, 0, 96, 32, 0, 0, 0], [0, 0, 0, 88, 40, 0, 0, 0], [0, 0, 0, 80, 48, 0, 0, 0], [0, 0, 0, 72, 56, 0, 0, 0],
     [0, 0, 0, 64, 64, 0, 0, 0], [0, 0, 0, 56, 72, 0, 0, 0], [0, 0, 0, 48, 80, 0, 0, 0], [0, 0, 0, 40, 88, 0, 0, 0],
     [0, 0, 0, 32, 96, 0, 0, 0], [0, 0, 0, 24, 104, 0, 0, 0], [0, 0, 0, 16, 112, 0, 0, 0], [0, 0, 0, 8, 120, 0, 0, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, -4, 126, 8, -2, 0, 0], [0, 0, -8, 122, 18, -4, 0, 0], [0, 0, -10, 116, 28, -6, 0, 0],
     [0, 0, -12, 110, 38, -8, 0, 0], [0, 0, -12, 102, 48, -10, 0, 0], [0, 0, -14, 94, 58, -10, 0, 0], [0, 0, -12, 84, 66, -10, 0, 0],
     [0, 0, -12, 76, 76, -12, 0, 0], [0, 0, -10, 66, 84, -12, 0, 0], [0, 0, -10, 58, 94, -14, 0, 0], [0, 0, -10, 48, 102, -12, 0, 0],
     [0, 0, -8, 38, 110, -12, 0, 0], [0, 0, -6, 28, 116, -10, 0, 0], [0, 0, -4, 18, 122, -8, 0, 0], [0, 0, -2, 8, 126, -4, 0, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, 30, 62, 34, 2, 0, 0], [0, 0, 26, 62, 36, 4, 0, 0], [0, 0, 22, 62, 40, 4, 0, 0],
     [0, 0, 20, 60, 42, 6, 0, 0], [0, 0, 18, 58, 44, 8, 0, 0], [0, 0, 16, 56, 46, 10, 0, 0], [0, 0, 14, 54, 48, 12, 0, 0],
     [0, 0, 12, 52, 52, 12, 0, 0], [0, 0, 12, 48, 54, 14, 0, 0], [0, 0, 10, 46, 56, 16, 0, 0], [0, 0, 8, 44, 58, 18, 0, 0],
     [0, 0, 6, 42, 60, 20, 0, 0], [0, 0, 4, 40, 62, 22, 0, 0], [0, 0, 4, 36, 62, 26, 0, 0], [0, 0, 2, 34, 62, 30, 0, 0]]], np.int64)


# ---- planes ---------------------------------------------------------------------------------------------------------------------------
def plane_dims(ss):
    """(visible width, visible height, padding) of a plane with sub-sampling ss in both directions"""
    return PIC_W >> ss, PIC_H >> ss, PAD >> ss


@functools.lru_cache(maxsize=None)
def plane(kind, bit_depth, ss, index=0):
    """A padded plane [height + 2 pad][width + 2 pad]: noise from a seed, all 0, all max, or a 0 / max checkerboard.  Do not write to it."""
    w, h, p = plane_dims(ss)
    shape = (h + 2 * p, w + 2 * p)
    dt, mx = (np.uint16 if bit_depth > 8 else np.uint8), (1 << bit_depth) - 1
    if kind == "noise":
        a = np.random.default_rng([20261018, bit_depth, ss, index]).integers(0, mx + 1, shape).astype(dt)
    elif kind == "zero":
        a = np.zeros(shape, dt)
    elif kind == "max":
        a = np.full(shape, mx, dt)
    else:
        yy, xx = np.indices(shape)
        a = (((yy + xx) & 1) * mx).astype(dt)
    a.setflags(write=False)
    return a


def batch_planes(b):
    """[(padded plane, org_x, org_y)] of a batch, in the order of its reference table"""
    p = plane_dims(b["ss"])[2]
    return [(plane(kind, b["bit_depth"], b["ss"], idx), p, p) for kind, idx in b["planes"]]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def clamp(v, lo, hi):  # clamp(), Codec/definitions.h
    return lo if v < lo else (hi if v > hi else v)


def is_block_size(w, h):
    return (int(w), int(h)) in BLOCK_SIZES


def filter_table(f, dim):  # av1_get_interp_filter_params_with_block_size
    if dim <= 4 and f in (0, 2):
        return 4
    if dim <= 4 and f == 1:
        return 5
    return f


def job_mv(job, k, mv_array):
    if int(job["flags"]) & (1 << k):
        return mv_array[int(job["mv_index"][k])]
    return job["mv"][k]


def job_defined(job, n_refs, mv_array, dst_samples, dst_stride):
    w, h = int(job["width"]), int(job["height"])
    comp = int(job["ref"][1]) != NO_REF
    ok = is_block_size(w, h) and job["filter_x"] <= 3 and job["filter_y"] <= 3 and job["ref"][0] < n_refs
    if comp:
        ok = ok and job["ref"][1] < n_refs and job["comp_mode"] <= 1
        if job["comp_mode"] == 1:
            ok = ok and (int(job["fwd_offset"]), int(job["bck_offset"])) in DIST_PAIRS
    for k in range(2 if comp else 1):
        if int(job["flags"]) & (1 << k):
            ok = ok and mv_array is not None and int(job["mv_index"][k]) < len(mv_array)
    return bool(ok and int(job["dst_offset"]) + (h - 1) * dst_stride + w <= dst_samples)


def position(job, mv, ss):
    """clamp_mv_to_umv_border_sb and the unscaled branch of compute_subpel_params: (pos_x, pos_y, subpel_x, subpel_y, sides the clamp moved)"""
    w, h = int(job["width"]), int(job["height"])
    m = 1 << (1 - ss)
    row, col = i16(int(mv[0]) * m), i16(int(mv[1]) * m)  # the (int16_t) cast of the doubled MV
    spel_left, spel_top = (4 + w) << 4, (4 + h) << 4
    min_col, max_col = int(job["mb_to_left_edge"]) * m - spel_left, int(job["mb_to_right_edge"]) * m + spel_left - 16
    min_row, max_row = int(job["mb_to_top_edge"]) * m - spel_top, int(job["mb_to_bottom_edge"]) * m + spel_top - 16
    moved = (col < min_col, col > max_col, row < min_row, row > max_row)  # left, right, top, bottom
    col, row = i16(clamp(col, min_col, max_col)), i16(clamp(row, min_row, max_row))
    return int(job["org_x"]) + (col >> 4), int(job["org_y"]) + (row >> 4), col & 15, row & 15, moved


def window(pl, org_x, org_y, x0, y0, cols, rows):
    """rows x cols samples from picture position (x0, y0), every coordinate clamped to the padded plane"""
    xs = np.clip(np.arange(x0, x0 + cols) + org_x, 0, pl.shape[1] - 1)
    ys = np.clip(np.arange(y0, y0 + rows) + org_y, 0, pl.shape[0] - 1)
    return pl[np.ix_(ys, xs)].astype(np.int64)


def restate_job(planes, bit_depth, ss, job, mv_array=None):
    """One job: (the predicted block [h][w] uint16, events).  events: per reference (variant, moved sides), which dimensions took a 4-tap table
    with an active filter, whether the output clipped at 0 / at the maximum, whether res was negative in the 2-D single path, whether the block
    plus the filter reach lies inside the padded plane (where the reference is defined)."""
    bd, mx = bit_depth, (1 << bit_depth) - 1
    w, h = int(job["width"]), int(job["height"])
    comp = int(job["ref"][1]) != NO_REF
    tabx, taby = filter_table(int(job["filter_x"]), w), filter_table(int(job["filter_y"]), h)
    ro = (1 << (bd + 4)) + (1 << (bd + 3))  # round_offset of the compound functions: offset_bits = bd + 11, round_1 = 7
    ev = {"refs": [], "tap4": set(), "clip_lo": False, "clip_hi": False, "neg_res": False, "inside": True}
    acc = None
    for k in range(2 if comp else 1):
        pl, ox, oy = planes[int(job["ref"][k])]
        px, py, sx, sy, moved = position(job, job_mv(job, k, mv_array), ss)
        S = window(pl, ox, oy, px - 3, py - 3, w + 7, h + 7)
        ev["inside"] = ev["inside"] and px - 3 + ox >= 0 and py - 3 + oy >= 0 and px + w + 4 + ox <= pl.shape[1] and py + h + 4 + oy <= pl.shape[0]
        fx, fy = FILTERS[tabx][sx], FILTERS[taby][sy]
        variant = (sx != 0) + 2 * (sy != 0)
        ev["refs"].append((variant, moved))
        if sx and tabx >= 4:
            ev["tap4"].add("x")
        if sy and taby >= 4:
            ev["tap4"].add("y")
        if variant == 0:
            s = S[3:3 + h, 3:3 + w]
            res = (((s << 4) & 0xFFFF) + ro) & 0xFFFF if comp else s
        elif variant == 1:
            r0 = (sum(int(fx[t]) * S[3:3 + h, t:t + w] for t in range(8)) + 4) >> 3
            res = r0 + ro if comp else (r0 + 8) >> 4
        elif variant == 2:
            v = sum(int(fy[t]) * S[t:t + h, 3:3 + w] for t in range(8))
            res = ((v * 16 + 64) >> 7) + ro if comp else (v + 64) >> 7
        else:
            im = (sum(int(fx[t]) * S[:, t:t + w] for t in range(8)) + (1 << (bd + 6)) + 4) >> 3
            im = im.astype(np.int16).astype(np.int64)  # im_block is int16
            v = sum(int(fy[t]) * im[t:t + h] for t in range(8)) + (1 << (bd + 11))
            if comp:
                res = ((v + 64) >> 7) & 0xFFFF
            else:
                res = ((v + 1024) >> 11) - ((1 << bd) + (1 << (bd - 1)))
                if bd == 8:
                    res = res.astype(np.uint16).astype(np.int16).astype(np.int64)  # int16_t res = (ConvBufType)(...)
                ev["neg_res"] = bool(ev["neg_res"] or (res < 0).any())
        if not comp:
            out = res
        elif k == 0:
            acc = res & 0xFFFF  # the CONV_BUF_TYPE store
            continue
        else:
            tmp = (acc * int(job["fwd_offset"]) + res * int(job["bck_offset"])) >> 4 if job["comp_mode"] else (acc + res) >> 1
            out = (tmp - ro + 8) >> 4
    ev["clip_lo"], ev["clip_hi"] = bool((out < 0).any()), bool((out > mx).any())
    return np.clip(out, 0, mx).astype(np.uint16), ev


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype="<u2").tobytes())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def make_job(ss, w, h, org, mvs, filters=(0, 0), refs=(0, NO_REF), comp_mode=0, offsets=(0, 0)):
    """org = (x, y) in the plane; mvs = [(row, col)] per reference; filters = (x, y).  The edges are MacroBlockD's for a block of the picture."""
    j = np.zeros((), JOB_DTYPE)
    j["width"], j["height"], j["org_x"], j["org_y"] = w, h, org[0], org[1]
    j["filter_x"], j["filter_y"] = filters
    j["ref"] = refs
    for k, mv in enumerate(mvs):
        j["mv"][k] = mv
    j["comp_mode"], j["fwd_offset"], j["bck_offset"] = comp_mode, offsets[0], offsets[1]
    lx, ly, lw, lh = org[0] << ss, org[1] << ss, w << ss, h << ss
    j["mb_to_left_edge"], j["mb_to_right_edge"] = -(lx * 8), (PIC_W - lw - lx) * 8
    j["mb_to_top_edge"], j["mb_to_bottom_edge"] = -(ly * 8), (PIC_H - lh - ly) * 8
    return j


def pack(jobs, stride, x_of=None):
    """dst_offset of every job: shelves of blocks, left to right (x_of(i, x): where job i goes at or after x); returns (jobs, rows)"""
    x = y = shelf = 0
    out = np.array(jobs, JOB_DTYPE)
    for i in range(len(out)):
        w, h = int(out[i]["width"]), int(out[i]["height"])
        x = x_of(i, x) if x_of else x
        if x + w > stride:
            x, y, shelf = (x_of(i, 0) if x_of else 0), y + shelf, 0
        out[i]["dst_offset"] = y * stride + x
        x, shelf = x + w, max(shelf, h)
    return out, y + shelf


def random_mv(rng, ss, variant, reach=12):
    """an MV in 1/8 luma sample whose phases select `variant` on a plane with sub-sampling ss"""
    unit = 8 << ss  # MV units per sample of the plane
    frac = lambda on: int(rng.integers(1, unit)) if on else 0
    return (int(rng.integers(-reach, reach + 1)) * unit + frac(variant & 2), int(rng.integers(-reach, reach + 1)) * unit + frac(variant & 1))


def random_org(rng, ss, w, h):
    pw, ph, _ = plane_dims(ss)
    return (int(rng.integers(0, (pw - w) // 4 + 1)) * 4, int(rng.integers(0, (ph - h) // 4 + 1)) * 4)


def mode_fields(rng, mode):
    """(refs, comp_mode, offsets) of MODES[mode] on a table of two noise planes"""
    if mode == 0:
        return (int(rng.integers(0, 2)), NO_REF), 0, (0, 0)
    return (0, 1), mode - 1, (DIST_PAIRS[int(rng.integers(0, 8))] if mode == 2 else (0, 0))


def finish(name, bit_depth, ss, planes, jobs, stride=None, x_of=None, mv_array=None):
    if stride is None:
        stride = max(256, 4 * max(int(j["width"]) for j in jobs))
    jobs, rows = pack(jobs, stride, x_of)
    return {"name": name, "bit_depth": bit_depth, "ss": ss, "planes": planes, "jobs": jobs, "mv_array": mv_array, "dst_shape": (rows, stride), "dst_stride": stride}


NOISE2 = [("noise", 0), ("noise", 1)]


def sizes_batch(w, h, bd, ss):
    """group 1: {copy, x, y, 2d} x {single, average, distance-weighted} (the second reference of a compound takes a variant of its own), random MVs,
    random dual filters, noise planes; twice each"""
    rng = np.random.default_rng([1, w, h, bd, ss])
    jobs = []
    for rep in range(2):
        for v in range(4):
            for mode in range(3):
                refs, cm, off = mode_fields(rng, mode)
                mvs = [random_mv(rng, ss, v)] + ([random_mv(rng, ss, int(rng.integers(0, 4)) if rep else v)] if mode else [])
                jobs.append(make_job(ss, w, h, random_org(rng, ss, w, h), mvs, (int(rng.integers(0, 4)), int(rng.integers(0, 4))), refs, cm, off))
    return finish(f"sizes_{w}x{h}_{bd}_ss{ss}", bd, ss, NOISE2, jobs)


def sweep_batch(w, h, bd):
    """group 2: all 256 phases x all 16 filter pairs, single reference, on the sub-sampled plane (a luma MV is doubled: even phases only)"""
    rng = np.random.default_rng([2, w, h, bd])
    org = random_org(rng, 1, w, h)
    jobs = [make_job(1, w, h, org, [(16 * ((p >> 4) % 3 - 1) + (p >> 4), 16 * ((p & 15) % 5 - 2) + (p & 15))], (f & 3, f >> 2)) for f in range(16) for p in range(256)]
    return finish(f"sweep_{w}x{h}_{bd}", bd, 1, [("noise", 2)], jobs, stride=64 * max(w, 4))


def compound_batch(bd):
    """group 3: the eight offset pairs on one plane and on two, every pairing of the four variants between the references (both modes)"""
    rng = np.random.default_rng([3, bd])
    jobs = []
    for pair in DIST_PAIRS:
        for refs in ((0, 0), (0, 1)):
            for w, h in ((8, 8), (4, 4)):
                jobs.append(make_job(1, w, h, random_org(rng, 1, w, h), [random_mv(rng, 1, 3), random_mv(rng, 1, 3)],
                                     (int(rng.integers(0, 4)), int(rng.integers(0, 4))), refs, 1, pair))
    for v0 in range(4):
        for v1 in range(4):
            for cm in (0, 1):
                for w, h in ((16, 16), (8, 4)):
                    jobs.append(make_job(1, w, h, random_org(rng, 1, w, h), [random_mv(rng, 1, v0), random_mv(rng, 1, v1)],
                                         (int(rng.integers(0, 4)), int(rng.integers(0, 4))), (0, 1) if v0 != v1 else (1, 1), cm,
                                         DIST_PAIRS[int(rng.integers(0, 8))] if cm else (0, 0)))
    return finish(f"compound_{bd}", bd, 1, NOISE2, jobs)


def clamp_limits(job, ss):
    """the clamp's limits as MVs (1/8 luma): (min_col, max_col, min_row, max_row)"""
    w, h, m = int(job["width"]), int(job["height"]), 1 << (1 - ss)
    lim = (int(job["mb_to_left_edge"]) * m - ((4 + w) << 4), int(job["mb_to_right_edge"]) * m + ((4 + w) << 4) - 16,
           int(job["mb_to_top_edge"]) * m - ((4 + h) << 4), int(job["mb_to_bottom_edge"]) * m + ((4 + h) << 4) - 16)
    assert all(v % m == 0 for v in lim)
    return [v // m for v in lim]


def clamp_batch(bd, ss):
    """group 4: blocks at the corners and edges of the picture; MVs far outside each side, at each limit, one below and one above it; one MV
    whose doubling leaves int16 (luma)"""
    rng = np.random.default_rng([4, bd, ss])
    pw, ph, _ = plane_dims(ss)
    big = 128 >> ss
    jobs = []
    for w, h in ((8, 8), (16, 16), (big, big), (4, 16), (big, big // 2)):
        xs, ys = sorted({0, ((pw - w) // 8) * 4, pw - w}), sorted({0, ((ph - h) // 8) * 4, ph - h})
        where = [(x, y) for x in xs for y in ys if x in (0, pw - w) or y in (0, ph - h)]
        if w == big:
            where = where[:2] + where[-1:]
        for org in where:
            f = (int(rng.integers(0, 4)), int(rng.integers(0, 4)))
            probe = make_job(ss, w, h, org, [(0, 0)], f)
            lo_c, hi_c, lo_r, hi_r = clamp_limits(probe, ss)
            far = 1900
            mvs = [(3, -far), (-5, far), (-far, 3), (far, -5), (-far + 1, -far + 2), (far - 1, far - 3)]
            for d in (-1, 0, 1):
                mvs += [(5, lo_c + d), (-3, hi_c + d), (lo_r + d, 7), (hi_r + d, -1)]
            if w == big:
                mvs = mvs[:6] + mvs[10:14]
            for mv in mvs:
                jobs.append(make_job(ss, w, h, org, [mv], f))
    jobs.append(make_job(ss, 16, 16, (16, 16), [(9, 20000 if ss == 0 else 9000)], (2, 0)))
    jobs.append(make_job(ss, 16, 16, (32, 16), [(-20000 if ss == 0 else -9000, 5)], (0, 2)))
    # a compound whose two references are clamped on opposite sides
    jobs.append(make_job(ss, 8, 8, (0, 0), [(-1900, -1900), (1900, 1900)], (0, 1), (0, 1), 0))
    return finish(f"clamp_{bd}_ss{ss}", bd, ss, NOISE2, jobs, stride=512 if ss == 0 else 256)


def extremes_batch(bd):
    """group 5: planes all 0, all max and a 0 / max checkerboard with the sharp filter (a dimension of 4 takes the 4-tap regular table)"""
    jobs = []
    planes = [("zero", 0), ("max", 0), ("checker", 0)]
    for w, h in ((8, 8), (16, 16), (4, 4), (4, 8), (8, 4)):
        for v in range(4):
            for phase in (8, 5, 15):
                mv = (16 * 2 + (phase if v & 2 else 0), -16 + (phase if v & 1 else 0))
                for ref in range(3):
                    jobs.append(make_job(1, w, h, (16, 8), [mv], (2, 2), (ref, NO_REF)))
                for refs, cm, off in (((2, 2), 0, (0, 0)), ((2, 0), 0, (0, 0)), ((1, 2), 1, (13, 3)), ((2, 1), 1, (3, 13)), ((1, 1), 0, (0, 0)), ((0, 0), 1, (9, 7))):
                    jobs.append(make_job(1, w, h, (20, 12), [mv, (mv[0] + 16, mv[1] + 1 if v & 1 else mv[1])], (2, 2), refs, cm, off))
    return finish(f"extremes_{bd}", bd, 1, planes, jobs)


def geometry_batch(bd, stride):
    """group 6: a stride that is no multiple of 16 samples, dst_offset at every multiple of 4 samples within 16 (an odd stride also moves the rows
    through every alignment)"""
    rng = np.random.default_rng([6, bd, stride])
    jobs = []
    for w, h in ((4, 4), (8, 8), (16, 16), (32, 8), (8, 32), (64, 16)):
        for k in range(4):
            v = (k + w // 4) & 3
            mode = k % 3
            refs, cm, off = mode_fields(rng, mode)
            jobs.append(make_job(0, w, h, random_org(rng, 0, w, h), [random_mv(rng, 0, v)] + ([random_mv(rng, 0, 3 - v)] if mode else []),
                                 (int(rng.integers(0, 4)), int(rng.integers(0, 4))), refs, cm, off))
    x_of = lambda i, x: x + ((4 * (i & 3) - x) % 16)  # the next column that is 4 * (i & 3) modulo 16
    return finish(f"geometry_{bd}_stride{stride}", bd, 0, NOISE2, jobs, stride=stride, x_of=x_of)


@functools.lru_cache(maxsize=None)
def batch_names():
    names = []
    for bd in (8, 10):
        names += [f"sizes_{w}x{h}_{bd}_ss0" for w, h in BLOCK_SIZES]
        names += [f"sizes_{w}x{h}_{bd}_ss1" for w, h in BLOCK_SIZES if w <= 64 and h <= 64]
        names += [f"sweep_{w}x{h}_{bd}" for w, h in SWEEP_SIZES]
        names += [f"compound_{bd}", f"clamp_{bd}_ss0", f"clamp_{bd}_ss1", f"extremes_{bd}", f"geometry_{bd}_stride204", f"geometry_{bd}_stride203"]
    return tuple(names)


@functools.lru_cache(maxsize=None)
def batch(name):
    p = name.split("_")
    if p[0] in ("sizes", "sweep"):
        w, h = (int(v) for v in p[1].split("x"))
        return sizes_batch(w, h, int(p[2]), int(p[3][2:])) if p[0] == "sizes" else sweep_batch(w, h, int(p[2]))
    if p[0] == "compound":
        return compound_batch(int(p[1]))
    if p[0] == "clamp":
        return clamp_batch(int(p[1]), int(p[2][2:]))
    if p[0] == "extremes":
        return extremes_batch(int(p[1]))
    return geometry_batch(int(p[1]), int(p[2][6:]))


@functools.lru_cache(maxsize=None)
def restated(name):
    """(blocks, events) of a batch, job by job"""
    b = batch(name)
    planes = batch_planes(b)
    res = [restate_job(planes, b["bit_depth"], b["ss"], j, b["mv_array"]) for j in b["jobs"]]
    return [r[0] for r in res], [r[1] for r in res]


def batch_crcs(name, blocks):
    """what the fixture holds of a batch: a CRC per job; for a sweep one CRC per filter pair over its 256 blocks"""
    if name.startswith("sweep"):
        return np.array([crc(np.stack(blocks[256 * f:256 * f + 256])) for f in range(16)], np.uint32)
    return np.array([crc(b) for b in blocks], np.uint32)


def sample_jobs():
    """(key, batch name, job index): the jobs whose full block the fixture holds -- the first of every variant x mode of the 16x16 luma batches"""
    out = []
    for bd in (8, 10):
        name = f"sizes_16x16_{bd}_ss0"
        for v in range(4):
            for mode in range(3):
                out.append((f"sample_{bd}_{VARIANTS[v]}_{MODES[mode]}", name, v * 3 + mode))
    return out


def expected_image(b, blocks, fill, defined=None):
    """the destination plane after the batch: `fill` samples everywhere but the defined jobs' blocks"""
    dt = np.uint16 if b["bit_depth"] > 8 else np.uint8
    img = np.full((b["dst_shape"][0], b["dst_stride"]), fill * 0x0101 if b["bit_depth"] > 8 else fill, dt)
    for i, (j, blk) in enumerate(zip(b["jobs"], blocks)):
        if defined is not None and not defined[i]:
            continue
        y, x = divmod(int(j["dst_offset"]), b["dst_stride"])
        img[y:y + int(j["height"]), x:x + int(j["width"])] = blk
    return img


def coverage_missing(records):
    """records: [(bit_depth, job, events)] of every job.  The conditions of the fixture that are not met, as text."""
    ran, tap4 = set(), set()
    moved, kept = [False] * 4, [False] * 4
    clip, neg = set(), False
    for bd, job, ev in records:
        comp = int(job["ref"][1]) != NO_REF
        for variant, mv in ev["refs"]:
            ran.add((bd, comp, variant))
            for s in range(4):
                moved[s], kept[s] = moved[s] or mv[s], kept[s] or not mv[s]
        if ev["tap4"]:
            tap4.add("".join(sorted(ev["tap4"])))
        if ev["clip_lo"]:
            clip.add((bd, 0))
        if ev["clip_hi"]:
            clip.add((bd, 1))
        neg = neg or ev["neg_res"]
    missing = [f"convolve function not run: depth {bd} compound {c} {VARIANTS[v]}" for bd in (8, 10) for c in (False, True) for v in range(4) if (bd, c, v) not in ran]
    sides = ("left", "right", "top", "bottom")
    missing += [f"the clamp never moved an MV on the {sides[s]}" for s in range(4) if not moved[s]]
    missing += [f"the clamp never left an MV alone on the {sides[s]}" for s in range(4) if not kept[s]]
    missing += [f"4-tap tables never used for {t}" for t in ("x", "y", "xy") if t not in tap4]
    missing += [f"the output never clipped at {'the maximum' if hi else '0'} at {bd} bits" for bd in (8, 10) for hi in (0, 1) if (bd, hi) not in clip]
    if not neg:
        missing.append("res was never negative in the 2-D single path")
    return missing


def undefined_batch(bd, kind_sizes=((4, 4), (16, 16))):
    """ordinary jobs with one undefined job of every kind among them: (batch, indices of the undefined jobs)"""
    rng = np.random.default_rng([7, bd])
    jobs, bad = [], []
    mv_array = rng.integers(-60, 61, (5, 2)).astype(np.int16)
    kinds = ["ref0", "ref1", "size", "size_1to8", "filter_x", "filter_y", "mv_index0", "mv_index1", "comp_mode", "offsets", "offsets_sum", "dst_end"]
    for w, h in kind_sizes:
        for kind in kinds:
            for _ in range(2):
                v = int(rng.integers(0, 4))
                jobs.append(make_job(0, w, h, random_org(rng, 0, w, h), [random_mv(rng, 0, v), random_mv(rng, 0, 3 - v)],
                                     (int(rng.integers(0, 4)), int(rng.integers(0, 4))), (0, 1), 1, DIST_PAIRS[int(rng.integers(0, 8))]))
            j = jobs[-1].copy()
            if kind == "ref0":
                j["ref"][0] = 2
            elif kind == "ref1":
                j["ref"][1] = 7
            elif kind == "size":
                j["width"] = 12
            elif kind == "size_1to8":
                j["width"], j["height"] = (4, 32) if w == 4 else (128, 32)
            elif kind in ("filter_x", "filter_y"):
                j[kind] = 4
            elif kind == "mv_index0":
                j["flags"], j["mv_index"][0] = MV0_FROM_ARRAY, 5
            elif kind == "mv_index1":
                j["flags"], j["mv_index"] = MV0_FROM_ARRAY | MV1_FROM_ARRAY, (4, 0xFFFFFFFF)
            elif kind == "comp_mode":
                j["comp_mode"] = 2
            elif kind == "offsets":
                j["fwd_offset"], j["bck_offset"] = 8, 8
            elif kind == "offsets_sum":
                j["fwd_offset"], j["bck_offset"] = 9, 9
            bad.append(len(jobs))
            jobs.append(j)
    # a job that takes both MVs from the array, defined
    j = jobs[0].copy()
    j["flags"], j["mv_index"] = MV0_FROM_ARRAY | MV1_FROM_ARRAY, (4, 0)
    jobs.append(j)
    # the packer gives the odd sizes room like any other; the dst_end jobs are moved past the end of the plane below
    packable = np.array(jobs, JOB_DTYPE)
    b = finish(f"undefined_{bd}", bd, 0, NOISE2, list(packable), mv_array=mv_array)
    k = 0
    for w, h in kind_sizes:
        for kind in kinds:
            k += 2
            if kind == "dst_end":
                b["jobs"][k]["dst_offset"] = b["dst_shape"][0] * b["dst_stride"] - (h - 1) * b["dst_stride"] - w + 1  # one sample too far
            k += 1
    return b, bad


def spoil_desc(d, bad):
    """a descriptor (abi.InterPredDesc with two 512 x 448 references) made invalid in the way `bad` names"""
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith(("bit_depth", "ss_", "n_refs")):
        name, v = bad.rsplit("_", 1)
        setattr(d, name, int(v))
    elif bad == "null_plane":
        d.refs[1].plane = None
    elif bad == "zero_stride":
        d.refs[1].stride = 0
    elif bad == "stride_below_width":
        d.refs[0].stride = 500
    elif bad == "zero_width":
        d.refs[0].width = 0
    elif bad == "org_outside":
        d.refs[1].org_y = 448
    elif bad == "zero_dst_stride":
        d.dst_stride = 0
    elif bad == "zero_dst_samples":
        d.dst_samples = 0
    else:
        d.n_mvs = 3
    return d
