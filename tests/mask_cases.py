"""The cases of the masked prediction entries (include/svt_hip_mask.h) and a numpy restatement of what one job of each computes: masked compound
prediction (svt_hip_masked_pred_batch), the inter-intra combination (svt_hip_interintra_blend_batch) and the three searches
(svt_hip_mask_search_batch).

The reference's own results -- tools/gen_mask_golden.py driving svt_aom_enc_make_inter_predictor, svt_aom_combine_interintra{,_highbd},
svt_aom_calc_pred_masked_compound + svt_aom_search_compound_diff_wedge and inter_intra_search job by job -- are in golden/mask.npz as numbers only:
CRC-32s of the wedge tables, a CRC-32 per predicted / blended block and per DIFFWTD mask, one whole block per size and depth, every output of
every search job.  Planes and jobs are regenerated from seeds here.

Restated (Source/Lib): init_wedge_primary_masks, init_wedge_signs, get_wedge_mask_inplace and the codebooks (Codec/inter_prediction.c:1436-2087),
av1_make_masked_scaled_inter_predictor (Codec/enc_inter_prediction.c:52-166) on the convolve restatement of tests/inter_pred_cases.py,
svt_av1_build_compound_diffwtd_mask_d16_c (C_DEFAULT/inter_prediction_c.c:15-40), svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c and
svt_aom_{,highbd_}blend_a64_mask_c (Codec/blend_a64_mask.c:34-299), build_smooth_interintra_mask and svt_aom_combine_interintra
(Codec/inter_prediction.c:2128-2214,2341-2372), the tail of svt_aom_calc_pred_masked_compound, pick_wedge, pick_wedge_fixed_sign,
pick_interinter_seg (Codec/enc_inter_prediction.c:338-544,4726-4769), svt_av1_wedge_sse_from_residuals_c (Codec/inter_prediction.c:2330-2339),
diffwtd_mask / diffwtd_mask_highbd (:61-129), pick_interintra_wedge and inter_intra_search with use_rd_model = 0 (Codec/mode_decision.c:253-480)."""
import functools
import os
import zlib

import numpy as np

import inter_pred_cases as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask.npz")
WEDGE, DIFFWTD = 0, 1
PARAMS_FROM_ARRAY = 4
ST_OK, ST_UNDEFINED = 0, 0xFF
KIND_WEDGE, KIND_DIFFWTD, KIND_INTERINTRA = 0, 1, 2
NO_RD = 0x7FFFFFFFFFFFFFFF
WEDGE_SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (8, 32), (32, 8)]  # (width, height), BlockSize's order
DIFFWTD_SIZES = [s for s in ip.BLOCK_SIZES if min(s) >= 8]
INTERINTRA_SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)]
SUBSAMPLINGS = [(0, 0), (1, 1), (1, 0), (0, 1)]  # (ss_x, ss_y)
PRED_JOB_DTYPE = [("pred", ip.JOB_DTYPE), ("comp_type", "u1"), ("wedge_index", "u1"), ("wedge_sign", "u1"), ("mask_type", "u1"), ("luma_width", "u1"),
                  ("luma_height", "u1"), ("reserved", "u1", (2,)), ("mask_offset", "<u4"), ("result_index", "<u4")]
BLEND_JOB_DTYPE = [("intra_offset", "<u4", (4,)), ("inter_offset", "<u4"), ("dst_offset", "<u4"), ("result_index", "<u4"), ("width", "u1"), ("height", "u1"),
                   ("luma_width", "u1"), ("luma_height", "u1"), ("interintra_mode", "u1"), ("use_wedge", "u1"), ("wedge_index", "u1"), ("wedge_sign", "u1"),
                   ("flags", "u1"), ("reserved", "u1", (3,))]
SEARCH_JOB_DTYPE = [("src_offset", "<u4"), ("pred0_offset", "<u4"), ("pred1_offset", "<u4"), ("intra_offset", "<u4", (4,)), ("width", "u1"), ("height", "u1"),
                    ("kind", "u1"), ("ii_wedge_mode", "u1")]
RESULT_DTYPE = [("best_rd", "<i8"), ("rd_wedge", "<i8"), ("wedge_index", "i1"), ("wedge_sign", "u1"), ("mask_type", "u1"), ("interintra_mode", "u1"),
                ("use_wedge_interintra", "u1"), ("exit", "u1"), ("reserved", "u1", (2,))]

# AV1 specification: Wedge_Master_Oblique_Odd / _Even / _Vertical, Wedge_Codebook, Ii_Weights_1d
OBLIQUE_ODD = np.array([0] * 28 + [1, 2, 6, 18, 37, 53, 60, 63] + [64] * 28, np.int64)
OBLIQUE_EVEN = np.array([0] * 28 + [1, 4, 11, 27, 46, 58, 62, 63] + [64] * 28, np.int64)
VERTICAL = np.array([0] * 29 + [2, 7, 21, 43, 57, 62] + [64] * 29, np.int64)
HOR, VER, O27, O63, O117, O153 = range(6)  # WedgeDirectionType
_TAIL = [(O27, 4, 2), (O27, 4, 6), (O153, 4, 2), (O153, 4, 6), (O63, 2, 4), (O63, 6, 4), (O117, 2, 4), (O117, 6, 4)]
_HEAD = [(O27, 4, 4), (O63, 4, 4), (O117, 4, 4), (O153, 4, 4)]
CODEBOOKS = {"hgtw": _HEAD + [(HOR, 4, 2), (HOR, 4, 4), (HOR, 4, 6), (VER, 4, 4)] + _TAIL,
             "hltw": _HEAD + [(VER, 2, 4), (VER, 4, 4), (VER, 6, 4), (HOR, 4, 4)] + _TAIL,
             "heqw": _HEAD + [(HOR, 4, 2), (HOR, 4, 6), (VER, 2, 4), (VER, 6, 4)] + _TAIL}
II_WEIGHTS = np.array([60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20, 19, 19, 18, 18,
                       17, 16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 4, 4,
                       4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2] + [1] * 22, np.int64)
assert len(II_WEIGHTS) == 128


def crc8(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes())


# ---- the wedge masks ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def primaries():
    """init_wedge_primary_masks: [2][6][64][64] = [negative][direction]"""
    p = np.zeros((2, 6, 64, 64), np.int64)
    shift = 16
    for i in range(0, 64, 2):  # shift_copy of the even / odd master row
        for row, master in ((i, OBLIQUE_EVEN), (i + 1, OBLIQUE_ODD)):
            if row & 1:
                shift -= 1
            p[0, O63, row] = master[np.clip(np.arange(64) - shift, 0, 63)]
        p[0, VER, i] = p[0, VER, i + 1] = VERTICAL
    msk, mskx = p[0, O63], p[0, VER]
    p[0, O27] = msk.T
    p[0, O117] = 64 - msk[:, ::-1]
    p[0, O153] = (64 - msk[:, ::-1]).T
    p[1, O63], p[1, O27] = 64 - msk, (64 - msk).T
    p[1, O117], p[1, O153] = msk[:, ::-1], msk[:, ::-1].T
    p[0, HOR] = mskx.T
    p[1, VER], p[1, HOR] = 64 - mskx, (64 - mskx).T
    p = p.astype(np.uint8)
    p.setflags(write=False)
    return p


def codebook(w, h):
    return CODEBOOKS["hgtw" if h > w else ("hltw" if h < w else "heqw")]


def window(w, h, index, neg):
    """get_wedge_mask_inplace without the sign-flip: the h x w window of primary [neg][direction]"""
    d, xo, yo = codebook(w, h)[index]
    y0, x0 = 32 - ((yo * h) >> 3), 32 - ((xo * w) >> 3)
    return primaries()[neg, d, y0:y0 + h, x0:x0 + w]


@functools.lru_cache(maxsize=None)
def signflip():
    """init_wedge_signs' rule on the nine sizes: [9][16]"""
    out = np.zeros((9, 16), np.uint8)
    for s, (w, h) in enumerate(WEDGE_SIZES):
        for k in range(16):
            m = window(w, h, k, 0).astype(np.int64)
            avg = int(m[0].sum() + m[1:, 0].sum())
            out[s, k] = ((avg + (w + h - 1) // 2) // (w + h - 1)) < 32
    out.setflags(write=False)
    return out


def wedge_mask(w, h, index, sign):
    """svt_aom_get_contiguous_soft_mask: [h][w] int64"""
    return window(w, h, index, sign ^ int(signflip()[WEDGE_SIZES.index((w, h)), index])).astype(np.int64)


def contiguous_masks():
    """the reference's 9 x 32 contiguous masks in wedge_mask_buf's order: per size, per index, sign 0 then sign 1"""
    return np.concatenate([wedge_mask(w, h, k, s).reshape(-1) for w, h in WEDGE_SIZES for k in range(16) for s in (0, 1)]).astype(np.uint8)


def subsample(m, subw, subh):
    """the mask of the plane's block: the four subw / subh branches of the blend functions"""
    if subw and subh:
        return (m[0::2, 0::2] + m[1::2, 0::2] + m[0::2, 1::2] + m[1::2, 1::2] + 2) >> 2
    if subw:
        return (m[:, 0::2] + m[:, 1::2] + 1) >> 1
    if subh:
        return (m[0::2] + m[1::2] + 1) >> 1
    return m


def smooth_mask(w, h, mode):
    """build_smooth_interintra_mask on a w x h block; ii_size_scales is 128 / max(w, h)"""
    scale = 128 // max(w, h)
    yy, xx = np.indices((h, w))
    if mode == 0:
        return np.full((h, w), 32, np.int64)
    return II_WEIGHTS[(yy if mode == 1 else (xx if mode == 2 else np.minimum(yy, xx))) * scale]


def blend_a64(m, a, b):  # AOM_BLEND_A64
    return (m * a + (64 - m) * b + 32) >> 6


# ---- masked compound prediction ------------------------------------------------------------------------------------------------------------
def position(job, mv, ss_x, ss_y):
    """clamp_mv_to_umv_border_sb and compute_subpel_params' unscaled branch with a sub-sampling per direction: (pos_x, pos_y, subpel_x, subpel_y)"""
    w, h = int(job["width"]), int(job["height"])
    mx, my = 1 << (1 - ss_x), 1 << (1 - ss_y)
    row, col = ip.i16(int(mv[0]) * my), ip.i16(int(mv[1]) * mx)
    spel_left, spel_top = (4 + w) << 4, (4 + h) << 4
    min_col, max_col = int(job["mb_to_left_edge"]) * mx - spel_left, int(job["mb_to_right_edge"]) * mx + spel_left - 16
    min_row, max_row = int(job["mb_to_top_edge"]) * my - spel_top, int(job["mb_to_bottom_edge"]) * my + spel_top - 16
    col, row = ip.i16(ip.clamp(col, min_col, max_col)), ip.i16(ip.clamp(row, min_row, max_row))
    return int(job["org_x"]) + (col >> 4), int(job["org_y"]) + (row >> 4), col & 15, row & 15


def conv_buf(plane, bd, ss_x, ss_y, job, mv):
    """what svt_av1_{,highbd_}jnt_convolve_{2d_copy,x,y,2d}_c leave in the CONV_BUF_TYPE buffer with do_average = 0: ([h][w] in 0..65535, variant,
    whether the block plus the filter reach lies inside the padded plane)"""
    pl, ox, oy = plane
    w, h = int(job["width"]), int(job["height"])
    px, py, sx, sy = position(job, mv, ss_x, ss_y)
    S = ip.window(pl, ox, oy, px - 3, py - 3, w + 7, h + 7)
    inside = px - 3 + ox >= 0 and py - 3 + oy >= 0 and px + w + 4 + ox <= pl.shape[1] and py + h + 4 + oy <= pl.shape[0]
    fx, fy = ip.FILTERS[ip.filter_table(int(job["filter_x"]), w)][sx], ip.FILTERS[ip.filter_table(int(job["filter_y"]), h)][sy]
    ro = (1 << (bd + 4)) + (1 << (bd + 3))
    variant = (sx != 0) + 2 * (sy != 0)
    if variant == 0:
        res = ((S[3:3 + h, 3:3 + w] << 4) & 0xFFFF) + ro
    elif variant == 1:
        res = ((sum(int(fx[t]) * S[3:3 + h, t:t + w] for t in range(8)) + 4) >> 3) + ro
    elif variant == 2:
        res = ((sum(int(fy[t]) * S[t:t + h, 3:3 + w] for t in range(8)) * 16 + 64) >> 7) + ro
    else:
        im = (sum(int(fx[t]) * S[:, t:t + w] for t in range(8)) + (1 << (bd + 6)) + 4) >> 3
        im = im.astype(np.int16).astype(np.int64)
        res = (sum(int(fy[t]) * im[t:t + h] for t in range(8)) + (1 << (bd + 11)) + 64) >> 7
    return res & 0xFFFF, variant, inside


def diffwtd_mask_d16(a, b, bd, mask_type):
    rnd = 4 + (bd - 8)
    m = np.clip(38 + (((np.abs(a - b) + (1 << (rnd - 1))) >> rnd) // 16), 0, 64)
    return 64 - m if mask_type else m


def blend_d16(m, a, b, bd):
    """svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c after the mask's sub-sampling: round_offset of round_1 = 7, round_bits = 4"""
    ro = (1 << (bd + 4)) + (1 << (bd + 3))
    return np.clip(((((m * a + (64 - m) * b) >> 6) - ro) + 8) >> 4, 0, (1 << bd) - 1).astype(np.uint16)


def job_params(job, flags, results):
    """(wedge_index, wedge_sign, mask_type) of a prediction job, or None when its result_index is outside the array"""
    if flags & PARAMS_FROM_ARRAY:
        if results is None or int(job["result_index"]) >= len(results):
            return None
        r = results[int(job["result_index"])]
        return int(r["wedge_index"]) & 0xFF, int(r["wedge_sign"]), int(r["mask_type"])
    return int(job["wedge_index"]), int(job["wedge_sign"]), int(job["mask_type"])


def pred_job_defined(b, job, mask_bytes):
    """the conditions of include/svt_hip_mask.h; mask_bytes None: no mask buffer"""
    p = job["pred"]
    w, h, lw, lh = int(p["width"]), int(p["height"]), int(job["luma_width"]), int(job["luma_height"])
    n_refs, flags = len(b["planes"]), int(p["flags"])
    ok = ip.is_block_size(lw, lh) and w >= 4 and h >= 4 and w == lw >> b["ss_x"] and h == lh >> b["ss_y"] and p["filter_x"] <= 3 and p["filter_y"] <= 3
    ok = ok and p["ref"][0] < n_refs and p["ref"][1] < n_refs and job["comp_type"] <= 1
    for k in range(2):
        if flags & (1 << k):
            ok = ok and b["mv_array"] is not None and int(p["mv_index"][k]) < len(b["mv_array"])
    prm = job_params(job, flags, b["results"])
    if not ok or prm is None:
        return False
    if job["comp_type"] == DIFFWTD:
        ok = lw >= 8 and lh >= 8 and prm[2] <= 1
        if b["plane"] != 0 or mask_bytes is not None:
            ok = ok and mask_bytes is not None and int(job["mask_offset"]) + lw * lh <= mask_bytes
    else:
        ok = (lw, lh) in WEDGE_SIZES and prm[0] < 16 and prm[1] <= 1
    return bool(ok and int(p["dst_offset"]) + (h - 1) * b["dst_stride"] + w <= b["dst_shape"][0] * b["dst_stride"])


def restate_pred_job(b, planes, job, mask_buf):
    """One defined job: (the block [h][w] uint16, the luma DIFFWTD mask [lh][lw] uint8 it computes or None, events).  mask_buf: the mask buffer as
    the job finds it (a chroma DIFFWTD job reads it)."""
    bd, p = b["bit_depth"], job["pred"]
    w, h, lw, lh = int(p["width"]), int(p["height"]), int(job["luma_width"]), int(job["luma_height"])
    widx, wsign, mtype = job_params(job, int(p["flags"]), b["results"])
    bufs, ev = [], {"variants": [], "inside": True}
    for k in range(2):
        res, variant, inside = conv_buf(planes[int(p["ref"][k])], bd, b["ss_x"], b["ss_y"], p, ip.job_mv(p, k, b["mv_array"]))
        bufs.append(res)
        ev["variants"].append(variant)
        ev["inside"] = ev["inside"] and inside
    made = None
    if job["comp_type"] == WEDGE:
        m = wedge_mask(lw, lh, widx, wsign)
    elif b["plane"] == 0:
        m = diffwtd_mask_d16(bufs[0], bufs[1], bd, mtype)
        made = m.astype(np.uint8)
    else:
        o = int(job["mask_offset"])
        m = mask_buf[o:o + lw * lh].reshape(lh, lw).astype(np.int64)
    out = blend_d16(subsample(m, lw == 2 * w, lh == 2 * h), bufs[0], bufs[1], bd)
    ev["clip_lo"], ev["clip_hi"] = bool((out == 0).any()), bool((out == (1 << bd) - 1).any())
    return out, made, ev


def make_pred_job(ss_x, ss_y, lw, lh, lorg, mvs, filters=(0, 0), refs=(0, 1), comp_type=WEDGE, wedge=(0, 0), mask_type=0, mask_offset=0):
    """lorg = the luma block's origin (x, y) in the 192 x 128 picture; mvs = [(row, col)] x 2; the edges are MacroBlockD's for that block"""
    j = np.zeros((), PRED_JOB_DTYPE)
    p = j["pred"]
    p["width"], p["height"], p["org_x"], p["org_y"] = lw >> ss_x, lh >> ss_y, lorg[0] >> ss_x, lorg[1] >> ss_y
    p["filter_x"], p["filter_y"] = filters
    p["ref"] = refs
    for k, mv in enumerate(mvs):
        p["mv"][k] = mv
    p["mb_to_left_edge"], p["mb_to_right_edge"] = -(lorg[0] * 8), (ip.PIC_W - lw - lorg[0]) * 8
    p["mb_to_top_edge"], p["mb_to_bottom_edge"] = -(lorg[1] * 8), (ip.PIC_H - lh - lorg[1]) * 8
    j["comp_type"], j["wedge_index"], j["wedge_sign"], j["mask_type"] = comp_type, wedge[0], wedge[1], mask_type
    j["luma_width"], j["luma_height"], j["mask_offset"] = lw, lh, mask_offset
    return j


def pack_pred(jobs, stride, x_of=None):
    """dst_offset of every job: shelves of blocks, left to right (x_of(i, x): where job i goes at or after x); returns (jobs, rows)"""
    x = y = shelf = 0
    out = np.array(jobs, PRED_JOB_DTYPE)
    for i in range(len(out)):
        w, h = int(out[i]["pred"]["width"]), int(out[i]["pred"]["height"])
        x = x_of(i, x) if x_of else x
        if x + w > stride:
            x, y, shelf = (x_of(i, 0) if x_of else 0), y + shelf, 0
        out["pred"]["dst_offset"][i] = y * stride + x
        x, shelf = x + w, max(shelf, h)
    return out, y + shelf


def finish_pred(name, bd, ss, plane, planes, jobs, stride=None, x_of=None, mv_array=None, results=None, mask_from=None, mask_bytes=None):
    """mask_from: the luma batch whose mask buffer this (chroma) batch reads; mask_bytes: the size of a luma batch's own mask buffer (None: none)"""
    if stride is None:
        stride = max(256, 4 * max(int(j["pred"]["width"]) for j in jobs))
    jobs, rows = pack_pred(jobs, stride, x_of)
    return {"name": name, "bit_depth": bd, "ss_x": ss[0], "ss_y": ss[1], "plane": plane, "planes": planes, "jobs": jobs, "mv_array": mv_array, "results": results,
            "dst_shape": (rows, stride), "dst_stride": stride, "mask_from": mask_from, "mask_bytes": mask_bytes}


def pred_planes(b):
    """[(padded plane, org_x, org_y)] of a batch: the 192 x 128 luma planes of tests/inter_pred_cases.py serve every sub-sampling"""
    pad = ip.plane_dims(0)[2]
    return [(ip.plane(kind, b["bit_depth"], 0, idx), pad, pad) for kind, idx in b["planes"]]


def luma_org(rng, lw, lh):
    return (int(rng.integers(0, (ip.PIC_W - lw) // 8 + 1)) * 8, int(rng.integers(0, (ip.PIC_H - lh) // 8 + 1)) * 8)


def random_mv(rng, ss_x, ss_y, variant, reach=12):
    """an MV in 1/8 luma sample whose phases select `variant` on the plane"""
    ux, uy = 8 << ss_x, 8 << ss_y
    return (int(rng.integers(-reach, reach + 1)) * uy + (int(rng.integers(1, uy)) if variant & 2 else 0),
            int(rng.integers(-reach, reach + 1)) * ux + (int(rng.integers(1, ux)) if variant & 1 else 0))


def random_filters(rng):
    return (int(rng.integers(0, 4)), int(rng.integers(0, 4)))


NOISE2, NOISE2C = [("noise", 0), ("noise", 1)], [("noise", 2), ("noise", 3)]


def wedge_batch(lw, lh, bd, ss):
    """every index x sign of a wedge size on one plane: luma (plane 0) or the same blocks' chroma (plane 1) under a sub-sampling"""
    rng = np.random.default_rng([11, lw, lh, bd])  # the same blocks, MVs and filters for every sub-sampling
    jobs = [make_pred_job(ss[0], ss[1], lw, lh, luma_org(rng, lw, lh), [random_mv(rng, 1, 1, int(rng.integers(0, 4))) for _ in range(2)], random_filters(rng),
                          wedge=(k, s)) for k in range(16) for s in (0, 1)]
    chroma = ss != (0, 0)
    return finish_pred(f"wedge_{lw}x{lh}_{bd}_ss{ss[0]}{ss[1]}", bd, ss, 1 if chroma else 0, NOISE2C if chroma else NOISE2, jobs)


def diffwtd_offsets(jobs):
    """each job's mask behind the previous one's, the first at byte 3 (no alignment is assumed); returns the buffer's size with 5 spare bytes"""
    o = 3
    for j in jobs:
        j["mask_offset"] = o
        o += int(j["luma_width"]) * int(j["luma_height"])
    return o + 5


def diffwtd_batch(lw, lh, bd, ss):
    """both mask types, twice each, on luma (which computes and stores the masks) or on the same blocks' chroma (which reads that buffer)"""
    rng = np.random.default_rng([12, lw, lh, bd])
    jobs = [make_pred_job(ss[0], ss[1], lw, lh, luma_org(rng, lw, lh), [random_mv(rng, 1, 1, int(rng.integers(0, 4))) for _ in range(2)], random_filters(rng),
                          comp_type=DIFFWTD, mask_type=t) for t in (0, 1, 1, 0)]
    nbytes = diffwtd_offsets(jobs)
    luma = f"diffwtd_{lw}x{lh}_{bd}_ss00"
    if ss == (0, 0):
        return finish_pred(luma, bd, ss, 0, NOISE2, jobs, mask_bytes=nbytes)
    return finish_pred(f"diffwtd_{lw}x{lh}_{bd}_ss{ss[0]}{ss[1]}", bd, ss, 2, NOISE2C, jobs, mask_from=luma)


def variants_batch(bd):
    """the 4 x 4 pairs of convolve variants (copy / x / y / 2d per reference) on 8x8 and 32x16, wedge and DIFFWTD"""
    rng = np.random.default_rng([13, bd])
    jobs = []
    for lw, lh in ((8, 8), (32, 16)):
        for v0 in range(4):
            for v1 in range(4):
                for ct in (WEDGE, DIFFWTD):
                    jobs.append(make_pred_job(0, 0, lw, lh, luma_org(rng, lw, lh), [random_mv(rng, 0, 0, v0), random_mv(rng, 0, 0, v1)], random_filters(rng),
                                              comp_type=ct, wedge=(int(rng.integers(0, 16)), int(rng.integers(0, 2))), mask_type=int(rng.integers(0, 2))))
    return finish_pred(f"variants_{bd}", bd, (0, 0), 0, NOISE2, jobs, mask_bytes=diffwtd_offsets(jobs))


def geometry_batch(bd, stride):
    """destination offsets that are not 4- or 8-byte aligned: a stride that is odd or no multiple of 8, every column modulo 8"""
    rng = np.random.default_rng([14, bd, stride])
    jobs = []
    for i, (lw, lh) in enumerate(((8, 8), (16, 16), (32, 8), (8, 32), (16, 8), (32, 32), (64, 64), (16, 64))):
        for k in range(4):
            wedge_size = (lw, lh) in WEDGE_SIZES
            ct = WEDGE if wedge_size and (k & 1) == 0 else DIFFWTD
            jobs.append(make_pred_job(0, 0, lw, lh, luma_org(rng, lw, lh), [random_mv(rng, 0, 0, (k + i) & 3), random_mv(rng, 0, 0, 3 - ((k + i) & 3))],
                                      random_filters(rng), comp_type=ct, wedge=(int(rng.integers(0, 16)), k >> 1), mask_type=k >> 1))
    x_of = lambda i, x: x + ((i - x) % 8)  # the next column that is i modulo 8
    return finish_pred(f"geometry_{bd}_stride{stride}", bd, (0, 0), 0, NOISE2, jobs, stride=stride, x_of=x_of, mask_bytes=diffwtd_offsets(jobs))


def fromarray_batch(bd):
    """parameters from the result array (the flag) and MVs from mv_array, beside jobs that carry their own"""
    rng = np.random.default_rng([15, bd])
    results = np.zeros(12, RESULT_DTYPE)
    results["wedge_index"], results["wedge_sign"], results["mask_type"] = rng.integers(0, 16, 12), rng.integers(0, 2, 12), rng.integers(0, 2, 12)
    mv_array = np.array([random_mv(rng, 0, 0, int(rng.integers(0, 4))) for _ in range(9)], np.int16)
    jobs = []
    for i in range(24):
        lw, lh = WEDGE_SIZES[i % 9]
        j = make_pred_job(0, 0, lw, lh, luma_org(rng, lw, lh), [random_mv(rng, 0, 0, i & 3), random_mv(rng, 0, 0, (i >> 2) & 3)], random_filters(rng),
                          comp_type=i & 1, wedge=(15 - i % 16, i & 1), mask_type=(i >> 1) & 1)
        if i % 3:
            j["pred"]["flags"] |= PARAMS_FROM_ARRAY
            j["result_index"] = (7 * i) % 12
        if i % 4 == 1:
            j["pred"]["flags"] |= ip.MV0_FROM_ARRAY | ip.MV1_FROM_ARRAY
            j["pred"]["mv_index"] = (i % 9, (i + 4) % 9)
        jobs.append(j)
    return finish_pred(f"fromarray_{bd}", bd, (0, 0), 0, NOISE2, jobs, mv_array=mv_array, results=results, mask_bytes=diffwtd_offsets(jobs))


@functools.lru_cache(maxsize=None)
def pred_batch_names():
    names = []
    for bd in (8, 10):
        names += [f"wedge_{w}x{h}_{bd}_ss{sx}{sy}" for w, h in WEDGE_SIZES for sx, sy in SUBSAMPLINGS]
        names += [f"diffwtd_{w}x{h}_{bd}_ss00" for w, h in DIFFWTD_SIZES] + [f"diffwtd_{w}x{h}_{bd}_ss11" for w, h in DIFFWTD_SIZES]
        names += [f"diffwtd_{w}x{h}_{bd}_ss{sx}{sy}" for w, h in ((8, 8), (16, 16), (32, 16)) for sx, sy in ((1, 0), (0, 1))]
        names += [f"variants_{bd}", f"geometry_{bd}_stride203", f"geometry_{bd}_stride204", f"fromarray_{bd}"]
    return tuple(names)


@functools.lru_cache(maxsize=None)
def pred_batch(name):
    p = name.split("_")
    if p[0] in ("wedge", "diffwtd"):
        w, h = (int(v) for v in p[1].split("x"))
        return (wedge_batch if p[0] == "wedge" else diffwtd_batch)(w, h, int(p[2]), (int(p[3][2]), int(p[3][3])))
    if p[0] == "variants":
        return variants_batch(int(p[1]))
    if p[0] == "geometry":
        return geometry_batch(int(p[1]), int(p[2][6:]))
    return fromarray_batch(int(p[1]))


def run_pred_restated(b, mask_in=None, planes=None):
    """Every job of a batch by the restatement: (blocks (None for an undefined job), defined flags, the mask buffer afterwards or None, events).
    mask_in: the mask buffer a chroma batch finds; planes: the batch's own reference planes when they are not the shared ones."""
    planes = pred_planes(b) if planes is None else planes
    mask_buf = mask_in.copy() if mask_in is not None else (np.full(b["mask_bytes"], 0xA5, np.uint8) if b["mask_bytes"] is not None else None)
    nbytes = len(mask_buf) if mask_buf is not None else None
    blocks, defined, events = [], [], []
    for j in b["jobs"]:
        ok = pred_job_defined(b, j, nbytes)
        defined.append(ok)
        if not ok:
            blocks.append(None)
            events.append(None)
            continue
        blk, made, ev = restate_pred_job(b, planes, j, mask_buf)
        if made is not None and mask_buf is not None:
            o = int(j["mask_offset"])
            mask_buf[o:o + made.size] = made.reshape(-1)
        blocks.append(blk)
        events.append(ev)
    return blocks, defined, mask_buf, events


@functools.lru_cache(maxsize=None)
def pred_restated(name):
    b = pred_batch(name)
    mask_in = pred_restated(b["mask_from"])[2] if b["mask_from"] else None
    return run_pred_restated(b, mask_in)


def pred_expected_image(b, blocks, fill):
    """the destination plane after the batch: `fill` bytes everywhere but the defined jobs' blocks"""
    dt = np.uint16 if b["bit_depth"] > 8 else np.uint8
    img = np.full((b["dst_shape"][0], b["dst_stride"]), fill * 0x0101 if b["bit_depth"] > 8 else fill, dt)
    for j, blk in zip(b["jobs"], blocks):
        if blk is not None:
            y, x = divmod(int(j["pred"]["dst_offset"]), b["dst_stride"])
            img[y:y + blk.shape[0], x:x + blk.shape[1]] = blk
    return img


def pred_sample_jobs():
    """(key, batch name, job index): one whole block per size and depth in the fixture"""
    out = []
    for bd in (8, 10):
        out += [(f"sample_wedge_{w}x{h}_{bd}", f"wedge_{w}x{h}_{bd}_ss00", 9) for w, h in WEDGE_SIZES]
        out += [(f"sample_diffwtd_{w}x{h}_{bd}", f"diffwtd_{w}x{h}_{bd}_ss00", 1) for w, h in DIFFWTD_SIZES]
    return out


def edge_batch(bd, pw, ph):
    """blocks that hang over each edge and each corner of an unpadded pw x ph plane: the kernel's clamp of every source coordinate runs (the
    reference is not defined there); the edges let every MV through"""
    rng = np.random.default_rng([16, bd, pw, ph])
    dt = np.uint16 if bd > 8 else np.uint8
    planes = [(rng.integers(0, 1 << bd, (ph, pw)).astype(dt), 0, 0) for _ in range(2)]
    jobs = []
    for lw, lh in ((8, 8), (16, 16), (32, 8)):
        xs, ys = (-lw // 2, (pw - lw) // 2, pw - lw // 2), (-lh // 2, (ph - lh) // 2, ph - lh // 2)
        for xi, x in enumerate(xs):
            for yi, y in enumerate(ys):
                if xi == 1 and yi == 1:
                    continue
                j = make_pred_job(0, 0, lw, lh, (0, 0), [random_mv(rng, 0, 0, 3, 1), random_mv(rng, 0, 0, int(rng.integers(0, 4)), 1)], random_filters(rng),
                                  comp_type=(xi + yi) & 1, wedge=(int(rng.integers(0, 16)), xi & 1), mask_type=yi & 1)
                p = j["pred"]
                p["org_x"], p["org_y"] = x, y
                p["mb_to_left_edge"], p["mb_to_top_edge"], p["mb_to_right_edge"], p["mb_to_bottom_edge"] = -(1 << 20), -(1 << 20), 1 << 20, 1 << 20
                jobs.append(j)
    b = finish_pred(f"edge_{bd}_{pw}x{ph}", bd, (0, 0), 0, [("own", 0), ("own", 1)], jobs, mask_bytes=diffwtd_offsets(jobs))
    return b, planes


def undefined_pred_batch(bd):
    """ordinary jobs with one undefined job of every kind among them: (batch, indices of the undefined jobs, the kinds)"""
    rng = np.random.default_rng([17, bd])
    kinds = ["wedge_size", "wedge_index", "wedge_sign", "mask_type", "comp_type", "diffwtd_below_8", "mask_end", "result_index", "single_ref", "ref0", "ref1",
             "filter_x", "filter_y", "mv_index0", "mv_index1", "dst_end", "plane_size", "luma_size"]
    results = np.zeros(3, RESULT_DTYPE)
    results["wedge_index"][2] = -1  # what a search without a wedge search leaves
    mv_array = rng.integers(-60, 61, (5, 2)).astype(np.int16)
    jobs, bad = [], []
    for kind in kinds:
        for i in range(2):
            lw, lh = ((16, 16), (8, 16))[i]
            jobs.append(make_pred_job(0, 0, lw, lh, luma_org(rng, lw, lh), [random_mv(rng, 0, 0, 3), random_mv(rng, 0, 0, int(rng.integers(0, 4)))],
                                      random_filters(rng), comp_type=i, wedge=(int(rng.integers(0, 16)), int(rng.integers(0, 2))), mask_type=i))
        diff = kind in ("mask_type", "diffwtd_below_8", "mask_end")
        j = make_pred_job(0, 0, 16, 16, luma_org(rng, 16, 16), [random_mv(rng, 0, 0, 3), random_mv(rng, 0, 0, 1)], random_filters(rng),
                          comp_type=DIFFWTD if diff else WEDGE, wedge=(5, 1), mask_type=1)
        p = j["pred"]
        if kind == "wedge_size":
            j["luma_width"], p["width"] = 64, 64
        elif kind == "wedge_index":
            j["wedge_index"] = 16
        elif kind == "wedge_sign":
            j["wedge_sign"] = 2
        elif kind == "mask_type":
            j["mask_type"] = 2
        elif kind == "comp_type":
            j["comp_type"] = 2
        elif kind == "diffwtd_below_8":
            j["luma_width"], p["width"] = 4, 4
        elif kind == "result_index":
            p["flags"], j["result_index"] = PARAMS_FROM_ARRAY, 3
        elif kind == "single_ref":
            p["ref"][1] = ip.NO_REF
        elif kind == "ref0":
            p["ref"][0] = 2
        elif kind == "ref1":
            p["ref"][1] = 7
        elif kind in ("filter_x", "filter_y"):
            p[kind] = 4
        elif kind == "mv_index0":
            p["flags"], p["mv_index"][0] = ip.MV0_FROM_ARRAY, 5
        elif kind == "mv_index1":
            p["flags"], p["mv_index"] = ip.MV0_FROM_ARRAY | ip.MV1_FROM_ARRAY, (4, 0xFFFFFFFF)
        elif kind == "plane_size":
            p["width"] = 8  # not the luma block on a plane without sub-sampling
        elif kind == "luma_size":
            j["luma_width"], p["width"] = 12, 12
        bad.append(len(jobs))
        jobs.append(j)
    # defined: both MVs and the parameters from the arrays; undefined: a wedge_index of -1 from the array
    j = jobs[0].copy()
    j["pred"]["flags"], j["pred"]["mv_index"], j["result_index"] = ip.MV0_FROM_ARRAY | ip.MV1_FROM_ARRAY | PARAMS_FROM_ARRAY, (4, 0), 1
    jobs.append(j)
    j = j.copy()
    j["result_index"] = 2
    bad.append(len(jobs))
    jobs.append(j)
    nbytes = diffwtd_offsets(jobs)
    b = finish_pred(f"undefined_{bd}", bd, (0, 0), 0, NOISE2, jobs, mv_array=mv_array, results=results, mask_bytes=nbytes)
    for k, kind in enumerate(kinds):
        j = b["jobs"][3 * k + 2]
        if kind == "dst_end":
            j["pred"]["dst_offset"] = b["dst_shape"][0] * b["dst_stride"] - 15 * b["dst_stride"] - 16 + 1  # one sample too far
        elif kind == "mask_end":
            j["mask_offset"] = nbytes - 256 + 1  # one byte too far
    return b, bad, kinds


def spoil_pred_desc(d, bad):
    """a descriptor (abi.MaskedPredDesc) made invalid in the way `bad` names; what inter_pred_cases.spoil_desc knows goes there"""
    if bad == "plane_3":
        d.plane = 3
    elif bad == "luma_with_ss":
        d.plane, d.ss_x = 0, 1
    elif bad == "n_results_without_results":
        d.n_results, d.results = 2, None
    elif bad == "mask_bytes_without_mask_buf":
        d.mask_bytes, d.mask_buf = 64, None
    else:
        ip.spoil_desc(d, bad)
    return d


# ---- the inter-intra combination -----------------------------------------------------------------------------------------------------------
def blend_job_defined(b, j, results):
    w, h, lw, lh = int(j["width"]), int(j["height"]), int(j["luma_width"]), int(j["luma_height"])
    ok = (lw, lh) in INTERINTRA_SIZES and w >= 4 and h >= 4 and w in (lw, lw // 2) and h in (lh, lh // 2)
    mode, use_wedge, widx = int(j["interintra_mode"]), int(j["use_wedge"]), int(j["wedge_index"])
    if int(j["flags"]) & PARAMS_FROM_ARRAY:
        if results is None or int(j["result_index"]) >= len(results):
            return False
        r = results[int(j["result_index"])]
        mode, use_wedge, widx = int(r["interintra_mode"]), int(r["use_wedge_interintra"]), int(r["wedge_index"]) & 0xFF
    ok = ok and mode <= 3 and use_wedge <= 1 and (not use_wedge or (widx < 16 and j["wedge_sign"] <= 1))
    if not ok:
        return False
    for name, o in (("intra", j["intra_offset"][mode]), ("inter", j["inter_offset"]), ("dst", j["dst_offset"])):
        rows, stride = b[f"{name}_shape"]
        ok = ok and int(o) + (h - 1) * stride + w <= rows * stride
    return bool(ok)


def restate_blend_job(b, intra, inter, j, results=None):
    """svt_aom_combine_interintra{,_highbd} on one defined job: the block [h][w] uint16"""
    w, h, lw, lh = int(j["width"]), int(j["height"]), int(j["luma_width"]), int(j["luma_height"])
    mode, use_wedge, widx = int(j["interintra_mode"]), int(j["use_wedge"]), int(j["wedge_index"])
    if int(j["flags"]) & PARAMS_FROM_ARRAY:
        r = results[int(j["result_index"])]
        mode, use_wedge, widx = int(r["interintra_mode"]), int(r["use_wedge_interintra"]), int(r["wedge_index"])
    blk = lambda pl, o: pl.reshape(-1)[np.add.outer(np.arange(h) * pl.shape[1], np.arange(w)) + int(o)].astype(np.int64)
    m = subsample(wedge_mask(lw, lh, widx, int(j["wedge_sign"])), lw == 2 * w, lh == 2 * h) if use_wedge else smooth_mask(w, h, mode)
    return blend_a64(m, blk(intra, j["intra_offset"][mode]), blk(inter, j["inter_offset"])).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def blend_batch(bd, ss_x, ss_y):
    """7 sizes x (4 modes + 16 wedges) on one plane: intra, inter and destination planes with unequal strides, the blocks at odd offsets.  The inter
    and destination offsets are equal, so the batch also runs in place on a destination of the inter plane's stride."""
    rng = np.random.default_rng([21, bd, ss_x, ss_y])
    dt = np.uint16 if bd > 8 else np.uint8
    jobs = []
    x = y = shelf = 0
    for lw, lh in INTERINTRA_SIZES:
        w, h = lw >> ss_x, lh >> ss_y
        for k in range(20):
            j = np.zeros((), BLEND_JOB_DTYPE)
            j["width"], j["height"], j["luma_width"], j["luma_height"] = w, h, lw, lh
            if k < 4:
                j["interintra_mode"], j["wedge_index"], j["wedge_sign"] = k, 0xEE, 0xEE  # the unused parameters are not looked at
            else:
                j["use_wedge"], j["wedge_index"], j["interintra_mode"] = 1, k - 4, k & 3
            x += 1 + (k & 1)
            if x + w > 300:
                x, y, shelf = 1, y + shelf, 0
            j["intra_offset"] = 0xFFFFFFFF  # of the four intra blocks only the mode's is looked at
            j["intra_offset"][int(j["interintra_mode"])], j["inter_offset"], j["dst_offset"] = y * 331 + x + 2, y * 308 + x, y * 308 + x
            x, shelf = x + w, max(shelf, h)
            jobs.append(j)
    rows = y + shelf
    intra, inter = rng.integers(0, 1 << bd, (rows + 1, 331)).astype(dt), rng.integers(0, 1 << bd, (rows, 308)).astype(dt)
    for a in (intra, inter):
        a.setflags(write=False)
    return {"name": f"blend_{bd}_ss{ss_x}{ss_y}", "bit_depth": bd, "jobs": np.array(jobs, BLEND_JOB_DTYPE), "intra": intra, "inter": inter,
            "intra_shape": intra.shape, "inter_shape": inter.shape, "dst_shape": inter.shape}


def blend_batch_names():
    return [f"blend_{bd}_ss{sx}{sy}" for bd in (8, 10) for sx, sy in SUBSAMPLINGS]


def blend_by_name(name):
    p = name.split("_")
    return blend_batch(int(p[1]), int(p[2][2]), int(p[2][3]))


@functools.lru_cache(maxsize=None)
def blend_restated(name):
    b = blend_by_name(name)
    return [restate_blend_job(b, b["intra"], b["inter"], j) for j in b["jobs"]]


def blend_expected_image(b, blocks, base):
    """`base` (the inter plane in place, a filled plane out of place) with the jobs' blocks"""
    img = base.copy()
    for j, blk in zip(b["jobs"], blocks):
        if blk is not None:
            y, x = divmod(int(j["dst_offset"]), img.shape[1])
            img[y:y + blk.shape[0], x:x + blk.shape[1]] = blk
    return img


# ---- the searches --------------------------------------------------------------------------------------------------------------------------
def sat16(v):
    return np.clip(v, -32768, 32767)


def wedge_sse(r1, d, m):
    """svt_av1_wedge_sse_from_residuals_c: (the rounded sse, whether the int16 clamp fired)"""
    t = 64 * r1 + m * d
    c = sat16(t)
    return (int((c * c).sum()) + 2048) >> 12, bool((c != t).any())


def gate_exits(p0, p1, mult):
    """the tail of svt_aom_calc_pred_masked_compound: the SAD of pred0 against pred1 below width x height x mult"""
    return int(np.abs(p0 - p1).sum()) < p0.size * mult


def pick_wedge(src, p0, p1):
    """pick_wedge: (wedge_index, wedge_sign, best_rd, events)"""
    h, w = src.shape
    r0, r1, d = src - p0, src - p1, p1 - p0
    sign_limit = (int((r0 * r0).sum()) - int((r1 * r1).sum())) * 32
    ds_full = r0 * r0 - r1 * r1
    ds = sat16(ds_full)  # svt_av1_wedge_compute_delta_squares_c
    ev = {"ds_saturated": bool((ds != ds_full).any()), "clamp": False}
    best = (None, None, None)
    for k in range(16):
        sign = int(int((ds * wedge_mask(w, h, k, 0)).sum()) > sign_limit)  # svt_av1_wedge_sign_from_residuals_c
        sse, fired = wedge_sse(r1, d, wedge_mask(w, h, k, sign))
        ev["clamp"] = ev["clamp"] or fired
        if best[2] is None or sse < best[2]:
            best = (k, sign, sse)
    return best + (ev,)


def pixel_diffwtd_mask(p0, p1, bd, mask_type):
    """svt_av1_build_compound_diffwtd_mask{,_highbd}_c on the pixel predictions"""
    m = np.minimum(38 + ((np.abs(p0 - p1) >> (bd - 8)) // 16), 64)
    return 64 - m if mask_type else m


def pick_seg(src, p0, p1, bd):
    """pick_interinter_seg: (mask_type, best_rd, events)"""
    r1, d = src - p1, p1 - p0
    rds, fired = zip(*(wedge_sse(r1, d, pixel_diffwtd_mask(p0, p1, bd, t)) for t in (0, 1)))
    t = int(rds[1] < rds[0])
    return t, rds[t], {"clamp": any(fired), "rds": rds}


def ii_search(src, intra4, inter, wedge_mode):
    """inter_intra_search with use_rd_model = 0: (interintra_mode, use_wedge_interintra, wedge_index, best_rd, rd_wedge)"""
    h, w = src.shape
    best_mode, best_rd = None, None
    for mode in range(4):
        e = src - blend_a64(smooth_mask(w, h, mode), intra4[mode], inter)
        rd = int((e * e).sum())
        if best_rd is None or rd < best_rd:
            best_mode, best_rd = mode, rd
    widx, rd_wedge = -1, NO_RD
    if wedge_mode:  # pick_interintra_wedge -> pick_wedge_fixed_sign, sign 0
        r1, d = src - inter, inter - intra4[best_mode]
        rd_wedge = None
        for k in range(16):
            sse, _ = wedge_sse(r1, d, wedge_mask(w, h, k, 0))
            if rd_wedge is None or sse < rd_wedge:
                widx, rd_wedge = k, sse
    return best_mode, int(wedge_mode == 1 or rd_wedge < best_rd), widx, best_rd, rd_wedge


class SearchBatch:
    """The planes and jobs of one search launch.  add() places a job's blocks: the same (x, y) in the source, pred0 and pred1 planes, whose strides
    differ, at an x that moves through every residue modulo 8; the four intra blocks side by side in the intra plane."""
    STRIDES = {"src": 531, "pred0": 538, "pred1": 547, "intra": 4 * 131 + 9}

    def __init__(self, name, bd, mult=0):
        self.name, self.bit_depth, self.mult = name, bd, mult
        self.specs, self.x, self.y, self.shelf, self.iy = [], 0, 0, 0, 0

    def add(self, kind, src, p0, p1, intra4=None, wedge_mode=0):
        h, w = src.shape
        x = self.x + 1 + len(self.specs) % 3
        if x + w > 520:
            x, self.y, self.shelf = 1 + len(self.specs) % 3, self.y + self.shelf, 0
        spec = {"kind": kind, "w": w, "h": h, "x": x, "y": self.y, "src": src, "pred0": p0, "pred1": p1, "intra4": intra4, "wedge_mode": wedge_mode, "iy": self.iy}
        self.x, self.shelf = x + w, max(self.shelf, h)
        if intra4 is not None:
            self.iy += h
        self.specs.append(spec)
        return self

    @functools.cached_property
    def built(self):
        dt = np.uint16 if self.bit_depth > 8 else np.uint8
        rows = self.y + self.shelf
        fill = lambda r, s, seed: np.random.default_rng([31, seed, len(self.specs)]).integers(0, 1 << self.bit_depth, (r, s)).astype(dt)
        pl = {k: fill(rows, self.STRIDES[k], i) for i, k in enumerate(("src", "pred0", "pred1"))}
        pl["intra"] = fill(max(self.iy, 1), self.STRIDES["intra"], 3)
        jobs = np.zeros(len(self.specs), SEARCH_JOB_DTYPE)
        for j, s in zip(jobs, self.specs):
            j["width"], j["height"], j["kind"], j["ii_wedge_mode"] = s["w"], s["h"], s["kind"], s["wedge_mode"]
            for k in ("src", "pred0", "pred1"):
                if s[k] is not None:
                    pl[k][s["y"]:s["y"] + s["h"], s["x"]:s["x"] + s["w"]] = s[k]
                j[f"{k}_offset"] = s["y"] * self.STRIDES[k] + s["x"]
            if s["intra4"] is not None:
                for m in range(4):
                    x = 2 + m * 131 + (m & 1)
                    pl["intra"][s["iy"]:s["iy"] + s["h"], x:x + s["w"]] = s["intra4"][m]
                    j["intra_offset"][m] = s["iy"] * self.STRIDES["intra"] + x
        for a in pl.values():
            a.setflags(write=False)
        return pl, jobs

    @property
    def planes(self):
        return self.built[0]

    @property
    def jobs(self):
        return self.built[1]


def block_of(plane, offset, w, h):
    return plane.reshape(-1)[np.add.outer(np.arange(h) * plane.shape[1], np.arange(w)) + int(offset)].astype(np.int64)


def search_job_defined(planes, j):
    w, h, kind = int(j["width"]), int(j["height"]), int(j["kind"])
    inside = lambda name, o: planes.get(name) is not None and int(o) + (h - 1) * planes[name].shape[1] + w <= planes[name].size
    ok = kind <= 2 and inside("src", j["src_offset"]) and inside("pred1", j["pred1_offset"])
    if kind == KIND_WEDGE:
        ok = ok and (w, h) in WEDGE_SIZES
    if kind == KIND_DIFFWTD:
        ok = ok and (w, h) in DIFFWTD_SIZES
    if kind <= 1:
        ok = ok and inside("pred0", j["pred0_offset"])
    if kind == KIND_INTERINTRA:
        ok = ok and (w, h) in INTERINTRA_SIZES and j["ii_wedge_mode"] <= 2 and all(inside("intra", o) for o in j["intra_offset"])
    return bool(ok)


def restate_search_job(planes, bd, mult, j, before=None):
    """One defined job: (the result record as the job leaves it -- `before` with exit = 1 when the gate fires -- and the events)"""
    w, h, kind = int(j["width"]), int(j["height"]), int(j["kind"])
    r = np.zeros((), RESULT_DTYPE)
    src, p1 = block_of(planes["src"], j["src_offset"], w, h), block_of(planes["pred1"], j["pred1_offset"], w, h)
    ev = {}
    if kind <= 1:
        p0 = block_of(planes["pred0"], j["pred0_offset"], w, h)
        ev["sad"] = int(np.abs(p0 - p1).sum())
        if gate_exits(p0, p1, mult):
            r = np.zeros((), RESULT_DTYPE) if before is None else before.copy()
            r["exit"] = 1
            return r, ev
        if kind == KIND_WEDGE:
            k, s, rd, e = pick_wedge(src, p0, p1)
            r["wedge_index"], r["wedge_sign"], r["best_rd"] = k, s, rd
        else:
            t, rd, e = pick_seg(src, p0, p1, bd)
            r["mask_type"], r["best_rd"] = t, rd
        ev.update(e)
    else:
        intra4 = [block_of(planes["intra"], o, w, h) for o in j["intra_offset"]]
        mode, use, widx, rd, rdw = ii_search(src, intra4, p1, int(j["ii_wedge_mode"]))
        r["interintra_mode"], r["use_wedge_interintra"], r["wedge_index"], r["best_rd"], r["rd_wedge"] = mode, use, widx, rd, rdw
    return r, ev


def noise(rng, bd, w, h, lo=None, hi=None):
    lo, hi = (0 if lo is None else lo), ((1 << bd) if hi is None else hi)
    return rng.integers(lo, hi, (h, w)).astype(np.int64)


RANGES = {"full8": (8, None, None), "mid8": (8, 96, 160), "full10": (10, None, None), "mid10": (10, 384, 640)}


@functools.lru_cache(maxsize=None)
def planted_wedge_batch(rng_name):
    """src = blend(mask(index, sign), p0, p1) with p0, p1 independent noise of the range: every (size, index, sign), 288 jobs"""
    bd, lo, hi = RANGES[rng_name]
    rng = np.random.default_rng([41, bd, lo or 0])
    sb = SearchBatch(f"planted_wedge_{rng_name}", bd)
    planted = []
    for w, h in WEDGE_SIZES:
        for k in range(16):
            for s in (0, 1):
                p0, p1 = noise(rng, bd, w, h, lo, hi), noise(rng, bd, w, h, lo, hi)
                sb.add(KIND_WEDGE, blend_a64(wedge_mask(w, h, k, s), p0, p1), p0, p1)
                planted.append((k, s))
    return sb, planted


@functools.lru_cache(maxsize=None)
def planted_seg_batch(bd):
    """src = blend(DIFFWTD mask of the type, p0, p1): both types on the 17 sizes; last, the job of the largest sums: 128 x 128, src = p0 = 0, p1 = max"""
    rng = np.random.default_rng([42, bd])
    sb = SearchBatch(f"planted_seg_{bd}", bd)
    planted = []
    for w, h in DIFFWTD_SIZES:
        for t in (0, 1):
            p0, p1 = noise(rng, bd, w, h), noise(rng, bd, w, h)
            sb.add(KIND_DIFFWTD, blend_a64(pixel_diffwtd_mask(p0, p1, bd, t), p0, p1), p0, p1)
            planted.append(t)
    z = np.zeros((128, 128), np.int64)
    sb.add(KIND_DIFFWTD, z, z, z + (1 << bd) - 1)
    return sb, planted


@functools.lru_cache(maxsize=None)
def ties_batch(bd):
    """p0 == p1 (multiplier 0): index 0, sign 0, mask type 0; four equal intra blocks: II_DC_PRED"""
    rng = np.random.default_rng([43, bd])
    sb = SearchBatch(f"ties_{bd}", bd)
    for w, h in ((8, 8), (16, 32), (32, 32)):
        p, s = noise(rng, bd, w, h), noise(rng, bd, w, h)
        sb.add(KIND_WEDGE, s, p, p).add(KIND_DIFFWTD, s, p, p)
        i = noise(rng, bd, w, h)
        sb.add(KIND_INTERINTRA, s, None, i, [i] * 4, 2)  # intra == inter: every blend is the same block
    return sb


@functools.lru_cache(maxsize=None)
def gate_batch(bd, mult):
    """jobs whose SAD is exactly w h mult - 1 (exit) and exactly w h mult (no exit), both kinds; mult 0: a SAD of 0 does not exit"""
    rng = np.random.default_rng([44, bd, mult])
    sb = SearchBatch(f"gate_{bd}_{mult}", bd, mult)
    want = []
    for w, h in ((8, 8), (32, 8), (16, 32), (32, 32)):
        for kind in (KIND_WEDGE, KIND_DIFFWTD):
            for less in ((1, 0) if mult else (0,)):
                p0 = noise(rng, bd, w, h, 0, (1 << bd) - 8)
                total = w * h * mult - less
                add = np.full(w * h, total // (w * h), np.int64)
                add[rng.permutation(w * h)[:total % (w * h)]] += 1
                add = add.reshape(h, w) * np.where(rng.integers(0, 2, (h, w)) == 1, 1, -1)
                p1 = p0 + add
                p1 = np.where(p1 < 0, p0 - add, p1)  # the sign does not change the SAD
                sb.add(kind, noise(rng, bd, w, h), p0, p1)
                want.append(bool(less))
    return sb, want


@functools.lru_cache(maxsize=None)
def ii_batch(bd):
    """7 sizes x 4 planted modes x ii_wedge_mode 0 / 1 / 2; for mode 2 a job on each side of rd_wedge < rd_best (a planted wedge; a planted smooth
    mode) and one with equality (everything equal: 0 == 0)"""
    rng = np.random.default_rng([45, bd])
    sb = SearchBatch(f"ii_{bd}", bd)
    info = []
    for w, h in INTERINTRA_SIZES:
        for mode in range(4):
            for wm in (0, 1, 2):
                intra4, inter = [noise(rng, bd, w, h) for _ in range(4)], noise(rng, bd, w, h)
                sb.add(KIND_INTERINTRA, blend_a64(smooth_mask(w, h, mode), intra4[mode], inter), None, inter, intra4, wm)
                info.append(("mode", mode, wm))
        intra, inter = noise(rng, bd, w, h), noise(rng, bd, w, h)
        k = int(rng.integers(0, 16))
        sb.add(KIND_INTERINTRA, blend_a64(wedge_mask(w, h, k, 0), intra, inter), None, inter, [intra] * 4, 2)
        info.append(("wedge", k, 2))
        sb.add(KIND_INTERINTRA, inter, None, inter, [inter] * 4, 2)
        info.append(("equal", 0, 2))
    return sb, info


def search_batches():
    """name -> SearchBatch, every batch of the fixture"""
    out = {}
    for r in RANGES:
        out[f"planted_wedge_{r}"] = planted_wedge_batch(r)[0]
    for bd in (8, 10):
        out[f"planted_seg_{bd}"] = planted_seg_batch(bd)[0]
        out[f"ties_{bd}"] = ties_batch(bd)
        out[f"ii_{bd}"] = ii_batch(bd)[0]
        for mult in (0, 1, 4):
            out[f"gate_{bd}_{mult}"] = gate_batch(bd, mult)[0]
    return out


@functools.lru_cache(maxsize=None)
def search_restated(name):
    sb = search_batches()[name]
    res = [restate_search_job(sb.planes, sb.bit_depth, sb.mult, j) for j in sb.jobs]
    return np.array([r for r, _ in res], RESULT_DTYPE), [e for _, e in res]


def reference_outputs(sb, results):
    """the restatement's records in the lay-out of the fixture: kinds 0 / 1 (exit, wedge_index, wedge_sign, mask_type), with 0xFF / 0xEE where the
    reference leaves its field untouched; kind 2 (interintra_mode, use_wedge_interintra, wedge_index, 0)"""
    out = np.zeros((len(sb.jobs), 4), np.int32)
    for i, (j, r) in enumerate(zip(sb.jobs, results)):
        kind = int(j["kind"])
        if kind == KIND_INTERINTRA:
            out[i] = (r["interintra_mode"], r["use_wedge_interintra"], r["wedge_index"], 0)
        elif r["exit"]:
            out[i] = (1, 0xFF, 0xFF, 0xEE)
        elif kind == KIND_WEDGE:
            out[i] = (0, r["wedge_index"], r["wedge_sign"], 0xEE)
        else:
            out[i] = (0, 0xFF, 0xFF, r["mask_type"])
    return out


def spoil_search_desc(d, bad):
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith("bit_depth"):
        d.bit_depth = int(bad.rsplit("_", 1)[1])
    elif bad in ("use_rate", "use_rd_model"):
        setattr(d, bad, 1)
    elif bad == "zero_src_stride":
        d.src_stride = 0
    elif bad == "zero_pred1_samples":
        d.pred1_samples = 0
    elif bad == "pred0_zero_stride":
        d.pred0_stride = 0
    else:
        d.intra_samples = 0
    return d


def spoil_blend_desc(d, bad):
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith("bit_depth"):
        d.bit_depth = int(bad.rsplit("_", 1)[1])
    elif bad == "zero_inter_stride":
        d.inter_stride = 0
    elif bad == "zero_dst_samples":
        d.dst_samples = 0
    else:
        d.n_results, d.results = 3, None
    return d
