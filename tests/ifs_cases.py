"""The cases of the interpolation-filter search (svt_hip_ifs_batch) and a numpy restatement of what one job computes.

The reference's own results -- its static interpolation_filter_search driven job by job by tools/gen_ifs_golden.py -- are in golden/ifs.npz as
numbers only: the nine costs and SSEs of every job, its winner, rate and best cost, a CRC-32 of the winner's prediction and the whole prediction of
the blocks of up to 16 x 16 samples.  The planes, sources, tables and jobs are regenerated from seeds here.

Restated (Source/Lib): interpolation_filter_search and filter_sets (Codec/enc_inter_prediction.c:2424-2577), svt_av1_get_switchable_rate
(:2146-2165), model_rd_for_sb's plane 0 (:2266-2388), model_rd_from_sse, svt_av1_model_rd_from_var_lapndz and model_rd_norm (:2167-2264),
svt_psy_distortion / svt_psy_distortion_hbd and get_svt_psy_full_dist (Codec/psy_rd.c:64-293, the 10-bit functions with the 32-bit temporaries
of their butterflies), RDCOST (Codec/rd_cost.h:37-39).  The luma prediction of a pair is inter_pred_cases.restate_job's.

A batch is one launch: one depth, one set of the per-batch parameters, one rate table.  The source plane of a batch is laid out like its
destination (src_offset == dst_offset): every job has a source block of its own, planted from the restated prediction of one pair plus noise, so
that the case list decides which pair wins."""
import functools
import os
import zlib

import numpy as np

import inter_pred_cases as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ifs.npz")
FILTER_SETS = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]  # (y filter, x filter)
SKIPPED = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_XSQ_Q10 = 245727
M64 = (1 << 64) - 1
ST_OK, ST_UNDEFINED = 0, 0xFF
JOB_DTYPE = [("pred", ip.JOB_DTYPE), ("src_offset", "<u4"), ("pred_ctx", "u1", (2,)), ("reserved", "u1", (2,))]
RESULT_DTYPE = [("best_rd", "<u8"), ("interp_filters", "<u4"), ("switchable_rate", "<i4"), ("filter_x", "u1"), ("filter_y", "u1"), ("winner", "u1"),
                ("reserved", "u1", (5,))]
PARAMS = {"enable_dual_filter": 1, "subsampled_distortion": 0, "skip_sse_rd_model": 0, "spy_rd": 0, "quantizer": 400, "lambda_": 3000, "smooth_bias_pct": 0,
          "psy_rd": 0.0}

RATE_TAB_Q10 = [65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376, 3307, 3244, 3186,
                3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001, 1928, 1862, 1802, 1748, 1698, 1651,
                1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963, 911, 864, 821, 781, 745, 680, 623, 574, 530, 490, 455, 424, 395, 345, 304,
                269, 239, 213, 190, 171, 154, 126, 104, 87, 73, 61, 52, 44, 38, 28, 21, 16, 12, 10, 8, 6, 5, 3, 2, 1, 1, 1, 0, 0]
DIST_TAB_Q10 = [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 21, 24, 26, 29, 31, 34, 36, 39, 44, 49, 54, 59, 64, 69, 73, 78, 88,
                97, 106, 115, 124, 133, 142, 151, 167, 184, 200, 215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458, 495, 528, 559, 587, 613, 637,
                659, 680, 717, 749, 777, 801, 823, 842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994, 1001, 1006, 1010, 1013, 1015, 1017, 1018, 1020,
                1022, 1022, 1023, 1023, 1023, 1024]
XSQ_IQ_Q10 = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96, 112, 128, 144, 160, 176, 192, 208, 224, 256, 288, 320, 352, 384, 416, 448, 480, 544,
              608, 672, 736, 800, 864, 928, 992, 1120, 1248, 1376, 1504, 1632, 1760, 1888, 2016, 2272, 2528, 2784, 3040, 3296, 3552, 3808, 4064, 4576, 5088, 5600,
              6112, 6624, 7136, 7648, 8160, 9184, 10208, 11232, 12256, 13280, 14304, 15328, 16352, 18400, 20448, 22496, 24544, 26592, 28640, 30688, 32736, 36832,
              40928, 45024, 49120, 53216, 57312, 61408, 65504, 73696, 81888, 90080, 98272, 106464, 114656, 122848, 131040, 147424, 163808, 180192, 196576,
              212960, 229344, 245728]
MODEL_TABLES = np.array([RATE_TAB_Q10, DIST_TAB_Q10, XSQ_IQ_Q10], np.int32)


# ---- the psy energy ---------------------------------------------------------------------------------------------------------------------
def _tiles(a, n):
    """[tiles][n][n] of a view whose sides are multiples of n"""
    h, w = a.shape
    return a.reshape(h // n, n, w // n, n).swapaxes(1, 2).reshape(-1, n, n)


def _hadamard(t):
    """the unnormalised 2-D Hadamard transform of [tiles][n][n] (any order of the coefficients)"""
    n = t.shape[1]
    for axis in (1, 2):
        step = 1
        while step < n:
            t = np.moveaxis(t, axis, -1).reshape(t.shape[0], n, n // (2 * step), 2, step)
            t = np.stack([t[:, :, :, 0] + t[:, :, :, 1], t[:, :, :, 0] - t[:, :, :, 1]], 3).reshape(t.shape[0], n, n)
            t = np.moveaxis(t, -1, axis)
            step *= 2
    return t


_U = np.uint64
_LOW = _U(0xFFFFFFFF)


def _pack32(x0, x1):
    return (x0 + x1).astype(np.int64).astype(_U) + ((x0 - x1).astype(np.int64).astype(_U) << _U(32))


def _bfly_low(s0, s1, s2, s3):
    """HADAMARD4 on packed sums whose temporaries are 32 bits wide: only the low halves survive (svt_sa8d_8x8_hbd / svt_satd_4x4_hbd)"""
    t0, t1, t2, t3 = (s0 + s1) & _LOW, (s0 - s1) & _LOW, (s2 + s3) & _LOW, (s2 - s3) & _LOW
    return (t0 + t2) & _LOW, (t1 + t3) & _LOW, (t0 - t2) & _LOW, (t1 - t3) & _LOW


def _abs_halves(a):  # abs2_hbd
    m = (a >> _U(31)) & _U(0x100000001)
    s = (m << _U(32)) - m
    return (a + s) ^ s


def _fold(b):
    return (b & _LOW) + (b >> _U(32))


def tile_energies(view, bit_depth, n):
    """svt_sa8d_8x8 / svt_satd_4x4 (or the _hbd forms) minus (svt_psy_sad_nxn >> 2) against zero, per n x n tile of the view: int64 [tiles]"""
    t = _tiles(view.astype(np.int64), n)
    total = t.sum((1, 2))
    if bit_depth == 8:
        acc = np.abs(_hadamard(t)).sum((1, 2))
        had = (acc + 2) >> 2 if n == 8 else acc >> 1
    else:
        with np.errstate(over="ignore"):
            if n == 8:
                rows = [_bfly_low(_pack32(t[:, i, 0], t[:, i, 1]), _pack32(t[:, i, 2], t[:, i, 3]), _pack32(t[:, i, 4], t[:, i, 5]), _pack32(t[:, i, 6], t[:, i, 7]))
                        for i in range(8)]
                hs = np.zeros(len(t), _U)
                for i in range(4):
                    a = _bfly_low(*[rows[r][i] for r in range(4)]) + _bfly_low(*[rows[r][i] for r in range(4, 8)])
                    b = np.zeros(len(t), _U)
                    for k in range(4):
                        b = b + _abs_halves(a[k] + a[k + 4]) + _abs_halves(a[k] - a[k + 4])
                    hs = hs + _fold(b)
                had = ((hs + _U(2)) >> _U(2)).astype(np.int64)
            else:
                rows = []
                for i in range(4):
                    b0, b1 = _pack32(t[:, i, 0], t[:, i, 1]), _pack32(t[:, i, 2], t[:, i, 3])
                    rows.append((b0 + b1, b0 - b1))
                hs = np.zeros(len(t), _U)
                for i in range(2):
                    a = _bfly_low(*[rows[r][i] for r in range(4)])
                    hs = hs + _fold(_abs_halves(a[0]) + _abs_halves(a[1]) + _abs_halves(a[2]) + _abs_halves(a[3]))
                had = (hs >> _U(1)).astype(np.int64)
    e = had - (total >> 2)
    return ((e + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # int32_t input_nrg / recon_nrg


def psy_distortion(src, rec, bit_depth):
    """svt_psy_distortion / svt_psy_distortion_hbd on two views of one size"""
    h, w = src.shape
    n = 8 if w >= 8 and h >= 8 else 4
    total = int(np.abs(tile_energies(src, bit_depth, n) - tile_energies(rec, bit_depth, n)).sum())
    return total >> 1 if bit_depth == 8 else total << 2


# ---- the model and the cost -------------------------------------------------------------------------------------------------------------
def model_rd_from_sse(w, h, quantizer, bit_depth, sse, ev=None):
    """model_rd_from_sse with simple_model_rd_from_var = 0: (rate, dist), dist after the << 4"""
    n_log2 = (w * h).bit_length() - 1  # num_pels_log2_lookup
    qstep = quantizer >> (bit_depth - 5)
    var = sse
    if var == 0:
        if ev is not None:
            ev["var0"] = True
        return 0, 0
    xsq64 = (((qstep * qstep) << (n_log2 + 10)) + (var >> 1)) // var
    if ev is not None and xsq64 > MAX_XSQ_Q10:
        ev["xsq_clamp"] = True
    xsq = min(xsq64, MAX_XSQ_Q10)
    tmp = (xsq >> 2) + 8
    k = tmp.bit_length() - 1 - 3
    xq = (k << 3) + ((tmp >> k) & 7)
    a = ((xsq - XSQ_IQ_Q10[xq]) << 10) >> (2 + k)
    b = 1024 - a
    r_q10 = (RATE_TAB_Q10[xq] * b + RATE_TAB_Q10[xq + 1] * a) >> 10
    d_q10 = (DIST_TAB_Q10[xq] * b + DIST_TAB_Q10[xq + 1] * a) >> 10
    return ((r_q10 << n_log2) + 1) >> 1, ((var * d_q10 + 512) >> 10) << 4


def switchable_rate(fac_bits, pred_ctx, yf, xf, dual):
    rs = int(fac_bits[int(pred_ctx[0])][yf])
    return rs + int(fac_bits[int(pred_ctx[1])][xf]) if dual else rs


def biased(rd, yf, xf, params):
    if params["smooth_bias_pct"] and (yf == 1 or xf == 1):
        rd = ((rd * params["smooth_bias_pct"]) & M64) // 100
    if params["spy_rd"]:
        if yf == 2 or xf == 2:
            rd = ((rd * 75) & M64) // 100
        if yf == 0 or xf == 0:
            rd = ((rd * 80) & M64) // 100
    return rd


def pair_prediction(planes, bit_depth, job, pair, mv_array=None):
    """the luma prediction of filter_sets[pair]: (block, events of inter_pred_cases.restate_job)"""
    j = job["pred"].copy()
    j["filter_y"], j["filter_x"] = FILTER_SETS[pair]
    return ip.restate_job(planes, bit_depth, 0, j, mv_array)


def job_defined(job, n_refs, mv_array, src_samples, src_stride, dst_samples=None, dst_stride=0):
    j = job["pred"].copy()
    j["filter_x"] = j["filter_y"] = 0
    w, h = int(j["width"]), int(j["height"])
    if dst_samples is None:  # dst == NULL: the destination is not checked
        dst_samples, dst_stride = 1 << 62, 0
    ok = ip.job_defined(j, n_refs, mv_array, dst_samples, dst_stride) and int(job["pred_ctx"][0]) < 16 and int(job["pred_ctx"][1]) < 16
    return bool(ok and int(job["src_offset"]) + (h - 1) * src_stride + w <= src_samples)


def restate_job(planes, src, bit_depth, job, params, fac_bits, mv_array=None):
    """One job.  src: the source plane [rows][stride].  Returns a dict: rd, sse (uint64 [9], SKIPPED for a skipped pair), unbiased (the costs before
    the biases, python ints or None), winner, switchable_rate, best_rd, interp_filters, pred (the winner's block), events."""
    w, h = int(job["pred"]["width"]), int(job["pred"]["height"])
    y0, x0 = divmod(int(job["src_offset"]), src.shape[1])
    shift = 1 if params["subsampled_distortion"] and h > 16 else 0
    s_view = src[y0:y0 + h:1 << shift, x0:x0 + w].astype(np.int64)
    dual = bool(params["enable_dual_filter"])
    ev = {"var0": False, "xsq_clamp": False, "inside": True, "variants": None}
    rd, sse_out, unbiased, preds = np.full(9, SKIPPED, np.uint64), np.full(9, SKIPPED, np.uint64), [None] * 9, {}
    best, winner, best_rs = M64, 0, 0
    for i, (yf, xf) in enumerate(FILTER_SETS):
        if not dual and yf != xf:
            continue
        rs = switchable_rate(fac_bits, job["pred_ctx"], yf, xf, dual)
        blk, pev = pair_prediction(planes, bit_depth, job, i, mv_array)
        ev["inside"], ev["variants"] = ev["inside"] and pev["inside"], tuple(v for v, _ in pev["refs"])
        preds[i] = blk
        p_view = blk[::1 << shift].astype(np.int64)
        sse = int(((s_view - p_view) ** 2).sum()) << shift
        if params["psy_rd"] > 0:
            # get_svt_psy_full_dist: (uint64_t)(dist * psy_rd), one double multiply
            sse += int(float(psy_distortion(s_view, p_view, bit_depth)) * float(params["psy_rd"])) << shift
        if params["skip_sse_rd_model"]:
            rate, dist = 0, sse * 10
        else:
            n = 2 * (bit_depth - 8)
            rate, dist = model_rd_from_sse(w, h, params["quantizer"], bit_depth, (sse + ((1 << n) >> 1)) >> n, ev)
        cost = ((((rs + rate) * params["lambda_"] + 256) >> 9) + dist * 128) & M64
        unbiased[i] = cost
        cost = biased(cost, yf, xf, params)
        rd[i], sse_out[i] = cost, sse
        if cost < best:
            best, winner, best_rs = cost, i, rs
    yf, xf = FILTER_SETS[winner]
    return {"rd": rd, "sse": sse_out, "unbiased": unbiased, "winner": winner, "switchable_rate": best_rs, "best_rd": best, "interp_filters": yf | (xf << 16),
            "filter_x": xf, "filter_y": yf, "pred": preds[winner], "events": ev}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype="<u2").tobytes())


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
NOISE2 = [("noise", 0), ("noise", 1)]
EDGE_PAD = 8  # the padding of the planes of the edge batches: a block pushed out of the picture reads past it, so the coordinate clamp works


@functools.lru_cache(maxsize=None)
def edge_plane(bit_depth, index):
    a = np.random.default_rng([20261020, bit_depth, index]).integers(0, 1 << bit_depth, (ip.PIC_H + 2 * EDGE_PAD, ip.PIC_W + 2 * EDGE_PAD))
    a = a.astype(np.uint16 if bit_depth > 8 else np.uint8)
    a.setflags(write=False)
    return a


def batch_planes(b):
    if b["edge_planes"]:
        return [(edge_plane(b["bit_depth"], k), EDGE_PAD, EDGE_PAD) for k in range(2)]
    return [(ip.plane(kind, b["bit_depth"], 0, idx), ip.PAD, ip.PAD) for kind, idx in NOISE2]


def fac_table(kind):
    """switchable_interp_fac_bitss, int32 [16][3]: random costs, all equal, or the rows the bias cases name by context"""
    if kind == "flat":
        return np.full((16, 3), 700, np.int32)
    t = np.random.default_rng([5, 1]).integers(100, 1500, (16, 3)).astype(np.int32)
    if kind == "bias":
        t[0] = t[8] = [1000, 900, 2000]    # both neighbours regular / regular
        t[1] = t[9] = [3000, 1000, 1200]   # smooth / smooth
        t[2] = t[10] = [1200, 1000, 3000]  # sharp / sharp
        t[3], t[11] = [1000, 950, 3000], [3000, 950, 1000]  # no neighbour: dir 0, dir 1
    return t


def pred_context(comp, direction, left, above):
    """svt_aom_get_pred_context_switchable_interp (Codec/entropy_coding.c:1563-1604).  left / above: the neighbour's (y filter, x filter) when it is
    available and uses the candidate's first reference frame, else None"""
    lt, at = [3 if n is None else int(n[direction]) for n in (left, above)]
    both = lt if lt == at else (at if lt == 3 else (lt if at == 3 else 3))
    return (4 if comp else 0) + 8 * direction + both


def spec(w, h, variants, target=0, noise=2, mode=0, nbr=None, org=None, mvs=None, from_array=False, plant="noise"):
    return {"w": w, "h": h, "variants": variants, "target": target, "noise": noise, "mode": mode, "nbr": nbr, "org": org, "mvs": mvs, "from_array": from_array,
            "plant": plant}


SIZES = [(4, 4), (4, 16), (16, 4), (8, 8), (8, 32), (16, 64), (16, 16), (32, 32)]


def batch_specs(name):
    """(bit depth, parameters, table kind, edge planes, job specs) of a batch"""
    kind, bd = name.rsplit("_", 1)
    bd = int(bd)
    p, table, edge, specs = dict(PARAMS), "random", False, []
    if bd == 10:
        p["quantizer"], p["lambda_"] = 1600, 3000  # 10-bit dequant steps are four times the 8-bit ones; full_lambda_divided is already divided
    if kind == "main":  # every size x every combination of phases, psy and the model on, subsampled distortion on; the target pair cycles
        p["psy_rd"], p["subsampled_distortion"] = 1.35, 1
        k = 0
        for w, h in SIZES:
            for v in range(4):
                specs.append(spec(w, h, (v,), target=k % 9))
                k += 1
        specs += [spec(16, 16, (3, 1), 5, mode=1), spec(16, 16, (2, 3), 7, mode=2), spec(8, 8, (0, 3), 3, mode=1), spec(16, 16, (1, 2), 2, mode=2),
                  spec(8, 8, (3, 3), 6, mode=2), spec(32, 32, (0, 0), 4, mode=1), spec(16, 16, (3,), 8, from_array=True),
                  spec(8, 8, (3, 2), 1, mode=1, from_array=True)]
    elif kind == "big":  # 64x64 and 128x128: one job each, and one compound
        p["psy_rd"], p["subsampled_distortion"] = 0.75, 1
        specs = [spec(64, 64, (3,), 5), spec(128, 128, (3,), 7), spec(64, 64, (3, 1), 2, mode=1)]
    elif kind == "nodual":  # equal pairs only
        p["enable_dual_filter"], p["psy_rd"] = 0, 1.0
        specs = [spec(w, h, (v,), target=4 * ((i + v) % 3)) for i, (w, h) in enumerate([(8, 8), (16, 16), (32, 32), (4, 4), (16, 64)]) for v in range(4)]
    elif kind == "skipmodel":  # dist = sse * 10, no psy, the full rows of a high block
        p["skip_sse_rd_model"] = 1
        specs = [spec(w, h, (v,), target=(2 * i + v) % 9) for i, (w, h) in enumerate([(8, 32), (16, 64), (16, 16), (4, 4), (32, 32)]) for v in (3, 1, 2)]
    elif kind == "exact":  # sse == 0 on the planted pair, a single sample off by one against a large quantizer, ties on integer MVs
        p["quantizer"], table = 32767, "flat"
        specs = [spec(w, h, (v,), target=(i + v) % 9, plant=pl) for i, (w, h) in enumerate([(8, 8), (16, 16), (4, 4)]) for v in (3, 0) for pl in ("exact", "one")]
        specs += [spec(16, 16, (0, 0), 0, mode=1, plant="exact"), spec(32, 32, (0,), 0, noise=9)]
    elif kind == "smooth":  # the smooth bias alone
        p["smooth_bias_pct"], table = 130, "bias"
        specs = [spec(16, 16, (0,), 0, plant="exact", nbr=((0, 0), (0, 0))), spec(8, 8, (0,), 0, plant="exact", nbr=((0, 0), (0, 0)))]
        specs += [spec(16, 16, (3,), t, noise=40) for t in (1, 4, 3)]
    elif kind == "spy":  # the spy-rd biases: sharp alone, regular alone, both on one pair (rows of fac_table("bias"))
        p["spy_rd"], p["psy_rd"], table = 1, 0.9, "bias"
        specs = [spec(16, 16, (0,), 0, plant="exact", nbr=((1, 1), (1, 1))), spec(16, 16, (0,), 0, plant="exact", nbr=((2, 2), (2, 2))), spec(16, 16, (0,), 0, plant="exact", nbr=(None, None))]
        specs += [spec(16, 16, (3,), t, noise=40) for t in (4, 8, 0)]
    elif kind == "edges":  # blocks at the corners of the picture with MVs far outside: the MV clamp, and the window clamped at each plane edge
        p["psy_rd"], edge = 1.0, True
        far = 1900
        for w, h in ((16, 16), (8, 8)):
            for org, mv in (((0, 32), (3, -far)), ((ip.PIC_W - w, 32), (-5, far)), ((48, 0), (-far, 3)), ((48, ip.PIC_H - h), (far, -5)),
                            ((0, 0), (-far + 1, -far + 2)), ((ip.PIC_W - w, ip.PIC_H - h), (far - 1, far - 3))):
                specs.append(spec(w, h, None, target=len(specs) % 9, org=org, mvs=[mv]))
        specs.append(spec(16, 16, None, 4, mode=1, org=(0, 0), mvs=[(-far, -far), (far, far)]))
    else:
        raise KeyError(name)
    return bd, p, table, edge, specs


@functools.lru_cache(maxsize=None)
def batch_names():
    return tuple(f"{k}_{bd}" for bd in (8, 10) for k in ("main", "big", "nodual", "skipmodel", "exact", "smooth", "spy", "edges"))


@functools.lru_cache(maxsize=None)
def batch(name):
    """{"bit_depth", "params", "fac_bits", "jobs", "mv_array", "src", "dst_shape", "dst_stride", "edge_planes", "specs", "nbrs": per job the scripted
    (left, above) neighbours behind pred_ctx}; src is laid out like dst"""
    bd, params, table, edge, specs = batch_specs(name)
    rng = np.random.default_rng([9, zlib.crc32(name.encode())])
    mv_array = rng.integers(-90, 91, (6, 2)).astype(np.int16)
    pjobs = []
    for s in specs:
        refs, cm, off = ip.mode_fields(rng, s["mode"])
        n = 2 if s["mode"] else 1
        mvs = s["mvs"] or [ip.random_mv(rng, 0, s["variants"][k % len(s["variants"])]) for k in range(n)]
        j = ip.make_job(0, s["w"], s["h"], s["org"] or ip.random_org(rng, 0, s["w"], s["h"]), mvs, (3, 3), refs, cm, off)  # the filters are ignored
        if s["from_array"]:
            for k in range(n):
                mv_array[k + 1] = mvs[k]
                j["mv"][k] = (77, -77)
                j["mv_index"][k] = k + 1
            j["flags"] = ip.MV0_FROM_ARRAY | (ip.MV1_FROM_ARRAY if n == 2 else 0)
        pjobs.append(j)
    pjobs, rows = ip.pack(pjobs, 256)
    jobs = np.zeros(len(pjobs), JOB_DTYPE)
    jobs["pred"], jobs["src_offset"] = pjobs, pjobs["dst_offset"]
    b = {"name": name, "bit_depth": bd, "params": params, "fac_bits": fac_table(table), "mv_array": mv_array, "dst_shape": (rows, 256), "dst_stride": 256,
         "edge_planes": edge, "specs": specs, "nbrs": []}
    planes, mx = batch_planes(b), (1 << bd) - 1
    src = rng.integers(0, mx + 1, (rows, 256)).astype(np.int64)
    for j, s in zip(jobs, specs):
        nbr = s["nbr"] if s["nbr"] is not None else tuple(None if rng.integers(0, 4) == 0 else (int(rng.integers(0, 3)), int(rng.integers(0, 3))) for _ in range(2))
        b["nbrs"].append(nbr)
        j["pred_ctx"] = [pred_context(s["mode"] != 0, d, nbr[0], nbr[1]) for d in (0, 1)]
        blk = pair_prediction(planes, bd, j, s["target"], mv_array)[0].astype(np.int64)
        if s["plant"] == "noise":
            blk = blk + rng.integers(-s["noise"], s["noise"] + 1, blk.shape)
        elif s["plant"] == "one":
            blk[1, 2] += 1 if blk[1, 2] < mx else -1
        y, x = divmod(int(j["src_offset"]), 256)
        src[y:y + s["h"], x:x + s["w"]] = np.clip(blk, 0, mx)
    b["jobs"], b["src"] = jobs, src.astype(np.uint16 if bd > 8 else np.uint8)
    b["src"].setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's results of a batch, job by job"""
    b = batch(name)
    planes = batch_planes(b)
    return [restate_job(planes, b["src"], b["bit_depth"], j, b["params"], b["fac_bits"], b["mv_array"]) for j in b["jobs"]]


def fixture_arrays(name, results):
    """what the fixture holds of a batch, from results laid out as restated()'s"""
    b = batch(name)
    out = {f"{name}_rd": np.array([r["rd"] for r in results], np.uint64), f"{name}_sse": np.array([r["sse"] for r in results], np.uint64),
           f"{name}_pick": np.array([[r["winner"], r["switchable_rate"], r["interp_filters"]] for r in results], np.int64),
           f"{name}_best": np.array([r["best_rd"] for r in results], np.uint64), f"{name}_crc": np.array([crc(r["pred"]) for r in results], np.uint32)}
    small = [np.asarray(r["pred"], np.uint16).reshape(-1) for r, j in zip(results, b["jobs"]) if int(j["pred"]["width"]) * int(j["pred"]["height"]) <= 256]
    out[f"{name}_small"] = np.concatenate(small) if small else np.zeros(0, np.uint16)
    return out


def expected_outputs(name, results, fill, with_dst=True):
    """(results records, rd, sse, dst image) a launch of the batch leaves behind, every byte the jobs do not write being `fill`"""
    b = batch(name)
    n = len(results)
    rec = np.frombuffer(bytes([fill]) * (n * np.dtype(RESULT_DTYPE).itemsize), RESULT_DTYPE).copy()
    for i, r in enumerate(results):
        rec[i] = np.zeros((), RESULT_DTYPE)
        for k in ("best_rd", "interp_filters", "switchable_rate", "filter_x", "filter_y", "winner"):
            rec[i][k] = r[k]
    img = None
    if with_dst:
        img = ip.expected_image({"bit_depth": b["bit_depth"], "dst_shape": b["dst_shape"], "dst_stride": b["dst_stride"], "jobs": b["jobs"]["pred"]},
                                [r["pred"] for r in results], fill)
    return rec, np.array([r["rd"] for r in results], np.uint64), np.array([r["sse"] for r in results], np.uint64), img


def coverage_missing():
    """The conditions of the fixture that are not met, as text (on the restatement, which the generator found equal to the reference)."""
    won_dual, won_single, variants, missing = set(), set(), set(), []
    tie = var0 = clamp = False
    flips = {"smooth": False, "sharp": False, "regular": False, "both": False}
    for name in batch_names():
        b = batch(name)
        for j, s, r in zip(b["jobs"], b["specs"], restated(name)):
            (won_dual if b["params"]["enable_dual_filter"] else won_single).add(r["winner"])
            variants.add(r["events"]["variants"])
            var0, clamp = var0 or r["events"]["var0"], clamp or r["events"]["xsq_clamp"]
            costs = [int(v) for v in r["rd"]]
            if b["params"]["enable_dual_filter"] and len(set(costs)) == 1 and set(r["events"]["variants"]) == {0} and len(set(b["fac_bits"].reshape(-1))) == 1:
                tie = tie or r["winner"] == 0
                if r["winner"] != 0:
                    missing.append(f"{name}: a job whose nine costs are equal did not pick pair 0")
            plain = min(range(9), key=lambda i: (r["unbiased"][i] is None, r["unbiased"][i] or 0, i))
            if plain != r["winner"]:
                yf, xf = FILTER_SETS[r["winner"]]
                if b["params"]["smooth_bias_pct"] and 1 in FILTER_SETS[plain]:
                    flips["smooth"] = True
                if b["params"]["spy_rd"]:
                    kind = "both" if {yf, xf} == {0, 2} else ("sharp" if 2 in (yf, xf) and 0 not in (yf, xf) else ("regular" if 0 in (yf, xf) and 2 not in (yf, xf) else None))
                    if kind:
                        flips[kind] = True
    missing += [f"pair {i} never won with the dual filter on" for i in range(9) if i not in won_dual]
    missing += [f"pair {i} never won with the dual filter off" for i in (0, 4, 8) if i not in won_single]
    if won_single - {0, 4, 8}:
        missing.append("an unequal pair won with the dual filter off")
    missing += [f"no single-reference job of variant {ip.VARIANTS[v]}" for v in range(4) if (v,) not in variants]
    if not any(len(v) == 2 and v[0] != v[1] for v in variants):
        missing.append("no compound whose references take different variants")
    missing += [text for ok, text in ((tie, "no tie of all nine costs"), (var0, "no job with sse == 0"), (clamp, "no job at the MAX_XSQ_Q10 clamp")) if not ok]
    missing += [f"no job on which the {k} bias flips the winner" for k, v in flips.items() if not v]
    return missing


def undefined_batch(bd):
    """the main batch's first jobs with one undefined job of every kind among them: (batch, indices of the undefined jobs)"""
    b = dict(batch(f"main_{bd}"))
    jobs, bad = [], []
    kinds = ["ref0", "ref1", "size", "mv_index0", "mv_index1", "comp_mode", "offsets", "dst_end", "src_end", "pred_ctx0", "pred_ctx1"]
    base = b["jobs"][32].copy()  # a compound 16x16
    assert int(base["pred"]["ref"][1]) != ip.NO_REF and int(base["pred"]["width"]) == 16
    for i, kind in enumerate(kinds):
        jobs.append(b["jobs"][3 * i + 1].copy())
        j = base.copy()
        if kind == "ref0":
            j["pred"]["ref"][0] = 2
        elif kind == "ref1":
            j["pred"]["ref"][1] = 7
        elif kind == "size":
            j["pred"]["width"] = 12
        elif kind == "mv_index0":
            j["pred"]["flags"], j["pred"]["mv_index"][0] = ip.MV0_FROM_ARRAY, 6
        elif kind == "mv_index1":
            j["pred"]["flags"], j["pred"]["mv_index"] = ip.MV0_FROM_ARRAY | ip.MV1_FROM_ARRAY, (4, 0xFFFFFFFF)
        elif kind == "comp_mode":
            j["pred"]["comp_mode"] = 2
        elif kind == "offsets":
            j["pred"]["comp_mode"], j["pred"]["fwd_offset"], j["pred"]["bck_offset"] = 1, 8, 8
        elif kind == "dst_end":
            j["pred"]["dst_offset"] = b["dst_shape"][0] * 256 - 15 * 256 - 16 + 1  # one sample too far
        elif kind == "src_end":
            j["src_offset"] = b["dst_shape"][0] * 256 - 15 * 256 - 16 + 1
        elif kind == "pred_ctx0":
            j["pred_ctx"][0] = 16
        else:
            j["pred_ctx"][1] = 255
        bad.append(len(jobs))
        jobs.append(j)
    b["jobs"] = np.array(jobs, JOB_DTYPE)
    return b, bad


def spoil_desc(d, bad):
    """a valid abi.IfsDesc made invalid in the way `bad` names"""
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad == "bit_depth_12":
        d.bit_depth = 12
    elif bad in ("n_refs_0", "n_refs_9"):
        d.n_refs = int(bad[-1])
    elif bad == "null_plane":
        d.refs[1].plane = None
    elif bad == "zero_stride":
        d.refs[1].stride = 0
    elif bad == "stride_below_width":
        d.refs[0].stride = 500
    elif bad == "org_outside":
        d.refs[1].org_y = 448
    elif bad == "zero_src_stride":
        d.src_stride = 0
    elif bad == "zero_src_samples":
        d.src_samples = 0
    elif bad == "zero_dst_stride":
        d.dst_stride = 0
    elif bad == "zero_dst_samples":
        d.dst_samples = 0
    elif bad == "n_mvs_without_array":
        d.mv_array, d.n_mvs = None, 3
    elif bad == "quantizer_0":
        d.quantizer = 0
    elif bad == "quantizer_32768":
        d.quantizer = 32768
    elif bad == "smooth_bias_1001":
        d.smooth_bias_pct = 1001
    else:
        raise KeyError(bad)
    return d


SPOILS = ["no_src", "no_jobs", "no_results", "no_status", "no_switchable_interp_fac_bits", "bit_depth_12", "n_refs_0", "n_refs_9", "null_plane", "zero_stride",
          "stride_below_width", "org_outside", "zero_src_stride", "zero_src_samples", "zero_dst_stride", "zero_dst_samples", "n_mvs_without_array", "quantizer_0",
          "quantizer_32768", "smooth_bias_1001"]
