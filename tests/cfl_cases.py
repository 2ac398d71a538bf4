"""Chroma-from-luma: the numpy restatement of svt_hip_cfl_pred_batch and svt_hip_cfl_pick_alpha_batch (include/svt_hip_cfl.h) and the case
generator shared by tests/test_cfl.py, tests/test_cfl_gpu.py, tests/test_cfl_chain_gpu.py and tools/gen_cfl_golden.py.

Prediction (Source/Lib of the reference): svt_cfl_luma_subsampling_420_{lbd,hbd}_c and svt_subtract_average_c (Codec/intra_prediction.c:420-465),
svt_cfl_predict_{lbd,hbd}_c (C_DEFAULT/cfl_c.c), as compute_cfl_ac_components and av1_cost_calc_cfl chain them
(Codec/product_coding_loop.c:3751-3786, 3453-3617).  Alpha search: md_cfl_rd_pick_alpha (:3624-3748) replayed over a complete cost table.

A batch is a mapping: name, bit_depth, width, height (of the chroma block), alphas, luma (the plane), luma_size (what the kernel is told), dc
(the two DC planes, one stride), jobs (JOB_DTYPE), dst_samples, dst_stride, slot_stride, kinds (what each job's luma block holds)."""
import functools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfl.npz")
JOB_DTYPE = [("luma_x", "<i4"), ("luma_y", "<i4"), ("dc_offset", "<u4", (2,)), ("dst_offset", "<u4", (2,))]
ST_OK, ST_UNDEFINED = 0, 0xFF
SLOTS = 33
ALPHAS_FULL = list(range(-16, 17))
SIDES = (4, 8, 16, 32)
SIZES = [(w, h) for w in SIDES for h in SIDES]
MAX_MODE_COST = 13754408443200 * 8
PICK_TRUNCATED, PICK_UNDEFINED = 1, 0xFF
U64_MAX = (1 << 64) - 1
SAMPLE_ALPHAS = (-16, 5, 16)  # of the full list, kept sample by sample in the fixture


def jobs_per_wave(w, h):
    return max(1, 64 // (w * h // 4))


# ---- the prediction ----
def restate_job(luma, bd, w, h, lx, ly, dc_blocks, alphas):
    """one job: (pred [2][n_alpha][h][w] uint16, ac [h][w] int16, events)"""
    mx = (1 << bd) - 1
    blk = luma[ly:ly + 2 * h, lx:lx + 2 * w].astype(np.int32)
    assert blk.shape == (2 * h, 2 * w), "the luma extent leaves the plane"
    q3 = (blk[0::2, 0::2] + blk[0::2, 1::2] + blk[1::2, 0::2] + blk[1::2, 1::2]) << 1  # svt_cfl_luma_subsampling_420_*_c
    total = int(q3.sum())
    avg = np.int16((total + ((w * h) >> 1)) >> (w * h).bit_length() - 1)  # svt_subtract_average_c
    ac = (q3 - np.int32(avg)).astype(np.int16)
    a32 = ac.astype(np.int32)
    pred = np.zeros((2, len(alphas), h, w), np.uint16)
    ev = {"clip0": False, "clipmax": False, "tie_pos": False, "tie_neg": False, "sum_rem": total % (w * h), "round_rem": (total + ((w * h) >> 1)) % (w * h),
          "ac_zero": not ac.any(), "ac_max": int(np.abs(a32).max())}
    for k, alpha in enumerate(alphas):
        t = int(alpha) * a32
        scaled = np.where(t < 0, -((-t + 32) >> 6), (t + 32) >> 6)  # ROUND_POWER_OF_TWO_SIGNED(alpha_q3 * ac, 6)
        ev["tie_pos"] |= bool(np.any((t > 0) & (t % 64 == 32)))
        ev["tie_neg"] |= bool(np.any((t < 0) & ((-t) % 64 == 32)))
        for p in range(2):
            v = scaled + dc_blocks[p].astype(np.int32)
            ev["clip0"] |= bool(np.any(v < 0))
            ev["clipmax"] |= bool(np.any(v > mx))
            pred[p, k] = np.clip(v, 0, mx)
    return pred, ac, ev


def job_defined(b, j):
    """the kernel's rule (include/svt_hip_cfl.h): the luma extent inside the luma plane, both DC blocks inside their planes, every slot inside
    its destination"""
    w, h = b["width"], b["height"]
    lw, lh = b["luma_size"]
    ok = int(j["luma_x"]) >= 0 and int(j["luma_y"]) >= 0 and int(j["luma_x"]) + 2 * w <= lw and int(j["luma_y"]) + 2 * h <= lh
    for p in range(2):
        ok = ok and int(j["dc_offset"][p]) + (h - 1) * b["dc"][p].shape[1] + w <= b["dc"][p].size
        ok = ok and int(j["dst_offset"][p]) + (len(b["alphas"]) - 1) * b["slot_stride"] + (h - 1) * b["dst_stride"] + w <= b["dst_samples"]
    return ok


def dc_block(b, j, p):
    w, h, s = b["width"], b["height"], b["dc"][p].shape[1]
    off = int(j["dc_offset"][p])
    flat = b["dc"][p].reshape(-1)
    return np.stack([flat[off + r * s:off + r * s + w] for r in range(h)])


def restate_batch(b, defined=None):
    """(preds, acs, events) per job; an undefined job gives None three times"""
    out = []
    for i, j in enumerate(b["jobs"]):
        if defined is not None and not defined[i]:
            out.append((None, None, None))
            continue
        out.append(restate_job(b["luma"], b["bit_depth"], b["width"], b["height"], int(j["luma_x"]), int(j["luma_y"]), [dc_block(b, j, 0), dc_block(b, j, 1)],
                               b["alphas"]))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


@functools.lru_cache(maxsize=None)
def restated(name):
    return restate_batch(batch(name))


def fill_sample(bd, fill):
    return fill * 0x0101 if bd > 8 else fill


def expected_dst(b, preds, fill, guard=0):
    """the two destinations (with their guard bands) as the batch leaves them: `fill` bytes wherever no defined job writes"""
    dt = np.uint16 if b["bit_depth"] > 8 else np.uint8
    w, h = b["width"], b["height"]
    out = [np.full(b["dst_samples"] + 2 * guard, fill_sample(b["bit_depth"], fill), dt) for _ in range(2)]
    for j, pr in zip(b["jobs"], preds):
        if pr is None:
            continue
        for p in range(2):
            for k in range(len(b["alphas"])):
                at = guard + int(j["dst_offset"][p]) + k * b["slot_stride"]
                for r in range(h):
                    out[p][at + r * b["dst_stride"]:at + r * b["dst_stride"] + w] = pr[p, k, r]
    return out


def blocks_of(b, dst, j, guard=0):
    """[2][n_alpha][h][w] of job j from the two destinations"""
    w, h = b["width"], b["height"]
    out = np.zeros((2, len(b["alphas"]), h, w), np.uint16)
    for p in range(2):
        for k in range(len(b["alphas"])):
            at = guard + int(j["dst_offset"][p]) + k * b["slot_stride"]
            for r in range(h):
                out[p, k, r] = dst[p][at + r * b["dst_stride"]:at + r * b["dst_stride"] + w]
    return out


def job_crc(pred, ac):
    return zlib.crc32(np.ascontiguousarray(ac, "<i2").tobytes(), zlib.crc32(np.ascontiguousarray(pred, "<u2").tobytes()))


def batch_crcs(preds, acs):
    return np.array([job_crc(p, a) for p, a in zip(preds, acs)], np.uint32)


# ---- the luma a job sits on ----
KINDS = ("noise", "zero", "max", "checker", "rows", "half", "checker1", "smooth")
EXTREME_KINDS = ("zero", "max", "checker", "rows", "half", "checker1")


def luma_block(kind, bd, w, h, rng):
    """the 2w x 2h luma samples of one job"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:2 * h, 0:2 * w]
    if kind == "noise":
        return rng.integers(0, mx + 1, (2 * h, 2 * w))
    if kind == "zero":
        return np.zeros((2 * h, 2 * w), np.int64)
    if kind == "max":
        return np.full((2 * h, 2 * w), mx)
    if kind == "checker":  # a checkerboard of 2x2 cells: neighbouring chroma samples see 0 and 8 * max
        return (((xx >> 1) + (yy >> 1)) & 1) * mx
    if kind == "rows":  # chroma rows alternate 0 / 8 * max: the largest |AC| (4 * max) in every sample
        return ((yy >> 1) & 1) * mx
    if kind == "checker1":  # a checkerboard of single samples: every 2x2 sums to 2 * max, the AC is zero
        return ((xx + yy) & 1) * mx
    if kind == "half":  # flat plus one on w * h / 4 samples: the sum is (8 * v) * w * h + w * h / 2, the average's remainder exactly one half
        blk = np.full((2 * h, 2 * w), int(rng.integers(1, mx)))
        blk.reshape(-1)[:w * h // 4] += 1
        return blk
    # smooth: a gradient with a little noise, what a reconstruction looks like
    return np.clip(mx * (xx * 3 + yy * 5) // (6 * w + 10 * h) + rng.integers(-3, 4, (2 * h, 2 * w)), 0, mx)


def make_batch(name, bd, w, h, alphas, kinds, cols, seed, dense=False, luma_pad=(0, 0), shift=(0, 0), dst_shift=0, dc_shift=0, dc_kinds=None):
    """jobs on a grid of `cols` cells per row, the last job in the grid's last cell.  luma_pad: columns / rows of the array behind the grid;
    shift: the grid's origin in the luma plane; dense: slots of w * h samples back to back (else every slot is a whole chroma picture);
    dst_shift / dc_shift: samples in front of the first block."""
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bd > 8 else np.uint8
    mx = (1 << bd) - 1
    n = len(kinds)
    rows = (n + cols - 1) // cols
    cells = list(range(n - 1)) + [rows * cols - 1]
    luma = rng.integers(0, mx + 1, (rows * 2 * h + shift[1] + luma_pad[1], cols * 2 * w + shift[0] + luma_pad[0])).astype(dt)
    cw, ch = cols * w + dc_shift, rows * h
    dc = [rng.integers(0, mx + 1, (ch + (1 if dc_shift else 0), cw)).astype(dt) for _ in range(2)]
    jobs = np.zeros(n, JOB_DTYPE)
    n_alpha = len(alphas)
    if dense:
        dst_stride, slot_stride = w + (1 if dst_shift else 0), (w + (1 if dst_shift else 0)) * h
        dst_samples = dst_shift + n * n_alpha * slot_stride
    else:
        dst_stride, slot_stride = cols * w, rows * h * cols * w
        dst_samples = dst_shift + n_alpha * slot_stride
    for i, (kind, cell) in enumerate(zip(kinds, cells)):
        cx, cy = cell % cols, cell // cols
        lx, ly = shift[0] + cx * 2 * w, shift[1] + cy * 2 * h
        luma[ly:ly + 2 * h, lx:lx + 2 * w] = luma_block(kind, bd, w, h, rng)
        dk = dc_kinds[i] if dc_kinds else ("noise", "noise")
        for p in range(2):
            if dk[p] != "noise":
                dc[p][cy * h:cy * h + h, dc_shift + cx * w:dc_shift + cx * w + w] = {"zero": 0, "max": mx, "low": 3, "high": mx - 3}[dk[p]]
        jobs[i]["luma_x"], jobs[i]["luma_y"] = lx, ly
        jobs[i]["dc_offset"] = cy * h * cw + dc_shift + cx * w
        jobs[i]["dst_offset"] = dst_shift + (i * n_alpha * slot_stride if dense else cy * h * dst_stride + cx * w)
    return {"name": name, "bit_depth": bd, "width": w, "height": h, "alphas": list(alphas), "luma": luma, "luma_size": (luma.shape[1], luma.shape[0]),
            "dc": dc, "jobs": jobs, "dst_samples": dst_samples, "dst_stride": dst_stride, "slot_stride": slot_stride, "kinds": list(kinds)}


def size_job_count(w, h):
    """not a multiple of the jobs per wave (a partial last wave) nor of the four waves of a workgroup"""
    return 201 if w * h <= 64 else (101 if w * h <= 256 else 37)


def size_kinds(w, h):
    """three waves of four begin and end with an extreme block (every kind comes by in both places), noise and smooth everywhere else"""
    jpw, n = jobs_per_wave(w, h), size_job_count(w, h)
    kinds = []
    for i in range(n):
        wave, at = divmod(i, jpw)
        e = wave - wave // 4  # the extreme waves so far
        if wave % 4 != 3 and at == 0:
            kinds.append(EXTREME_KINDS[e % len(EXTREME_KINDS)])
        elif wave % 4 != 3 and at == jpw - 1:
            kinds.append(EXTREME_KINDS[(e + 3) % len(EXTREME_KINDS)])
        else:
            kinds.append("smooth" if i % 3 == 0 else "noise")
    return kinds


DC_CYCLE = [("noise", "noise"), ("zero", "max"), ("max", "zero"), ("low", "high"), ("high", "low"), ("noise", "zero")]
UNORDERED_33 = [3, -16, 0, 16, -1, 1, 9, -9, 2, -2, 15, -15, 4, -4, 8, -8, 5, -5, 14, -14, 6, -6, 13, -13, 7, -7, 12, -12, 10, -10, 11, -11, -3]
ALPHA_LISTS = {"a1": [-7], "a2": [16, -16], "a33": UNORDERED_33}
GEOMETRY_SIZES = [(4, 4), (8, 8), (4, 16), (16, 8), (16, 16), (32, 32)]


def batch_names():
    names = [f"size_{w}x{h}_{bd}" for bd in (8, 10) for w, h in SIZES]
    names += [f"geometry_{w}x{h}_{bd}" for bd in (8, 10) for w, h in GEOMETRY_SIZES]
    names += [f"alist_{k}_{w}x{h}_{bd}" for bd in (8, 10) for k in ALPHA_LISTS for w, h in ((8, 8), (4, 16))]
    return names


@functools.lru_cache(maxsize=None)
def batch(name):
    group, rest = name.split("_", 1)
    if group == "size":  # every alpha, every kind of block, the grid's last job on the plane's last row and column, the stride the width
        size, bd = rest.split("_")
        w, h = (int(v) for v in size.split("x"))
        kinds = size_kinds(w, h)
        dcs = [DC_CYCLE[i % len(DC_CYCLE)] for i in range(len(kinds))]
        return make_batch(name, int(bd), w, h, ALPHAS_FULL, kinds, 16 if w * h <= 64 else 8, 7000 + 100 * w + h + int(bd), dc_kinds=dcs)
    if group == "geometry":  # odd origins and pitches: no load or store is aligned; a plane narrower than its array; dense slots
        size, bd = rest.split("_")
        w, h = (int(v) for v in size.split("x"))
        n = 2 * jobs_per_wave(w, h) + 3
        kinds = [KINDS[i % len(KINDS)] for i in range(n)]
        b = make_batch(name, int(bd), w, h, [-16, -3, 0, 7, 16], kinds, 5, 7500 + 100 * w + h + int(bd), dense=True, luma_pad=(5, 2), shift=(3, 1), dst_shift=3,
                       dc_shift=1)
        b["luma_size"] = (b["luma"].shape[1] - 5, b["luma"].shape[0] - 2)  # the grid's last column and row end on the plane the kernel is told of
        return b
    kind, size, bd = rest.split("_")
    w, h = (int(v) for v in size.split("x"))
    n = 3 * jobs_per_wave(w, h) + 1
    return make_batch(name, int(bd), w, h, ALPHA_LISTS[kind], [KINDS[i % len(KINDS)] for i in range(n)], 7, 7800 + len(kind) + w + int(bd))


def sample_jobs():
    """(key of the predictions, key of the AC, batch, job): one whole block per size and depth, the first noise block of the size batch, three of its
    alphas (the slots of SAMPLE_ALPHAS)"""
    out = []
    for bd in (8, 10):
        for w, h in SIZES:
            name = f"size_{w}x{h}_{bd}"
            out.append((f"pred_{w}x{h}_{bd}", f"ac_{w}x{h}_{bd}", name, batch(name)["kinds"].index("noise")))
    return out


def sample_slots():
    return [ALPHAS_FULL.index(a) for a in SAMPLE_ALPHAS]


def undefined_batch(bd, w, h):
    """good jobs with an undefined one between every two of them: (batch, indices of the undefined jobs)"""
    n_bad = 11
    b = make_batch(f"undefined_{w}x{h}_{bd}", bd, w, h, ALPHAS_FULL, ["noise"] * (2 * n_bad + 2), 6, 7900 + w + h + bd, dense=True)
    lw, lh = b["luma_size"]
    spoil = [("luma_x", -1), ("luma_y", -2), ("luma_x", lw - 2 * w + 1), ("luma_y", lh - 2 * h + 1), ("luma_x", 0x7FFFFFFF), ("luma_y", -0x80000000),
             ("dc0", b["dc"][0].size - (h - 1) * b["dc"][0].shape[1] - w + 1), ("dc1", 0xFFFFFFFF), ("dst0", b["dst_samples"] - SLOTS * b["slot_stride"] + 1),
             ("dst1", 0xFFFFFFF0), ("dst1", b["dst_samples"] - 1)]
    assert len(spoil) == n_bad
    bad = list(range(1, 2 * n_bad, 2))
    for i, (field, v) in zip(bad, spoil):
        if field.startswith("luma"):
            b["jobs"][i][field] = v
        else:
            b["jobs"][i]["dc_offset" if field.startswith("dc") else "dst_offset"][int(field[-1])] = v
    return b, bad


def coverage_missing(records):
    """records: (bit depth, width, height, alphas, kind, job, batch, events) per job.  The conditions of the prediction's cases, per depth."""
    missing = []
    for bd in (8, 10):
        rs = [r for r in records if r[0] == bd]
        ev = [r[7] for r in rs]
        mx = (1 << bd) - 1
        for key, what in (("clip0", "a prediction clipped at 0"), ("clipmax", "a prediction clipped at the maximum"),
                          ("tie_pos", "alpha * ac = 32 mod 64, positive"), ("tie_neg", "alpha * ac = 32 mod 64, negative")):
            if not any(e[key] for e in ev):
                missing.append(f"{bd} bits: {what}")
        if not any(e["round_rem"] != 0 for e in ev):
            missing.append(f"{bd} bits: sum + round is not a multiple of W * H")
        if not any(e["sum_rem"] * 2 == r[1] * r[2] for r, e in zip(rs, ev)):
            missing.append(f"{bd} bits: the average's remainder is exactly one half")
        for kind in ("zero", "max", "checker", "rows"):
            if not any(r[4] == kind for r in rs):
                missing.append(f"{bd} bits: a {kind} block")
        if not any(r[4] in ("zero", "max") and e["ac_zero"] for r, e in zip(rs, ev)):
            missing.append(f"{bd} bits: flat luma with an AC of zero")
        if not any(r[4] == "rows" and e["ac_max"] == 4 * mx for r, e in zip(rs, ev)):
            missing.append(f"{bd} bits: the largest |AC|, 4 * max")
        if not any(r[4] == "checker" and e["ac_max"] == 4 * mx for r, e in zip(rs, ev)):
            missing.append(f"{bd} bits: a 2x2 checkerboard of 0 / max")
        if {a for r in rs for a in r[3]} != set(ALPHAS_FULL):
            missing.append(f"{bd} bits: every alpha -16 .. 16")
        if {(r[1], r[2]) for r in rs} != set(SIZES):
            missing.append(f"{bd} bits: all 16 sizes")
        for w, h in SIZES:
            if not any((r[1], r[2]) == (w, h) and int(r[5]["luma_x"]) + 2 * w == r[6]["luma"].shape[1] == r[6]["luma_size"][0]
                       and int(r[5]["luma_y"]) + 2 * h == r[6]["luma_size"][1] for r in rs):
                missing.append(f"{bd} bits, {w}x{h}: a luma extent ending on the plane's last row and column, the stride equal to the width")
    return missing


def all_records(names=None):
    records = []
    for name in names or batch_names():
        b = batch(name)
        records += [(b["bit_depth"], b["width"], b["height"], b["alphas"], k, j, b, e) for k, j, e in zip(b["kinds"], b["jobs"], restated(name)[2])]
    return records


def spoil_desc(d, bad):
    """a good abi.CflPredDesc made bad in one way"""
    px = 2 if d.bit_depth > 8 else 1
    luma_end = d.luma + ((d.luma_height - 1) * d.luma_stride + d.luma_width) * px
    if bad.startswith("no_"):
        field = bad[3:]
        if field in ("luma", "jobs", "status"):
            setattr(d, field, None)
        else:
            setattr(d.plane[int(field[-1])], field[:-1], None)
    elif bad.startswith("bit_depth_"):
        d.bit_depth = int(bad[10:])
    elif bad.startswith("width_"):
        d.width = int(bad[6:])
    elif bad.startswith("height_"):
        d.height = int(bad[7:])
    elif bad.startswith("n_alpha_"):
        d.n_alpha = int(bad[8:])
    elif bad == "alpha_17":
        d.alpha_q3[d.n_alpha - 1] = 17
    elif bad == "alpha_-17":
        d.alpha_q3[0] = -17
    elif bad == "alpha_127":
        d.alpha_q3[1] = 127
    elif bad == "stride_below_width":
        d.luma_stride = d.luma_width - 1
    elif bad.startswith("zero_"):
        field = bad[5:]
        if hasattr(d, field):
            setattr(d, field, 0)
        else:
            setattr(d.plane[int(field[-1])], field[:-1], 0)
    elif bad == "ac_unaligned":
        d.ac = 0x300004
    elif bad == "dst0_inside_luma":
        d.plane[0].dst = d.luma + 64
    elif bad == "dst1_ends_in_luma":
        d.plane[1].dst = d.luma - d.plane[1].dst_samples * px + px
    elif bad == "luma_ends_in_dst0":
        d.plane[0].dst = luma_end - px
    elif bad == "dst0_inside_dc0":
        d.plane[0].dst = d.plane[0].dc + px
    elif bad == "dst0_inside_dc1":
        d.plane[0].dst = d.plane[1].dc + (d.plane[1].dc_samples - 1) * px
    elif bad == "dst1_inside_dc0":
        d.plane[1].dst = d.plane[0].dc - (d.plane[1].dst_samples - 1) * px
    else:
        raise KeyError(bad)
    return d


# ---- the alpha search ----
def rdcost(lam, rate, dist):
    """RDCOST(RM, R, D) on int64, the result as the reference's uint64_t holds it"""
    r = rate & U64_MAX
    r = r - (1 << 64) if r >> 63 else r
    return ((((r * lam + 256) >> 9) + dist * 128)) & U64_MAX


def joint_sign(plane, a, b):  # PLANE_SIGN_TO_JOINT_SIGN
    return a * 3 + b - 1 if plane == 0 else b * 3 + a - 1


def pick_alpha(bits, dist, fac, mode_bits, lam, itr_th, n_mag=16):
    """md_cfl_rd_pick_alpha replayed over the table: bits / dist [2][33] (slot k = alpha_q3 + 16), fac [8][2][16].  Returns best_rd, idx, signs,
    status, evals (per plane the bit mask of the slots read) and the events the coverage conditions look at."""
    bits, dist, fac = np.asarray(bits).reshape(2, SLOTS), np.asarray(dist).reshape(2, SLOTS), np.asarray(fac).reshape(8, 2, 16)
    mode_rd = rdcost(lam, int(mode_bits), 0)
    best_uv = [[MAX_MODE_COST, MAX_MODE_COST] for _ in range(8)]
    best_c = [[0, 0] for _ in range(8)]
    evals, undef, trunc = [0, 0], False, False
    ev = {"last_c": {}, "break_c": {}, "ties": 0, "pair_ties": 0}

    def read(plane, k):
        nonlocal undef
        evals[plane] |= 1 << k
        undef = undef or int(bits[plane][k]) == U64_MAX
        return int(bits[plane][k]), int(dist[plane][k])

    for plane in range(2):
        b, d = read(plane, 16)
        for sign in (1, 2):
            js = joint_sign(plane, 0, sign)
            best_uv[js][plane] = rdcost(lam, b + int(fac[js][plane][0]), d)
    best_rd, best_js = MAX_MODE_COST, 0
    for plane in range(2):
        for pn in (1, 2):
            progress = 0
            for c in range(16):
                if c > itr_th and progress < c:
                    ev["break_c"][(plane, pn)] = c
                    break
                if c >= n_mag:
                    trunc = True
                    break
                b, d = read(plane, 15 - c if pn == 1 else 17 + c)
                ev["last_c"][(plane, pn)] = c
                flag = 0
                for i in range(3):
                    js = joint_sign(plane, pn, i)
                    this_rd = rdcost(lam, b + int(fac[js][plane][c]), d)
                    if this_rd >= best_uv[js][plane]:
                        ev["ties"] += this_rd == best_uv[js][plane]
                        continue
                    best_uv[js][plane], best_c[js][plane], flag = this_rd, c, itr_th
                    if best_uv[js][1 - plane] == MAX_MODE_COST:
                        continue
                    this_rd = (this_rd + mode_rd + best_uv[js][1 - plane]) & U64_MAX
                    if this_rd >= best_rd:
                        ev["pair_ties"] += this_rd == best_rd
                        continue
                    best_rd, best_js = this_rd, js
                progress = (progress + flag) & 0xFF
    found = not undef and best_rd != MAX_MODE_COST
    return {"best_rd": best_rd if found else MAX_MODE_COST, "idx": (best_c[best_js][0] << 4) + best_c[best_js][1] if found else 0,
            "signs": best_js if found else 0, "status": PICK_UNDEFINED if undef else (PICK_TRUNCATED if trunc else 0), "evals": evals, "events": ev,
            "found": found}


def _valley(rng, lo, slope, m, noise=0):
    """16 distortions that fall to c = m and rise behind it"""
    return np.array([lo + slope * abs(c - m) + int(rng.integers(0, noise + 1)) for c in range(16)], np.uint64)


@functools.lru_cache(maxsize=None)
def pick_cases():
    """the alpha-search tables: name, bits, dist [2][33] uint64, fac [8][2][16] int32, mode_bits, lam, itr_th, n_mag"""
    cases = []

    def add(name, bits, dist, fac, mode_bits, lam, itr_th, n_mag=16):
        cases.append({"name": name, "bits": np.array(bits, np.uint64).reshape(2, SLOTS), "dist": np.array(dist, np.uint64).reshape(2, SLOTS),
                      "fac": np.array(fac, np.int32).reshape(8, 2, 16), "mode_bits": int(mode_bits), "lam": int(lam), "itr_th": itr_th, "n_mag": n_mag})

    def table(rng, plane_signs, m, hi=60000):
        """per plane the sign (0 zero, 1 negative, 2 positive) whose alphas are cheap, the cheapest magnitude m[plane]"""
        bits = rng.integers(500, 4000, (2, SLOTS)).astype(np.uint64)
        dist = rng.integers(hi, hi + 5000, (2, SLOTS)).astype(np.uint64)
        for plane, s in enumerate(plane_signs):
            if s == 0:
                dist[plane][16] = 50
            else:
                v = _valley(rng, 80, 900, m[plane], 20)
                for c in range(16):
                    dist[plane][15 - c if s == 1 else 17 + c] = v[c]
        return bits, dist

    for itr_th in (1, 2):
        rng = np.random.default_rng(9100 + itr_th)
        fac = rng.integers(300, 5000, (8, 2, 16))
        for js in range(8):  # every joint sign as the winner
            su, sv = (js + 1) // 3, (js + 1) % 3
            bits, dist = table(rng, (su, sv), ((2 * js + 1) % 7, (3 * js + 2) % 5))
            add(f"winner_js{js}_th{itr_th}", bits, dist, fac, 2100 + 37 * js, 41000 + 1000 * js, itr_th)
        # costs that rise from c = 0 on: every magnitude loop breaks at c = itr_th + 1
        bits = np.full((2, SLOTS), 2000, np.uint64)
        dist = np.array([[1000 + 400 * abs(k - 16) for k in range(SLOTS)]] * 2, np.uint64)
        add(f"rising_th{itr_th}", bits, dist, np.full((8, 2, 16), 900), 1500, 52000, itr_th)
        # costs that fall all the way: every loop runs to c = 15
        dist = np.array([[90000 - 5000 * abs(k - 16) for k in range(SLOTS)]] * 2, np.uint64)
        add(f"falling_th{itr_th}", bits, dist, np.full((8, 2, 16), 900), 1500, 52000, itr_th)
        # one cost everywhere: the first of the equal candidates wins, in the magnitude, in the joint sign and in the pair
        add(f"flat_th{itr_th}", bits, np.full((2, SLOTS), 7000, np.uint64), np.full((8, 2, 16), 1200), 1500, 30000, itr_th)
        # equal minima at two magnitudes of one sign
        bits2, dist2 = table(rng, (2, 1), (3, 2))
        dist2[0][17 + 5], bits2[0][17 + 5] = dist2[0][17 + 3], bits2[0][17 + 3]
        fac2 = fac.copy()
        fac2[:, 0, 5] = fac2[:, 0, 3]
        add(f"two_minima_th{itr_th}", bits2, dist2, fac2, 1800, 47000, itr_th)
        # no pair: every cost is at or above MAX_MODE_COST
        add(f"no_pair_th{itr_th}", bits, np.full((2, SLOTS), 1 << 41, np.uint64), fac, 1500, 52000, itr_th)
        add(f"no_pair_bits_th{itr_th}", np.full((2, SLOTS), 1 << 42, np.uint64), np.full((2, SLOTS), 100, np.uint64), fac, 1500, 1 << 17, itr_th)
        # one plane without a cost below MAX_MODE_COST: its partners stay MAX_MODE_COST, no pair is formed
        dist3 = np.full((2, SLOTS), 3000, np.uint64)
        dist3[1] = 1 << 41
        add(f"one_plane_th{itr_th}", bits, dist3, fac, 1500, 52000, itr_th)
        for i in range(24):  # random tables, a few lambdas; every second one with valleys, so that the loops run on
            lam = (700, 41000, 333333, 2500000)[i % 4]
            if i % 2:
                bits, dist = table(rng, (1 + i % 2, 1 + (i // 2) % 2), (int(rng.integers(0, 16)), int(rng.integers(0, 16))), hi=30000)
            else:
                bits, dist = rng.integers(0, 30000, (2, SLOTS)).astype(np.uint64), rng.integers(0, 60000, (2, SLOTS)).astype(np.uint64)
            add(f"random{i}_th{itr_th}", bits, dist, rng.integers(100, 9000, (8, 2, 16)), int(rng.integers(200, 8000)), lam, itr_th)
    # fewer magnitudes than the reference's 16: with the truncation bit (the loop wanted to go on) and without (it had stopped by itself)
    base = {c["name"]: c for c in cases}
    for name, n_mag in (("rising_th1", 4), ("rising_th1", 2), ("rising_th2", 4), ("rising_th2", 3), ("falling_th1", 8), ("falling_th2", 15), ("winner_js4_th1", 1),
                        ("winner_js4_th1", 12), ("winner_js7_th2", 14), ("random3_th1", 8), ("random4_th2", 6), ("flat_th1", 2), ("flat_th2", 3), ("flat_th2", 2)):
        c = base[name]
        add(f"{name}_mag{n_mag}", c["bits"], c["dist"], c["fac"], c["mode_bits"], c["lam"], c["itr_th"], n_mag)
    return cases


def pick_coverage_missing(cases, results):
    missing = []
    full = [(c, r) for c, r in zip(cases, results) if c["n_mag"] == 16]
    winners = {r["signs"] for c, r in full if r["found"] and c["name"].startswith("winner")}
    if winners != set(range(8)):
        missing.append(f"every joint sign as the winner: {sorted(winners)}")
    for th in (1, 2):
        rs = [r for c, r in full if c["itr_th"] == th]
        if not rs:
            missing.append(f"itr_th {th}")
            continue
        if not any(th + 1 in r["events"]["break_c"].values() for r in rs):
            missing.append(f"itr_th {th}: a break at c = itr_th + 1")
        if not any(15 in r["events"]["last_c"].values() for r in rs):
            missing.append(f"itr_th {th}: a run to c = 15")
        if not any(r["events"]["ties"] and r["events"]["pair_ties"] and r["found"] for r in rs):
            missing.append(f"itr_th {th}: ties in the magnitude and in the pair")
        if not any(not r["found"] for r in rs):
            missing.append(f"itr_th {th}: a block with no pair")
    short = [r for c, r in zip(cases, results) if c["n_mag"] < 16]
    if not any(r["status"] == PICK_TRUNCATED for r in short):
        missing.append("n_mag < 16 with the truncation bit")
    if not any(r["status"] == 0 for r in short):
        missing.append("n_mag < 16 without the truncation bit")
    return missing


def pick_results():
    return [pick_alpha(c["bits"], c["dist"], c["fac"], c["mode_bits"], c["lam"], c["itr_th"], c["n_mag"]) for c in pick_cases()]
