"""The cases of the warped-motion entries (svt_hip_warp_pred_batch, svt_hip_warp_model_batch, svt_hip_wm_refine_batch) and numpy restatements of all three, shared by
tests/test_warp.py, tests/test_warp_gpu.py, tests/test_warp_chain_gpu.py, tests/warp_edge_cases.py and tools/gen_warp_golden.py, which compares the restatements with the
reference encoder on every job and writes golden/warp.npz.  The restatements follow the reference's C line by line (Source/Lib/Codec/
warped_motion.c: svt_av1_warp_affine_c, svt_av1_highbd_warp_affine_c, svt_aom_select_samples, find_affine_int, svt_get_shear_params;
adaptive_mv_pred.c: svt_aom_warped_motion_parameters from the MV on; mode_decision.c: the loop of svt_aom_wm_motion_refinement), in Python integers where C has 32- and 64-bit ones.  The 193 x 8 filter
table is the library's host copy (svt_hip_warp_filter_table): the fixture pins its CRC-32 on the reference's table, so there is one typed copy."""
import functools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp.npz")
ST_OK, ST_NO_MODEL, ST_UNDEFINED = 0, 0xFE, 0xFF
ROTZOOM, AFFINE = 2, 3
NO_REF = 0xFF
MODEL0_FROM_ARRAY, MODEL1_FROM_ARRAY, MV_FROM_ARRAY = 1, 2, 1
FILL = 0xA5
SIDES = (8, 16, 32, 64, 128)
SIZES = [(w, h) for w in SIDES for h in SIDES if max(w, h) <= 2 * min(w, h) or (max(w, h) == 4 * min(w, h) and max(w, h) <= 64)]
QUANT_DIST = [(9, 7), (11, 5), (12, 4), (13, 3), (7, 9), (5, 11), (4, 12), (3, 13)]
MODEL_DTYPE = [("wmmat", "<i4", (6,)), ("alpha", "<i2"), ("beta", "<i2"), ("gamma", "<i2"), ("delta", "<i2"), ("wmtype", "u1"), ("valid", "u1"),
               ("num_samples", "<u2"), ("reserved", "<u4")]
PRED_JOB_DTYPE = [("dst_offset", "<u4"), ("p_col", "<i2"), ("p_row", "<i2"), ("width", "u1"), ("height", "u1"), ("ref", "u1", (2,)), ("flags", "u1"),
                  ("comp_mode", "u1"), ("fwd_offset", "u1"), ("bck_offset", "u1"), ("model_index", "<u4", (2,)), ("model", MODEL_DTYPE, (2,))]
MODEL_JOB_DTYPE = [("pts", "<i4", (16,)), ("pts_inref", "<i4", (16,)), ("blk_org_x", "<u2"), ("blk_org_y", "<u2"), ("bwidth", "u1"), ("bheight", "u1"),
                   ("n_samples", "u1"), ("flags", "u1"), ("mv", "<i2", (2,)), ("mv_index", "<u4")]


def i32(v):
    """a Python integer wrapped to int32, as the reference's 32-bit arithmetic wraps"""
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def i16(v):
    return ((int(v) + (1 << 15)) & 0xFFFF) - (1 << 15)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def round_signed(v, n):
    """ROUND_POWER_OF_TWO_SIGNED / _64"""
    half = (1 << n) >> 1
    return -((-v + half) >> n) if v < 0 else (v + half) >> n


@functools.lru_cache(maxsize=None)
def filter_table():
    from svt_av1_psyex_amd import warp
    return warp.tables()[0].astype(np.int64)


def div_lut():
    """round(2^22 / (256 + i)), i = 0 .. 256"""
    return np.array([((1 << 22) + (256 + i) // 2) // (256 + i) for i in range(257)], np.uint16)


def table_crc(a, dt):
    return zlib.crc32(np.ascontiguousarray(a, dtype=dt).tobytes())


# ---- the prediction ----
def shear_allowed(alpha, beta, gamma, delta):
    """is_affine_shear_allowed on multiples of 64"""
    if (alpha | beta | gamma | delta) & 63:
        return False
    return 4 * abs(alpha) + 7 * abs(beta) < (1 << 16) and 4 * abs(gamma) + 4 * abs(delta) < (1 << 16)


def model_of(rec):
    """(mat[6], (alpha, beta, gamma, delta)) of a MODEL_DTYPE record as svt_warp_plane uses it"""
    mat = [int(v) for v in rec["wmmat"]]
    if int(rec["wmtype"]) == ROTZOOM:
        mat[5], mat[4] = mat[2], i32(-mat[3])
    return mat, tuple(int(rec[k]) for k in ("alpha", "beta", "gamma", "delta"))


def warp_tile(plane, org_x, org_y, pw, ph, mat, shear, jx, iy, ss_x, ss_y, bd, reduce_vert, seen=None):
    """one 8x8 tile of svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c: the vertical sums after ROUND_POWER_OF_TWO(., reduce_vert), int64 [8][8]"""
    F = filter_table()
    alpha, beta, gamma, delta = shear
    src_x, src_y = i32((jx + 4) << ss_x), i32((iy + 4) << ss_y)
    x4 = i32(mat[2] * src_x + mat[3] * src_y + mat[0]) >> ss_x
    y4 = i32(mat[4] * src_x + mat[5] * src_y + mat[1]) >> ss_y
    ix4, iy4 = x4 >> 16, y4 >> 16
    sx4 = ((x4 & 0xFFFF) - 4 * (alpha + beta)) & ~63
    sy4 = ((y4 & 0xFFFF) - 4 * (gamma + delta)) & ~63
    ys = np.clip(iy4 + np.arange(-7, 8), 0, ph - 1) + org_y
    xs = np.clip(ix4 + np.arange(-7, 8), 0, pw - 1) + org_x
    win = plane[np.ix_(ys, xs)].astype(np.int64)  # rows k = -7 .. 7, columns ix4 - 7 .. ix4 + 7
    c = np.arange(8)
    sx = sx4 + beta * (np.arange(-7, 8)[:, None] + 4) + alpha * c[None, :]
    offs_h = ((sx + 512) >> 10) + 64
    sy = sy4 + delta * c[:, None] + gamma * c[None, :]
    offs_v = ((sy + 512) >> 10) + 64
    assert offs_h.min() >= 0 and offs_h.max() <= 192 and offs_v.min() >= 0 and offs_v.max() <= 192
    mid = ((1 << (bd + 6)) + (win[:, c[:, None] + c[None, :]] * F[offs_h]).sum(-1) + 4) >> 3
    col = mid[c[:, None, None] + c[None, None, :], c[None, :, None]]  # [r][c][t] = mid[r + t][c]
    s = (1 << (bd + 11)) + (col * F[offs_v]).sum(-1)
    if seen is not None:
        seen["offs_h"] |= {int(offs_h.min()), int(offs_h.max())}
        seen["offs_v"] |= {int(offs_v.min()), int(offs_v.max())}
        seen["tiles"].append((ix4, iy4, pw, ph))
        seen["neg"] = seen["neg"] or ((ss_x or ss_y) and (i32(mat[2] * src_x + mat[3] * src_y + mat[0]) < 0 or i32(mat[4] * src_x + mat[5] * src_y + mat[1]) < 0))
    return (s + ((1 << reduce_vert) >> 1)) >> reduce_vert


def new_seen():
    return {"offs_h": set(), "offs_v": set(), "tiles": [], "neg": False}


def job_status(b, j):
    """the status svt_hip_warp_pred_batch gives the job, and its models when it is 0"""
    w, h = int(j["width"]), int(j["height"])
    comp = int(j["ref"][1]) != NO_REF
    n_refs, models = len(b["planes"]), b.get("models")
    n_models = 0 if models is None else len(models)
    ok = (w, h) in SIZES and int(j["ref"][0]) < n_refs
    if comp:
        ok = ok and int(j["ref"][1]) < n_refs and int(j["comp_mode"]) <= 1
        if int(j["comp_mode"]) == 1:
            ok = ok and (int(j["fwd_offset"]), int(j["bck_offset"])) in QUANT_DIST
    arr = [bool(int(j["flags"]) & MODEL0_FROM_ARRAY), comp and bool(int(j["flags"]) & MODEL1_FROM_ARRAY)]
    for r in range(2):
        if arr[r]:
            ok = ok and int(j["model_index"][r]) < n_models
    rows, stride = b["dst_shape"][0], b["dst_stride"]
    ok = ok and int(j["dst_offset"]) + (h - 1) * stride + w <= rows * stride
    if not ok:
        return ST_UNDEFINED, None
    recs = [models[int(j["model_index"][r])] if arr[r] else j["model"][r] for r in range(2 if comp else 1)]
    if any(arr[r] and int(recs[r]["valid"]) == 0 for r in range(len(recs))):
        return ST_NO_MODEL, None
    out = []
    for rec in recs:
        mat, shear = model_of(rec)
        if int(rec["wmtype"]) not in (ROTZOOM, AFFINE) or not shear_allowed(*shear):
            return ST_UNDEFINED, None
        out.append((mat, shear))
    return ST_OK, out


def warp_block(b, j, models, seen=None):
    """the job's block [h][w] as the reference writes it"""
    bd, ss_x, ss_y = b["bit_depth"], b["ss_x"], b["ss_y"]
    w, h = int(j["width"]), int(j["height"])
    out = np.zeros((h, w), np.int64)
    for ty in range(h // 8):
        for tx in range(w // 8):
            jx, iy = int(j["p_col"]) + 8 * tx, int(j["p_row"]) + 8 * ty
            if len(models) == 1:
                v = warp_tile(*b["planes"][int(j["ref"][0])], *models[0], jx, iy, ss_x, ss_y, bd, 11, seen) - (1 << (bd - 1)) - (1 << bd)
            else:
                a0 = warp_tile(*b["planes"][int(j["ref"][0])], *models[0], jx, iy, ss_x, ss_y, bd, 7, seen)
                a1 = warp_tile(*b["planes"][int(j["ref"][1])], *models[1], jx, iy, ss_x, ss_y, bd, 7, seen)
                t = (a0 * int(j["fwd_offset"]) + a1 * int(j["bck_offset"])) >> 4 if int(j["comp_mode"]) else (a0 + a1) >> 1
                v = (t - (1 << (bd + 4)) - (1 << (bd + 3)) + 8) >> 4
            out[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = np.clip(v, 0, (1 << bd) - 1)
    return out


def dst_dtype(b):
    return np.uint16 if b["bit_depth"] > 8 else np.uint8


def fresh_dst(b):
    return np.frombuffer(bytes([FILL]) * (b["dst_shape"][0] * b["dst_stride"] * np.dtype(dst_dtype(b)).itemsize), dst_dtype(b)).reshape(b["dst_shape"][0], b["dst_stride"]).copy()


def restate_pred(b, seen=None):
    """(the destination plane as the batch leaves it, from the byte FILL; status [n]; the blocks of the defined jobs by index)"""
    dst, status, blocks = fresh_dst(b), np.zeros(len(b["jobs"]), np.uint8), {}
    flat = dst.reshape(-1)
    for i, j in enumerate(b["jobs"]):
        status[i], models = job_status(b, j)
        if status[i] == ST_OK:
            blk = warp_block(b, j, models, seen)
            blocks[i] = blk
            w, h = int(j["width"]), int(j["height"])
            for r in range(h):
                o = int(j["dst_offset"]) + r * b["dst_stride"]
                flat[o:o + w] = blk[r]
    return dst, status, blocks


def block_crc(blk):
    return zlib.crc32(np.ascontiguousarray(blk, dtype="<u2").tobytes())


# the case lists
def make_plane(rng, bd, pw, ph, pad=8, kind="noise"):
    """a padded plane around a pw x ph picture; the padding holds a value no picture sample has a reason to equal, so a read of it shows"""
    dt = np.uint16 if bd > 8 else np.uint8
    top = (1 << bd) - 1
    if kind == "noise":
        pic = rng.integers(0, top + 1, (ph, pw))
    elif kind == "smooth":
        yy, xx = np.mgrid[0:ph, 0:pw]
        pic = np.clip((top / 2) * (1 + np.sin(xx / 5.0 + yy / 9.0)) + rng.integers(-6, 7, (ph, pw)), 0, top)
    else:
        pic = np.where((np.mgrid[0:ph, 0:pw].sum(0) // 3) & 1, top, 0)  # extremes: both clips
    plane = np.full((ph + 2 * pad, pw + 2 * pad + 3), 0x155 if bd > 8 else 0x55, dt)
    plane[pad:pad + ph, pad:pad + pw] = pic
    return (plane, pad, pad, pw, ph)


def model_rec(mat, shear=None, wmtype=AFFINE, valid=1):
    """a MODEL_DTYPE record; shear None: what svt_get_shear_params derives from the matrix (which must then allow it)"""
    rec = np.zeros((), MODEL_DTYPE)
    rec["wmmat"], rec["wmtype"], rec["valid"] = mat, wmtype, valid
    if shear is None:
        m = list(mat)
        if wmtype == ROTZOOM:
            m[5], m[4] = m[2], -m[3]
        ok, shear = shear_params(m)
        assert ok, mat
    rec["alpha"], rec["beta"], rec["gamma"], rec["delta"] = shear
    return rec


def random_model(rng, w_pic, h_pic, scale, wmtype=AFFINE, span=16):
    """a matrix near the identity with a translation of up to `span` samples; scale: the size of the off-identity terms (up to 8191)"""
    while True:
        d = rng.integers(-scale, scale + 1, 4)
        mat = [int(rng.integers(-span << 16, (span << 16) + 1)), int(rng.integers(-span << 16, (span << 16) + 1)), (1 << 16) + int(d[0]), int(d[1]), int(d[2]),
               (1 << 16) + int(d[3])]
        m = list(mat)
        if wmtype == ROTZOOM:
            m[5], m[4] = m[2], -m[3]
        ok, shear = shear_params(m)
        if ok:
            return model_rec(mat, shear, wmtype)


def pred_job(dst_offset, p_col, p_row, w, h, refs, models, comp_mode=0, offsets=(0, 0), flags=0, model_index=(0, 0)):
    j = np.zeros((), PRED_JOB_DTYPE)
    j["dst_offset"], j["p_col"], j["p_row"], j["width"], j["height"] = dst_offset, p_col, p_row, w, h
    j["ref"] = list(refs) + [NO_REF] * (2 - len(refs))
    j["flags"], j["comp_mode"], j["fwd_offset"], j["bck_offset"], j["model_index"] = flags, comp_mode, offsets[0], offsets[1], model_index
    for r, m in enumerate(models):
        j["model"][r] = m
    return j


def pack_jobs(jobs, dtype):
    out = np.zeros(len(jobs), dtype)
    for i, j in enumerate(jobs):
        out[i] = j
    return out


MODES = ("single", "average", "distance")


def _mode_args(mode, k):
    if mode == "single":
        return dict(refs=[k % 2], comp_mode=0)
    if mode == "average":
        return dict(refs=[0, 1], comp_mode=0)
    return dict(refs=[1, 0] if k & 1 else [0, 1], comp_mode=1, offsets=QUANT_DIST[k % 8])


@functools.lru_cache(maxsize=None)
def batch(name):
    """a prediction batch by name: size_{bd}_{ss}, edge_{bd}_{w}x{h}, ends_{bd}, big_{bd}, count_{n}"""
    kind, *rest = name.split("_")
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    if kind == "size":
        # every size x every mode on one plane pair; ss 0: all 17 sizes, ss 1: the sizes up to 64x64
        bd, ss = int(rest[0]), int(rest[1])
        pw, ph = (128, 96) if ss == 0 else (64, 48)
        planes = [make_plane(rng, bd, pw, ph, kind="noise"), make_plane(rng, bd, pw, ph, kind="smooth")]
        sizes = [s for s in SIZES if ss == 0 or max(s) <= 64]
        if ss == 0:
            sizes = [s for s in sizes if s != (128, 128)]  # big_{bd} has it
        jobs, off, k = [], 5, 0
        stride = 131
        for (w, h) in sizes:
            for mode in MODES:
                a = _mode_args(mode, k)
                models = [random_model(rng, pw, ph, 3000, ROTZOOM if (k + r) % 3 == 0 else AFFINE, span=12) for r in range(len(a["refs"]))]
                p_col, p_row = int(rng.integers(0, max(1, pw - w + 1)) // 2 * 2), int(rng.integers(0, max(1, ph - h + 1)))
                jobs.append(pred_job(off, p_col, p_row, w, h, models=models, **a))
                off += h * stride + (3 if k & 1 else 0)
                k += 1
        return dict(name=name, bit_depth=bd, ss_x=ss, ss_y=ss, planes=planes, jobs=pack_jobs(jobs, PRED_JOB_DTYPE), dst_shape=(off // stride + 2, stride),
                    dst_stride=stride)
    if kind == "edge":
        # tiles wholly outside each edge, straddling each edge, a negative projection on the sub-sampled plane; 40x24 and 37x21 pictures
        bd = int(rest[0])
        pw, ph = (int(v) for v in rest[1].split("x"))
        jobs, off, stride, k = [], 0, 67, 0
        planes = [make_plane(rng, bd, pw, ph, kind="noise"), make_plane(rng, bd, pw, ph, kind="extreme")]
        ss = 1 if pw == 40 else 0
        for tx, ty in ((-40, 0), (pw + 30, 0), (0, -40), (0, ph + 30), (-6, 3), (pw - 5, 2), (4, -5), (3, ph - 4), (-100, -100), (pw + 90, ph + 90), (0, 0)):
            for mode in MODES:
                a = _mode_args(mode, k)
                models = []
                for r in range(len(a["refs"])):
                    m = random_model(rng, pw, ph, 2500, AFFINE if (k + r) & 1 else ROTZOOM, span=0)
                    m["wmmat"][0], m["wmmat"][1] = (tx << ss) << 16, (ty << ss) << 16  # sends the block there
                    models.append(m)
                w, h = ((16, 8), (8, 16), (16, 16), (8, 8))[k % 4]
                jobs.append(pred_job(off, int(rng.integers(0, 9)), int(rng.integers(0, 5)), w, h, models=models, **a))
                off += h * stride
                k += 1
        return dict(name=name, bit_depth=bd, ss_x=ss, ss_y=ss, planes=planes, jobs=pack_jobs(jobs, PRED_JOB_DTYPE), dst_shape=(off // stride + 1, stride),
                    dst_stride=stride)
    if kind == "ends":
        # both ends of the filter table in each direction, all shears zero, a shear of each sign
        bd = int(rest[0])
        pw, ph = 48, 40
        planes = [make_plane(rng, bd, pw, ph, kind="noise"), make_plane(rng, bd, pw, ph, kind="extreme")]
        jobs, off, stride = [], 0, 32
        shears = [(0, 0, 0, 0), (16320, 0, 0, 0), (-16320, 0, 0, 0), (0, 9344, 0, 0), (0, -9344, 0, 0), (0, 0, 16320, 0), (0, 0, -16320, 0), (0, 0, 0, 16320),
                  (0, 0, 0, -16320), (8192, 4672, 8128, 8192), (-8192, -4672, -8128, -8192), (8192, -4672, -8128, 8192), (64, -64, 64, -64)]
        for k, sh in enumerate(shears):
            for frac in (0, 0xFFFF, 0x8000):
                mat = [(5 << 16) + frac, (3 << 16) + frac, 1 << 16, 0, 0, 1 << 16]
                a = _mode_args(MODES[k % 3], k)
                models = [model_rec(mat, sh, AFFINE) for _ in a["refs"]]
                jobs.append(pred_job(off, 8, 8, 16, 16, models=models, **a))
                off += 16 * stride
        return dict(name=name, bit_depth=bd, ss_x=0, ss_y=0, planes=planes, jobs=pack_jobs(jobs, PRED_JOB_DTYPE), dst_shape=(off // stride, stride), dst_stride=stride)
    if kind == "big":
        bd = int(rest[0])
        planes = [make_plane(rng, bd, 128, 96, kind="smooth")]
        jobs = [pred_job(0, 0, 0, 128, 128, refs=[0], models=[random_model(rng, 128, 96, 1500, AFFINE, span=6)])]
        return dict(name=name, bit_depth=bd, ss_x=0, ss_y=0, planes=planes, jobs=pack_jobs(jobs, PRED_JOB_DTYPE), dst_shape=(128, 128), dst_stride=128)
    if kind == "count":
        # n jobs of 8x8 and 16x8, so that waves and workgroups run empty and partial; 8-bit and 10-bit alternate by n
        n = int(rest[0])
        bd = 10 if n & 1 else 8
        planes = [make_plane(rng, bd, 56, 40, kind="noise")]
        jobs, stride = [], 24
        for k in range(n):
            w = 16 if k % 3 == 0 else 8
            jobs.append(pred_job(k * 8 * stride + (k % 5), int(rng.integers(0, 40)), int(rng.integers(0, 32)), w, 8, refs=[0],
                                 models=[random_model(rng, 56, 40, 2000, AFFINE, span=4)]))
        return dict(name=name, bit_depth=bd, ss_x=0, ss_y=0, planes=planes, jobs=pack_jobs(jobs, PRED_JOB_DTYPE), dst_shape=(n * 8 + 1, stride), dst_stride=stride)
    raise KeyError(name)


COUNTS = (1, 63, 64, 65)


def batch_names():
    return ([f"size_{bd}_{ss}" for bd in (8, 10) for ss in (0, 1)] + [f"edge_{bd}_{p}" for bd in (8, 10) for p in ("40x24", "37x21")]
            + [f"ends_{bd}" for bd in (8, 10)] + [f"big_{bd}" for bd in (8, 10)] + [f"count_{n}" for n in COUNTS])


@functools.lru_cache(maxsize=None)
def restated(name):
    seen = new_seen()
    dst, status, blocks = restate_pred(batch(name), seen)
    return dst, status, blocks, seen


def sample_jobs():
    """(fixture key, batch, job): one whole block per size and depth"""
    out = []
    for bd in (8, 10):
        b = batch(f"size_{bd}_0")
        for (w, h) in SIZES:
            if (w, h) == (128, 128):
                out.append((f"block_{bd}_{w}x{h}", f"big_{bd}", 0))
            else:
                i = next(i for i, j in enumerate(b["jobs"]) if (int(j["width"]), int(j["height"])) == (w, h))
                out.append((f"block_{bd}_{w}x{h}", f"size_{bd}_0", i))
    return out


def pred_coverage_missing():
    """the issue's conditions on the warp filter that the case list does not meet"""
    missing = []
    oh, ov, tiles, neg = set(), set(), [], False
    zero = pos = negs = rot = aff = False
    pairs = set()
    for name in batch_names():
        b = batch(name)
        _, status, _, seen = restated(name)
        oh |= seen["offs_h"]; ov |= seen["offs_v"]; tiles += seen["tiles"]; neg = neg or seen["neg"]
        for j, st in zip(b["jobs"], status):
            if st != ST_OK:
                missing.append(f"{name}: an undefined job")
            for r in range(2 if int(j["ref"][1]) != NO_REF else 1):
                sh = [int(j["model"][r][k]) for k in ("alpha", "beta", "gamma", "delta")]
                zero = zero or not any(sh)
                pos = pos or all(v > 0 for v in sh)
                negs = negs or all(v < 0 for v in sh)
                rot = rot or int(j["model"][r]["wmtype"]) == ROTZOOM
                aff = aff or int(j["model"][r]["wmtype"]) == AFFINE
            if int(j["ref"][1]) != NO_REF and int(j["comp_mode"]) == 1:
                pairs.add((int(j["fwd_offset"]), int(j["bck_offset"])))
    for label, s in (("horizontal", oh), ("vertical", ov)):
        if not {0, 192} <= s:
            missing.append(f"filter index 0 and 192, {label}: {sorted(s)[:2]} .. {sorted(s)[-2:]}")
    where = {"left": lambda x, y, w, h: x + 7 < 0, "right": lambda x, y, w, h: x - 7 > w - 1, "above": lambda x, y, w, h: y + 7 < 0,
             "below": lambda x, y, w, h: y - 7 > h - 1, "straddles left": lambda x, y, w, h: x - 7 < 0 <= x + 7, "straddles right": lambda x, y, w, h: x - 7 <= w - 1 < x + 7,
             "straddles top": lambda x, y, w, h: y - 7 < 0 <= y + 7, "straddles bottom": lambda x, y, w, h: y - 7 <= h - 1 < y + 7}
    for label, f in where.items():
        if not any(f(*t) for t in tiles):
            missing.append(f"a tile {label}")
    if not any(w % 8 and h % 8 for _, _, w, h in tiles):
        missing.append("a picture whose width and height are no multiples of 8")
    for label, v in (("a negative projection on a sub-sampled plane", neg), ("all shears zero", zero), ("all shears positive", pos), ("all shears negative", negs),
                     ("ROTZOOM", rot), ("AFFINE", aff), ("every quant_dist pair", pairs == set(QUANT_DIST))):
        if not v:
            missing.append(label)
    return missing


def undefined_batch(bd):
    """a batch of good 8x8 / 16x16 jobs with one job of every undefined kind between them; returns (batch, {index: the status expected})"""
    rng = np.random.default_rng(77 + bd)
    planes = [make_plane(rng, bd, 40, 24), make_plane(rng, bd, 40, 24, kind="smooth")]
    good = random_model(rng, 40, 24, 2000)
    models = pack_jobs([good, model_rec([0] * 6, (0, 0, 0, 0), AFFINE, valid=0), good], MODEL_DTYPE)
    stride = 40
    spoil = [("size_8x4", dict(h=4)), ("size_24x8", dict(w=24)), ("size_128x32", dict(w=128, h=32)), ("ref0", dict(refs=[2])), ("ref1", dict(refs=[0, 7])),
             ("model_index", dict(flags=MODEL0_FROM_ARRAY, model_index=(3, 0))), ("model_index1", dict(refs=[0, 1], flags=MODEL1_FROM_ARRAY, model_index=(0, 9))),
             ("dst_end", dict(dst_offset="end")), ("comp_mode", dict(refs=[0, 1], comp_mode=2)),
             ("offsets", dict(refs=[0, 1], comp_mode=1, offsets=(8, 8))), ("offsets_sum", dict(refs=[0, 1], comp_mode=1, offsets=(9, 6))),
             ("wmtype", dict(wmtype=1)), ("wmtype_4", dict(wmtype=4)), ("shear_32", dict(shear=(32, 0, 0, 0))), ("shear_ab", dict(shear=(16384, 0, 0, 0))),
             ("shear_gd", dict(shear=(0, 0, 8192, -8192))), ("shear_second", dict(refs=[0, 1], shear1=(0, 9408, 0, 0))),
             ("no_model", dict(flags=MODEL0_FROM_ARRAY, model_index=(1, 0))), ("no_model1", dict(refs=[1, 0], flags=MODEL0_FROM_ARRAY | MODEL1_FROM_ARRAY, model_index=(2, 1)))]
    jobs, expect = [], {}
    rows = 16 * (2 * len(spoil) + 1)  # a slot of 16 rows per job
    for k in range(2 * len(spoil) + 1):
        a = dict(dst_offset=k * 16 * stride, w=16, h=16, refs=[k % 2], comp_mode=0, offsets=(0, 0), flags=0, model_index=(0, 0))
        ms = [good.copy(), good.copy()]
        if k & 1:
            label, ch = spoil[k // 2]
            ch = dict(ch)
            if "wmtype" in ch:
                ms[0]["wmtype"] = ch.pop("wmtype")
            if "shear" in ch:
                ms[0]["alpha"], ms[0]["beta"], ms[0]["gamma"], ms[0]["delta"] = ch.pop("shear")
            if "shear1" in ch:
                ms[1]["alpha"], ms[1]["beta"], ms[1]["gamma"], ms[1]["delta"] = ch.pop("shear1")
            a.update(ch)
            if a["dst_offset"] == "end":
                a["dst_offset"] = rows * stride - 15 * stride - 15  # the last row ends one sample past the plane
            expect[k] = ST_NO_MODEL if label.startswith("no_model") else ST_UNDEFINED
        jobs.append(pred_job(a["dst_offset"], 4, 2, a["w"], a["h"], a["refs"], ms[:len(a["refs"])], a["comp_mode"], a["offsets"], a["flags"], a["model_index"]))
    b = dict(name=f"undefined_{bd}", bit_depth=bd, ss_x=0, ss_y=0, planes=planes, jobs=pack_jobs(jobs, PRED_JOB_DTYPE), dst_shape=(rows, stride), dst_stride=stride,
             models=models)
    return b, expect


# ---- the fit ----
def select_samples(mv_row, mv_col, pts, pts_inref, n, bw, bh):
    """svt_aom_select_samples, in place; returns what it returns and which branch it took"""
    thresh = clamp(max(bw, bh), 16, 112)
    mvd = [0] * 16
    ret = 0
    for i in range(n):
        mvd[i] = abs(pts_inref[2 * i] - pts[2 * i] - mv_col) + abs(pts_inref[2 * i + 1] - pts[2 * i + 1] - mv_row)
        if mvd[i] > thresh:
            mvd[i] = -1
        else:
            ret += 1
    if not ret:
        return 1, "none"
    i, j, swaps = 0, n - 1, 0
    for _ in range(n - ret):
        while mvd[i] != -1:
            i += 1
        if j < 0:
            break
        while mvd[j] == -1:
            j -= 1
            if j < 0:
                break
        if i > j:
            break
        mvd[i] = mvd[j]
        pts[2 * i], pts[2 * i + 1] = pts[2 * j], pts[2 * j + 1]
        pts_inref[2 * i], pts_inref[2 * i + 1] = pts_inref[2 * j], pts_inref[2 * j + 1]
        i += 1
        j -= 1
        swaps += 1
    return ret, "all" if ret == n else ("swap" if swaps else "tail")


def resolve_divisor(D):
    """resolve_divisor_64 / _32: (the multiplier, the shift)"""
    shift = D.bit_length() - 1
    e = D - (1 << shift)
    f = (e + ((1 << (shift - 8)) >> 1)) >> (shift - 8) if shift > 8 else e << (8 - shift)
    assert f <= 256
    return int(div_lut()[f]), shift + 14


def shear_params(mat):
    """svt_get_shear_params: (1 or 0, (alpha, beta, gamma, delta) reduced to multiples of 64)"""
    if mat[2] <= 0:
        return 0, (0, 0, 0, 0)
    alpha, beta = clamp(mat[2] - (1 << 16), -32768, 32767), clamp(mat[3], -32768, 32767)
    y, shift = resolve_divisor(abs(mat[2]))
    y = i16(y * (-1 if mat[2] < 0 else 1))
    gamma = clamp(i32(round_signed(mat[4] * (1 << 16) * y, shift)), -32768, 32767)
    delta = clamp(mat[5] - i32(round_signed(mat[3] * mat[4] * y, shift)) - (1 << 16), -32768, 32767)
    sh = tuple(i16(round_signed(v, 6) * 64) for v in (alpha, beta, gamma, delta))
    if 4 * abs(sh[0]) + 7 * abs(sh[1]) >= (1 << 16) or 4 * abs(sh[2]) + 4 * abs(sh[3]) >= (1 << 16):
        return 0, sh
    return 1, sh


def find_affine_int(n, pts, pts_inref, bw, bh, mvy, mvx, mi_row, mi_col, trace):
    """find_affine_int: (1 on failure, wmmat[6])"""
    A, bx, by = [[0, 0], [0, 0]], [0, 0], [0, 0]
    rsuy, rsux = max(bh, 4) // 2 - 1, max(bw, 4) // 2 - 1
    suy, sux = rsuy * 8, rsux * 8
    duy, dux = suy + mvy, sux + mvx
    isuy, isux = mi_row * 4 + rsuy, mi_col * 4 + rsux
    sq = lambda a: (a * a * 4 + a * 4 * 8 + 8 * 8 * 2) >> 4
    p1 = lambda a, b: (a * b * 4 + (a + b) * 2 * 8 + 8 * 8) >> 4
    p2 = lambda a, b: (a * b * 4 + (a + b) * 2 * 8 + 8 * 8 * 2) >> 4
    wide = []  # what the reference holds in 32 bits, unwrapped here: for the trace alone
    for i in range(n):
        dx, dy = pts_inref[2 * i] - dux, pts_inref[2 * i + 1] - duy
        sx, sy = pts[2 * i] - sux, pts[2 * i + 1] - suy
        if abs(sx - dx) < 256 and abs(sy - dy) < 256:
            A[0][0] += sq(sx); A[0][1] += p1(sx, sy); A[1][1] += sq(sy)
            bx[0] += p2(sx, dx); bx[1] += p1(sy, dx); by[0] += p1(sx, dy); by[1] += p2(sy, dy)
            wide += [4 * a * b + 16 * (abs(a) + abs(b)) + 128 for a in (sx, sy) for b in (sx, sy, dx, dy)] + A[0] + A[1] + bx + by
        else:
            trace.add("ls_mv_max")
    det = A[0][0] * A[1][1] - A[0][1] * A[0][1]
    if det == 0:
        trace.add("det0")
        return 1, [0] * 6
    y, shift = resolve_divisor(abs(det))
    i_det = i16(y * (-1 if det < 0 else 1))
    shift -= 16
    if shift < 0:
        trace.add("shift_neg")
        i_det = i16(i_det * (1 << -shift))
        shift = 0
    px = [A[1][1] * bx[0] - A[0][1] * bx[1], -A[0][1] * bx[0] + A[0][0] * bx[1]]
    py = [A[1][1] * by[0] - A[0][1] * by[1], -A[0][1] * by[0] + A[0][0] * by[1]]
    lo, hi = -(1 << 13) + 1, (1 << 13) - 1

    def mult(p, diag, tag):
        v = round_signed(p * i_det, shift)
        l, h = ((1 << 16) + lo, (1 << 16) + hi) if diag else (lo, hi)
        if v < l:
            trace.add(tag + "_lo")
        if v > h:
            trace.add(tag + "_hi")
        return clamp(v, l, h)
    m = [0, 0, mult(px[0], True, "diag"), mult(px[1], False, "ndiag"), mult(py[0], False, "ndiag"), mult(py[1], True, "diag")]
    vx = i32(mvx * (1 << 13) - (isux * (m[2] - (1 << 16)) + isuy * m[3]))
    vy = i32(mvy * (1 << 13) - (isux * m[4] + isuy * (m[5] - (1 << 16))))
    wide += [mvx * (1 << 13), isux * (m[2] - (1 << 16)), isuy * m[3], isux * (m[2] - (1 << 16)) + isuy * m[3], mvx * (1 << 13) - (isux * (m[2] - (1 << 16)) + isuy * m[3]),
             mvy * (1 << 13), isux * m[4], isuy * (m[5] - (1 << 16)), isux * m[4] + isuy * (m[5] - (1 << 16)), mvy * (1 << 13) - (isux * m[4] + isuy * (m[5] - (1 << 16)))]
    if any(i32(v) != v for v in wide):
        trace.add("int32_left")  # a 32-bit intermediate of the reference wrapped
    for k, v in enumerate((vx, vy)):
        if v < -(1 << 23):
            trace.add(f"trans_lo_{k}")
        if v > (1 << 23) - 1:
            trace.add(f"trans_hi_{k}")
    m[0], m[1] = clamp(vx, -(1 << 23), (1 << 23) - 1), clamp(vy, -(1 << 23), (1 << 23) - 1)
    return 0, m


def fit_model(job, mv, shut_approx, lower_band_th, upper_band_th, trace=None):
    """the MV-dependent half of svt_aom_warped_motion_parameters on a MODEL_JOB_DTYPE record and an MV (row, col): a MODEL_DTYPE record"""
    trace = set() if trace is None else trace
    out = np.zeros((), MODEL_DTYPE)
    out["wmtype"] = AFFINE
    n, bw, bh = int(job["n_samples"]), int(job["bwidth"]), int(job["bheight"])
    if n == 0:
        return out
    pts, ref = [int(v) for v in job["pts"]], [int(v) for v in job["pts_inref"]]
    if n > 1:
        n, how = select_samples(mv[0], mv[1], pts, ref, n, bw, bh)
        trace.add("select_" + how)
    trace.add(f"thresh_{clamp(max(bw, bh), 16, 112)}")
    out["num_samples"] = n
    bad, mat = find_affine_int(n, pts, ref, bw, bh, mv[0], mv[1], int(job["blk_org_y"]) >> 2, int(job["blk_org_x"]) >> 2, trace)
    if bad:
        return out
    ok, sh = shear_params(mat)
    if not ok:
        trace.add("shear_refused")
        return out
    if not shut_approx:
        if abs(sh[0]) + abs(sh[1]) < lower_band_th and abs(sh[2]) + abs(sh[3]) < lower_band_th:
            trace.add("band_lower")
            ok = 0
        if 4 * abs(sh[0]) + 7 * abs(sh[1]) > upper_band_th and 4 * abs(sh[2]) + 4 * abs(sh[3]) > upper_band_th:
            trace.add("band_upper")
            ok = 0
    if ok:
        out["wmmat"], out["valid"] = mat, 1
        out["alpha"], out["beta"], out["gamma"], out["delta"] = sh
        trace.add("valid")
    return out


def model_job_status(job, n_mvs):
    if (int(job["bwidth"]), int(job["bheight"])) not in SIZES or int(job["n_samples"]) > 8:
        return ST_UNDEFINED
    if int(job["flags"]) & MV_FROM_ARRAY and int(job["mv_index"]) >= n_mvs:
        return ST_UNDEFINED
    return ST_OK


def restate_models(b, traces=None):
    """(MODEL_DTYPE [n] from the byte FILL, status [n]) as svt_hip_warp_model_batch leaves them"""
    n = len(b["jobs"])
    models = np.frombuffer(bytes([FILL]) * (n * np.dtype(MODEL_DTYPE).itemsize), MODEL_DTYPE).copy()
    status = np.zeros(n, np.uint8)
    mvs = b.get("mv_array")
    for i, j in enumerate(b["jobs"]):
        status[i] = model_job_status(j, 0 if mvs is None else len(mvs))
        if status[i] == ST_OK:
            mv = mvs[int(j["mv_index"])] if int(j["flags"]) & MV_FROM_ARRAY else j["mv"]
            t = set()
            models[i] = fit_model(j, (int(mv[0]), int(mv[1])), b["shut_approx"], b["lower_band_th"], b["upper_band_th"], t)
            if traces is not None:
                traces.append(t)
    return models, status


def model_job(rng, bw, bh, n, regime, mv=None):
    """a fit job: n samples around a bw x bh block whose motion is the MV plus an affine distortion and noise of the regime's size"""
    j = np.zeros((), MODEL_JOB_DTYPE)
    mv = (int(rng.integers(-200, 201)), int(rng.integers(-200, 201))) if mv is None else mv
    j["blk_org_x"], j["blk_org_y"] = int(rng.integers(0, 480)) * 4, int(rng.integers(0, 270)) * 4
    j["bwidth"], j["bheight"], j["n_samples"], j["mv"] = bw, bh, n, mv
    dist, noise, far = {"calm": (0.004, 2, 0), "mild": (0.03, 6, 0), "wild": (0.25, 20, 0), "huge": (0.9, 40, 0), "mixed": (0.03, 6, 200), "lost": (0.02, 4, 1200),
                        "same": (0.0, 0, 0)}[regime]
    a = rng.uniform(-dist, dist, 4)
    cx, cy = (bw // 2 - 1) * 8, (bh // 2 - 1) * 8
    for i in range(n):
        x, y = int(rng.integers(-33, bw + 33)) * 8 // 2 * 2, int(rng.integers(-33, bh + 33)) * 8 // 2 * 2
        if regime == "same":
            x, y = cx - 32, cy - 32  # every sample the same point: a singular system
        dx = a[0] * (x - cx) + a[1] * (y - cy) + rng.integers(-noise, noise + 1) + (far * int(rng.integers(-1, 2)) if i % 3 == 1 or regime == "lost" else 0)
        dy = a[2] * (x - cx) + a[3] * (y - cy) + rng.integers(-noise, noise + 1) + (far if regime == "lost" else 0)
        j["pts"][2 * i], j["pts"][2 * i + 1] = x, y
        j["pts_inref"][2 * i], j["pts_inref"][2 * i + 1] = x + mv[1] + int(round(dx)), y + mv[0] + int(round(dy))
    return j


MODEL_BATCHES = {"open": (1, 0, 65535), "m6": (0, 0, 65535), "bands": (0, 1 << 10, 1 << 14)}  # shut_approx, lower_band_th, upper_band_th


@functools.lru_cache(maxsize=None)
def model_batch(name):
    shut, lower, upper = MODEL_BATCHES[name]
    rng = np.random.default_rng(zlib.crc32(("model_" + name).encode()))
    jobs = []
    regimes = ("calm", "mild", "wild", "huge", "mixed", "lost", "same")
    for k in range(130):
        bw, bh = SIZES[k % len(SIZES)]
        jobs.append(model_job(rng, bw, bh, k % 9, regimes[(k // 3) % len(regimes)]))
    mvs = rng.integers(-300, 301, (16, 2)).astype(np.int16)
    for k in range(12):  # the MV from the array: the samples follow that MV
        j = model_job(rng, *SIZES[(5 * k) % len(SIZES)], 3 + k % 6, ("mild", "mixed", "calm")[k % 3], mv=(int(mvs[k][0]), int(mvs[k][1])))
        j["flags"], j["mv_index"], j["mv"] = MV_FROM_ARRAY, k, (-7, 9)
        jobs.append(j)
    return dict(name=name, shut_approx=shut, lower_band_th=lower, upper_band_th=upper, jobs=pack_jobs(jobs, MODEL_JOB_DTYPE), mv_array=mvs)


@functools.lru_cache(maxsize=None)
def restated_models(name):
    traces = []
    models, status = restate_models(model_batch(name), traces)
    return models, status, traces


MODEL_CONDITIONS = ["ls_mv_max", "det0", "shear_refused", "band_lower", "band_upper", "diag_lo", "diag_hi", "ndiag_lo", "ndiag_hi", "select_none", "select_all",
                    "select_swap", "thresh_16", "thresh_112", "valid"]


def model_coverage_missing(names=None):
    """the issue's conditions on the fit that the case lists do not meet.  Two are not in the list because no input reaches them: wmmat[2] <= 0
    (get_mult_shift_diag clamps wmmat[2] to at least 2^16 - 2^13 + 1) and the shift < 0 branch of find_affine_int (it needs |det| < 4; see
    tools/gen_warp_golden.py, which searches for such a system)."""
    seen, counts = set(), set()
    for name in (MODEL_BATCHES if names is None else names):
        b = model_batch(name)
        models, status, traces = restated_models(name)
        for t in traces:
            seen |= t
        counts |= {int(j["n_samples"]) for j in b["jobs"]}
    return [c for c in MODEL_CONDITIONS if c not in seen] + [f"n_samples {n}" for n in range(1, 9) if n not in counts]


def models_crc(models, status):
    """a CRC-32 per job over what the header defines: valid and num_samples always, the matrix and the shears of a valid fit"""
    out = np.zeros(len(models), np.uint32)
    for i, (m, st) in enumerate(zip(models, status)):
        if st != ST_OK:
            out[i] = 0xFFFFFFFF
            continue
        words = [int(m["valid"]), int(m["num_samples"]), int(m["wmtype"])]
        if int(m["valid"]):
            words += [int(v) for v in m["wmmat"]] + [int(m[k]) for k in ("alpha", "beta", "gamma", "delta")]
        out[i] = zlib.crc32(np.array(words, "<i4").tobytes())
    return out


# ---- the refinement ----
WM_START_FROM_ARRAY = 1
INT_MAX = 0x7FFFFFFF
MV_CENTRE = 1 << 14
REFINE_JOB_DTYPE = [("pts", "<i4", (16,)), ("pts_inref", "<i4", (16,)), ("src_offset", "<u4"), ("blk_org_x", "<u2"), ("blk_org_y", "<u2"), ("bwidth", "u1"),
                    ("bheight", "u1"), ("n_samples", "u1"), ("flags", "u1"), ("start_mv", "<i2", (2,)), ("pred_mv", "<i2", (2,)), ("mv_index", "<u4"), ("ref", "u1"),
                    ("reserved", "u1", (7,))]
NEIGHBOURS = [(0, 0), (0, -1), (1, 0), (0, 1), (-1, 0), (-1, 1), (1, 1), (1, -1), (-1, -1)]  # (row, col)


def mv_err_cost(mv, ref, tables, error_per_bit):
    """svt_aom_mv_err_cost: mv, ref = (row, col); tables = (mvjcost, row table, column table), the tables indexed from -16384"""
    jc, tr, tc = tables
    dr, dc = i16(int(mv[0]) - int(ref[0])), i16(int(mv[1]) - int(ref[1]))
    joint = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
    bits = int(jc[joint]) + int(tr[MV_CENTRE + clamp(dr, -MV_CENTRE, MV_CENTRE)]) + int(tc[MV_CENTRE + clamp(dc, -MV_CENTRE, MV_CENTRE)])
    return i32((bits * error_per_bit + (1 << 13)) >> 14)


def mv_err_cost_light(mv, ref):
    return 1296 + 50 * (abs(int(mv[1]) - int(ref[1])) + abs(int(mv[0]) - int(ref[0])))  # int arithmetic on the int16 fields: no wrap


def refine_cost(b, job, mv, detail=None):
    """the cost svt_aom_wm_motion_refinement gives the MV (row, col), or None when its fit is invalid; detail: a dict that receives the sum and the SSE
    of the differences, and the tiles of the warp in detail["seen"] (new_seen()) when it holds one"""
    s = b["settings"]
    fit = fit_model(job, mv, s["shut_approx"], s["lower_band_th"], s["upper_band_th"])
    if not int(fit["valid"]):
        return None
    bw, bh = int(job["bwidth"]), int(job["bheight"])
    view = dict(bit_depth=8, ss_x=0, ss_y=0, planes=b["planes"])
    pj = pred_job(0, int(job["blk_org_x"]), int(job["blk_org_y"]), bw, bh, [int(job["ref"])], [fit])
    pred = warp_block(view, pj, [model_of(fit)], None if detail is None else detail.get("seen"))
    y, x = divmod(int(job["src_offset"]), b["src"].shape[1])
    diff = pred - b["src"][y:y + bh, x:x + bw].astype(np.int64)
    sse, total = int((diff * diff).sum()), int(diff.sum())
    if detail is not None:
        detail["sum"], detail["sse"] = total, sse
    var = i32((sse - ((total * total) // (bw * bh) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    rate = mv_err_cost_light(mv, job["pred_mv"]) if s["approx_inter_rate"] else mv_err_cost(mv, job["pred_mv"], b["cost_tables"], max(1, s["error_per_bit"]))
    return i32(var + int(rate))


def refine_job_status(b, job):
    bw, bh = int(job["bwidth"]), int(job["bheight"])
    mvs = b.get("mv_array")
    ok = (bw, bh) in SIZES and int(job["n_samples"]) <= 8 and int(job["ref"]) < len(b["planes"])
    if int(job["flags"]) & WM_START_FROM_ARRAY:
        ok = ok and mvs is not None and int(job["mv_index"]) < len(mvs)
    ok = ok and int(job["src_offset"]) + (bh - 1) * b["src"].shape[1] + bw <= b["src"].size
    return ST_OK if ok else ST_UNDEFINED


def refine(b, job, trace=None, log=None):
    """the loop of svt_aom_wm_motion_refinement: ((row, col), best_cost, tot_checked_pos, the positions whose fit was valid).  log: a dict that receives
    "start", "costed" (the MV, its cost, the sum and the SSE of each warped position, in order), "record_hits" (the record index of every skip by
    mv_record), "wrapped" ((the component 0 row / 1 col, the value before the int16 wrap, the value recorded) of every recorded position that wrapped)
    and "seen" (the tiles of every warp)"""
    trace = set() if trace is None else trace
    if log is not None:
        log.update(costed=[], record_hits=[], wrapped=[], seen=new_seen())
    s = b["settings"]
    start = b["mv_array"][int(job["mv_index"])] if int(job["flags"]) & WM_START_FROM_ARRAY else job["start_mv"]
    centre = best = prev = (int(start[0]), int(start[1]))
    if log is not None:
        log["start"] = centre
    best_cost, record, n_valid = INT_MAX, [], 0
    stopped = "iterations"
    seen_valid = False
    for it in range(s["iterations"]):
        for i in range(1 if it else 0, 9 if s["refine_diag"] else 5):
            wide = (centre[0] + (NEIGHBOURS[i][0] << s["mv_prec_shift"]), centre[1] + (NEIGHBOURS[i][1] << s["mv_prec_shift"]))
            test = (i16(wide[0]), i16(wide[1]))
            if it:
                if test == prev:
                    trace.add("skip_prev")
                    continue
                if test in record:
                    trace.add("skip_record")
                    if log is not None:
                        log["record_hits"].append(record.index(test))
                    continue
            record.append(test)
            detail = None if log is None else {"seen": log["seen"]}
            if log is not None:
                log["wrapped"] += [(k, wide[k], test[k]) for k in range(2) if wide[k] != test[k]]
            cost = refine_cost(b, job, test, detail)
            if cost is None:
                trace.add("invalid_after_valid" if seen_valid else "invalid")
                continue
            seen_valid = True
            n_valid += 1
            if log is not None:
                log["costed"].append((test, cost, detail["sum"], detail["sse"]))
            if cost == best_cost:
                trace.add("tie")
            if cost < best_cost:
                best, best_cost = test, cost
        prev, centre = centre, best
        if prev == best:
            stopped = "centre"
            break
    trace.add("stop_" + stopped)
    if best_cost == INT_MAX:
        trace.add("none_valid")
    return best, best_cost, len(record), n_valid


def restate_refine(b, traces=None, logs=None):
    """the four outputs as svt_hip_wm_refine_batch leaves them, from the byte FILL, and n_valid [n]: the warps the reference runs per job; logs: a list
    that receives refine()'s log of every defined job"""
    n = len(b["jobs"])
    fill16, fill32 = np.frombuffer(bytes([FILL] * 2), "<i2")[0], np.frombuffer(bytes([FILL] * 4), "<i4")[0]
    out = {"best_mv": np.full((n, 2), fill16, np.int16), "best_cost": np.full(n, fill32, np.int32), "n_checked": np.full(n, fill32, np.int32).view(np.uint32),
           "status": np.zeros(n, np.uint8), "n_valid": np.zeros(n, np.int32)}
    for i, j in enumerate(b["jobs"]):
        out["status"][i] = refine_job_status(b, j)
        if out["status"][i] == ST_OK:
            t = set()
            log = None if logs is None else {}
            mv, cost, tot, n_valid = refine(b, j, t, log)
            if logs is not None:
                logs.append(log)
            out["best_mv"][i], out["best_cost"][i], out["n_checked"][i], out["n_valid"][i] = mv, cost, tot, n_valid
            if traces is not None:
                traces.append(t)
    return out


def cost_tables(rng):
    """(mvjcost [4], row table, column table [32769]): the rate grows with the component, like a real table"""
    ramp = (np.abs(np.arange(-MV_CENTRE, MV_CENTRE + 1)) * 3 + 200).astype(np.int32)
    return (np.array([11, 54, 5437, 342], np.int32), (ramp + rng.integers(0, 64, ramp.size)).astype(np.int32), (ramp + rng.integers(0, 64, ramp.size)).astype(np.int32))


def moving_planes(rng, pw, ph, pad=8):
    """an 8-bit source picture and a padded reference that is the source warped a little and displaced, so that the search has a minimum to find"""
    yy, xx = np.mgrid[0:ph + 2 * pad, 0:pw + 2 * pad + 3]
    base = 128 + 70 * np.sin(xx / 4.3 + yy / 11.0) + 50 * np.cos(yy / 3.7 - xx / 13.0) + rng.normal(0, 6, xx.shape)
    ref = np.clip(base, 0, 255).astype(np.uint8)
    src = np.clip(base[pad + 1:pad + 1 + ph, pad - 2:pad - 2 + pw] + rng.normal(0, 3, (ph, pw)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(src), (ref, pad, pad, pw, ph)


def refine_job(rng, x, y, bw, bh, pw, n, regime, start, pred, ref=0):
    m = model_job(rng, bw, bh, n, regime, mv=start)
    j = np.zeros((), REFINE_JOB_DTYPE)
    j["pts"], j["pts_inref"] = m["pts"], m["pts_inref"]
    j["src_offset"], j["blk_org_x"], j["blk_org_y"], j["bwidth"], j["bheight"], j["n_samples"] = y * pw + x, x, y, bw, bh, n
    j["start_mv"], j["pred_mv"], j["ref"] = start, pred, ref
    return j


REFINE_BATCHES = {  # iterations, refine_diag, mv_prec_shift, shut_approx, lower_band_th, upper_band_th, approx_inter_rate, error_per_bit
    "m6": (8, 0, 1, 0, 0, 65535, 0, 120), "full": (16, 1, 0, 0, 0, 65535, 0, 60), "light": (8, 1, 1, 1, 0, 65535, 1, 0), "one": (1, 0, 0, 0, 1 << 10, 65535, 0, 0),
    "flat": (8, 1, 0, 1, 0, 65535, 1, 1)}
SETTING_KEYS = ("iterations", "refine_diag", "mv_prec_shift", "shut_approx", "lower_band_th", "upper_band_th", "approx_inter_rate", "error_per_bit")
REFINE_SIZES = [(8, 8), (16, 16), (32, 16), (8, 8), (16, 16), (32, 16), (16, 8), (8, 16)]


@functools.lru_cache(maxsize=None)
def refine_batch(name):
    """a refinement batch on a 96x64 picture: blocks 8x8, 16x16, 32x16 (and one 64x64 in "m6"), the start MV given or taken from an array"""
    rng = np.random.default_rng(zlib.crc32(("refine_" + name).encode()))
    pw, ph = 96, 64
    src, plane = moving_planes(rng, pw, ph)
    if name == "flat":  # a flat source and reference: every position costs its rate alone, so equal rates tie and the first tested wins
        src = np.full_like(src, 90)
        plane = (np.full_like(plane[0], 90),) + plane[1:]
    planes = [plane, moving_planes(rng, pw, ph)[1]]
    jobs = []
    mvs = (rng.integers(-3, 4, (6, 2)) * 8).astype(np.int16)
    regimes = ("calm", "mild", "mixed", "mild", "wild", "lost", "same", "mild")
    for k in range(12 if name != "flat" else 6):
        bw, bh = REFINE_SIZES[k % len(REFINE_SIZES)]
        x, y = int(rng.integers(0, (pw - bw) // 4 + 1)) * 4, int(rng.integers(0, (ph - bh) // 4 + 1)) * 4
        start = (int(rng.integers(-3, 4)) * 8 + 8, int(rng.integers(-3, 4)) * 8 - 16)
        pred = (start[0] + int(rng.integers(-20, 21)), start[1] + int(rng.integers(-20, 21))) if name != "flat" else (start[0] - 3, start[1] - 3)  # two neighbours tie
        j = refine_job(rng, x, y, bw, bh, pw, (3 + k) % 9, regimes[k % len(regimes)], start, pred, ref=k % 2)
        if k % 4 == 3:
            j["flags"], j["mv_index"] = WM_START_FROM_ARRAY, k % len(mvs)
            j2 = refine_job(rng, x, y, bw, bh, pw, 5, "mild", (int(mvs[k % len(mvs)][0]), int(mvs[k % len(mvs)][1])), pred, ref=k % 2)
            j["pts"], j["pts_inref"], j["n_samples"] = j2["pts"], j2["pts_inref"], 5
        jobs.append(j)
    if name == "m6":
        jobs.append(refine_job(rng, 16, 0, 64, 64, pw, 6, "mild", (8, -16), (3, -9)))
    return dict(name=name, settings=dict(zip(SETTING_KEYS, REFINE_BATCHES[name])), planes=planes, src=src, jobs=pack_jobs(jobs, REFINE_JOB_DTYPE), mv_array=mvs,
                cost_tables=cost_tables(rng))


@functools.lru_cache(maxsize=None)
def restated_refine(name):
    traces = []
    return restate_refine(refine_batch(name), traces), traces


REFINE_CONDITIONS = ["stop_centre", "stop_iterations", "skip_record", "skip_prev", "invalid_after_valid", "none_valid", "tie"]


def refine_coverage_missing(names=None):
    seen = set()
    for name in (REFINE_BATCHES if names is None else names):
        for t in restated_refine(name)[1]:
            seen |= t
    return [c for c in REFINE_CONDITIONS if c not in seen]
