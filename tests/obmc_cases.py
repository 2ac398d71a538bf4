"""The cases of the OBMC entries (svt_hip_obmc_neighbour_batch, svt_hip_obmc_blend_batch, svt_hip_obmc_target_batch) and a numpy restatement of what
their jobs compute.

The reference's own results -- build_prediction_by_above_preds / _left_preds, av1_build_obmc_inter_prediction and calc_target_weighted_pred driven
block by block by tools/gen_obmc_golden.py on a scripted mode-info grid -- are in golden/obmc.npz as numbers only: per batch a CRC-32 per block and
plane of the two strip areas and of the blended block, a CRC-32 per block of wsrc and of mask, one whole block per size and depth, and the CRC-32 of
the mask rows.  The planes, blocks and predictions are regenerated from seeds here.

Restated (Source/Lib/Codec/enc_inter_prediction.c): the per-neighbour size, origin, strip position and edges of build_prediction_by_above_pred /
_left_pred (:743-777, 1133-1417) around inter_pred_cases.restate_job (svt_aom_enc_make_inter_predictor, single reference);
svt_av1_skip_u4x4_pred_in_obmc (Codec/inter_prediction.c:2282-2298); build_obmc_inter_pred_above / _left with the a64 vmask / hmask blends (:1430-1579);
calc_target_weighted_pred with its two visitors and the un_pack of 10-bit strips (:1581-1638, 1756-1816, 1857-1874); the mask rows (Codec/inter_prediction.c:2406-2429).

Geometry: inter_pred_cases' picture (192x128 in a padding of 160; 4:2:0 chroma 96x64 in 80).  A batch is one block array that every entry reads:
three neighbour launches (one per plane), three blend launches, one target launch."""
import functools
import os
import zlib

import numpy as np

import inter_pred_cases as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obmc.npz")
SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (8, 32), (32, 8), (16, 64), (64, 16)]  # luma (width, height)
MAX_NB = 4
MV_FROM_ARRAY = 1
ST_OK, ST_UNDEFINED = 0, 0xFF
FILL = 0xA5  # what every output buffer starts as, byte by byte
# the row of length n at [n, 2n): Obmc_Mask_1 .. Obmc_Mask_32
MASKS = np.array([0, 64, 45, 64, 39, 50, 59, 64, 36, 42, 48, 53, 57, 61, 64, 64, 34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64,
                  33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64], np.uint8)
NB_DTYPE = [("rel_pos", "u1"), ("size", "u1"), ("ref", "u1"), ("filter_x", "u1"), ("filter_y", "u1"), ("flags", "u1"), ("mv", "<i2", (2,)), ("reserved", "<u2"),
            ("mv_index", "<u4")]
BLOCK_DTYPE = [("org_x", "<i2"), ("org_y", "<i2"), ("width", "u1"), ("height", "u1"), ("n_above", "u1"), ("n_left", "u1"), ("mb_to_left_edge", "<i4"),
               ("mb_to_right_edge", "<i4"), ("mb_to_top_edge", "<i4"), ("mb_to_bottom_edge", "<i4"), ("strip_offset", "<u4"), ("reserved", "<u4"),
               ("above", NB_DTYPE, (MAX_NB,)), ("left", NB_DTYPE, (MAX_NB,))]
JOB_DTYPE = [("block", "<u4"), ("offset", "<u4")]
SS = (0, 1, 1)  # the sub-sampling of the three planes (4:2:0)


def crc(a, dtype="<u2"):
    return zlib.crc32(np.ascontiguousarray(a, dtype=dtype).tobytes())


def fill_array(n, dtype):
    return np.full(n, FILL * 0x0101 if np.dtype(dtype).itemsize == 2 else FILL, dtype)


def fill_i32(n):
    return np.full(n, FILL * 0x01010101, np.uint32).view(np.int32)


# ---- records --------------------------------------------------------------------------------------------------------------------------
def nb(rel, size, mv, ref=0, filters=(0, 0), mv_index=None):
    """one span: rel / size in 4-sample units, mv = (row, col) in 1/8 luma sample, filters = (x, y)"""
    r = np.zeros((), NB_DTYPE)
    r["rel_pos"], r["size"], r["ref"], r["filter_x"], r["filter_y"], r["mv"] = rel, size, ref, filters[0], filters[1], mv
    if mv_index is not None:
        r["flags"], r["mv_index"] = MV_FROM_ARRAY, mv_index
    return r


def make_block(w, h, org, above=(), left=(), edges=None):
    """org = (x, y) in luma samples; the edges are MacroBlockD's for a block of the picture unless given as (left, right, top, bottom)"""
    b = np.zeros((), BLOCK_DTYPE)
    b["org_x"], b["org_y"], b["width"], b["height"], b["n_above"], b["n_left"] = org[0], org[1], w, h, len(above), len(left)
    e = edges or (-(org[0] * 8), (ip.PIC_W - w - org[0]) * 8, -(org[1] * 8), (ip.PIC_H - h - org[1]) * 8)
    b["mb_to_left_edge"], b["mb_to_right_edge"], b["mb_to_top_edge"], b["mb_to_bottom_edge"] = e
    for k, r in enumerate(above):
        b["above"][k] = r
    for k, r in enumerate(left):
        b["left"][k] = r
    return b


def finish(name, bd, blocks, planes=ip.NOISE2, mv_array=None, run_planes=(0, 1, 2), src="noise", pred="noise", gap=24):
    """strip_offset of every block (areas of 3 * w * h samples, `gap` untouched samples between them) and the batch"""
    out = np.array(blocks, BLOCK_DTYPE)
    at = 8
    for i in range(len(out)):
        out[i]["strip_offset"] = at
        at += 3 * int(out[i]["width"]) * int(out[i]["height"]) + gap
    return {"name": name, "bit_depth": bd, "blocks": out, "planes": planes, "mv_array": mv_array, "run_planes": tuple(run_planes), "src": src, "pred": pred,
            "strip_samples": at}


def ref_planes(b, plane):
    """[(padded plane, org_x, org_y)] of one plane of every reference of a batch"""
    ss = SS[plane]
    p = ip.plane_dims(ss)[2]
    return [(ip.plane(kind, b["bit_depth"], ss, idx + 10 * plane if kind == "noise" else idx), p, p) for kind, idx in b["planes"]]


@functools.lru_cache(maxsize=None)
def src_plane(kind):
    """the 8-bit source luma plane from its sample (0, 0), [PIC_H][PIC_W]"""
    if kind == "noise":
        a = np.random.default_rng([20261020, 1]).integers(0, 256, (ip.PIC_H, ip.PIC_W)).astype(np.uint8)
    else:
        a = np.full((ip.PIC_H, ip.PIC_W), {"zero": 0, "max": 255}[kind], np.uint8)
    a.setflags(write=False)
    return a


# ---- the rule of a record -------------------------------------------------------------------------------------------------------------
def spans_ok(nbs, n, n4):
    end = 0
    for k in range(n):
        rel, size = int(nbs[k]["rel_pos"]), int(nbs[k]["size"])
        if rel & 1 or size < 2 or size & (size - 1) or rel < end or rel + size > n4:
            return False
        end = rel + size
    return True


def block_ok(blk):
    w, h = int(blk["width"]), int(blk["height"])
    if (w, h) not in SIZES or blk["n_above"] > MAX_NB or blk["n_left"] > MAX_NB:
        return False
    return spans_ok(blk["above"], int(blk["n_above"]), w >> 2) and spans_ok(blk["left"], int(blk["n_left"]), h >> 2)


def neighbour_job_defined(b, job, plane, n_refs=None, strip_samples=None):
    n_refs = len(b["planes"]) if n_refs is None else n_refs
    strip_samples = b["strip_samples"] if strip_samples is None else strip_samples
    if int(job["block"]) >= len(b["blocks"]):
        return False
    blk = b["blocks"][int(job["block"])]
    if not block_ok(blk):
        return False
    ok = int(blk["strip_offset"]) + (plane + 1) * int(blk["width"]) * int(blk["height"]) <= strip_samples
    for nbs, n in ((blk["above"], int(blk["n_above"])), (blk["left"], int(blk["n_left"]))):
        for k in range(n):
            ok = ok and nbs[k]["ref"] < n_refs and nbs[k]["filter_x"] <= 3 and nbs[k]["filter_y"] <= 3
            if nbs[k]["flags"] & MV_FROM_ARRAY:
                ok = ok and b["mv_array"] is not None and int(nbs[k]["mv_index"]) < len(b["mv_array"])
    return bool(ok)


def blend_job_defined(b, job, plane, dst_stride, dst_samples, strip_samples=None):
    strip_samples = b["strip_samples"] if strip_samples is None else strip_samples
    if int(job["block"]) >= len(b["blocks"]):
        return False
    blk = b["blocks"][int(job["block"])]
    if not block_ok(blk):
        return False
    w, h, ss = int(blk["width"]), int(blk["height"]), SS[plane]
    return int(blk["strip_offset"]) + (plane + 1) * w * h <= strip_samples and int(job["offset"]) + ((h >> ss) - 1) * dst_stride + (w >> ss) <= dst_samples


def target_job_defined(b, job, src_shape, out_values, strip_samples=None):
    strip_samples = b["strip_samples"] if strip_samples is None else strip_samples
    if int(job["block"]) >= len(b["blocks"]):
        return False
    blk = b["blocks"][int(job["block"])]
    if not block_ok(blk):
        return False
    w, h, x, y = int(blk["width"]), int(blk["height"]), int(blk["org_x"]), int(blk["org_y"])
    return int(blk["strip_offset"]) + w * h <= strip_samples and int(job["offset"]) + w * h <= out_values and x >= 0 and y >= 0 and \
        (y + h - 1) * src_shape[1] + x + w <= src_shape[0] * src_shape[1]


def skips_above(pw, ph):  # svt_av1_skip_u4x4_pred_in_obmc, dir 0
    return (pw, ph) in ((4, 4), (8, 4), (4, 8))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def strip_jobs(blk, plane, mv_array=None):
    """per predicted span of one plane of a block: (dir, the prediction as an inter_pred_cases job, strip row, strip column)"""
    ss, chroma = SS[plane], plane != 0
    W, H, ox, oy = int(blk["width"]), int(blk["height"]), int(blk["org_x"]), int(blk["org_y"])
    out = []
    for d in (0, 1):
        if d == 0 and skips_above(W >> ss, H >> ss):
            continue
        nbs, n = (blk["left"], int(blk["n_left"])) if d else (blk["above"], int(blk["n_above"]))
        for k in range(n):
            r = nbs[k]
            rel, size = int(r["rel_pos"]), int(r["size"])
            e = [int(blk[f]) for f in ("mb_to_left_edge", "mb_to_right_edge", "mb_to_top_edge", "mb_to_bottom_edge")]
            lx, ly, drow, dcol = ox, oy, 0, 0
            if d == 0:
                bw, bh = (size * 4) >> ss, ip.clamp(H >> (ss + 1), 4, 64 >> (ss + 1))
                lx += rel * 4
                dcol = (((rel * 4) >> 3) << 3) >> ss if chroma else rel * 4
                e[0], e[1], e[3] = -32 * ((ox >> 2) + rel), e[1] + ((W >> 2) - rel - size) * 32, e[3] + (H - min(H // 2, 32)) * 8
            else:
                bw, bh = ip.clamp(W >> (ss + 1), 4, 64 >> (ss + 1)), (size * 4) >> ss
                ly += rel * 4
                drow = (((rel * 4) >> 3) << 3) >> ss if chroma else rel * 4
                e[2], e[3], e[1] = -32 * ((oy >> 2) + rel), e[3] + ((H >> 2) - rel - size) * 32, e[1] + (W - min(W // 2, 32)) * 8
            j = np.zeros((), ip.JOB_DTYPE)
            j["width"], j["height"] = bw, bh
            j["org_x"], j["org_y"] = (((lx >> 3) << 3) >> ss, ((ly >> 3) << 3) >> ss) if chroma else (lx, ly)
            j["filter_x"], j["filter_y"], j["ref"] = r["filter_x"], r["filter_y"], (r["ref"], ip.NO_REF)
            j["mv"][0] = mv_array[int(r["mv_index"])] if r["flags"] & MV_FROM_ARRAY else r["mv"]
            j["mb_to_left_edge"], j["mb_to_right_edge"], j["mb_to_top_edge"], j["mb_to_bottom_edge"] = e
            out.append((d, j, drow, dcol))
    return out


def restate_neighbours(b, jobs_by_plane=None):
    """(above, left, events) after the neighbour launches of a batch: the two strip buffers (they start as FILL) and per plane and block the
    events of every predicted span: (dir, inter_pred_cases events).  jobs_by_plane: {plane: job array}, default every block on b["run_planes"]."""
    dt = np.uint16 if b["bit_depth"] > 8 else np.uint8
    bufs = [fill_array(b["strip_samples"], dt), fill_array(b["strip_samples"], dt)]
    events = {}
    for plane in b["run_planes"]:
        planes = ref_planes(b, plane)
        jobs = all_jobs(b) if jobs_by_plane is None else jobs_by_plane[plane]
        for job in jobs:
            if not neighbour_job_defined(b, job, plane):
                continue
            i = int(job["block"])
            blk = b["blocks"][i]
            W, H = int(blk["width"]), int(blk["height"])
            base = int(blk["strip_offset"]) + plane * W * H
            ev = []
            for d, j, drow, dcol in strip_jobs(blk, plane, b["mv_array"]):
                out, e = ip.restate_job(planes, b["bit_depth"], SS[plane], j)
                view = bufs[d][base:base + W * H].reshape(H, W)
                view[drow:drow + out.shape[0], dcol:dcol + out.shape[1]] = out
                ev.append((d, e))
            events[(plane, i)] = ev
    return bufs[0], bufs[1], events


def all_jobs(b, offsets=None):
    j = np.zeros(len(b["blocks"]), JOB_DTYPE)
    j["block"] = np.arange(len(j))
    if offsets is not None:
        j["offset"] = offsets
    return j


def covering(nbs, n, pos, ss):
    for k in range(n):
        if (int(nbs[k]["rel_pos"]) * 4) >> ss <= pos < ((int(nbs[k]["rel_pos"]) + int(nbs[k]["size"])) * 4) >> ss:
            return True
    return False


def a64(m, a, c):  # AOM_BLEND_A64
    return (m * a + (64 - m) * c + 32) >> 6


def restate_blend_block(blk, plane, above, left, block):
    """av1_build_obmc_inter_prediction on one plane block [ph][pw] (int64 in, int64 out); above / left: the block's strip areas of this plane"""
    ss = SS[plane]
    W, H = int(blk["width"]), int(blk["height"])
    pw, ph = W >> ss, H >> ss
    A, L = above.reshape(H, W).astype(np.int64), left.reshape(H, W).astype(np.int64)
    out = block.astype(np.int64).copy()
    if not skips_above(pw, ph):
        ov = (min(H, 64) >> 1) >> ss
        m = MASKS[ov:2 * ov].astype(np.int64)[:, None]
        for k in range(int(blk["n_above"])):
            r = blk["above"][k]
            c0, bw = (int(r["rel_pos"]) * 4) >> ss, (int(r["size"]) * 4) >> ss
            out[:ov, c0:c0 + bw] = a64(m, out[:ov, c0:c0 + bw], A[:ov, c0:c0 + bw])
    ov = (min(W, 64) >> 1) >> ss
    m = MASKS[ov:2 * ov].astype(np.int64)[None, :]
    for k in range(int(blk["n_left"])):
        r = blk["left"][k]
        r0, bh = (int(r["rel_pos"]) * 4) >> ss, (int(r["size"]) * 4) >> ss
        out[r0:r0 + bh, :ov] = a64(m, out[r0:r0 + bh, :ov], L[r0:r0 + bh, :ov])
    return out


def restate_target_block(blk, above, left, src, bd):
    """calc_target_weighted_pred on one block: (wsrc, mask) int32 [h * w]; above / left: the block's luma strip areas, src: the source block"""
    W, H = int(blk["width"]), int(blk["height"])
    un = (lambda a: (a.astype(np.int64) >> 2) & 0xFF) if bd > 8 else (lambda a: a.astype(np.int64))
    A, L = un(above.reshape(H, W)), un(left.reshape(H, W))
    wsrc, mask = np.zeros((H, W), np.int64), np.full((H, W), 64, np.int64)
    ov = min(H, 64) >> 1
    m0 = MASKS[ov:2 * ov].astype(np.int64)[:, None]
    for k in range(int(blk["n_above"])):
        c0, bw = int(blk["above"][k]["rel_pos"]) * 4, int(blk["above"][k]["size"]) * 4
        wsrc[:ov, c0:c0 + bw] = (64 - m0) * A[:ov, c0:c0 + bw]
        mask[:ov, c0:c0 + bw] = m0
    wsrc *= 64
    mask *= 64
    ov = min(W, 64) >> 1
    m0 = MASKS[ov:2 * ov].astype(np.int64)[None, :]
    for k in range(int(blk["n_left"])):
        r0, bh = int(blk["left"][k]["rel_pos"]) * 4, int(blk["left"][k]["size"]) * 4
        wsrc[r0:r0 + bh, :ov] = (wsrc[r0:r0 + bh, :ov] >> 6) * m0 + (L[r0:r0 + bh, :ov] << 6) * (64 - m0)
        mask[r0:r0 + bh, :ov] = (mask[r0:r0 + bh, :ov] >> 6) * m0
    wsrc = src.astype(np.int64) * 4096 - wsrc
    return wsrc.astype(np.int32).reshape(-1), mask.astype(np.int32).reshape(-1)


# ---- the prediction planes the blend works on and the outputs of a batch ----------------------------------------------------------------
PRED_STRIDE = 203  # odd: the rows of a block move through every alignment


@functools.lru_cache(maxsize=None)
def pred_layout(name, plane):
    """(job offsets, rows) of the blocks of a batch in the prediction plane of `plane`: shelves, every third block one sample further right"""
    b = batch(name)
    ss = SS[plane]
    fake = np.zeros(len(b["blocks"]), ip.JOB_DTYPE)
    fake["width"], fake["height"] = b["blocks"]["width"] >> ss, b["blocks"]["height"] >> ss
    packed, rows = ip.pack(list(fake), PRED_STRIDE, x_of=lambda i, x: x + i % 3)
    return packed["dst_offset"].astype(np.uint32), rows + 1


@functools.lru_cache(maxsize=None)
def pred_plane(name, plane):
    """the prediction plane [rows][PRED_STRIDE] before the blend: noise, or all 0 / all max"""
    b = batch(name)
    bd = b["bit_depth"]
    rows = pred_layout(name, plane)[1]
    dt, mx = (np.uint16 if bd > 8 else np.uint8), (1 << bd) - 1
    if b["pred"] == "noise":
        a = np.random.default_rng([20261020, 2, bd, plane, zlib.crc32(name.encode())]).integers(0, mx + 1, (rows, PRED_STRIDE)).astype(dt)
    else:
        a = np.full((rows, PRED_STRIDE), {"zero": 0, "max": mx}[b["pred"]], dt)
    a.setflags(write=False)
    return a


def block_of(plane, offset, w, h):
    y, x = divmod(int(offset), plane.shape[1])
    return plane[y:y + h, x:x + w]


def restate_blend(b, plane, above, left, dst, jobs):
    """the prediction plane after one blend launch (the jobs in order, on a copy of dst)"""
    out = dst.copy()
    ss = SS[plane]
    for job in jobs:
        if not blend_job_defined(b, job, plane, dst.shape[1], dst.size):
            continue
        blk = b["blocks"][int(job["block"])]
        W, H = int(blk["width"]), int(blk["height"])
        base = int(blk["strip_offset"]) + plane * W * H
        view = block_of(out, job["offset"], W >> ss, H >> ss)
        view[:] = restate_blend_block(blk, plane, above[base:base + W * H], left[base:base + W * H], view)
    return out


def target_offsets(b):
    """where every block's w * h values go in wsrc and mask: one after the other, three untouched values between them; (offsets, out_values)"""
    sizes = b["blocks"]["width"].astype(np.int64) * b["blocks"]["height"] + 3
    off = np.concatenate([[5], 5 + np.cumsum(sizes)[:-1]]) if len(sizes) else np.zeros(0, np.int64)
    return off.astype(np.uint32), int(5 + sizes.sum())


def restate_target(b, above, left, jobs, out_values, src=None):
    """(wsrc, mask) int32 [out_values] after the target launch; they start as FILL"""
    src = src_plane(b["src"]) if src is None else src
    wsrc, mask = fill_i32(out_values), fill_i32(out_values)
    for job in jobs:
        if not target_job_defined(b, job, src.shape, out_values):
            continue
        blk = b["blocks"][int(job["block"])]
        W, H, x, y, o, so = int(blk["width"]), int(blk["height"]), int(blk["org_x"]), int(blk["org_y"]), int(job["offset"]), int(blk["strip_offset"])
        wsrc[o:o + W * H], mask[o:o + W * H] = restate_target_block(blk, above[so:so + W * H], left[so:so + W * H], src[y:y + H, x:x + W], b["bit_depth"])
    return wsrc, mask


@functools.lru_cache(maxsize=None)
def restated(name):
    """everything a batch computes, every block a job of every launch: {"above", "left", "events", "blend": {plane: plane after}, "wsrc", "mask"}"""
    b = batch(name)
    above, left, events = restate_neighbours(b)
    out = {"above": above, "left": left, "events": events, "blend": {}}
    for plane in b["run_planes"]:
        out["blend"][plane] = restate_blend(b, plane, above, left, pred_plane(name, plane), all_jobs(b, pred_layout(name, plane)[0]))
    if 0 in b["run_planes"]:
        off, n = target_offsets(b)
        out["wsrc"], out["mask"] = restate_target(b, above, left, all_jobs(b, off), n)
    return out


def fixture_arrays(name, res):
    """what the fixture holds of a batch, from results laid out as restated()'s: CRCs [n_blocks][planes run] of the strip areas and the blended
    blocks, CRCs [n_blocks] of wsrc and mask"""
    b = batch(name)
    out = {}
    n, planes = len(b["blocks"]), b["run_planes"]
    crcs = {k: np.zeros((n, len(planes)), np.uint32) for k in ("above", "left", "blend")}
    for i, blk in enumerate(b["blocks"]):
        W, H = int(blk["width"]), int(blk["height"])
        for c, plane in enumerate(planes):
            base = int(blk["strip_offset"]) + plane * W * H
            crcs["above"][i, c], crcs["left"][i, c] = crc(res["above"][base:base + W * H]), crc(res["left"][base:base + W * H])
            crcs["blend"][i, c] = crc(block_of(res["blend"][plane], pred_layout(name, plane)[0][i], W >> SS[plane], H >> SS[plane]))
    for k, v in crcs.items():
        out[f"{k}_{name}"] = v
    if 0 in planes:
        off = target_offsets(b)[0]
        area = lambda a, i: a[int(off[i]):int(off[i]) + int(b["blocks"][i]["width"]) * int(b["blocks"][i]["height"])]
        out[f"wsrc_{name}"] = np.array([crc(area(res["wsrc"], i), "<i4") for i in range(n)], np.uint32)
        out[f"mask_{name}"] = np.array([crc(area(res["mask"], i), "<i4") for i in range(n)], np.uint32)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def rnd_mv(rng, reach=10):
    """an MV in 1/8 luma sample, any phase"""
    return (int(rng.integers(-reach * 8, reach * 8 + 1)), int(rng.integers(-reach * 8, reach * 8 + 1)))


def rnd_nb(rng, rel, size, n_refs=2):
    return nb(rel, size, rnd_mv(rng), int(rng.integers(0, n_refs)), (int(rng.integers(0, 4)), int(rng.integers(0, 4))))


def rnd_org(rng, w, h):
    """a luma origin on the 8-sample grid, the block inside the picture"""
    return (int(rng.integers(0, (ip.PIC_W - w) // 8 + 1)) * 8, int(rng.integers(0, (ip.PIC_H - h) // 8 + 1)) * 8)


def span_patterns(n4):
    """the span lists of one side of n4 4-sample units, as [(rel, size)], within max_neighbor_obmc's cap (1, 2, 3, 4 spans on 8, 16, 32, 64 samples):
    none, one over the whole side, halves, a gap at either end, a gap in the middle, gaps at both ends, and `most`: as many spans as the cap allows
    (on 32 and 64 samples 8-sample spans up to the cap, so that the cap leaves a gap at the end; on 64 also the four quarters)"""
    pats = {"none": [], "full": [(0, n4)]}
    if n4 >= 4:
        pats["halves"] = [(0, n4 // 2), (n4 // 2, n4 // 2)]
        pats["gap_start"] = [(n4 // 2, n4 // 2)]
        pats["gap_end"] = [(0, n4 // 2)]
    if n4 >= 8:
        q = n4 // 4
        pats["gap_middle"] = [(0, q), (3 * q, q)]
        pats["gap_both_ends"] = [(q, q), (2 * q, q)]
        pats["capped"] = [(2 * k, 2) for k in range(3 if n4 == 8 else 4)]
    if n4 == 8:
        pats["three"] = [(0, 2), (2, 2), (4, 4)]
    if n4 == 16:
        pats["quarters"] = [(4 * k, 4) for k in range(4)]
    return pats


def most(pats):
    return "quarters" if "quarters" in pats else "three" if "three" in pats else "halves" if "halves" in pats else "full"


def sizes_batch(w, h, bd):
    """group 1, per size and depth: every pairing of an above pattern with `full` / `none` on the left and the reverse, random MVs of any phase, two
    references, random dual filters (each of the four, different in x and y), at random origins"""
    rng = np.random.default_rng([1, w, h, bd])
    pa, pl = span_patterns(w >> 2), span_patterns(h >> 2)
    combos = [(a, l) for a in pa for l in ("full", "none")] + [(a, l) for l in pl for a in ("full", "none") if l not in ("full", "none")]
    combos.append((most(pa), most(pl)))
    blocks = []
    for a, l in combos:
        blocks.append(make_block(w, h, rnd_org(rng, w, h), [rnd_nb(rng, r, s) for r, s in pa[a]], [rnd_nb(rng, r, s) for r, s in pl[l]]))
    return finish(f"sizes_{w}x{h}_{bd}", bd, blocks)


def phases_batch(bd):
    """group 2: all 16 x 16 phase pairs of the chroma planes (all 8 x 8 of luma) on 16x16 blocks, one above and one left neighbour each, the four
    filters in turn"""
    blocks = []
    for p in range(256):
        pr, pc = p >> 4, p & 15
        f = (p & 3, (p >> 2) & 3)
        blocks.append(make_block(16, 16, (16 + 8 * (p % 19), 16 + 8 * (p % 11)), [nb(0, 4, (16 * (p % 3 - 1) + pr, 16 * (p % 5 - 2) + pc), p & 1, f)],
                                 [nb(0, 4, (-16 + pc, 32 + pr), 1 - (p & 1), f[::-1])]))
    return finish(f"phases_{bd}", bd, blocks)


def clamp_batch(bd):
    """group 3: blocks at the four corners and edges of the picture whose neighbours' MVs point far outside each side, at each limit of the
    neighbour's own (modified) edges, one below and one above it; one MV taken from mv_array"""
    rng = np.random.default_rng([3, bd])
    blocks = []
    mv_array = np.array([[-1900, 1900], [7, -1900], [1900, -3], [33, 21]], np.int16)
    for w, h in ((16, 16), (32, 16), (8, 32), (64, 64)):
        xs, ys = sorted({0, ((ip.PIC_W - w) // 16) * 8, ip.PIC_W - w}), sorted({0, ((ip.PIC_H - h) // 16) * 8, ip.PIC_H - h})
        for org in [(x, y) for x in xs for y in ys if x in (0, ip.PIC_W - w) or y in (0, ip.PIC_H - h)]:
            probe = make_block(w, h, org, [nb(0, w >> 2, (0, 0))], [nb(0, h >> 2, (0, 0))])
            ja, jl = (j for _, j, _, _ in strip_jobs(probe, 0))
            far = 1900
            for k, mv in enumerate([(3, -far), (-5, far), (-far, 3), (far, -5), (-far + 1, -far + 2), (far - 1, far - 3)]):
                f = (int(rng.integers(0, 4)), int(rng.integers(0, 4)))
                blocks.append(make_block(w, h, org, [nb(0, w >> 2, mv, k & 1, f)], [nb(0, h >> 2, mv[::-1] if k < 4 else mv, 1 - (k & 1), f)]))
            if w == 64:
                continue
            la, ll = ip.clamp_limits(ja, 0), ip.clamp_limits(jl, 0)
            for d in (-1, 0, 1):
                for side in range(4):
                    mva = (5, la[side] + d) if side < 2 else (la[side] + d, 7)
                    mvl = (-3, ll[side] + d) if side < 2 else (ll[side] + d, -1)
                    blocks.append(make_block(w, h, org, [nb(0, w >> 2, mva, 0, (0, 2))], [nb(0, h >> 2, mvl, 1, (1, 3))]))
    for i in range(4):
        blocks.append(make_block(16, 16, (0, 0) if i < 2 else (ip.PIC_W - 16, ip.PIC_H - 16), [nb(0, 2, (0, 0), 0, (0, 0), mv_index=i), nb(2, 2, (9, 9), 1, (2, 1))],
                                 [nb(0, 4, (0, 0), 1, (3, 0), mv_index=3 - i)]))
    return finish(f"clamp_{bd}", bd, blocks, mv_array=mv_array)


def plane_edge_batch(bd, chroma):
    """group 4: records whose own edges let the clamped MV take the reads to the first and the last row and column of the padded plane (the
    conservative bound of inter_pred_cases: three samples before, four after the block); luma launches only, or chroma launches only"""
    ss = 1 if chroma else 0
    pw, ph, pad = ip.plane_dims(ss)
    m = 1 << (1 - ss)  # the clamp works in 1/16 of this plane's samples; the record's edges are 1/8 luma
    blocks = []
    for w, h in ((16, 16), (32, 16)):
        ox, oy = 48, 32
        bwa, bha = w >> ss, max(h >> (ss + 1), 4)  # the above strip on this plane
        bwl, bhl = max(w >> (ss + 1), 4), h >> ss
        px, py = ox >> ss, oy >> ss
        nat = [-(ox * 8), (ip.PIC_W - w - ox) * 8, -(oy * 8), (ip.PIC_H - h - oy) * 8]
        edged = lambda side, v: tuple(v if s == side else e for s, e in enumerate(nat))
        # an above strip takes the record's top, a left strip its left: pos = org + edge * m / 16 - (4 + b), and the reads start at pos - 3 = -pad
        blocks.append(make_block(w, h, (ox, oy), [nb(0, w >> 2, (-3000, 5), 0, (0, 0))], [], edged(2, (-pad + 7 + bha - py) * 16 // m)))
        blocks.append(make_block(w, h, (ox, oy), [], [nb(0, h >> 2, (3, -3000), 1, (2, 2))], edged(0, (-pad + 7 + bwl - px) * 16 // m)))
        # above: bottom = record + (h - h / 2) * 8, pos = org + bottom * m / 16 + 4 + b - 1, and the reads end at pos + b + 4 = plane height + pad
        blocks.append(make_block(w, h, (ox, oy), [nb(0, w >> 2, (3000, 5), 0, (0, 0))], [], edged(3, (ph + pad - py - 2 * bha - 7) * 16 // m - (h - h // 2) * 8)))
        blocks.append(make_block(w, h, (ox, oy), [], [nb(0, h >> 2, (3, 3000), 1, (2, 2))], edged(1, (pw + pad - px - 2 * bwl - 7) * 16 // m - (w - w // 2) * 8)))
    return finish(f"plane_edge_{'chroma' if chroma else 'luma'}_{bd}", bd, blocks, run_planes=(1, 2) if chroma else (0,))


def extremes_batch(bd, pred, src):
    """group 5: strips of all 0 and all max (references 0 and 1) under a prediction and a source of all 0 / all max: the ends of the blend and of wsrc;
    the corner where both passes act is in every block"""
    blocks = []
    for w, h in ((8, 8), (16, 8), (32, 32), (64, 64)):
        for ra, rl in ((0, 0), (1, 1), (0, 1), (1, 0)):
            blocks.append(make_block(w, h, (64, 32), [nb(0, w >> 2, (5, -3), ra, (2, 2))], [nb(0, h >> 2, (-7, 9), rl, (2, 2))]))
    return finish(f"extremes_{bd}_{pred}_{src}", bd, blocks, planes=[("zero", 0), ("max", 0)], src=src, pred=pred)


@functools.lru_cache(maxsize=None)
def batch_names():
    names = []
    for bd in (8, 10):
        names += [f"sizes_{w}x{h}_{bd}" for w, h in SIZES]
        names += [f"phases_{bd}", f"clamp_{bd}", f"plane_edge_luma_{bd}", f"plane_edge_chroma_{bd}", f"extremes_{bd}_zero_max", f"extremes_{bd}_max_zero"]
    return tuple(names)


@functools.lru_cache(maxsize=None)
def batch(name):
    p = name.split("_")
    if p[0] == "sizes":
        w, h = (int(v) for v in p[1].split("x"))
        return sizes_batch(w, h, int(p[2]))
    if p[0] == "phases":
        return phases_batch(int(p[1]))
    if p[0] == "clamp":
        return clamp_batch(int(p[1]))
    if p[0] == "plane":
        return plane_edge_batch(int(p[3]), p[2] == "chroma")
    return extremes_batch(int(p[1]), p[2], p[3])


def sample_blocks():
    """(key, batch name, block index): the blocks whose whole luma results the fixture holds -- per size and depth the block with the most spans on both sides, the last of its batch"""
    return [(f"sample_{w}x{h}_{bd}", f"sizes_{w}x{h}_{bd}", len(batch(f"sizes_{w}x{h}_{bd}")["blocks"]) - 1) for bd in (8, 10) for w, h in SIZES]


def sample_arrays(name, i, res):
    """the whole luma results of one block: above area, left area, blended block, wsrc, mask, concatenated as int32"""
    b = batch(name)
    blk = b["blocks"][i]
    W, H, so = int(blk["width"]), int(blk["height"]), int(blk["strip_offset"])
    o = int(target_offsets(b)[0][i])
    parts = [res["above"][so:so + W * H], res["left"][so:so + W * H], block_of(res["blend"][0], pred_layout(name, 0)[0][i], W, H).reshape(-1),
             res["wsrc"][o:o + W * H], res["mask"][o:o + W * H]]
    return np.concatenate([np.asarray(p).astype(np.int32) for p in parts])


def coverage_missing():
    """the conditions of the issue's case list that the batches do not meet, as text (on the restatement, which the generator compares with the
    reference on every job)"""
    missing = []
    moved, kept, phases, filters, variants = set(), set(), {1: set(), 0: set()}, set(), set()
    for name in batch_names():
        b, res = batch(name), restated(name)
        for (plane, i), evs in res["events"].items():
            for d, e in evs:
                if not e["inside"]:
                    missing.append(f"{name} block {i} plane {plane}: a read leaves the padded plane")
                variant, mv = e["refs"][0]
                variants.add((b["bit_depth"], plane != 0, variant))
                for s in range(4):
                    (moved if mv[s] else kept).add((d, s))
        if name.startswith("phases"):
            for blk in b["blocks"]:
                for r in (blk["above"][0], blk["left"][0]):
                    phases[1].add((int(r["mv"][0]) & 15, int(r["mv"][1]) & 15))
                    phases[0].add((int(r["mv"][0]) * 2 & 15, int(r["mv"][1]) * 2 & 15))
        for blk in b["blocks"]:
            for nbs, n in ((blk["above"], int(blk["n_above"])), (blk["left"], int(blk["n_left"]))):
                filters |= {(int(nbs[k]["filter_x"]), int(nbs[k]["filter_y"])) for k in range(n)}
    sides = ("left", "right", "top", "bottom")
    missing += [f"the clamp never moved an MV of {'a left' if d else 'an above'} neighbour on the {sides[s]}" for d in (0, 1) for s in range(4) if (d, s) not in moved]
    missing += [f"the clamp never left an MV alone: dir {d} side {sides[s]}" for d in (0, 1) for s in range(4) if (d, s) not in kept]
    if len(phases[1]) != 256 or len(phases[0]) != 64:
        missing.append(f"phase pairs: {len(phases[1])} of 256 on chroma, {len(phases[0])} of 64 on luma")
    if filters != {(x, y) for x in range(4) for y in range(4)}:
        missing.append("a pair of filters never appears")
    missing += [f"convolve function not run: depth {bd} chroma {c} {ip.VARIANTS[v]}" for bd in (8, 10) for c in (False, True) for v in range(4) if (bd, c, v) not in variants]
    return missing


# ---- per-job refusals and descriptors made invalid --------------------------------------------------------------------------------------
UNDEFINED_KINDS = ["size_128", "size_4", "size_8x64", "n_above", "n_left", "span_leaves", "span_odd_rel", "span_odd_size", "span_size_6", "span_zero", "span_order", "ref",
                   "filter_x", "filter_y", "mv_index", "strip_end"]


def undefined_batch(bd):
    """ordinary blocks with one undefined block of every kind among them, and the jobs of the three launches with a block index outside the array
    last: (batch, {kind: block index})"""
    rng = np.random.default_rng([7, bd])
    blocks, bad = [], {}
    mv_array = rng.integers(-60, 61, (5, 2)).astype(np.int16)
    for kind in UNDEFINED_KINDS:
        for _ in range(2):
            w, h = SIZES[int(rng.integers(0, len(SIZES)))]
            blocks.append(make_block(w, h, rnd_org(rng, w, h), [rnd_nb(rng, 0, w >> 2)], [rnd_nb(rng, 0, h >> 2)] if h == 8 else [rnd_nb(rng, 0, h >> 3), rnd_nb(rng, h >> 3, h >> 3)]))
        b = make_block(16, 16, (32, 32), [rnd_nb(rng, 0, 2), rnd_nb(rng, 2, 2)], [nb(0, 4, (3, 3), 1, (1, 2), mv_index=4)])
        if kind.startswith("size"):
            b["width"], b["height"] = {"size_128": (128, 64), "size_4": (16, 4), "size_8x64": (8, 64)}[kind]
            b["above"][0]["size"], b["above"][1]["rel_pos"], b["above"][1]["size"], b["left"][0]["size"] = 2, 0, 0, 1  # spans a smaller side would hold
            b["n_above"], b["n_left"] = 1, 0
        elif kind == "n_above":
            b["n_above"] = 5
        elif kind == "n_left":
            b["n_left"] = 200
        elif kind == "span_leaves":
            b["above"][1]["size"] = 4
        elif kind == "span_odd_rel":
            b["above"][1]["rel_pos"], b["above"][1]["size"] = 3, 1
        elif kind == "span_odd_size":
            b["left"][0]["size"] = 3
        elif kind == "span_size_6":
            b["width"], b["above"][0]["size"], b["n_above"] = 32, 6, 1
        elif kind == "span_zero":
            b["above"][0]["size"] = 0
        elif kind == "span_order":
            b["above"][1]["rel_pos"] = 0
        elif kind == "ref":
            b["above"][1]["ref"] = 2
        elif kind in ("filter_x", "filter_y"):
            b["left"][0][kind] = 4
        elif kind == "mv_index":
            b["left"][0]["mv_index"] = 5
        bad[kind] = len(blocks)
        blocks.append(b)
    out = finish(f"undefined_{bd}", bd, blocks, mv_array=mv_array)
    out["blocks"][bad["strip_end"]]["strip_offset"] = out["strip_samples"] - 3 * 16 * 16 + 1  # one sample too far for the last plane
    return out, bad


NEIGHBOUR_ONLY = ("ref", "filter_x", "filter_y", "mv_index")  # what only the neighbour launch refuses


def spoil_desc(d, bad):
    """a descriptor of any of the three entries made invalid in the way `bad` names"""
    if bad == "zero_ref_stride":
        d.refs[1].stride = 0
    elif bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith("zero_"):
        assert hasattr(type(d), bad[5:])
        setattr(d, bad[5:], 0)
    elif bad.startswith(("bit_depth", "strip_bit_depth", "ss_", "n_refs", "plane")):
        name, v = bad.rsplit("_", 1)
        setattr(d, name, int(v))
    elif bad == "luma_with_ss":
        d.plane, d.ss_x = 0, 1
    elif bad == "null_plane":
        d.refs[1].plane = None
    elif bad == "stride_below_width":
        d.refs[0].stride = 200
    elif bad == "org_outside":
        d.refs[1].org_y = 224
    else:
        assert bad == "n_mvs_without_mv_array"
        d.n_mvs = 3
    return d
