"""Shared pieces of the full-pel refinement search tests (svt_pme_sad_loop_kernel): job grids after test/SadTest.cc:1580-1640 (large and
small blocks, search areas, sparse steps, random 16-bit component costs), the edge sets (edge_sets: every search width and height that moves
a loop bound, item counts around the wave size, ties, source and reference planes of different widths) with a plain walk of the reference's
visiting order to count what they cover, and the three runners (reference build, oracle, HIP)."""
import ctypes as C
import os

import numpy as np

from svt_av1_psyex_amd import abi

MV_CENTRE = 1 << 14  # tables of 2 * MV_CENTRE + 1 entries: every index the reference's clamp (MV_LOW .. MV_UPP) can produce is valid


def cost_tables(rng):
    """(mvjcost[4], row table, column table) with the centre at index MV_CENTRE"""
    j = np.array([11, 54, 5437, 342], np.int32)
    return j, rng.integers(0, 1 << 16, 2 * MV_CENTRE + 1).astype(np.int32), rng.integers(0, 1 << 16, 2 * MV_CENTRE + 1).astype(np.int32)


def random_jobs(rng, plane_w, plane_h, n, wild=False):
    """n searches inside a plane_w x plane_h reference plane; wild: base vectors and start positions over the whole int16 range (the
    reference's own unit test), otherwise values a mode-decision call site produces (small refinements around the candidate)"""
    sizes = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 16), (16, 8), (32, 16), (16, 64), (64, 128), (128, 128), (128, 64), (4, 16), (64, 16)]
    jobs = np.zeros(n, abi.PME_JOB_DTYPE)
    for i in range(n):
        bw, bh = sizes[rng.integers(len(sizes))]
        step = int(rng.choice([1, 1, 2, 3, 8]))
        sa_w = int(rng.choice([8, 16, 24, 40])); sa_h = int(rng.integers(1, 24))
        sa_w = min(sa_w, (plane_w - bw - 8) // 8 * 8); sa_h = max(1, min(sa_h, plane_h - bh - 1))
        x0, y0 = rng.integers(0, plane_w - bw - sa_w - 3), rng.integers(0, plane_h - bh - sa_h + 1)
        sx, sy = rng.integers(0, plane_w - bw + 1), rng.integers(0, plane_h - bh + 1)
        j = jobs[i]
        j["src_offset"], j["ref_offset"], j["width"], j["height"] = sy * plane_w + sx, y0 * plane_w + x0, bw, bh
        j["sa_w"], j["sa_h"], j["step"] = sa_w, sa_h, step
        if wild:
            j["mvx"], j["mvy"], j["start_x"], j["start_y"] = rng.integers(-32768, 32768, 4)
            j["ref_mv"] = (23, 76)
        else:
            j["mvx"], j["mvy"] = rng.integers(-400, 401, 2) * 8
            j["start_x"], j["start_y"] = -(sa_w // 2), -(sa_h // 2)
            j["ref_mv"] = rng.integers(-300, 301, 2)
        j["best_cost"] = int(rng.choice([0xFFFFFFFF, 0xFFFFFFFF, 5000, 200000, 0]))
        j["best_mvx"], j["best_mvy"] = rng.integers(-100, 100, 2)
    return jobs


# ---- edge cases: widths that are no multiple of 8, empty searches, item counts around the wave size, ties, unequal strides ----------------
GOLDEN_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pme_edges.npz")
EDGE_STRIDES = (131, 227)  # source / reference plane widths
EDGE_H = 200               # both planes' height
EDGE_STEPS = (1, 2, 3, 8, 9)
EDGE_BLOCKS = [(4, 4), (8, 8), (16, 8)]
EDGE_EPB = 20542


def visit_order(sa_w, sa_h, step):
    """the (xs, ys) svt_pme_sad_loop_kernel_c visits, in its order: a plain walk of its two loops (Codec/product_coding_loop.c:1916-1953),
    col_num and search_step_x carried from row to row as the reference carries them"""
    out, col_num, step_x, ys = [], 0, 1, 0
    while ys < sa_h:
        xs = 0
        while xs < sa_w:
            if sa_w - xs < 8 and col_num == 0:
                xs += step_x
                continue
            if col_num == 7:
                col_num, step_x = 0, step
            else:
                col_num, step_x = col_num + 1, 1
            out.append((xs, ys))
            xs += step_x
        ys += step
    return out


def visit_sads(src, ref, job):
    """(positions, SADs) of one job in visiting order, in numpy on the 2-D planes"""
    pos = visit_order(int(job["sa_w"]), int(job["sa_h"]), int(job["step"]))
    bw, bh = int(job["width"]), int(job["height"])
    (sy, sx), (ry, rx) = divmod(int(job["src_offset"]), src.shape[1]), divmod(int(job["ref_offset"]), ref.shape[1])
    blk = src[sy:sy + bh, sx:sx + bw].astype(np.int32)
    return pos, np.array([np.abs(blk - ref[ry + ys:ry + ys + bh, rx + xs:rx + xs + bw]).sum() for xs, ys in pos], np.int64)


def read_extent(job):
    """(columns, rows) of the reference window the reference reads for one job: (0, 0) when nothing is visited"""
    pos = visit_order(int(job["sa_w"]), int(job["sa_h"]), int(job["step"]))
    if not pos:
        return 0, 0
    return max(x for x, _ in pos) + int(job["width"]), max(y for _, y in pos) + int(job["height"])


def _job(rng, src_xy, ref_xy, block, sa_w, sa_h, step, best=None):
    j = np.zeros(1, abi.PME_JOB_DTYPE)[0]
    j["src_offset"], j["ref_offset"] = src_xy[1] * EDGE_STRIDES[0] + src_xy[0], ref_xy[1] * EDGE_STRIDES[1] + ref_xy[0]
    j["width"], j["height"], j["sa_w"], j["sa_h"], j["step"] = block[0], block[1], sa_w, sa_h, step
    j["mvx"], j["mvy"] = rng.integers(-400, 401, 2) * 8
    j["start_x"], j["start_y"] = -(sa_w // 2), -(sa_h // 2)
    j["ref_mv"] = rng.integers(-300, 301, 2)
    j["best_cost"] = int(rng.choice([0xFFFFFFFF, 0xFFFFFFFF, 5000, 200000, 0])) if best is None else best
    j["best_mvx"], j["best_mvy"] = rng.integers(-100, 100, 2)
    return j


def _placed(rng, block, sa_w, sa_h, step, best=None):
    """a job at a random place where its window (at least one sample wide and high) fits the reference plane"""
    bw, bh = block
    sx, sy = int(rng.integers(0, EDGE_STRIDES[0] - bw + 1)), int(rng.integers(0, EDGE_H - bh + 1))
    rx, ry = int(rng.integers(0, EDGE_STRIDES[1] - bw - max(sa_w, 1) + 1)), int(rng.integers(0, EDGE_H - bh - max(sa_h, 1) + 1))
    return _job(rng, (sx, sy), (rx, ry), block, sa_w, sa_h, step, best)


def _tie_incoming(src, ref, jobs, every):
    """every `every`-th job that visits something: best_cost = its smallest SAD (the strict `<` loses under the cost types without an MV
    rate) or one more (it wins)"""
    for k, i in enumerate(range(0, len(jobs), every)):
        sads = visit_sads(src, ref, jobs[i])[1]
        if len(sads):
            jobs[i]["best_cost"] = int(sads.min()) + (k & 1)


def edge_sets():
    """{name: (src, ref, jobs, tables)}, seeded.  The planes are 2-D arrays EDGE_STRIDES wide (source 131, reference 227)."""
    sw, rw = EDGE_STRIDES
    sets = {}
    # grid: every width / height that moves a loop bound, blocks cycling through 4x4, 8x8 and 16x8
    rng = np.random.default_rng(4100)
    base = rng.integers(0, 256, (EDGE_H, rw), dtype=np.uint8)
    ref = np.clip(base.astype(np.int32) + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)
    src = np.ascontiguousarray(np.roll(base, (3, -5), (0, 1))[:, 48:48 + sw])
    jobs, k = [], 0
    for step in EDGE_STEPS:
        widths = sorted({1, 7, 8, 9, 15, 16, 17} | {8 + n * (7 + step) - d for n in (1, 2) for d in (1, 0)})
        for sa_w in widths:
            for sa_h in sorted({1, step, step + 1, 2 * step + 1}):
                jobs.append(_placed(rng, EDGE_BLOCKS[k % 3], sa_w, sa_h, step))
                k += 1
    last = _job(rng, (40, 17), (rw - 23, EDGE_H - 11), (8, 8), 16, 4, 1, best=0xFFFFFFFF)  # its window ends at the plane's last sample
    assert int(last["ref_offset"]) + 10 * rw + 15 + 8 == ref.size
    jobs = np.array([last] + jobs, abi.PME_JOB_DTYPE)
    _tie_incoming(src, ref, jobs, 4)
    sets["grid"] = (src, ref, jobs, cost_tables(rng))
    # counts: n_groups * n_rows groups of 8 positions = 2 * n_groups * n_rows quads, one lane each, 64 per pass.  A quad count is even: the
    # quad counts around 64 and 128 are 62 / 64 / 66 and 126 / 128 / 130, and 1, 63, 65 and 129 are taken as group counts
    rng = np.random.default_rng(4200)
    jobs = []
    for groups, rows, step in [(1, 1, 1), (1, 31, 1), (2, 16, 2), (4, 8, 1), (3, 11, 3), (7, 9, 1), (8, 8, 1), (2, 32, 2), (5, 13, 1), (3, 43, 1), (10, 50, 2)]:
        jobs.append(_placed(rng, (4, 4) if groups * rows < 400 else (8, 8), 8 + (groups - 1) * (7 + step), (rows - 1) * step + 1, step))
    jobs = np.array(jobs, abi.PME_JOB_DTYPE)
    _tie_incoming(src, ref, jobs, 3)
    sets["counts"] = (src, ref, jobs, cost_tables(rng))
    # ties: content periodic by 16 columns and 8 rows, the block cut from it 4 .. 15 columns into the period: every 16th column of every 8th
    # row scores 0.  Constant rate tables: cost type 0 ties like type 5.
    rng = np.random.default_rng(4300)
    tile = rng.integers(0, 256, (8, 16), dtype=np.uint8)
    per = np.tile(tile, (EDGE_H // 8 + 1, rw // 16 + 1))
    src, ref = np.ascontiguousarray(per[:EDGE_H, :sw]), np.ascontiguousarray(per[:EDGE_H, :rw])
    jobs = []
    for i in range(48):
        block = EDGE_BLOCKS[i % 3]
        sa_w, sa_h, step = [(32, 17, 1), (40, 17, 1), (56, 25, 1), (24, 9, 1), (44, 33, 2), (33, 19, 1)][i % 6]
        j = _placed(rng, block, sa_w, sa_h, step)
        (sy, sx), (ry, rx) = divmod(int(j["src_offset"]), sw), divmod(int(j["ref_offset"]), rw)
        sx += (rx + int(rng.integers(4, 16)) - sx) % 16  # the first zero of a row at xs = 4 .. 15
        if sx + block[0] > sw:
            sx -= 16
        jobs.append(_job(rng, (sx, sy), (rx, ry), block, sa_w, sa_h, step, best=[0xFFFFFFFF, 0xFFFFFFFF, 0, 1][i % 4]))
    sets["ties"] = (src, ref, np.array(jobs, abi.PME_JOB_DTYPE), (np.full(4, 77, np.int32), np.full(2 * MV_CENTRE + 1, 100, np.int32), np.full(2 * MV_CENTRE + 1, 100, np.int32)))
    # flat: every position has the same SAD; the L1 rates then tie on rings around ref_mv, and the type without a rate everywhere
    rng = np.random.default_rng(4400)
    src, ref = np.full((EDGE_H, sw), 90, np.uint8), np.full((EDGE_H, rw), 97, np.uint8)
    jobs = np.array([_placed(rng, EDGE_BLOCKS[i % 3], [16, 24, 40, 23][i % 4], [5, 9, 16][i % 3], [1, 2, 1, 3][i % 4]) for i in range(24)], abi.PME_JOB_DTYPE)
    jobs["ref_mv"] = np.stack([jobs["mvy"] + 8 * (jobs["start_y"] + jobs["sa_h"] // 2), jobs["mvx"] + 8 * (jobs["start_x"] + jobs["sa_w"] // 2)], axis=1)  # (row, col): mid-window
    _tie_incoming(src, ref, jobs, 3)
    sets["flat"] = (src, ref, jobs, cost_tables(rng))
    # extremes: 0 against 255, the largest SADs (a 128-sample row fills the packed 16-bit accumulators to 32640)
    rng = np.random.default_rng(4500)
    src, ref = np.zeros((EDGE_H, sw), np.uint8), np.full((EDGE_H, rw), 255, np.uint8)
    jobs = np.array([_job(rng, (3, 0), (17, 2), (128, 128), 16, 5, 2, best=0xFFFFFFFF), _job(rng, (60, 1), (90, 100), (64, 64), 17, 3, 1, best=0xFFFFFFFF),
                     _job(rng, (0, 0), (0, 0), (128, 128), 9, 1, 1, best=128 * 128 * 255), _job(rng, (7, 120), (31, 66), (64, 64), 8, 2, 1, best=64 * 64 * 255 + 1)], abi.PME_JOB_DTYPE)
    sets["extremes"] = (src, ref, jobs, cost_tables(rng))
    for name, (src, ref, jobs, _) in sets.items():  # every window inside its plane, and inside the common buffer length with either stride
        size = max(src.size, ref.size)
        for j in jobs:
            cols, rows = read_extent(j)
            (sy, sx), (ry, rx) = divmod(int(j["src_offset"]), sw), divmod(int(j["ref_offset"]), rw)
            assert sx + j["width"] <= sw and sy + j["height"] <= EDGE_H and rx + cols <= rw and ry + rows <= EDGE_H, (name, j)
            if rows:
                assert int(j["src_offset"]) + (int(j["height"]) - 1) * rw + int(j["width"]) <= size and int(j["ref_offset"]) + (rows - 1) * rw + cols <= size, (name, j)
    return sets


def tie_census(src, ref, jobs):
    """per job under a cost without an MV rate (cost = SAD): (positions visited, quads holding a minimal position, incoming best == minimum)"""
    out = []
    for j in jobs:
        pos, sads = visit_sads(src, ref, j)
        quads = sorted({int(v) // 4 for v in np.nonzero(sads == sads.min())[0]}) if len(pos) else []
        out.append((len(pos), quads, bool(len(pos)) and int(j["best_cost"]) == int(sads.min())))
    return out


def run_oracle(oracle, src, ref, jobs, cost_type, epb, tables):
    jc, tr, tc = tables
    n = len(jobs)
    cost, mv = np.zeros(n, np.uint32), np.zeros((n, 2), np.int16)
    d = abi.PmeBatchDesc(n_jobs=n, src_stride=src.shape[1], ref_stride=ref.shape[1], src=src.ctypes.data, ref=ref.ctypes.data, jobs=jobs.ctypes.data, mv_cost_type=cost_type,
                         error_per_bit=epb, mvjcost=jc.ctypes.data, best_cost=cost.ctypes.data, best_mv=mv.ctypes.data)
    d.mvcost[0], d.mvcost[1] = tr.ctypes.data + 4 * MV_CENTRE, tc.ctypes.data + 4 * MV_CENTRE
    assert oracle.orc_pme_sad_batch(C.byref(d)) == 0
    return cost, mv


def run_ref(ref_lib, src, ref, jobs, cost_type, epb, tables, garbage=None, fn="svt_pme_sad_loop_kernel_c"):
    """the reference's svt_pme_sad_loop_kernel_c (or another function with its prototype), call by call; garbage: byte the parameter struct
    is filled with before its fields are assigned (the padding bytes keep it)"""
    jc, tr, tc = tables
    n = len(jobs)
    cost, mv = np.zeros(n, np.uint32), np.zeros((n, 2), np.int16)
    for i, j in enumerate(jobs):
        rmv = abi.Mv(int(j["ref_mv"][0]), int(j["ref_mv"][1]))
        p = abi.MvCostParam()
        if garbage is not None:
            C.memset(C.byref(p), garbage, C.sizeof(p))
        p.ref_mv, p.mv_cost_type, p.mvjcost, p.error_per_bit = C.pointer(rmv), cost_type, jc.ctypes.data, epb
        p.mvcost[0], p.mvcost[1] = tr.ctypes.data + 4 * MV_CENTRE, tc.ctypes.data + 4 * MV_CENTRE
        bc, bx, by = C.c_uint32(int(j["best_cost"])), C.c_int16(int(j["best_mvx"])), C.c_int16(int(j["best_mvy"]))
        getattr(ref_lib, fn)(C.byref(p), C.c_void_p(src.ctypes.data + int(j["src_offset"])), C.c_uint32(src.shape[1]),
                                          C.c_void_p(ref.ctypes.data + int(j["ref_offset"])), C.c_uint32(ref.shape[1]), C.c_uint32(int(j["height"])), C.c_uint32(int(j["width"])),
                                          C.byref(bc), C.byref(bx), C.byref(by), C.c_int16(int(j["start_x"])), C.c_int16(int(j["start_y"])), C.c_int16(int(j["sa_w"])),
                                          C.c_int16(int(j["sa_h"])), C.c_int16(int(j["step"])), C.c_int16(int(j["mvx"])), C.c_int16(int(j["mvy"])))
        cost[i], mv[i] = bc.value, (bx.value, by.value)
    return cost, mv


REF_SLACK = 1  # bytes behind the last reference sample a search reads that the batch may load (include/svt_hip_pme.h)


def run_hip(ctx, src, ref, jobs, cost_type, epb, tables, fill=None, spare_jobs=0):
    """svt_hip_pme_sad_batch on host planes (2-D arrays; their widths are the strides and may differ).  Both device planes are as long as
    the larger of the two (a kernel that takes one stride for the other then reads wrong samples, never unmapped memory); the reference
    plane carries REF_SLACK bytes more, nothing else.  fill: a byte both output arrays are pre-filled with (default: zeros); the arrays
    are then n + spare_jobs slots long, and the spare slots and every input buffer are asserted to read back unchanged."""
    import torch
    from svt_av1_psyex_amd import api
    jc, tr, tc = tables
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    n = len(jobs)
    size = max(src.size, ref.size)
    padded = lambda a, extra: np.concatenate([a.reshape(-1), np.zeros(size - a.size + extra, np.uint8)])
    inputs = [padded(src, 0), padded(ref, REF_SLACK), jobs if n else np.zeros(1, abi.PME_JOB_DTYPE), jc, tr, tc]
    t = [dev(a) for a in inputs]
    n_alloc = max(n + (spare_jobs if fill is not None else 0), 1)
    cost, mv = (torch.full((n_alloc * 4,), fill or 0, dtype=torch.uint8, device="cuda") for _ in range(2))
    d = abi.PmeBatchDesc(n_jobs=n, src_stride=src.shape[1], ref_stride=ref.shape[1], src=t[0].data_ptr(), ref=t[1].data_ptr(), jobs=t[2].data_ptr(), mv_cost_type=cost_type,
                         error_per_bit=epb, mvjcost=t[3].data_ptr(), best_cost=cost.data_ptr(), best_mv=mv.data_ptr())
    d.mvcost[0], d.mvcost[1] = t[4].data_ptr() + 4 * MV_CENTRE, t[5].data_ptr() + 4 * MV_CENTRE
    torch.cuda.synchronize()
    ctx.check(api.lib().svt_hip_pme_sad_batch(ctx._h, C.byref(d)), "svt_hip_pme_sad_batch")
    ctx.sync()
    cost, mv = cost.cpu().numpy(), mv.cpu().numpy()
    if fill is not None:
        assert (cost[4 * n:] == fill).all() and (mv[4 * n:] == fill).all(), f"a slot past the batch's {n} was written"
        for a, b in zip(inputs, t):
            assert np.array_equal(b.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input buffer of the batch was written"
    return cost[:4 * n].view(np.uint32), mv[:4 * n].view(np.int16).reshape(n, 2)
