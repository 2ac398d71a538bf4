"""Shared pieces of the mode-decision side motion-search tests (include/svt_hip_md_search.h): planes with real motion, job grids shaped like
the reference's call sites (md_nsq_motion_search's chain of md_full_pel_search calls, product_coding_loop.c:2260-2375; md_subpel_search's
parameters, :2637-2750 and the MdSubPelSearchCtrls levels of enc_mode_config.c) and the three runners (reference build, oracle, HIP)."""
import ctypes as C

import numpy as np

from svt_av1_psyex_amd import abi

MV_CENTRE = 1 << 14
PAD = 80          # EbPictureBufferDesc padding of the reference planes
W, H = 320, 192   # picture size (max_width / max_height)
SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 16), (16, 8), (32, 16), (16, 64), (64, 32), (128, 128), (4, 16), (64, 16), (8, 32)]


def planes(seed):
    """source picture (W x H) and a padded reference plane: the source displaced by a few samples + noise, so that searches have a minimum to find"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H + 2 * PAD + 16, W + 2 * PAD + 16)).astype(np.float32)
    k = np.ones(5, np.float32) / 5
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.apply_along_axis(lambda c: np.convolve(c, k, "same"), 0, base)
    base = np.clip((base - 128) * 3 + 128, 0, 255)
    ref = np.ascontiguousarray(base[:H + 2 * PAD, :W + 2 * PAD]).astype(np.uint8)
    dy, dx = 3, -5
    src = np.clip(base[PAD + dy:PAD + dy + H, PAD + dx:PAD + dx + W] + rng.normal(0, 4, (H, W)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(src), ref


def cost_tables(rng):
    j = np.array([11, 54, 5437, 342], np.int32)
    ramp = (np.abs(np.arange(-MV_CENTRE, MV_CENTRE + 1)) * 3 + 200).astype(np.int32)  # rate grows with the component, like a real table
    return j, (ramp + rng.integers(0, 64, ramp.size)).astype(np.int32), (ramp + rng.integers(0, 64, ramp.size)).astype(np.int32)


def fullpel_chain(rng, n_blocks, dist_type, psad):
    """md_nsq_motion_search's chain for n_blocks blocks, as ROUNDS of jobs (one batch per round, job i of every round = block i, results in place):
    two candidate centres (one position each, the second keeps the running best), the step-4 area around the winner (fresh best), +-2 step 2,
    +-1 step 1.  Returns [jobs_round0, jobs_round1, ...]."""
    rounds = []
    geo = []
    for i in range(n_blocks):
        bw, bh = SIZES[rng.integers(len(SIZES))]
        x, y = int(rng.integers(0, (W - bw) // 4 + 1)) * 4, int(rng.integers(0, (H - bh) // 4 + 1)) * 4
        if i % 7 == 0:  # blocks in the picture corners (centres and areas this small stay far inside the padding: the search-area adjustment is edge_chain's)
            x, y = [(0, 0), (W - bw, H - bh), (0, H - bh), (W - bw, 0)][(i // 7) % 4]
        geo.append((bw, bh, x, y, rng.integers(-60, 61, 2)))

    def base(i):
        bw, bh, x, y, rmv = geo[i]
        j = np.zeros(1, abi.FULLPEL_JOB_DTYPE)[0]
        j["src_offset"], j["blk_org_x"], j["blk_org_y"], j["width"], j["height"] = y * W + x, x, y, bw, bh
        j["dist_type"], j["flags"], j["ref_mv"], j["chain_from"] = dist_type, (abi.FP_ENABLE_PSAD if psad else 0), rmv, -1
        j["best_cost"], j["best_mvx"], j["best_mvy"] = 0xFFFFFFFF, -1, -1
        return j

    def make(fn):
        jobs = np.zeros(n_blocks, abi.FULLPEL_JOB_DTYPE)
        for i in range(n_blocks):
            j = base(i)
            fn(i, j)
            jobs[i] = j
        return jobs

    def cand0(i, j):
        j["mvx"], j["mvy"] = (rng.integers(-12, 13, 2) * 8)
        j["step"] = 1

    def cand1(i, j):
        j["mvx"], j["mvy"] = (rng.integers(-12, 13, 2) * 8)
        j["step"] = 1
        j["flags"] |= abi.FP_BEST_FROM_CHAIN
        j["chain_from"] = i

    def area(i, j):
        wdt, hgt = int(rng.choice([7, 15, 31])), int(rng.choice([5, 7, 15]))
        j["flags"] |= abi.FP_CENTRE_FROM_CHAIN
        j["chain_from"] = i
        j["start_x"], j["end_x"], j["start_y"], j["end_y"], j["step"] = -(wdt >> 1), wdt >> 1, -(hgt >> 1), hgt >> 1, 4

    def refine(r, st):
        def f(i, j):
            j["flags"] |= abi.FP_CENTRE_FROM_CHAIN | abi.FP_BEST_FROM_CHAIN
            j["chain_from"] = i
            j["start_x"], j["end_x"], j["start_y"], j["end_y"], j["step"] = -r, r, -r, r, st
            if st == 2:
                j["flags"] |= abi.FP_SPRS_LEV0_DONE
                j["sprs_lev0_start_x"], j["sprs_lev0_end_x"], j["sprs_lev0_start_y"], j["sprs_lev0_end_y"] = -3, 4, -2, 3
        return f

    return [make(cand0), make(cand1), make(area), make(refine(2, 2)), make(refine(1, 1))]


def fullpel_desc(src, ref, jobs, cost_type, epb, tables, cost, mv):
    jc, tr, tc = tables
    d = abi.FullpelBatchDesc(n_jobs=len(jobs), src_stride=src.strides[0], ref_stride=ref.strides[0], src=src.ctypes.data, ref=ref.ctypes.data, ref_org_x=PAD, ref_org_y=PAD,
                             ref_max_width=W, ref_max_height=H, jobs=jobs.ctypes.data, mv_cost_type=cost_type, error_per_bit=epb, mvjcost=jc.ctypes.data,
                             best_cost=cost.ctypes.data, best_mv=mv.ctypes.data)
    d.mvcost[0], d.mvcost[1] = tr.ctypes.data + 4 * MV_CENTRE, tc.ctypes.data + 4 * MV_CENTRE
    return d


def run_fullpel_cpu(fn, src, ref, rounds, cost_type, epb, tables):
    """fn = oracle.orc_md_fullpel_batch or ref.ref_md_fullpel_batch; the rounds share the output arrays (in-place chains)"""
    n = len(rounds[0])
    cost, mv = np.zeros(n, np.uint32), np.zeros((n, 2), np.int16)
    trace = []
    for jobs in rounds:
        d = fullpel_desc(src, ref, jobs, cost_type, epb, tables, cost, mv)
        assert fn(C.byref(d)) == 0
        trace.append((cost.copy(), mv.copy()))
    return trace


def _upload(torch, a):
    """(device tensor, device address of a's first element): a view into a wider array travels as its whole parent, so that its strides hold"""
    root = a
    while isinstance(root.base, np.ndarray):
        root = root.base
    if root is a or not root.flags.c_contiguous:
        root = a = np.ascontiguousarray(a)
    t = torch.from_numpy(root.view(np.uint8).reshape(-1)).cuda()
    return t, t.data_ptr() + (a.ctypes.data - root.ctypes.data)


GUARD_COST, GUARD_MV = 0x1234, (77, -77)  # what run_fullpel_hip(guard=True) leaves in front of the output arrays


def run_fullpel_hip(ctx, src, ref, rounds, cost_type, epb, tables, sync_each=True, guard=False):
    """sync_each=False: every round is enqueued back to back on the context stream (the job tensors stay alive), one sync at the end, and the
    trace holds the final round alone.  guard=True: one sentinel entry lies in front of the output arrays' base pointers, so that a read of
    index -1 stays inside the allocation (and would bring GUARD_COST / GUARD_MV)."""
    import torch
    from svt_av1_psyex_amd import api
    L = api.lib()
    ext = torch.cuda.ExternalStream(ctx.stream)
    n = len(rounds[0])
    g = 1 if guard else 0
    trace = []
    with torch.cuda.stream(ext):
        t, p = {}, {}
        for k, v in dict(src=src, ref=ref, jc=tables[0], tr=tables[1], tc=tables[2]).items():
            t[k], p[k] = _upload(torch, v)
        cost, mv = torch.zeros(n + g, dtype=torch.int32, device="cuda"), torch.zeros(2 * (n + g), dtype=torch.int16, device="cuda")
        if guard:
            cost[0] = GUARD_COST
            mv[0], mv[1] = GUARD_MV
        tjs = [torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).cuda() for jobs in rounds]
        ctx.sync()
        for r, tj in enumerate(tjs):
            d = abi.FullpelBatchDesc(n_jobs=n, src_stride=src.strides[0], ref_stride=ref.strides[0], src=p["src"], ref=p["ref"], ref_org_x=PAD, ref_org_y=PAD,
                                     ref_max_width=W, ref_max_height=H, jobs=tj.data_ptr(), mv_cost_type=cost_type, error_per_bit=epb, mvjcost=p["jc"],
                                     best_cost=cost.data_ptr() + 4 * g, best_mv=mv.data_ptr() + 4 * g)
            d.mvcost[0], d.mvcost[1] = p["tr"] + 4 * MV_CENTRE, p["tc"] + 4 * MV_CENTRE
            ctx.check(L.svt_hip_md_fullpel_batch(ctx._h, C.byref(d)), "svt_hip_md_fullpel_batch")
            if sync_each or r == len(tjs) - 1:
                ctx.sync()
                trace.append((cost.cpu().numpy().view(np.uint32)[g:].copy(), mv.cpu().numpy().reshape(n + g, 2)[g:].copy()))
        if guard:
            assert int(cost[0]) == GUARD_COST and (int(mv[0]), int(mv[1])) == GUARD_MV  # nobody wrote in front of the arrays
    return trace


# MdSubPelSearchCtrls-like settings: (allow_hp, forced_stop, iters_per_step, pred_variance_th, abs_th_mult, round_dev_th, skip_diag_refinement, bias_fp, mv_cost_type
#                                       [, search_method, subpel_search_type, mvp_th, hp_mv_th])
SUBPEL_SETTINGS = [
    (0, 0, 2, 0, 0, 2147483647, 0, 0, 0),        # everything on: quarter-pel (no hp), two levels per step, entropy MV cost
    (1, 0, 2, 0, 0, 2147483647, 1, 0, 0),        # eighth-pel, diagonal refinement only when the cardinal points improved
    (0, 1, 1, 50, 2, -25, 2, 0, 0),              # quarter-pel, one level, variance / absolute thresholds, early round exit
    (0, 2, 2, 0, 0, 2147483647, 3, 100, 4),      # half-pel only, MV_COST_OPT with its early exit, full-pel bias
    (1, 0, 2, 0, 0, 2147483647, 4, 110, 4),      # org_error 0: never the diagonal / second level
    (0, 3, 2, 0, 0, 2147483647, 0, 0, 0),        # forced_stop FULL_PEL: the centre error only
    # svt_av1_find_best_sub_pixel_tree (search_method 1): the accurate search on svt_aom_upsampled_pred
    (1, 0, 2, 0, 0, 2147483647, 0, 0, 0, 1, 3, 0, 0),    # eighth-pel, 8 taps, two levels per step
    (0, 0, 2, 0, 0, 2147483647, 0, 0, 0, 1, 2, 0, 0),    # quarter-pel, 4 taps
    (1, 0, 1, 30, 1, 2147483647, 0, 105, 4, 1, 1, 0, 0),  # 2 taps (bilinear table), one level, variance / absolute thresholds, full-pel bias, MV_COST_OPT
    (1, 0, 2, 0, 0, 2147483647, 0, 0, 0, 1, 3, 20, 16),   # the PD_PASS_1 branch: round limited by the distance to the best MVP (mvp_th, hp_mv_th)
    (0, 2, 2, 0, 0, 2147483647, 0, 0, 0, 1, 3, 0, 0),     # half-pel only
]


def full_setting(setting):
    return tuple(setting) + (0, 0, 0, 0)[len(setting) - 9:] if len(setting) < 13 else tuple(setting)


def subpel_jobs(rng, n):
    jobs = np.zeros(n, abi.SUBPEL_JOB_DTYPE)
    for i in range(n):
        bw, bh = SIZES[rng.integers(len(SIZES))]
        x, y = int(rng.integers(8, (W - bw - 8) // 4)) * 4, int(rng.integers(8, (H - bh - 8) // 4)) * 4
        j = jobs[i]
        j["src_offset"], j["ref_offset"] = y * W + x, (y + PAD) * (W + 2 * PAD) + x + PAD
        j["width"], j["height"], j["log2_pels"] = bw, bh, int(np.log2(bw * bh))
        j["early_neigh_check_exit"] = 1 if i % 11 == 5 else 0
        smv = rng.integers(-6, 7, 2) * 8
        j["start_mv"] = smv
        j["ref_mv"] = smv + rng.integers(-30, 31, 2)
        lim = int(rng.choice([9, 40, 2000]))  # tight limits cut the tree at the range test
        j["col_min"], j["col_max"], j["row_min"], j["row_max"] = smv[1] - lim, smv[1] + lim, smv[0] - lim, smv[0] + lim
        j["early_exit_th"] = 1020 - (max(bw, bh) >> 2)
        j["best_mvp_dist"] = int(rng.integers(0, 40000))  # (read by the tree search's PD_PASS_1 branch only)
        j["best_mvp"] = smv + rng.integers(-40, 41, 2)
    return jobs


def subpel_desc(src, ref, jobs, setting, epb, qp, tables, out):
    jc, tr, tc = tables
    hp, stop, iters, pvt, atm, rdt, sdr, bias, ctype, method, taps, mvp_th, hp_mv_th = full_setting(setting)
    d = abi.SubpelBatchDesc(n_jobs=len(jobs), src_stride=src.strides[0], ref_stride=ref.strides[0], src=src.ctypes.data, ref=ref.ctypes.data, jobs=jobs.ctypes.data, allow_hp=hp,
                            forced_stop=stop, iters_per_step=iters, pred_variance_th=pvt, abs_th_mult=atm, round_dev_th=rdt, skip_diag_refinement=sdr, bias_fp=bias, qp=qp,
                            search_method=method, subpel_search_type=taps, mvp_th=mvp_th, hp_mv_th=hp_mv_th,
                            mv_cost_type=ctype, error_per_bit=epb, mvjcost=jc.ctypes.data, best_mv=out["best_mv"].ctypes.data, besterr=out["besterr"].ctypes.data,
                            distortion=out["distortion"].ctypes.data, sse=out["sse"].ctypes.data, center_err=out["center_err"].ctypes.data)
    d.mvcost[0], d.mvcost[1] = tr.ctypes.data + 4 * MV_CENTRE, tc.ctypes.data + 4 * MV_CENTRE
    return d


def subpel_out(n):
    return {"best_mv": np.zeros((n, 2), np.int16), "besterr": np.zeros(n, np.uint32), "distortion": np.zeros(n, np.int32), "sse": np.zeros(n, np.uint32),
            "center_err": np.zeros(n, np.uint32)}


def run_subpel_cpu(fn, src, ref, jobs, setting, epb, qp, tables):
    out = subpel_out(len(jobs))
    assert fn(C.byref(subpel_desc(src, ref, jobs, setting, epb, qp, tables, out))) == 0
    return out


def run_subpel_hip(ctx, src, ref, jobs, setting, epb, qp, tables, center_err=True):
    """center_err=False: the optional output is a null pointer, and is left out of the result"""
    import torch
    from svt_av1_psyex_amd import api
    L = api.lib()
    ext = torch.cuda.ExternalStream(ctx.stream)
    jc, tr, tc = tables
    hp, stop, iters, pvt, atm, rdt, sdr, bias, ctype, method, taps, mvp_th, hp_mv_th = full_setting(setting)
    n = len(jobs)
    with torch.cuda.stream(ext):
        t, p = {}, {}
        for k, v in dict(src=src, ref=ref, jc=jc, tr=tr, tc=tc, jobs=jobs).items():
            t[k], p[k] = _upload(torch, v)
        o = {"best_mv": torch.zeros(2 * n, dtype=torch.int16, device="cuda"), "besterr": torch.zeros(n, dtype=torch.int32, device="cuda"),
             "distortion": torch.zeros(n, dtype=torch.int32, device="cuda"), "sse": torch.zeros(n, dtype=torch.int32, device="cuda"),
             "center_err": torch.zeros(n, dtype=torch.int32, device="cuda")}
        d = abi.SubpelBatchDesc(n_jobs=n, src_stride=src.strides[0], ref_stride=ref.strides[0], src=p["src"], ref=p["ref"], jobs=p["jobs"], allow_hp=hp,
                                forced_stop=stop, iters_per_step=iters, pred_variance_th=pvt, abs_th_mult=atm, round_dev_th=rdt, skip_diag_refinement=sdr, bias_fp=bias, qp=qp,
                                search_method=method, subpel_search_type=taps, mvp_th=mvp_th, hp_mv_th=hp_mv_th,
                                mv_cost_type=ctype, error_per_bit=epb, mvjcost=p["jc"], best_mv=o["best_mv"].data_ptr(), besterr=o["besterr"].data_ptr(),
                                distortion=o["distortion"].data_ptr(), sse=o["sse"].data_ptr(), center_err=o["center_err"].data_ptr() if center_err else None)
        d.mvcost[0], d.mvcost[1] = p["tr"] + 4 * MV_CENTRE, p["tc"] + 4 * MV_CENTRE
        ctx.check(L.svt_hip_md_subpel_batch(ctx._h, C.byref(d)), "svt_hip_md_subpel_batch")
        ctx.sync()
    out = {"best_mv": o["best_mv"].cpu().numpy().reshape(n, 2), "besterr": o["besterr"].cpu().numpy().view(np.uint32), "distortion": o["distortion"].cpu().numpy(),
           "sse": o["sse"].cpu().numpy().view(np.uint32), "center_err": o["center_err"].cpu().numpy().view(np.uint32)}
    if not center_err:
        assert not out.pop("center_err").any()  # a null pointer: the array of this runner is never written
    return out


FULLPEL_GRID = [(dist, psad, ctype) for dist in (0, 1) for psad in (0, 1) for ctype in (0, 4)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# Plane edges, ties, every cost mode, odd strides (tests/golden/md_search_edges.npz).  Everything below draws from generators of its own:
# the streams of planes / cost_tables / fullpel_chain / subpel_jobs above are what md_search.npz was recorded with.
# ---------------------------------------------------------------------------------------------------------------------------------------
TIE_KINDS = ("flat", "extremes", "stripes")
CONTENTS = ("noise",) + TIE_KINDS


def tie_planes(kind):
    """content on which many positions cost exactly the same, so that the visiting order and the strictness of every comparison decide"""
    if kind == "flat":  # distortion 0 everywhere: the MV rate alone decides
        return np.full((H, W), 97, np.uint8), np.full((H + 2 * PAD, W + 2 * PAD), 97, np.uint8)
    if kind == "extremes":  # the largest SAD a block can have, everywhere
        return np.zeros((H, W), np.uint8), np.full((H + 2 * PAD, W + 2 * PAD), 255, np.uint8)
    if kind == "stripes":  # period-4 columns, the source cut from the reference: positions 4 columns apart tie exactly
        ref = np.ascontiguousarray(np.tile(np.array([10, 200, 60, 140], np.uint8), (H + 2 * PAD, (W + 2 * PAD) // 4)))
        return np.ascontiguousarray(ref[PAD:PAD + H, PAD:PAD + W]), ref
    raise ValueError(kind)


def content_planes(kind, seed=5):
    return planes(seed) if kind == "noise" else tie_planes(kind)


def mixed_planes(seed):
    """one picture with the four contents by quadrant (noise | stripes over flat | extremes), source and reference cut alike"""
    src, ref = planes(seed)
    for kind, (qy, qx) in (("stripes", (0, 1)), ("flat", (1, 0)), ("extremes", (1, 1))):
        s, r = tie_planes(kind)
        ys, xs = slice(qy * H // 2, (qy + 1) * H // 2), slice(qx * W // 2, (qx + 1) * W // 2)
        src[ys, xs] = s[ys, xs]
        yr = slice(PAD + H // 2, None) if qy else slice(0, PAD + H // 2)
        xr = slice(PAD + W // 2, None) if qx else slice(0, PAD + W // 2)
        ref[yr, xr] = r[yr, xr]
    return src, ref


STRIDE_EXTRA = 2 * 16 + 2  # a parent row is this much longer than the plane's: a stride that is not a multiple of 4


def strided(plane, seed=0):
    """the plane as a view into a wider (and slightly taller) array of other bytes: src_stride / ref_stride = the parent's row length"""
    h, w = plane.shape
    parent = np.random.default_rng(seed).integers(0, 256, (h + 8, w + STRIDE_EXTRA), dtype=np.uint8)
    parent[4:4 + h, 16:16 + w] = plane
    return parent[4:4 + h, 16:16 + w]


def restride(jobs, src_stride, ref_stride=None):
    """the jobs of fullpel rounds / a sub-pel list (built for the tight strides W and W + 2 PAD) on planes with other strides"""
    jobs = jobs.copy()
    y, x = np.divmod(jobs["src_offset"].astype(np.int64), W)
    jobs["src_offset"] = y * src_stride + x
    if "ref_offset" in jobs.dtype.names:
        jobs["ref_offset"] = (y + PAD) * ref_stride + x + PAD
    return jobs


def edge_chain(rng, n_blocks, dist_type, psad):
    """Two rounds on blocks in the four corners and along the four edges of the picture, the centres 55 .. 90 samples outward on the block's
    side: with a padding of 80 the search-area adjustment (product_coding_loop.c:2057-2072) clips areas, empties some, and leaves wide
    (psad) areas fewer than 8 columns.  Round 0: the block's own centre, an area of width {7, 8, 15, 16, 31} x height {1, 5, 7, 15}, step
    1 .. 4, an incoming best of {none, 3000, 0}.  Round 1: chained from the job's own slot (centre and best), +-2 step 2 with a sparse
    level 0 so wide that its skip rule fires wherever the clipped area allows."""
    geo = []
    for i in range(n_blocks):
        bw, bh = SIZES[rng.integers(len(SIZES))]
        rx, ry = int(rng.integers(0, (W - bw) // 4 + 1)) * 4, int(rng.integers(0, (H - bh) // 4 + 1)) * 4
        x, y, sgx, sgy = [(0, 0, -1, -1), (W - bw, H - bh, 1, 1), (0, H - bh, -1, 1), (W - bw, 0, 1, -1),
                          (0, ry, -1, 0), (W - bw, ry, 1, 0), (rx, 0, 0, -1), (rx, H - bh, 0, 1)][i % 8]
        geo.append((bw, bh, x, y, sgx, sgy))
    rounds = []
    for r in range(2):
        jobs = np.zeros(n_blocks, abi.FULLPEL_JOB_DTYPE)
        for i in range(n_blocks):
            bw, bh, x, y, sgx, sgy = geo[i]
            j = jobs[i]
            j["src_offset"], j["blk_org_x"], j["blk_org_y"], j["width"], j["height"] = y * W + x, x, y, bw, bh
            j["dist_type"], j["flags"], j["ref_mv"], j["chain_from"] = dist_type, (abi.FP_ENABLE_PSAD if psad else 0), rng.integers(-700, 701, 2), -1
            j["best_cost"], j["best_mvx"], j["best_mvy"] = int(rng.choice([0xFFFFFFFF, 0xFFFFFFFF, 3000, 0])), -1, -1
            # outward on the block's side(s); along an edge the other component stays small
            j["mvx"] = (sgx * int(rng.integers(55, 91)) if sgx else int(rng.integers(-12, 13))) * 8
            j["mvy"] = (sgy * int(rng.integers(55, 91)) if sgy else int(rng.integers(-12, 13))) * 8
            wdt, hgt = int(rng.choice([7, 8, 15, 16, 31])), int(rng.choice([1, 5, 7, 15]))
            j["start_x"], j["end_x"], j["start_y"], j["end_y"], j["step"] = -(wdt >> 1), wdt >> 1, -(hgt >> 1), hgt >> 1, int(rng.choice([1, 2, 3, 4]))
            if r == 1:
                j["flags"] |= abi.FP_CENTRE_FROM_CHAIN | abi.FP_BEST_FROM_CHAIN | abi.FP_SPRS_LEV0_DONE
                j["chain_from"] = i
                j["start_x"], j["end_x"], j["start_y"], j["end_y"], j["step"] = -2, 2, -2, 2, 2
                j["sprs_lev0_start_x"], j["sprs_lev0_end_x"], j["sprs_lev0_start_y"], j["sprs_lev0_end_y"] = -90, 90, -90, 90
        rounds.append(jobs)
    return rounds


def adjusted_area(j, mvx, mvy):
    """The four comparisons of the search-area adjustment restated on a job's fields and its centre (1/8 sample): the area md_full_pel_search
    is left with, which sides it moved, and whether the wide (psad) form runs.  What the tests use to prove that they reach these paths."""
    bx, by, bw, bh = int(j["blk_org_x"]), int(j["blk_org_y"]), int(j["width"]), int(j["height"])
    sx, ex, sy, ey = (int(j[k]) for k in ("start_x", "end_x", "start_y", "end_y"))
    cx, cy = int(mvx) >> 3, int(mvy) >> 3
    wide_before = int(j["dist_type"]) == 0 and bool(int(j["flags"]) & abi.FP_ENABLE_PSAD) and ex - sx >= 7
    sides = [False] * 4
    if bx + cx + sx < -PAD + 1:
        sx, sides[0] = -PAD + 1 - (bx + cx), True
    if bx + bw + cx + ex > PAD + W - 1:
        ex, sides[1] = PAD + W - 1 - (bx + bw + cx), True
    if by + cy + sy < -PAD + 1:
        sy, sides[2] = -PAD + 1 - (by + cy), True
    if by + bh + cy + ey > PAD + H - 1:
        ey, sides[3] = PAD + H - 1 - (by + bh + cy), True
    wide = int(j["dist_type"]) == 0 and bool(int(j["flags"]) & abi.FP_ENABLE_PSAD) and ex - sx >= 7
    empty = ex < sx or ey < sy
    return dict(area=(sx, ex, sy, ey), sides=sides, empty=empty, wide=wide, wide_before=wide_before)


def visited_positions(j, mvx, mvy):
    """(px, py) of every position md_full_pel_search evaluates for the job, in the reference's visiting order"""
    a = adjusted_area(j, mvx, mvy)
    sx, ex, sy, ey = a["area"]
    step = max(int(j["step"]), 1)
    out = []
    if a["wide"]:  # md_full_pel_search_large_lbd: width rounded up to a multiple of 8; svt_pme_sad_loop_kernel: rows outer, groups of 8 columns
        remain = 8 - ((ex - sx) % 8)
        ex += 0 if remain == 8 else remain
        sa_w, sa_h = (ex - sx) & ~7, ey - sy + 1
        for ys in range(0, sa_h, step):
            xs = 0
            while sa_w - xs >= 8:
                out += [(sx + xs + k, sy + ys) for k in range(8)]
                xs += 7 + step
        return out
    skip = step == 2 and int(j["flags"]) & abi.FP_SPRS_LEV0_DONE
    for px in range(sx, ex + 1, step):  # columns outer, rows inner
        for py in range(sy, ey + 1, step):
            if skip and int(j["sprs_lev0_start_x"]) <= px + (int(mvx) >> 3) <= int(j["sprs_lev0_end_x"]) and \
                    int(j["sprs_lev0_start_y"]) <= py + (int(mvy) >> 3) <= int(j["sprs_lev0_end_y"]) and px % 4 == 0 and py % 4 == 0:
                continue
            out.append((px, py))
    return out


def fullpel_mv_rate(j, mvx, mvy, px, py, cost_type, epb, tables):
    """svt_mv_err_cost of the position for MV_COST_ENTROPY (0) and MV_COST_OPT (4), the two modes md_full_pel_search takes"""
    i16 = lambda v: ((int(v) + 32768) & 0xFFFF) - 32768
    dr, dc = i16(i16(int(mvy) + py * 8) - int(j["ref_mv"][0])), i16(i16(int(mvx) + px * 8) - int(j["ref_mv"][1]))
    if cost_type == 0:
        jc, tr, tc = tables
        bits = int(jc[(2 if dr else 0) + (1 if dc else 0)]) + int(tr[MV_CENTRE + dr]) + int(tc[MV_CENTRE + dc])
        return (bits * epb + (1 << 13)) >> 14
    assert cost_type == 4
    return (((abs(dr) + abs(dc)) << 8) * epb + (1 << 13)) >> 14


def position_costs(src, ref, j, mvx, mvy, cost_type, epb, tables):
    """plain numpy: distortion (SAD, or the variance in uint32 arithmetic) + MV rate of every visited position, in visiting order"""
    bx, by, bw, bh = int(j["blk_org_x"]), int(j["blk_org_y"]), int(j["width"]), int(j["height"])
    blk = src[by:by + bh, bx:bx + bw].astype(np.int64)
    flat, stride = ref.reshape(-1), ref.shape[1]  # (a rounded-up wide area runs a few columns past the row's end: addresses, not 2-D slices)
    win = np.arange(bh)[:, None] * stride + np.arange(bw)
    costs = []
    for px, py in visited_positions(j, mvx, mvy):
        y0, x0 = PAD + by + (int(mvy) >> 3) + py, PAD + bx + (int(mvx) >> 3) + px
        d = flat[y0 * stride + x0 + win].astype(np.int64) - blk
        dist = int(np.abs(d).sum()) if int(j["dist_type"]) == 0 else (int((d * d).sum()) - (int(d.sum()) ** 2) // (bw * bh)) & 0xFFFFFFFF
        costs.append(dist + fullpel_mv_rate(j, mvx, mvy, px, py, cost_type, epb, tables))
    return costs


def subpel_far_jobs(rng, n):
    """sub-pel jobs at the plane's limits: blocks on the picture corners and at arbitrary (odd) origins, start vectors up to +-60 samples
    (60 + 4 filter taps + 1 stays inside the padding of 80), the MV predictor up to +-3000 eighths away (the cost tables far from their centre),
    limit boxes down to +-3 eighths"""
    jobs = np.zeros(n, abi.SUBPEL_JOB_DTYPE)
    for i in range(n):
        bw, bh = SIZES[rng.integers(len(SIZES))]
        x, y = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
        if i % 3 == 0:
            x, y = [(0, 0), (W - bw, H - bh), (0, H - bh), (W - bw, 0)][(i // 3) % 4]
        j = jobs[i]
        j["src_offset"], j["ref_offset"] = y * W + x, (y + PAD) * (W + 2 * PAD) + x + PAD
        j["width"], j["height"], j["log2_pels"] = bw, bh, int(np.log2(bw * bh))
        j["early_neigh_check_exit"] = 1 if i % 13 == 7 else 0
        smv = rng.integers(-60, 61, 2) * 8
        j["start_mv"] = smv
        j["ref_mv"] = smv + rng.integers(-3000, 3001, 2)
        lim = int(rng.choice([3, 9, 40, 2000]))
        j["col_min"], j["col_max"], j["row_min"], j["row_max"] = smv[1] - lim, smv[1] + lim, smv[0] - lim, smv[0] + lim
        j["early_exit_th"] = 1020 - (max(bw, bh) >> 2)
        j["best_mvp_dist"] = int(rng.integers(0, 40000))
        j["best_mvp"] = smv + rng.integers(-40, 41, 2)
    return jobs


def with_cost_type(setting, cost_type):
    s = list(full_setting(setting))
    s[8] = cost_type
    return tuple(s)


# the case lists of tests/golden/md_search_edges.npz (oracle/gen_golden.py md_edges); a case's index in its list is its row in the fixture
FULLPEL_EDGE_GRID = [(kind, dist, psad, ctype) for kind in CONTENTS for dist, psad, ctype in FULLPEL_GRID]   # edge_chain, 48 blocks, and fullpel_chain, 40 blocks
SUBPEL_TIE_GRID = [(kind, si, ctype) for kind in CONTENTS for si in range(len(SUBPEL_SETTINGS)) for ctype in range(6)]       # subpel_jobs, 40 jobs
SUBPEL_FAR_GRID = [(kind, si, ctype) for kind in ("noise", "stripes") for si in range(len(SUBPEL_SETTINGS)) for ctype in range(6)]  # subpel_far_jobs, 48 jobs
# error_per_bit by MV cost type.  MV_COST_OPT charges 256 epb / 2^14 per eighth of |dr| + |dc|: at 37 neighbouring positions differ by 4 or 5 and
# the winner of a flat area is nearly always alone; at 1 (its floor, AOMMAX(rdmult >> RD_EPB_SHIFT, 1)) positions within 8 samples share a cost and
# the visiting order decides.  The entropy tables are coarse enough at 37.
EDGE_EPB = {0: 37, 4: 1}
SUBPEL_EPB, SUBPEL_QP = 41, 36


def fullpel_edge_case(ci, chain="edge"):
    """(src, ref, tables, rounds, cost type, error_per_bit) of FULLPEL_EDGE_GRID[ci]: the edge chain, or md_nsq_motion_search's five-round chain on the same content"""
    kind, dist, psad, ctype = FULLPEL_EDGE_GRID[ci]
    rng = np.random.default_rng([5000 if chain == "edge" else 7000, ci])
    src, refp = content_planes(kind)
    tables = cost_tables(rng)
    rounds = edge_chain(rng, 48, dist, psad) if chain == "edge" else fullpel_chain(rng, 40, dist, psad)
    return src, refp, tables, rounds, ctype, EDGE_EPB[ctype]


def subpel_edge_case(ci, far=False):
    """(src, ref, tables, jobs, setting) of SUBPEL_FAR_GRID[ci] / SUBPEL_TIE_GRID[ci]; the setting carries the case's MV cost type"""
    kind, si, ctype = (SUBPEL_FAR_GRID if far else SUBPEL_TIE_GRID)[ci]
    rng = np.random.default_rng([9000 if far else 8000, ci])
    src, refp = content_planes(kind)
    tables = cost_tables(rng)
    jobs = subpel_far_jobs(rng, 48) if far else subpel_jobs(rng, 40)
    return src, refp, tables, jobs, with_cost_type(SUBPEL_SETTINGS[si], ctype)


def mixed_fullpel_rounds(rng, n_each, dist_type, psad):
    """two rounds of 2 n_each jobs: edge_chain's blocks in front, fullpel_chain's first candidate and its chained step-4 area behind them"""
    e, c = edge_chain(rng, n_each, dist_type, psad), fullpel_chain(rng, n_each, dist_type, psad)
    out = []
    for a, b in ((e[0], c[0]), (e[1], c[2])):
        b = b.copy()
        b["chain_from"] = np.where(b["chain_from"] >= 0, b["chain_from"] + n_each, -1)  # a job chains from its own slot
        out.append(np.concatenate([a, b]))
    return out
