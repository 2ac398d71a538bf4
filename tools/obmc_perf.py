#!/usr/bin/env python3
"""Times svt_hip_obmc_neighbour_batch, svt_hip_obmc_blend_batch and svt_hip_obmc_target_batch on 2160p 10-bit luma tiled with 16x16, 32x32 and 64x64 blocks.

Every block has one above neighbour over its whole width and one left neighbour over its whole height (the two strips together are one block's
worth of samples), EIGHTTAP_REGULAR, MVs (13, -11) / 8 and (-5, 19) / 8: the 8-tap 2-D path.  The yardstick, which exists without this feature, is
svt_hip_inter_pred_batch's single-reference prediction of the same blocks with the first MV: one block's worth of the same convolution.  The reference
plane is padded by 160 samples.  HIP events around each launch on the context stream, 5 warm-up launches, --reps timed ones: median, quartiles,
minimum, maximum.  Six blocks of every batch are compared with the restatement of tests/obmc_cases.py after the timed launches (the blend on a copy of
the prediction: a timed blend launch works in place on what the launch before it left, which costs the same).  Prints a table (and, with --out, writes it)."""

import numpy as np

import perf_common

perf_common.repo_paths()
import inter_pred_cases as ip  # noqa: E402
import obmc_cases as oc  # noqa: E402
from svt_av1_psyex_amd import abi, api, obmc, pred  # noqa: E402

W, H, PAD = 3840, 2160, 160
MV_A, MV_L = (13, -11), (-5, 19)


def make_blocks(size):
    ys, xs = np.meshgrid(np.arange(0, H - size + 1, size), np.arange(0, W - size + 1, size), indexing="ij")
    n = ys.size
    b = np.zeros(n, abi.OBMC_BLOCK_DTYPE)
    b["org_x"], b["org_y"], b["width"], b["height"], b["n_above"], b["n_left"] = xs.ravel(), ys.ravel(), size, size, 1, 1
    b["mb_to_left_edge"], b["mb_to_right_edge"] = -(xs.ravel() * 8), (W - size - xs.ravel()) * 8
    b["mb_to_top_edge"], b["mb_to_bottom_edge"] = -(ys.ravel() * 8), (H - size - ys.ravel()) * 8
    b["strip_offset"] = np.arange(n, dtype=np.int64) * size * size  # luma only: the areas one after the other
    for side, mv in (("above", MV_A), ("left", MV_L)):
        b[side]["size"][:, 0], b[side]["mv"][:, 0] = size >> 2, mv
    jobs = np.zeros(n, abi.OBMC_JOB_DTYPE)
    jobs["block"], jobs["offset"] = np.arange(n), ys.ravel() * W + xs.ravel()
    pj = np.zeros(n, abi.INTER_PRED_JOB_DTYPE)
    pj["dst_offset"], pj["org_x"], pj["org_y"], pj["width"], pj["height"] = jobs["offset"], xs.ravel(), ys.ravel(), size, size
    pj["ref"][:, 1], pj["mv"][:, 0] = abi.INTER_PRED_NO_REF, MV_A
    for f in ("mb_to_left_edge", "mb_to_right_edge", "mb_to_top_edge", "mb_to_bottom_edge"):
        pj[f] = b[f]
    return b, jobs, pj


def search_timings(ctx, ext, reps, dev):
    """svt_hip_obmc_search_batch (refine level 2: the sub-pel tree alone, and level 0 with range 8 and the diagonal sites) beside svt_hip_md_subpel_batch
    with search_method 1 and USE_8_TAPS on the same blocks, start MVs and cost tables; 8-bit planes; the source is the reference 3/8 down, 5/8 right"""
    import ctypes as C
    import torch
    import md_search_cases as mdc
    import obmc_search_cases as sc
    L = api.lib()
    rng = np.random.default_rng(16)
    ref = rng.integers(0, 256, (H + 2 * PAD, W + 2 * PAD)).astype(np.uint8)
    k = np.ones(5) / 5
    for ax in (0, 1):
        ref = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, ref.astype(np.float64))
    ref = np.ascontiguousarray(ref.astype(np.uint8))
    src = sc.upsampled(ref, PAD, PAD, W, H, 3, 5).astype(np.uint8)
    tables = [np.ascontiguousarray(t, dtype=np.int32) for t in sc.cost_tables()]
    t_ref, t_src, t_tab = dev(ref), dev(src), [dev(t) for t in tables]
    out = ["", f"{'what':<40}{'block':>6}{'jobs':>8}{'median':>9}{'q1':>9}{'q3':>9}{'min':>9}{'max':>9}{'us / block':>14}"]
    ratios = []
    for size in (16, 32, 64):
        ys, xs = np.meshgrid(np.arange(0, H - size + 1, size), np.arange(0, W - size + 1, size), indexing="ij")
        n = ys.size
        # wsrc / mask of a block without neighbours: the plain source, so that both searches score the same prediction against the same target
        wsrc = np.zeros(n * size * size, np.int32)
        for i, (y, x) in enumerate(zip(ys.ravel(), xs.ravel())):
            wsrc[i * size * size:(i + 1) * size * size] = src[y:y + size, x:x + size].astype(np.int32).reshape(-1) * 4096
        t_wsrc, t_mask = dev(wsrc), dev(np.full(n * size * size, 4096, np.int32))
        oj = np.zeros(n, abi.OBMC_SEARCH_JOB_DTYPE)
        oj["target_offset"], oj["ref_offset"] = np.arange(n) * size * size, (ys.ravel() + PAD) * (W + 2 * PAD) + xs.ravel() + PAD
        oj["width"], oj["height"] = size, size
        oj["col_min"], oj["col_max"], oj["row_min"], oj["row_max"] = -(xs.ravel() + size + 4), W - xs.ravel() + 4, -(ys.ravel() + size + 4), H - ys.ravel() + 4
        mj = np.zeros(n, abi.SUBPEL_JOB_DTYPE)
        mj["src_offset"], mj["ref_offset"], mj["width"], mj["height"], mj["log2_pels"] = ys.ravel() * W + xs.ravel(), oj["ref_offset"], size, size, int(np.log2(size * size))
        mj["col_min"], mj["col_max"], mj["row_min"], mj["row_max"], mj["early_exit_th"] = -2000, 2000, -2000, 2000, 1000
        t_oj, t_mj = dev(oj), dev(mj)
        t_best, t_res, t_st = (torch.zeros(n * k_, dtype=torch.uint8, device="cuda") for k_ in (4, 24, 1))
        o = {k_: torch.zeros(n * 2, dtype=torch.int32, device="cuda") for k_ in ("best_mv", "besterr", "distortion", "sse", "center_err")}
        d = abi.SubpelBatchDesc(n_jobs=n, src_stride=W, ref_stride=W + 2 * PAD, src=t_src.data_ptr(), ref=t_ref.data_ptr(), jobs=t_mj.data_ptr(), allow_hp=1, forced_stop=0,
                                iters_per_step=2, round_dev_th=2147483647, search_method=1, subpel_search_type=3, mv_cost_type=0, error_per_bit=60,
                                mvjcost=t_tab[0].data_ptr(), best_mv=o["best_mv"].data_ptr(), besterr=o["besterr"].data_ptr(), distortion=o["distortion"].data_ptr(),
                                sse=o["sse"].data_ptr(), center_err=o["center_err"].data_ptr())
        d.mvcost[0], d.mvcost[1] = t_tab[1].data_ptr() + 4 * mdc.MV_CENTRE, t_tab[2].data_ptr() + 4 * mdc.MV_CENTRE
        torch.cuda.synchronize()
        t = {}
        runs = [("svt_hip_md_subpel_batch (8 taps)", lambda: ctx.check(L.svt_hip_md_subpel_batch(ctx._h, C.byref(d)), "svt_hip_md_subpel_batch"))]
        for what, level in (("svt_hip_obmc_search_batch (level 2)", 2), ("svt_hip_obmc_search_batch (level 0)", 0)):
            p = sc.params(level, 0, 1, 8, 1)
            runs.append((what, lambda p=p: obmc.run_search_device(ctx, p, t_ref, W + 2 * PAD, t_wsrc, t_mask, t_oj, n, t_best, t_res, t_st, tables=t_tab)))
        for what, launch in runs:
            t[what] = r = perf_common.quartiles(perf_common.timed(ctx, ext, reps, launch))
            out.append(f"{what:<40}{size:>6}{n:>8}{r['median']:>9.4f}{r['q1']:>9.4f}{r['q3']:>9.4f}{r['min']:>9.4f}{r['max']:>9.4f}{r['median'] * 1e3 / n:>14.4f}")
            print(out[-1], flush=True)
        if t_st.cpu().numpy().any():
            raise SystemExit(f"{size}: a search job reported a status other than 0")
        best = t_best.cpu().numpy().view(np.int16).reshape(n, 2)  # the last launch: level 0
        p = sc.params(0, 0, 1, 8, 1)
        for i in np.linspace(0, n - 1, 4).astype(int):
            want = sc.restate_job(p, ref, wsrc, np.full(len(wsrc), 4096, np.int32), oj[i], tables)
            if want is None or tuple(best[i]) != want[0]:
                raise SystemExit(f"{size}: search job {i} differs from the restatement")
        base = t["svt_hip_md_subpel_batch (8 taps)"]["median"]
        ratios.append(f"{size}x{size} level 2 {t['svt_hip_obmc_search_batch (level 2)']['median'] / base:.2f}, level 0 {t['svt_hip_obmc_search_batch (level 0)']['median'] / base:.2f}")
    out += ["", "OBMC search / svt_hip_md_subpel_batch (medians):  " + "   ".join(ratios)]
    print(out[-1], flush=True)
    return out


def main():
    a = perf_common.arguments(__doc__, 30, "also write the table to this file")
    import torch
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(15)
    plane = rng.integers(0, 1024, (H + 2 * PAD, W + 2 * PAD)).astype(np.uint16)
    src = rng.integers(0, 256, (H, W)).astype(np.uint8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_plane, t_src = dev(plane), dev(src)
    refs = [pred.plane_ref(t_plane, W + 2 * PAD, PAD, PAD, W + 2 * PAD, H + 2 * PAD)]
    planes = [(plane, PAD, PAD)]
    lines = [f"{'what':<40}{'block':>6}{'jobs':>8}{'median':>9}{'q1':>9}{'q3':>9}{'min':>9}{'max':>9}{'ns / sample':>14}"]
    ratios = []
    for size in (16, 32, 64):
        blocks, jobs, pj = make_blocks(size)
        n = len(blocks)
        t_blocks, t_jobs, t_pj = dev(blocks), dev(jobs), dev(pj)
        tjobs = jobs.copy()
        tjobs["offset"] = blocks["strip_offset"]
        t_tjobs = dev(tjobs)
        t_pred = torch.zeros(H * W * 2, dtype=torch.uint8, device="cuda")
        t_above, t_left = (torch.zeros(n * size * size * 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        t_wsrc, t_mask = (torch.zeros(n * size * size * 4, dtype=torch.uint8, device="cuda") for _ in range(2))
        t_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        runs = [("svt_hip_inter_pred_batch (single)", lambda: pred.run_inter_pred_device(ctx, 10, 0, 0, refs, t_pred, W, t_pj, n, t_st)),
                ("svt_hip_obmc_neighbour_batch", lambda: obmc.run_neighbour_device(ctx, 10, 0, 0, 0, refs, t_blocks, n, t_jobs, n, t_above, t_left, t_st)),
                ("svt_hip_obmc_blend_batch", lambda: obmc.run_blend_device(ctx, 10, 0, 0, 0, t_blocks, n, t_jobs, n, t_above, t_left, t_pred, W, t_st)),
                ("svt_hip_obmc_target_batch", lambda: obmc.run_target_device(ctx, 10, t_blocks, n, t_tjobs, n, t_above, t_left, t_src, W, t_wsrc, t_mask, t_st))]
        t = {}
        for what, launch in runs:
            t[what] = r = perf_common.quartiles(perf_common.timed(ctx, ext, a.reps, launch))
            if t_st.cpu().numpy().any():
                raise SystemExit(f"{size} {what}: a job reported a status other than 0")
            lines.append(f"{what:<40}{size:>6}{n:>8}{r['median']:>9.4f}{r['q1']:>9.4f}{r['q3']:>9.4f}{r['min']:>9.4f}{r['max']:>9.4f}{r['median'] * 1e6 / (n * size * size):>14.4f}")
            print(lines[-1], flush=True)
        # a sample of the blocks against the restatement, from a fresh prediction
        pred.run_inter_pred_device(ctx, 10, 0, 0, refs, t_pred, W, t_pj, n, t_st)
        ctx.sync()
        own = t_pred.cpu().numpy().view(np.uint16).reshape(H, W).copy()
        obmc.run_blend_device(ctx, 10, 0, 0, 0, t_blocks, n, t_jobs, n, t_above, t_left, t_pred, W, t_st)
        ctx.sync()
        got = t_pred.cpu().numpy().view(np.uint16).reshape(H, W)
        above, left = t_above.cpu().numpy().view(np.uint16), t_left.cpu().numpy().view(np.uint16)
        wsrc, mask = t_wsrc.cpu().numpy().view(np.int32), t_mask.cpu().numpy().view(np.int32)
        for i in np.linspace(0, n - 1, 6).astype(int):
            blk = blocks[i]
            x, y, so = int(blk["org_x"]), int(blk["org_y"]), int(blk["strip_offset"])
            for d, j, drow, dcol in oc.strip_jobs(blk, 0):
                want = ip.restate_job(planes, 10, 0, j)[0]
                strip = (left if d else above)[so:so + size * size].reshape(size, size)
                if not np.array_equal(strip[drow:drow + want.shape[0], dcol:dcol + want.shape[1]], want):
                    raise SystemExit(f"{size}: block {i}: a strip differs from the restatement")
            A, Lf = above[so:so + size * size], left[so:so + size * size]
            if not np.array_equal(got[y:y + size, x:x + size], oc.restate_blend_block(blk, 0, A, Lf, own[y:y + size, x:x + size])):
                raise SystemExit(f"{size}: block {i}: the blend differs from the restatement")
            w_, m_ = oc.restate_target_block(blk, A, Lf, src[y:y + size, x:x + size], 10)
            if not (np.array_equal(wsrc[so:so + size * size], w_) and np.array_equal(mask[so:so + size * size], m_)):
                raise SystemExit(f"{size}: block {i}: the target differs from the restatement")
        base = t["svt_hip_inter_pred_batch (single)"]["median"]
        both = t["svt_hip_obmc_neighbour_batch"]["median"] + t["svt_hip_obmc_blend_batch"]["median"]
        ratios.append(f"{size}x{size} {both / base:.2f} (neighbours alone {t['svt_hip_obmc_neighbour_batch']['median'] / base:.2f})")
    lines.append("")
    lines.append("(neighbours + blend) / single-reference prediction (medians):  " + "   ".join(ratios))
    print("\n".join(lines[-2:]), flush=True)
    lines += search_timings(ctx, ext, a.reps, dev)
    ctx.close()
    perf_common.write_lines(a.out, lines)


if __name__ == "__main__":
    main()
