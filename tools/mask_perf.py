#!/usr/bin/env python3
"""Times the masked prediction entries and their searches on one 2160p picture, beside the entries that exist without them.

Prediction, 10-bit luma, the plane tiled with one block size per batch:
  svt_hip_masked_pred_batch  wedge at 8x8 / 16x16 / 32x32 (every job its own index and sign), DIFFWTD at 64x64 (and at the wedge sizes), the masks
                             stored; both references EIGHTTAP_REGULAR with MVs fractional on both axes (the 8-tap 2-D path twice)
  svt_hip_inter_pred_batch   the yardstick: the compound average on the same job list and MVs -- the same two convolutions
Searches, on the same tilings, 10-bit: svt_hip_mask_search_batch kind 0 (8x8 / 16x16 / 32x32), kind 1 (the same and 64x64), kind 2 (8x8 / 16x16 /
32x32, ii_wedge_mode 2), beside svt_hip_block_stats_batch's SSE on the same blocks (one pass over two planes).
HIP events around each launch on the context stream, 5 warm-up launches, the median of --reps with the quartiles, minimum and maximum.  After
the timed launches a sample of the jobs of every batch is compared with the restatement of tests/mask_cases.py.  Prints one JSON line per
measurement (and, with --out, writes them as JSON)."""
import ctypes as C

import numpy as np

import perf_common

perf_common.repo_paths()
import mask_cases as mc  # noqa: E402
from svt_av1_psyex_amd import abi, api, mask, pred  # noqa: E402

LW, LH, PAD = 3840, 2160, 80


def ms_fields(ms):
    return {f"ms_{k}": round(v, 4) for k, v in perf_common.quartiles(ms).items()}


def grid(size):
    ys, xs = np.meshgrid(np.arange(0, LH - size + 1, size), np.arange(0, LW - size + 1, size), indexing="ij")
    return xs.ravel(), ys.ravel()


def pred_fields(jobs, size):
    xs, ys = grid(size)
    jobs["dst_offset"] = (ys * LW + xs).astype(np.uint32)
    jobs["org_x"], jobs["org_y"], jobs["width"], jobs["height"] = xs, ys, size, size
    jobs["ref"][:, 0], jobs["ref"][:, 1] = 0, 1
    jobs["mv"][:, 0, 0], jobs["mv"][:, 0, 1], jobs["mv"][:, 1, 0], jobs["mv"][:, 1, 1] = 13, -11, -5, 19  # (row, col) in 1/8: fractional on both axes
    jobs["mb_to_left_edge"], jobs["mb_to_right_edge"] = -(xs * 8), (LW - xs - size) * 8
    jobs["mb_to_top_edge"], jobs["mb_to_bottom_edge"] = -(ys * 8), (LH - ys - size) * 8


def main():
    a = perf_common.arguments(__doc__, 30)
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(14)
    planes = [rng.integers(0, 1024, (LH + 2 * PAD, LW + 2 * PAD)).astype(np.uint16) for _ in range(2)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_planes = [dev(p) for p in planes]
    stride, rows = LW + 2 * PAD, LH + 2 * PAD
    refs = [pred.plane_ref(t, stride, PAD, PAD, stride, rows) for t in t_planes]
    rplanes = [(p, PAD, PAD) for p in planes]
    t_dst = torch.zeros(LW * LH * 2, dtype=torch.uint8, device="cuda")
    t_mask = torch.zeros(LW * LH, dtype=torch.uint8, device="cuda")
    results = []

    def report(**kw):
        perf_common.emit(kw)
        results.append(kw)

    # ---- prediction
    for size in (8, 16, 32, 64):
        n = len(grid(size)[0])
        t_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        medians = {}
        for what in ("average", "wedge", "diffwtd"):
            if what == "wedge" and size == 64:
                continue
            if what == "average":
                jobs = np.zeros(n, abi.INTER_PRED_JOB_DTYPE)
                pred_fields(jobs, size)
                t_jobs = dev(jobs)
                torch.cuda.synchronize()
                d = pred.run_inter_pred_device(ctx, 10, 0, 0, refs, t_dst, LW, t_jobs, n, t_status)
                t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_inter_pred_batch(ctx._h, C.byref(d)), "svt_hip_inter_pred_batch")))
            else:
                jobs = np.zeros(n, abi.MASKED_PRED_JOB_DTYPE)
                pred_fields(jobs["pred"], size)
                jobs["comp_type"] = mc.WEDGE if what == "wedge" else mc.DIFFWTD
                jobs["wedge_index"], jobs["wedge_sign"], jobs["mask_type"] = np.arange(n) % 16, (np.arange(n) >> 4) & 1, np.arange(n) & 1
                jobs["luma_width"], jobs["luma_height"], jobs["mask_offset"] = size, size, np.arange(n, dtype=np.uint32) * size * size
                t_jobs = dev(jobs)
                torch.cuda.synchronize()
                d = mask.run_masked_pred_device(ctx, 10, 0, 0, 0, refs, t_dst, LW, t_jobs, n, t_status, mask_buf=t_mask)
                t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_masked_pred_batch(ctx._h, C.byref(d)), "svt_hip_masked_pred_batch")))
                got = t_dst.cpu().numpy().view(np.uint16).reshape(LH, LW)
                b = {"bit_depth": 10, "ss_x": 0, "ss_y": 0, "plane": 0, "planes": rplanes, "mv_array": None, "results": None, "dst_shape": (LH, LW), "dst_stride": LW}
                for i in np.linspace(0, n - 1, 6).astype(int):  # a sample of the jobs against the restatement
                    x, y = int(jobs[i]["pred"]["org_x"]), int(jobs[i]["pred"]["org_y"])
                    if not np.array_equal(got[y:y + size, x:x + size], mc.restate_pred_job(b, rplanes, jobs[i], None)[0]):
                        raise SystemExit(f"{what} {size}x{size}: job {i} differs from the restatement")
            if t_status.cpu().numpy().any():
                raise SystemExit(f"{what} {size}x{size}: a job reported a status other than 0")
            medians[what] = t["ms_median"]
            report(entry="svt_hip_inter_pred_batch (average)" if what == "average" else f"svt_hip_masked_pred_batch ({what})", block=size, jobs=n, **t,
                   ns_per_sample=round(t["ms_median"] * 1e6 / (n * size * size), 4))
        report(block=size, **{f"{k}_over_average": round(v / medians["average"], 2) for k, v in medians.items() if k != "average"})

    # ---- searches: the source is the first plane's picture, pred0 / pred1 the two planes displaced, the four intra blocks rows of a fifth plane
    src = np.ascontiguousarray(planes[0][PAD:PAD + LH, PAD:PAD + LW])
    p0 = np.clip(src.astype(np.int32) + rng.integers(-40, 41, src.shape), 0, 1023).astype(np.uint16)
    p1 = np.clip(src.astype(np.int32) + rng.integers(-40, 41, src.shape), 0, 1023).astype(np.uint16)
    t_src, t_p0, t_p1 = dev(src), dev(p0), dev(p1)
    sp = {"src": src, "pred0": p0, "pred1": p1, "intra": p0}
    for size in (8, 16, 32, 64):
        xs, ys = grid(size)
        n = len(xs)
        t_res, t_status = torch.zeros(n * 24, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        medians = {}
        for kind in (0, 1, 2):
            if size == 64 and kind != 1:
                continue
            jobs = np.zeros(n, abi.MASK_SEARCH_JOB_DTYPE)
            jobs["src_offset"] = jobs["pred0_offset"] = jobs["pred1_offset"] = (ys * LW + xs).astype(np.uint32)
            for m in range(4):  # the intra plane is pred0: four blocks a few samples apart
                jobs["intra_offset"][:, m] = ((ys * LW + np.minimum(xs + m, LW - size))).astype(np.uint32)
            jobs["width"], jobs["height"], jobs["kind"], jobs["ii_wedge_mode"] = size, size, kind, 2
            t_jobs = dev(jobs)
            torch.cuda.synchronize()
            d = mask.run_mask_search_device(ctx, 10, 0, t_src, LW, t_p0, LW, t_p1, LW, t_p0, LW, t_jobs, n, t_res, t_status)
            t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_mask_search_batch(ctx._h, C.byref(d)), "svt_hip_mask_search_batch")))
            got = t_res.cpu().numpy().view(abi.MASK_SEARCH_RESULT_DTYPE)
            if t_status.cpu().numpy().any():
                raise SystemExit(f"search kind {kind} {size}x{size}: a job reported a status other than 0")
            for i in np.linspace(0, n - 1, 6).astype(int):
                if got[i].tobytes() != mc.restate_search_job(sp, 10, 0, jobs[i])[0].tobytes():
                    raise SystemExit(f"search kind {kind} {size}x{size}: job {i} differs from the restatement")
            medians[kind] = t["ms_median"]
            report(entry=f"svt_hip_mask_search_batch (kind {kind})", block=size, jobs=n, **t, us_per_launch=round(t["ms_median"] * 1e3, 1),
                   ns_per_sample=round(t["ms_median"] * 1e6 / (n * size * size), 4))
        # the yardstick: one SSE pass over two planes on the same blocks
        bjobs = np.zeros(n, abi.BLOCK_JOB_DTYPE)
        bjobs["src_offset"] = bjobs["ref_offset"] = (ys * LW + xs).astype(np.uint32)
        bjobs["width"], bjobs["height"] = size, size
        t_bjobs, t_sse = dev(bjobs), torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        db = abi.BlockStatsDesc(bit_depth=10, n_jobs=n, src_stride=LW, ref_stride=LW, src=t_src.data_ptr(), ref=t_p1.data_ptr(), jobs=t_bjobs.data_ptr(),
                                sse=t_sse.data_ptr())
        torch.cuda.synchronize()
        t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_block_stats_batch(ctx._h, C.byref(db)), "svt_hip_block_stats_batch")))
        report(entry="svt_hip_block_stats_batch (SSE)", block=size, jobs=n, **t, us_per_launch=round(t["ms_median"] * 1e3, 1),
               ns_per_sample=round(t["ms_median"] * 1e6 / (n * size * size), 4))
        report(block=size, **{f"kind{k}_over_sse": round(v / t["ms_median"], 2) for k, v in medians.items()})
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
