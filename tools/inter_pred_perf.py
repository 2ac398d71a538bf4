#!/usr/bin/env python3
"""Times svt_hip_inter_pred_batch on one 2160p 10-bit picture tiled with 16x16, 32x32 and 64x64 blocks (the RD job sets of bench.py), beside the copy kernel.

Per block size three batches: a single reference with random 1/8 MVs (within +-16 samples, random dual filters), an average compound of two
such references, and a single reference with full-pel MVs only.  The reference planes are padded by 160 samples.  HIP events around each launch
on the context stream, 5 warm-up launches, median of --reps.  A sample of the jobs of every batch is compared with the restatement of
tests/inter_pred_cases.py.  Per batch: ms, the bytes read and written (the samples of every job's source window, tile by tile as the kernel
stages them, plus the samples it writes; the job records and status bytes on top) and the GB/s that makes.
Beside it: svt_hip_fullpel_pred_batch on the same picture (one reference, random full-pel MVs per 16x16 PU) -- the full-pel batches move the
same bytes, so its time is what they are measured against -- and the PCIe bytes the host path would move: the prediction up, per candidate
(2 bytes per sample).  Prints one JSON line per batch (and, with --out, writes the figures as JSON)."""
import ctypes as C
import statistics

import numpy as np

import perf_common

perf_common.repo_paths()
import inter_pred_cases as ip  # noqa: E402
from svt_av1_psyex_amd import abi, api, pred  # noqa: E402

W, H, PAD = 3840, 2160, 160


def median_min(ms):
    return statistics.median(ms), min(ms)


def make_jobs(rng, size, kind):
    """one job per block of the picture: kind 'single' / 'average' (random 1/8 MVs) or 'fullpel'"""
    ys, xs = np.meshgrid(np.arange(0, H - size + 1, size), np.arange(0, W - size + 1, size), indexing="ij")
    n = ys.size
    jobs = np.zeros(n, abi.INTER_PRED_JOB_DTYPE)
    jobs["dst_offset"] = (ys.ravel() * W + xs.ravel()).astype(np.uint32)
    jobs["org_x"], jobs["org_y"], jobs["width"], jobs["height"] = xs.ravel(), ys.ravel(), size, size
    jobs["filter_x"], jobs["filter_y"] = rng.integers(0, 4, n), rng.integers(0, 4, n)
    jobs["ref"][:, 0], jobs["ref"][:, 1] = 0, (1 if kind == "average" else abi.INTER_PRED_NO_REF)
    mv = rng.integers(-128, 129, (n, 2, 2))
    jobs["mv"] = mv * 8 if kind == "fullpel" else mv
    jobs["mb_to_left_edge"], jobs["mb_to_right_edge"] = -(xs.ravel() * 8), (W - size - xs.ravel()) * 8
    jobs["mb_to_top_edge"], jobs["mb_to_bottom_edge"] = -(ys.ravel() * 8), (H - size - ys.ravel()) * 8
    return jobs


def traffic(jobs, size, kind):
    """(bytes read, bytes written) by the kernel's own count: per reference and tile, the window the variant stages"""
    tw, th = min(size, 16), 16
    tiles = (size // tw) * (size // th)
    fx, fy = (jobs["mv"][:, :, 1] * 2) & 15 != 0, (jobs["mv"][:, :, 0] * 2) & 15 != 0
    win = (tw + 7 * fx) * (th + 7 * fy) * tiles  # [n][2]: samples per reference
    refs = 2 if kind == "average" else 1
    return int(win[:, :refs].sum()) * 2 + len(jobs) * 56, len(jobs) * (size * size * 2 + 1)


def main():
    a = perf_common.arguments(__doc__, 30)
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(9)
    planes = [rng.integers(0, 1024, (H + 2 * PAD, W + 2 * PAD)).astype(np.uint16) for _ in range(2)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_planes = [dev(p) for p in planes]
    refs = [pred.plane_ref(t, W + 2 * PAD, PAD, PAD, W + 2 * PAD, H + 2 * PAD) for t in t_planes]
    t_dst = torch.zeros(H * W * 2, dtype=torch.uint8, device="cuda")
    results = []
    for size in (16, 32, 64):
        for kind in ("single", "average", "fullpel"):
            jobs = make_jobs(rng, size, kind)
            n = len(jobs)
            t_jobs, t_status = dev(jobs), torch.zeros(n, dtype=torch.uint8, device="cuda")
            d = abi.InterPredDesc(bit_depth=10, n_refs=2, n_jobs=n, dst=t_dst.data_ptr(), dst_stride=W, dst_samples=W * H, jobs=t_jobs.data_ptr(),
                                  status=t_status.data_ptr())
            d.refs[0], d.refs[1] = refs
            torch.cuda.synchronize()
            ms, ms_min = median_min(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_inter_pred_batch(ctx._h, C.byref(d)), "svt_hip_inter_pred_batch")))
            got = t_dst.cpu().numpy().view(np.uint16).reshape(H, W)
            if t_status.cpu().numpy().any():
                raise SystemExit(f"{size} {kind}: a job reported a status other than 0")
            for i in np.linspace(0, n - 1, 40).astype(int):  # a sample of the jobs against the restatement
                want, _ = ip.restate_job([(p, PAD, PAD) for p in planes], 10, 0, jobs[i])
                x, y = int(jobs[i]["org_x"]), int(jobs[i]["org_y"])
                if not np.array_equal(got[y:y + size, x:x + size], want):
                    raise SystemExit(f"{size} {kind}: job {i} differs from the restatement")
            rd_b, wr_b = traffic(jobs, size, kind)
            res = dict(entry="svt_hip_inter_pred_batch", block=size, kind=kind, jobs=n, ms_median=round(ms, 4), ms_min=round(ms_min, 4), bytes_read=rd_b,
                       bytes_written=wr_b, gb_per_s=round((rd_b + wr_b) / ms / 1e6, 1), host_path_pcie_bytes_up=n * size * size * 2)
            results.append(res)
            perf_common.emit(res)
    # the copy kernel on the same picture: one reference, random full-pel MVs per 16x16 PU
    nb = ((W + 63) // 64) * ((H + 63) // 64)
    mvx, mvy = rng.integers(-128, 129, (nb, 8, 85)), rng.integers(-128, 129, (nb, 8, 85))
    t_mv = dev(((mvy.astype(np.int64) & 0xFFFF) << 16 | (mvx.astype(np.int64) & 0xFFFF)).astype(np.uint32))
    t_ref = dev(np.ascontiguousarray(planes[0][PAD:PAD + H, PAD:PAD + W]))
    pj = (abi.PredJob * 1)()
    pj[0].ref, pj[0].sb_best_mv, pj[0].pred = t_ref.data_ptr(), t_mv.data_ptr(), t_dst.data_ptr()
    torch.cuda.synchronize()
    ms, ms_min = median_min(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_fullpel_pred_batch(ctx._h, W, W, H, 10, W, 1, pj), "svt_hip_fullpel_pred_batch")))
    res = dict(entry="svt_hip_fullpel_pred_batch", block=16, kind="fullpel", jobs=(W // 16) * (H // 16), ms_median=round(ms, 4), ms_min=round(ms_min, 4),
               bytes_read=W * H * 2, bytes_written=W * H * 2, gb_per_s=round(W * H * 4 / ms / 1e6, 1))
    results.append(res)
    perf_common.emit(res)
    for r in results[:-1]:
        if r["kind"] == "fullpel":
            perf_common.emit(dict(block=r["block"], fullpel_over_copy_kernel=round(r["ms_median"] / ms, 2)))
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
