#!/usr/bin/env python3
"""Times svt_hip_intra_pred_batch on one 2160p 10-bit picture tiled with 16x16, 32x32 and 64x64 blocks (the RD job sets of bench.py), beside the copy kernel.

Per block size three mixes, every block of the picture one job: the non-directional modes (DC, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH at random), the
directional modes with the edge filter on (the eight modes, angle_delta and filt_type at random), and filter-intra (the five modes at random;
16x16 and 32x32 only).  The neighbours are read from a second plane of the same size (the open-loop case); the counts are what a block at that
place of the picture has: nothing above the first row or left of the first column, no top-right / bottom-left past the picture.  HIP events
around each launch on the context stream, 5 warm-up launches, median of --reps with the quartiles, minimum and maximum.  A sample of the jobs of
every batch is compared with the restatement of tests/intra_pred_cases.py.  Per batch: ms, the bytes moved (the neighbour samples the jobs name,
two bytes each, the job records, the samples and status bytes written) and the GB/s that makes.  Beside it: svt_hip_fullpel_pred_batch on the
same picture, which writes the same plane with no arithmetic -- the floor the ratios are taken against -- and the PCIe bytes the host path
would move: the prediction up, per candidate (2 bytes per sample).  Prints one JSON line per batch (and, with --out, writes them as JSON)."""
import ctypes as C

import numpy as np

import perf_common

perf_common.repo_paths()
import intra_pred_cases as ic  # noqa: E402
from svt_av1_psyex_amd import abi, api  # noqa: E402

W, H = 3840, 2160
TX_OF = {16: 2, 32: 3, 64: 4}


def ms_fields(ms):
    return {f"ms_{k}": round(v, 4) for k, v in perf_common.quartiles(ms).items()}


def make_jobs(rng, size, mix):
    """one job per block of the picture: mix 'nondir' / 'dir' / 'fi'"""
    ys, xs = np.meshgrid(np.arange(0, H - size + 1, size), np.arange(0, W - size + 1, size), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()
    n = ys.size
    jobs = np.zeros(n, abi.INTRA_PRED_JOB_DTYPE)
    jobs["dst_offset"] = (ys * W + xs).astype(np.uint32)
    jobs["nbr_x"], jobs["nbr_y"], jobs["tx_size"], jobs["filter_intra_mode"] = xs, ys, TX_OF[size], ic.NO_FI
    jobs["n_top_px"], jobs["n_left_px"] = np.where(ys > 0, size, 0), np.where(xs > 0, size, 0)
    jobs["n_topright_px"] = np.where((ys > 0) & (xs + 2 * size <= W), size, 0)
    jobs["n_bottomleft_px"] = np.where((xs > 0) & (ys + 2 * size <= H), size, 0)
    if mix == "nondir":
        jobs["mode"] = np.array(ic.NON_DIRECTIONAL)[rng.integers(0, 5, n)]
    elif mix == "dir":
        jobs["mode"], jobs["angle_delta"], jobs["filt_type"] = rng.integers(1, 9, n), rng.integers(-3, 4, n), rng.integers(0, 2, n)
    else:
        jobs["mode"], jobs["filter_intra_mode"] = ic.DC_PRED, rng.integers(0, 5, n)
    return jobs


def traffic(jobs, size):
    reads = sum(a + l + int(c) for a, l, c in (ic.job_reads(j) for j in jobs))
    return reads * 2 + len(jobs) * 24, len(jobs) * (size * size * 2 + 1)


def main():
    a = perf_common.arguments(__doc__, 30)
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(11)
    nbr = rng.integers(0, 1024, (H, W)).astype(np.uint16)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_nbr = dev(nbr)
    t_dst = torch.zeros(H * W * 2, dtype=torch.uint8, device="cuda")
    results = []
    for size in (16, 32, 64):
        for mix in ("nondir", "dir", "fi"):
            if mix == "fi" and size > 32:
                continue
            jobs = make_jobs(rng, size, mix)
            n = len(jobs)
            t_jobs, t_status = dev(jobs), torch.zeros(n, dtype=torch.uint8, device="cuda")
            d = abi.IntraPredDesc(bit_depth=10, disable_edge_filter=0, n_jobs=n, nbr=t_nbr.data_ptr(), nbr_stride=W, nbr_width=W, nbr_height=H,
                                  dst=t_dst.data_ptr(), dst_stride=W, dst_samples=W * H, jobs=t_jobs.data_ptr(), status=t_status.data_ptr())
            torch.cuda.synchronize()
            t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_intra_pred_batch(ctx._h, C.byref(d)), "svt_hip_intra_pred_batch")))
            got = t_dst.cpu().numpy().view(np.uint16).reshape(H, W)
            if t_status.cpu().numpy().any():
                raise SystemExit(f"{size} {mix}: a job reported a status other than 0")
            for i in np.linspace(0, n - 1, 40).astype(int):  # a sample of the jobs against the restatement
                want, _ = ic.restate_job(nbr, 10, 0, jobs[i])
                x, y = int(jobs[i]["nbr_x"]), int(jobs[i]["nbr_y"])
                if not np.array_equal(got[y:y + size, x:x + size], want):
                    raise SystemExit(f"{size} {mix}: job {i} differs from the restatement")
            rd_b, wr_b = traffic(jobs, size)
            res = dict(entry="svt_hip_intra_pred_batch", block=size, mix=mix, jobs=n, **t, bytes_read=rd_b, bytes_written=wr_b,
                       gb_per_s=round((rd_b + wr_b) / t["ms_median"] / 1e6, 1), host_path_pcie_bytes_up=n * size * size * 2)
            results.append(res)
            perf_common.emit(res)
    # the copy kernel on the same picture: one reference, random full-pel MVs per 16x16 PU
    nb = ((W + 63) // 64) * ((H + 63) // 64)
    mvx, mvy = rng.integers(-128, 129, (nb, 8, 85)), rng.integers(-128, 129, (nb, 8, 85))
    t_mv = dev(((mvy.astype(np.int64) & 0xFFFF) << 16 | (mvx.astype(np.int64) & 0xFFFF)).astype(np.uint32))
    pj = (abi.PredJob * 1)()
    pj[0].ref, pj[0].sb_best_mv, pj[0].pred = t_nbr.data_ptr(), t_mv.data_ptr(), t_dst.data_ptr()
    torch.cuda.synchronize()
    t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_fullpel_pred_batch(ctx._h, W, W, H, 10, W, 1, pj), "svt_hip_fullpel_pred_batch")))
    floor = dict(entry="svt_hip_fullpel_pred_batch", block=16, mix="copy", jobs=(W // 16) * (H // 16), **t, bytes_read=W * H * 2, bytes_written=W * H * 2,
                 gb_per_s=round(W * H * 4 / t["ms_median"] / 1e6, 1))
    perf_common.emit(floor)
    for r in results:
        r["over_copy_kernel"] = round(r["ms_median"] / floor["ms_median"], 2)
        perf_common.emit(dict(block=r["block"], mix=r["mix"], over_copy_kernel=r["over_copy_kernel"]))
    results.append(floor)
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
