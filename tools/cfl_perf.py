#!/usr/bin/env python3
"""Times svt_hip_cfl_pred_batch on every chroma block of one 2160p 10-bit picture, beside a device-to-device copy of the bytes it writes.

The chroma planes are 1920 x 1080; the picture is tiled with 8x8 and with 16x16 chroma blocks, every block one job with the alpha search's 33
alphas, so a job writes 2 * 33 * W * H samples: the slots of a job lie back to back (slot_stride = W * H, the lay-out svt_hip_rd_batch reads
through pred_offset).  The luma is a random 3840 x 2160 plane, the DC planes random 1920 x 1080 planes.  HIP events around each launch on the
context stream, 5 warm-up launches, median of --reps with the quartiles, minimum and maximum.  A sample of the jobs of every batch is compared
with the restatement of tests/cfl_cases.py.  Per batch: ms, the bytes read (the luma extent and the two DC blocks, two bytes a sample, and the
job records) and written (the slots and the status bytes) and the GB/s that makes.  The yardstick is a device-to-device copy (torch's copy_ on
the same stream, timed the same way) of as many bytes as the batch writes; the ratio batch / copy is printed per batch.  Prints one JSON line per
measurement (and, with --out, writes them as JSON)."""
import ctypes as C

import numpy as np

import perf_common

perf_common.repo_paths()
import cfl_cases as cc  # noqa: E402
from svt_av1_psyex_amd import abi, api, cfl  # noqa: E402

LW, LH = 3840, 2160
CW, CH = LW // 2, LH // 2


def ms_fields(ms):
    return {f"ms_{k}": round(v, 4) for k, v in perf_common.quartiles(ms).items()}


def make_jobs(size):
    ys, xs = np.meshgrid(np.arange(0, CH - size + 1, size), np.arange(0, CW - size + 1, size), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()
    jobs = np.zeros(ys.size, abi.CFL_PRED_JOB_DTYPE)
    jobs["luma_x"], jobs["luma_y"] = 2 * xs, 2 * ys
    jobs["dc_offset"] = (ys * CW + xs).astype(np.uint32)[:, None]
    jobs["dst_offset"] = (np.arange(ys.size, dtype=np.uint64) * (abi.CFL_SLOTS * size * size)).astype(np.uint32)[:, None]
    return jobs


def main():
    a = perf_common.arguments(__doc__, 30)
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(12)
    luma = rng.integers(0, 1024, (LH, LW)).astype(np.uint16)
    dc = [rng.integers(0, 1024, (CH, CW)).astype(np.uint16) for _ in range(2)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_luma, t_dc = dev(luma), [dev(p) for p in dc]
    results = []
    for size in (8, 16):
        jobs = make_jobs(size)
        n = len(jobs)
        slot = size * size
        samples = n * abi.CFL_SLOTS * slot
        t_jobs, t_status = dev(jobs), torch.zeros(n, dtype=torch.uint8, device="cuda")
        t_dst = [torch.zeros(samples * 2, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        d = cfl.run_cfl_pred_device(ctx, 10, size, size, cfl.ALPHAS_FULL, t_luma, LW, LW, LH, t_dc, CW, t_dst, size, slot, t_jobs, n, t_status)
        t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_cfl_pred_batch(ctx._h, C.byref(d)), "svt_hip_cfl_pred_batch")))
        if t_status.cpu().numpy().any():
            raise SystemExit(f"{size}x{size}: a job reported a status other than 0")
        got = [x.cpu().numpy().view(np.uint16) for x in t_dst]
        b = {"bit_depth": 10, "width": size, "height": size, "alphas": cfl.ALPHAS_FULL, "dc": dc, "dst_stride": size, "slot_stride": slot}
        for i in np.linspace(0, n - 1, 40).astype(int):  # a sample of the jobs against the restatement
            j = jobs[i]
            want, _, _ = cc.restate_job(luma, 10, size, size, int(j["luma_x"]), int(j["luma_y"]), [cc.dc_block(b, j, 0), cc.dc_block(b, j, 1)], cfl.ALPHAS_FULL)
            if not np.array_equal(cc.blocks_of(b, got, j), want):
                raise SystemExit(f"{size}x{size}: job {i} differs from the restatement")
        rd_b, wr_b = n * (4 * slot * 2 + 2 * slot * 2 + 24), 2 * samples * 2 + n
        res = dict(entry="svt_hip_cfl_pred_batch", block=size, n_alpha=abi.CFL_SLOTS, jobs=n, **t, bytes_read=rd_b, bytes_written=wr_b,
                   gb_per_s=round((rd_b + wr_b) / t["ms_median"] / 1e6, 1), gb_per_s_written=round(wr_b / t["ms_median"] / 1e6, 1))
        perf_common.emit(res)
        # the yardstick: as many bytes, device to device
        t_from, t_to = torch.zeros(wr_b, dtype=torch.uint8, device="cuda"), torch.zeros(wr_b, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(ext):
            c = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: t_to.copy_(t_from)))
        copy = dict(entry="device_to_device_copy", block=size, bytes=wr_b, **c, gb_per_s_written=round(wr_b / c["ms_median"] / 1e6, 1))
        perf_common.emit(copy)
        res["over_copy"] = round(t["ms_median"] / c["ms_median"], 2)
        perf_common.emit(dict(block=size, over_copy=res["over_copy"]))
        results += [res, copy]
        del t_dst, t_from, t_to, got
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
