#!/usr/bin/env python3
"""Times svt_hip_ssim_batch on one 2160p 10-bit and one 1080p 8-bit picture (src against a noisy copy standing in for the reconstruction).

Variants per picture: every full 64x64 region as a pyramid (85 nested blocks each, the region read once), then the same 85 * N blocks as plain
jobs, each with psy_rd 0 and 1.  HIP events around each launch on the context stream, 5 warm-up launches, median of --reps.  Bytes read are
the samples the variant needs (pyramid: each region's src and ref once; plain: every block's own samples), over the median time; the share
of HBM peak is that rate over 8.0 TB/s (the spec peak: an upper bound on what the kernel could stream).  The two forms' outputs are
compared, bit for bit.  Prints one line per variant (and, with --out, writes the figures as JSON)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")]
from svt_av1_psyex_amd import abi, api, stats  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s: the MI355X's HBM3E spec peak


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the figures as JSON to this file")
    a = ap.parse_args()
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(5)
    results = []
    for (W, H, bd) in ((3840, 2160, 10), (1920, 1080, 8)):
        mx, dt = (1 << bd) - 1, (np.uint8 if bd == 8 else np.uint16)
        src = rng.integers(0, mx + 1, (H, W)).astype(dt)
        ref = np.clip(src.astype(np.int32) + rng.integers(-mx // 16, mx // 16 + 1, src.shape), 0, mx).astype(dt)
        regions = np.array([(y * W + x, y * W + x, 64, 64, 0, 0) for y in range(0, H - 63, 64) for x in range(0, W - 63, 64)], dtype=abi.BLOCK_JOB_DTYPE)
        plain = np.concatenate([stats.expand_pyramid(r, W, W) for r in regions])
        n = len(plain)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
        t_src, t_ref, t_reg, t_plain = dev(src), dev(ref), dev(regions), dev(plain)
        outs = {}
        for form in ("pyramid", "plain"):
            for psy in (0.0, 1.0):
                t_ssim, t_dist = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
                d = abi.SsimBatchDesc(bit_depth=bd, src_stride=W, ref_stride=W, src=t_src.data_ptr(), ref=t_ref.data_ptr(), psy_rd=psy,
                                      ssim=t_ssim.data_ptr(), ssim_dist=t_dist.data_ptr())
                if form == "pyramid":
                    d.n_pyramids, d.pyramid_out_base, d.pyramids, d.jobs = len(regions), 0, t_reg.data_ptr(), t_plain.data_ptr()
                else:
                    d.n_jobs, d.jobs = n, t_plain.data_ptr()
                torch.cuda.synchronize()
                for _ in range(5):
                    ctx.check(L.svt_hip_ssim_batch(ctx._h, C.byref(d)), "svt_hip_ssim_batch")
                ctx.sync()
                ms = []
                with torch.cuda.stream(ext):
                    for _ in range(a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        ctx.check(L.svt_hip_ssim_batch(ctx._h, C.byref(d)), "svt_hip_ssim_batch")
                        e1.record()
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                ctx.sync()
                outs[(form, psy)] = (t_ssim.cpu().numpy().view(np.uint64).copy(), t_dist.cpu().numpy().copy())
                area = 64 * 64 * len(regions) if form == "pyramid" else int((plain["width"].astype(np.int64) * plain["height"]).sum())
                nbytes = 2 * area * src.itemsize
                t = statistics.median(ms)
                r = dict(picture=f"{W}x{H}", bit_depth=bd, form=form, psy_rd=psy, regions=len(regions), blocks=n, ms_median=round(t, 4),
                         ms_min=round(min(ms), 4), bytes_read=nbytes, gb_per_s=round(nbytes / t / 1e6, 1), hbm_peak_share=round(nbytes / t / 1e-3 / HBM_PEAK, 4))
                results.append(r)
                print(json.dumps(r), flush=True)
        for psy in (0.0, 1.0):
            same = all(np.array_equal(x, y) for x, y in zip(outs[("pyramid", psy)], outs[("plain", psy)]))
            ratio = next(r["ms_median"] for r in results if r["picture"] == f"{W}x{H}" and r["form"] == "plain" and r["psy_rd"] == psy) / \
                next(r["ms_median"] for r in results if r["picture"] == f"{W}x{H}" and r["form"] == "pyramid" and r["psy_rd"] == psy)
            r = dict(picture=f"{W}x{H}", psy_rd=psy, plain_over_pyramid=round(ratio, 2), outputs_identical=same)
            results.append(r)
            print(json.dumps(r), flush=True)
            if not same:
                raise SystemExit("pyramid and plain outputs differ")
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(results, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
