#!/usr/bin/env python3
"""Times the three CDEF entries on one 3840x2160 picture's work.

  svt_hip_cdef_search_batch   2,040 filter blocks, full masks, at 8 and at 10 bits, with 64 and with 4 strengths, subsampling_factor 1
  svt_hip_cdef_pick_batch     on the search's mse: 75 rounds of two launches
  svt_hip_cdef_apply_batch    three planes, four strength pairs in turn over the filter blocks
HIP events around each batch on the context stream, 5 warm-up batches, the median of --reps (default 20) with the quartiles, minimum and maximum.
Two runs of the search and of the apply must give the same bytes (the pick biases its input in place, so its second run is another problem).  With
--resources the tool compiles csrc/cdef_kernel.hip once more for its kernels' registers, scratch, LDS and occupancy as the compiler reports them.
Prints one JSON line per measurement (and, with --out, writes them as text)."""
import json
import os
import re
import subprocess
import sys

import numpy as np

import perf_common

ROOT = perf_common.repo_paths()
import cdef_cases as cc  # noqa: E402
from svt_av1_psyex_amd import api, cdef  # noqa: E402


def ms_fields(ms):
    return {f"ms_{k}": round(v, 4) for k, v in perf_common.quartiles(ms).items()}


def resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} from hipcc's kernel-resource-usage remarks"""
    src = os.path.join(ROOT, "svt-av1-psyex_amd", "csrc", "cdef_kernel.hip")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-x", "hip", "--cuda-device-only",
                        "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull], capture_output=True, text=True, check=True)
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", m.group(2))
            name = re.sub(r"E\d*Svt.*$|ILb([01])EEEv.*$", lambda q: f"<{'hbd' if q.group(1) == '1' else 'lbd'}>" if q.group(1) else "", name)
            out[name] = {}
        elif name:
            out[name][keys[m.group(1)]] = int(m.group(2))
    return out


def picture_case(ctx, ext, reps, bd, n):
    import ctypes as C
    w, h = 3840, 2160
    recon, src = cc.picture("noise", w, h, bd, 99)
    masks = cc.masks_of("full", w, h)
    sy = list(range(64)) if n == 64 else [0, 9, 33, 63]
    dt = api.sample_dtype(bd)
    t_recon, t_src = [api.to_device(p, dt) for p in recon], [api.to_device(p, dt) for p in src]
    t_masks = api.to_device(masks)
    n_fb = cdef.n_fb_of(w, h)
    so = cdef.run_cdef_search_device(ctx, t_recon, t_src, w, h, bd, 100, 1, sy, sy, t_masks, with_block_dist=False)
    ctx.sync()
    first = {k: t.cpu().numpy().copy() for k, t in so.items()}
    sd = cdef.search_desc(cdef.planes_of(t_recon, w, h), cdef.planes_of(t_src, w, h), bd, 100, 1, sy, sy, n_fb, t_masks.data_ptr(), so["mse"].data_ptr(), so["dir"].data_ptr(),
                          so["var"].data_ptr())
    rows = []
    r = ms_fields(perf_common.timed(ctx, ext, reps, lambda: ctx.check(api.lib().svt_hip_cdef_search_batch(ctx._h, C.byref(sd)), "svt_hip_cdef_search_batch")))
    assert all(np.array_equal(first[k], t.cpu().numpy()) for k, t in so.items()), "two runs of the search differ"
    samples = n_fb * 64 * 64 * n + 2 * n_fb * 32 * 32 * n
    r.update(what="cdef_search", picture=f"{w}x{h}", bit_depth=bd, strengths=n, filter_blocks=n_fb, filtered_samples=samples,
             gsamples_per_s=round(samples / r["ms_median"] / 1e6, 2))
    rows.append(r)
    po, work = cdef.run_cdef_pick_device(ctx, w, h, n, int(bd > 8), 60, 500, sy, sy, t_masks, so["mse"])
    ctx.sync()
    pd = cdef.pick_desc(w, h, n, int(bd > 8), 60, 500, sy, sy, t_masks.data_ptr(), so["mse"].data_ptr(), work.data_ptr(), po["result"].data_ptr(), po["fb_strength"].data_ptr())
    r = ms_fields(perf_common.timed(ctx, ext, reps, lambda: ctx.check(api.lib().svt_hip_cdef_pick_batch(ctx._h, C.byref(pd)), "svt_hip_cdef_pick_batch")))
    r.update(what="cdef_pick", picture=f"{w}x{h}", bit_depth=bd, strengths=n, filter_blocks=n_fb, launches=151)
    rows.append(r)
    if n == 64:
        rec = np.zeros(1, cdef.PICK_DTYPE)
        rec["y_strength"][0, :4], rec["uv_strength"][0, :4] = [13, 40, 63, 2], [13, 40, 63, 2]
        t_rec, t_fbs = api.to_device(rec), api.to_device((np.arange(n_fb) % 4).astype(np.int8))
        ao = cdef.run_cdef_apply_device(ctx, t_recon, w, h, bd, 4, 3, t_masks, t_fbs, t_rec)
        ctx.sync()
        first = [t.cpu().numpy().copy() for t in ao]
        ad = cdef.apply_desc(cdef.planes_of(t_recon, w, h), cdef.planes_of(ao, w, h), bd, 4, 3, n_fb, t_masks.data_ptr(), t_fbs.data_ptr(),
                             t_rec.data_ptr() + cdef.CdefPick.y_strength.offset, t_rec.data_ptr() + cdef.CdefPick.uv_strength.offset)
        r = ms_fields(perf_common.timed(ctx, ext, reps, lambda: ctx.check(api.lib().svt_hip_cdef_apply_batch(ctx._h, C.byref(ad)), "svt_hip_cdef_apply_batch")))
        assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(first, ao)), "two runs of the apply differ"
        r.update(what="cdef_apply", picture=f"{w}x{h}", bit_depth=bd, planes=3, filter_blocks=n_fb)
        rows.append(r)
    return rows


def main():
    import torch
    resources_wanted = "--resources" in sys.argv
    if resources_wanted:
        sys.argv.remove("--resources")
    a = perf_common.arguments(__doc__, 20)
    ctx = api.Context()
    ext = torch.cuda.ExternalStream(ctx.stream)
    rows = []
    for bd in (8, 10):
        for n in (64, 4):
            for r in picture_case(ctx, ext, a.reps, bd, n):
                rows.append(r)
                perf_common.emit(r)
    ctx.close()
    if resources_wanted:
        rows.append({"what": "kernel_resources", **resources()})
        perf_common.emit(rows[-1])
    perf_common.write_lines(a.out, [json.dumps(r) for r in rows])


if __name__ == "__main__":
    main()
