"""Host-side helpers of the batched block-statistics entry (svt_hip_block_stats_batch) and of the SSIM batch (svt_hip_ssim_batch)."""
import ctypes as C

import numpy as np

from . import abi


def random_jobs(rng, plane_w, plane_h, n, sizes=None, square_only=False, subpel=False):
    """n block jobs with AV1 block shapes at random positions inside a plane_w x plane_h plane."""
    sizes = sizes or [(w, h) for w in (4, 8, 16, 32, 64, 128) for h in (4, 8, 16, 32, 64, 128) if max(w, h) <= 4 * min(w, h)]
    if square_only:
        sizes = [s for s in sizes if s[0] == s[1]]
    jobs = np.zeros(n, dtype=abi.BLOCK_JOB_DTYPE)
    for i in range(n):
        w, h = sizes[rng.integers(len(sizes))]
        w, h = min(w, plane_w), min(h, plane_h)
        x0, y0 = rng.integers(0, plane_w - w + 1 - int(subpel)), rng.integers(0, plane_h - h + 1 - int(subpel))  # sub-pel reads one more row / column
        x1, y1 = rng.integers(0, plane_w - w + 1), rng.integers(0, plane_h - h + 1)
        jobs[i] = (y0 * plane_w + x0, y1 * plane_w + x1, w, h, 0, 0)
    if subpel:
        jobs["subpel_x"] = rng.integers(0, 8, n)
        jobs["subpel_y"] = rng.integers(0, 8, n)
    return jobs


def expand_pyramid(region, src_stride, ref_stride):
    """the 85 plain jobs a hierarchical 64x64 region stands for, in its output-slot order: 64x64, 4 x 32x32, 16 x 16x16, 64 x 8x8, each level
    in raster order (SvtHipBlockStatsDesc.pyramids)"""
    out = np.zeros(abi.PYRAMID_BLOCKS, dtype=abi.BLOCK_JOB_DTYPE)
    k = 0
    for n in (64, 32, 16, 8):
        for y in range(0, 64, n):
            for x in range(0, 64, n):
                out[k] = (int(region["src_offset"]) + y * src_stride + x, int(region["ref_offset"]) + y * ref_stride + x, n, n, 0, 0)
                k += 1
    return out


def jobs_per_wave(ctx, n_jobs, satd=True):
    """svt_hip_block_stats_jobs_per_wave: the flat jobs one wave of a batch of n_jobs works through (the launch asks the same function)"""
    from . import api
    d = abi.BlockStatsDesc(bit_depth=8, n_jobs=n_jobs, satd=1 if satd else 0)  # only the pointer's presence is read
    return int(api.lib().svt_hip_block_stats_jobs_per_wave(ctx._h, C.byref(d)))


def run_hip(ctx, src, ref, jobs, bit_depth, satd=True, psy_rd=None, facade=None, pyramids=None, spare_jobs=0, fill=None, outputs=None):
    """facade: dict(pred_mode=u8[n], compound_type=u8[n], temporal_layer_index=int, spy_rd=int) -> also `facade_dist`.
    pyramids: optional array of 64x64 region jobs; their 85 outputs each follow the plain jobs' (slots len(jobs) + 85 k ...; the facade
    arrays then cover those slots too).
    fill: a byte every output array is pre-filled with (default: zeros); the arrays are then n + spare_jobs slots long, and the spare
    slots and the source, reference and job buffers are asserted to read back unchanged.
    outputs: the names of the output pointers to set (the others stay null; `satd` is then read from this list); the arrays of the
    others are returned as well, as they were filled."""
    import torch
    from . import api
    L = api.lib()
    dev = api.to_device
    n_plain = len(jobs)
    n = n_plain + (abi.PYRAMID_BLOCKS * len(pyramids) if pyramids is not None else 0)
    inputs = [src, ref, jobs if n_plain else np.zeros(1, abi.BLOCK_JOB_DTYPE)]
    t_src, t_ref, t_jobs = (dev(a) for a in inputs)
    fields = list(abi.STATS_OUT_FIELDS) + (list(abi.PSY_OUT_FIELDS) if psy_rd is not None else []) + (list(abi.FACADE_OUT_FIELDS) if facade else []) + (list(abi.VAR10_OUT_FIELDS) if bit_depth == 10 else [])
    if outputs is not None:
        assert set(outputs) <= {name for name, _ in fields}, outputs
        satd = "satd" in outputs
    wanted = lambda name: (name in outputs) if outputs is not None else (satd or name != "satd")
    n_alloc = n + (spare_jobs if fill is not None else 0)
    outs = {name: torch.full((n_alloc * np.dtype(dt).itemsize,), fill or 0, dtype=torch.uint8, device="cuda") for name, dt in fields}
    d = abi.BlockStatsDesc(bit_depth=bit_depth, n_jobs=n_plain, src_stride=src.shape[1], ref_stride=ref.shape[1])
    if pyramids is not None and len(pyramids):
        inputs.append(pyramids)
        t_pyr = dev(pyramids)
        d.n_pyramids, d.pyramid_out_base, d.pyramids = len(pyramids), n_plain, t_pyr.data_ptr()
    if psy_rd is not None:
        d.psy_rd = psy_rd
    if facade:
        t_mode, t_comp = dev(np.asarray(facade["pred_mode"], np.uint8)), dev(np.asarray(facade["compound_type"], np.uint8))
        d.pred_mode, d.compound_type = t_mode.data_ptr(), t_comp.data_ptr()
        d.temporal_layer_index, d.spy_rd = facade["temporal_layer_index"], facade["spy_rd"]
    d.src, d.ref, d.jobs = t_src.data_ptr(), t_ref.data_ptr(), t_jobs.data_ptr()
    for name, _ in fields:
        if wanted(name):
            setattr(d, name, outs[name].data_ptr())
    torch.cuda.synchronize()
    rc = L.svt_hip_block_stats_batch(ctx._h, C.byref(d))
    ctx.check(rc, "svt_hip_block_stats_batch")
    ctx.sync()
    res = {name: api.to_host(outs[name], dt) for name, dt in fields}
    if fill is not None:
        for name in res:
            assert (res[name][n:].view(np.uint8) == fill).all(), f"{name}: a slot past the batch's {n} was written"
            res[name] = res[name][:n]
        for a, t in zip(inputs, [t_src, t_ref, t_jobs] + ([t_pyr] if len(inputs) == 4 else [])):
            assert np.array_equal(api.to_host(t), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input buffer of the batch was written"
    if outputs is None and not satd:
        res.pop("satd")
    return res


def check_ssim_jobs(jobs, pyramids=False):
    """svt_hip_ssim_check_jobs on a host job array: raises api.SvtHipError when a job's size or sub-pixel phase is not one the SSIM batch takes."""
    from . import api
    L = api.lib()
    jobs = np.ascontiguousarray(jobs, dtype=abi.BLOCK_JOB_DTYPE)
    rc = L.svt_hip_ssim_check_jobs(C.c_void_p(jobs.ctypes.data), C.c_uint32(len(jobs)), C.c_int(1 if pyramids else 0))
    if rc:
        raise api.SvtHipError(f"svt_hip_ssim_check_jobs: {api.ERRORS.get(rc, rc)}: {L.svt_hip_last_error(None).decode()}")


def run_ssim_hip(ctx, src, ref, jobs, bit_depth, psy_rd=None, pyramids=None, spare_jobs=0, fill=None, outputs=None, out_base=None, check=True):
    """svt_hip_ssim_batch on host planes: {"ssim": float64[n], "ssim_dist": uint64[n]} with n = len(jobs) + 85 * len(pyramids), the regions'
    outputs behind the plain jobs' (slots len(jobs) + 85 k ...).  psy_rd None: no psy term.
    src / ref: 2-D arrays (the width is the stride) or (array, stride) views; the two strides may differ.  Both device planes are as long
    as the larger of the two, and every offset a job names must lie inside them: a kernel that takes one stride for the other, or reads
    for a job it should refuse, then reads wrong samples, never unmapped memory.
    fill: a byte both output arrays are pre-filled with (default: zeros); the arrays are then n + spare_jobs slots long, and the spare
    slots and the source, reference, job and region buffers are asserted to read back unchanged.
    outputs: the names of the output pointers to set (default: both); the array of the other is returned as well, as it was filled.
    out_base: pyramid_out_base (default len(jobs)); the arrays then cover the slots in between, n = out_base + 85 * len(pyramids).
    check: False skips svt_hip_ssim_check_jobs, so that the kernel itself meets the jobs the host check refuses."""
    import torch
    from . import api
    L = api.lib()
    if check:
        check_ssim_jobs(jobs)
        if pyramids is not None:
            check_ssim_jobs(pyramids, pyramids=True)
    (src, src_stride), (ref, ref_stride) = (a if isinstance(a, tuple) else (a, a.shape[1]) for a in (src, ref))
    dev = api.to_device
    n_plain, n_pyr = len(jobs), (len(pyramids) if pyramids is not None else 0)
    out_base = n_plain if out_base is None else out_base
    assert out_base >= n_plain
    n = out_base + abi.PYRAMID_BLOCKS * n_pyr if n_pyr else n_plain
    size = max(src.size, ref.size)
    for jb in (jobs, pyramids if n_pyr else jobs[:0]):
        assert (jb["src_offset"] < size).all() and (jb["ref_offset"] < size).all(), "a job names an offset outside the device planes"
    padded = lambda a: np.concatenate([np.ascontiguousarray(a).reshape(-1), np.zeros(size - a.size, a.dtype)])
    inputs = [padded(src), padded(ref), jobs if n_plain else np.zeros(1, abi.BLOCK_JOB_DTYPE)] + ([pyramids] if n_pyr else [])
    t_in = [dev(a) for a in inputs]
    n_alloc = max(n + (spare_jobs if fill is not None else 0), 1)
    outs = {name: torch.full((n_alloc * np.dtype(dt).itemsize,), fill or 0, dtype=torch.uint8, device="cuda") for name, dt in abi.SSIM_OUT_FIELDS}
    d = abi.SsimBatchDesc(bit_depth=bit_depth, n_jobs=n_plain, src_stride=src_stride, ref_stride=ref_stride, psy_rd=psy_rd or 0.0)
    if n_pyr:
        d.n_pyramids, d.pyramid_out_base, d.pyramids = n_pyr, out_base, t_in[3].data_ptr()
    d.src, d.ref, d.jobs = t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr()
    for name, _ in abi.SSIM_OUT_FIELDS:
        if outputs is None or name in outputs:
            setattr(d, name, outs[name].data_ptr())
    torch.cuda.synchronize()
    ctx.check(L.svt_hip_ssim_batch(ctx._h, C.byref(d)), "svt_hip_ssim_batch")
    ctx.sync()
    res = {name: api.to_host(outs[name], dt) for name, dt in abi.SSIM_OUT_FIELDS}
    if fill is not None:
        for name in res:
            assert (res[name][n:].view(np.uint8) == fill).all(), f"{name}: a slot past the batch's {n} was written"
        for a, t in zip(inputs, t_in):
            assert np.array_equal(api.to_host(t), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "an input buffer of the batch was written"
    return {name: res[name][:n] for name in res}
