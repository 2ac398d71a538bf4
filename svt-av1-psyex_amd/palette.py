"""Host-side helpers of the luma palette search (svt_hip_palette_search_batch) and of the palette prediction that follows it
(svt_hip_palette_pred_batch): runners on device buffers and on host arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api
from .api import samples as _samples

PARAMS = ("cost_bit_depth", "dominant_color_step", "reduce_palette_cost_precision")


def check_desc(d):
    """svt_hip_palette_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_palette_check_desc", d)


def check_pred_desc(d):
    """svt_hip_palette_pred_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_palette_pred_check_desc", d)


def run_search_device(ctx, bit_depth, src, src_stride, jobs, n_jobs, tables, results, status, params, color_maps=None, src_samples=None, map_bytes=None):
    """Enqueues svt_hip_palette_search_batch on the context stream, without waiting.  Every array is a device tensor: src the source luma plane, jobs
    abi.PALETTE_JOB_DTYPE records, tables the three int32 rate tables (palette_ycolor_fac_bitss [7][5][8], palette_ysize_fac_bits [7][8],
    palette_ymode_fac_bits [7][3][3]), results abi.PALETTE_RESULT_DTYPE records, status one byte per job, color_maps bytes or None.  params: a dict
    of PARAMS."""
    ycolor, ysize, ymode = tables
    d = abi.PaletteDesc(bit_depth=bit_depth, n_jobs=n_jobs, src=src.data_ptr(), src_stride=src_stride,
                        src_samples=_samples(src, bit_depth) if src_samples is None else src_samples, palette_ycolor_fac_bitss=ycolor.data_ptr(),
                        palette_ysize_fac_bits=ysize.data_ptr(), palette_ymode_fac_bits=ymode.data_ptr(), jobs=jobs.data_ptr(), results=results.data_ptr(),
                        status=status.data_ptr(), color_maps=color_maps.data_ptr() if color_maps is not None else None,
                        map_bytes=(color_maps.numel() if color_maps is not None else 0) if map_bytes is None else map_bytes)
    for k in PARAMS:
        setattr(d, k, params[k])
    ctx.check(api.lib().svt_hip_palette_search_batch(ctx._h, C.byref(d)), "svt_hip_palette_search_batch")
    return d


def run_pred_device(ctx, bit_depth, src, src_stride, dst, dst_stride, search_jobs, search_results, search_status, n_search_jobs, jobs, n_jobs, status,
                    color_map=None, src_samples=None, dst_samples=None, map_bytes=None):
    """Enqueues svt_hip_palette_pred_batch on the context stream, without waiting; all arrays are device tensors, the three search arrays the ones
    svt_hip_palette_search_batch read and wrote (no host look in between), jobs abi.PALETTE_PRED_JOB_DTYPE records."""
    d = abi.PalettePredDesc(bit_depth=bit_depth, n_jobs=n_jobs, n_search_jobs=n_search_jobs, src_stride=src_stride, src=src.data_ptr(),
                            src_samples=_samples(src, bit_depth) if src_samples is None else src_samples, dst=dst.data_ptr(), dst_stride=dst_stride,
                            dst_samples=_samples(dst, bit_depth) if dst_samples is None else dst_samples, search_jobs=search_jobs.data_ptr(),
                            search_results=search_results.data_ptr(), search_status=search_status.data_ptr(), jobs=jobs.data_ptr(), status=status.data_ptr(),
                            color_map=color_map.data_ptr() if color_map is not None else None,
                            map_bytes=(color_map.numel() if color_map is not None else 0) if map_bytes is None else map_bytes)
    ctx.check(api.lib().svt_hip_palette_pred_batch(ctx._h, C.byref(d)), "svt_hip_palette_pred_batch")
    return d


def run_palette_hip(ctx, bit_depth, src, jobs, tables, params, map_bytes=0, pred_jobs=None, dst_samples=0, dst_stride=0, pred_map_bytes=0, spare_jobs=0, fill=0):
    """The search, and with pred_jobs the predictions right behind it on the stream, on host arrays.  src: the source plane [H][W]; jobs:
    abi.PALETTE_JOB_DTYPE; tables: (ycolor, ysize, ymode) int32 arrays; map_bytes: size of color_maps, 0 for none; pred_jobs:
    abi.PALETTE_PRED_JOB_DTYPE or None; pred_map_bytes: size of the predictions' color_map, 0 for none.  Every output starts as the byte `fill`.
    Returns {"results", "status", "color_maps", "dst", "pred_status", "pred_map"} as they are after the calls (None for what was not asked for)."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    slots = max(1, n + spare_jobs)
    full = lambda nbytes: api.filled(nbytes, fill)
    t_src = api.to_device(src, dt)
    t_jobs = api.records_to_device(jobs, abi.PALETTE_JOB_DTYPE)
    t_tab = [api.to_device(t, np.int32) for t in tables]
    t_res, t_status = full(slots * np.dtype(abi.PALETTE_RESULT_DTYPE).itemsize), full(slots)
    t_maps = full(map_bytes) if map_bytes else None
    out = {"color_maps": None, "dst": None, "pred_status": None, "pred_map": None}
    if pred_jobs is not None:
        m = len(pred_jobs)
        t_pjobs = api.records_to_device(pred_jobs, abi.PALETTE_PRED_JOB_DTYPE)
        t_dst, t_pst = full(dst_samples * np.dtype(dt).itemsize), full(m)
        t_pmap = full(pred_map_bytes) if pred_map_bytes else None
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_search_device(ctx, bit_depth, t_src, src.shape[1], t_jobs, n, t_tab, t_res, t_status, params, color_maps=t_maps, map_bytes=map_bytes if map_bytes else None)
    if pred_jobs is not None:
        run_pred_device(ctx, bit_depth, t_src, src.shape[1], t_dst, dst_stride, t_jobs, t_res, t_status, max(1, n), t_pjobs, m, t_pst, color_map=t_pmap,
                        dst_samples=dst_samples, map_bytes=pred_map_bytes if pred_map_bytes else None)
    ctx.sync()
    out["results"], out["status"] = api.to_host(t_res, abi.PALETTE_RESULT_DTYPE), api.to_host(t_status)
    if t_maps is not None:
        out["color_maps"] = api.to_host(t_maps)
    if pred_jobs is not None:
        out["dst"], out["pred_status"] = api.to_host(t_dst, dt, count=dst_samples), api.to_host(t_pst, count=m)
        out["pred_map"] = api.to_host(t_pmap) if t_pmap is not None else None
    return out
