"""Host-side helpers of the four OBMC entries (include/svt_hip_obmc.h): svt_hip_obmc_neighbour_batch, svt_hip_obmc_blend_batch,
svt_hip_obmc_target_batch and svt_hip_obmc_search_batch as runners on device buffers (the links between svt_hip_inter_pred_batch's prediction plane,
the strip buffers, wsrc / mask, the search's best_mv and rd.enqueue_hip's prediction plane) and on host arrays, and the library's mask rows.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api
from .api import ptr as _ptr, samples as _samples


def check_neighbour_desc(d):
    """svt_hip_obmc_neighbour_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_obmc_neighbour_check_desc", d)


def check_blend_desc(d):
    api.check_desc("svt_hip_obmc_blend_check_desc", d)


def check_target_desc(d):
    api.check_desc("svt_hip_obmc_target_check_desc", d)


def masks():
    """the library's host copy of the 1-D mask rows: 64 bytes, the row of length n at [n, 2n)"""
    L = api.lib()
    L.svt_hip_obmc_masks.restype = C.POINTER(C.c_uint8 * 64)
    return np.array(L.svt_hip_obmc_masks().contents, np.uint8)


def run_neighbour_device(ctx, bit_depth, ss_x, ss_y, plane, refs, blocks, n_blocks, jobs, n_jobs, above, left, status, mv_array=None, n_mvs=0, strip_samples=None):
    """Enqueues svt_hip_obmc_neighbour_batch on the context stream, without waiting.  refs: a list of abi.InterPredRef (pred.plane_ref) of this
    plane; blocks / jobs / above / left / status / mv_array are device tensors: blocks abi.OBMC_BLOCK_DTYPE records, jobs abi.OBMC_JOB_DTYPE
    records, above / left the two strip buffers, mv_array int16 (row, col) pairs such as svt_hip_md_subpel_batch's best_mv."""
    if len(refs) > abi.INTER_PRED_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.INTER_PRED_MAX_REFS}")
    d = abi.ObmcNeighbourDesc(bit_depth=bit_depth, ss_x=ss_x, ss_y=ss_y, plane=plane, n_refs=len(refs), n_jobs=n_jobs, n_blocks=n_blocks, blocks=blocks.data_ptr(),
                              jobs=jobs.data_ptr(), above=above.data_ptr(), left=left.data_ptr(),
                              strip_samples=min(_samples(above, bit_depth), _samples(left, bit_depth)) if strip_samples is None else strip_samples,
                              mv_array=_ptr(mv_array), n_mvs=n_mvs, status=status.data_ptr())
    for i, r in enumerate(refs):
        d.refs[i] = r
    ctx.check(api.lib().svt_hip_obmc_neighbour_batch(ctx._h, C.byref(d)), "svt_hip_obmc_neighbour_batch")
    return d


def run_blend_device(ctx, bit_depth, ss_x, ss_y, plane, blocks, n_blocks, jobs, n_jobs, above, left, dst, dst_stride, status, strip_samples=None, dst_samples=None):
    """Enqueues svt_hip_obmc_blend_batch on the context stream, without waiting; dst is the prediction plane svt_hip_inter_pred_batch wrote."""
    d = abi.ObmcBlendDesc(bit_depth=bit_depth, ss_x=ss_x, ss_y=ss_y, plane=plane, n_jobs=n_jobs, n_blocks=n_blocks, dst_stride=dst_stride, blocks=blocks.data_ptr(),
                          jobs=jobs.data_ptr(), above=above.data_ptr(), left=left.data_ptr(),
                          strip_samples=min(_samples(above, bit_depth), _samples(left, bit_depth)) if strip_samples is None else strip_samples,
                          dst=dst.data_ptr(), dst_samples=_samples(dst, bit_depth) if dst_samples is None else dst_samples, status=status.data_ptr())
    ctx.check(api.lib().svt_hip_obmc_blend_batch(ctx._h, C.byref(d)), "svt_hip_obmc_blend_batch")
    return d


def run_target_device(ctx, strip_bit_depth, blocks, n_blocks, jobs, n_jobs, above, left, src, src_stride, wsrc, mask, status, strip_samples=None, src_samples=None,
                      out_values=None):
    """Enqueues svt_hip_obmc_target_batch on the context stream, without waiting; src is the 8-bit source luma plane from its sample (0, 0), wsrc and
    mask int32 buffers."""
    d = abi.ObmcTargetDesc(strip_bit_depth=strip_bit_depth, n_jobs=n_jobs, n_blocks=n_blocks, src_stride=src_stride, blocks=blocks.data_ptr(), jobs=jobs.data_ptr(),
                           above=above.data_ptr(), left=left.data_ptr(),
                           strip_samples=min(_samples(above, strip_bit_depth), _samples(left, strip_bit_depth)) if strip_samples is None else strip_samples,
                           src=src.data_ptr(), src_samples=src.numel() * src.element_size() if src_samples is None else src_samples, wsrc=wsrc.data_ptr(),
                           mask=mask.data_ptr(),
                           out_values=min(wsrc.numel() * wsrc.element_size(), mask.numel() * mask.element_size()) // 4 if out_values is None else out_values,
                           status=status.data_ptr())
    ctx.check(api.lib().svt_hip_obmc_target_batch(ctx._h, C.byref(d)), "svt_hip_obmc_target_batch")
    return d


def run_neighbour_hip(ctx, bit_depth, ss_x, ss_y, plane, planes, blocks, jobs, above, left, mv_array=None, spare_jobs=0, fill=0):
    """svt_hip_obmc_neighbour_batch on host arrays.  planes: a list of (padded plane, org_x, org_y) of this plane; blocks: abi.OBMC_BLOCK_DTYPE;
    jobs: abi.OBMC_JOB_DTYPE; above / left: the strip buffers as they are before the call (1-D, uint8 or uint16).  Returns {"above", "left",
    "status" [n + spare_jobs] (the spare slots start as the byte `fill`), "planes": the reference planes read back}."""
    import torch
    from . import pred
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    t_planes = [api.to_device(p, dt) for p, _, _ in planes]
    refs = [pred.plane_ref(t, p.shape[1], ox, oy, p.shape[1], p.shape[0]) for t, (p, ox, oy) in zip(t_planes, planes)]
    t_above, t_left = api.to_device(above, dt), api.to_device(left, dt)
    t_status = api.filled(n + spare_jobs, fill)
    t_blocks, t_jobs = api.records_to_device(blocks, abi.OBMC_BLOCK_DTYPE), api.records_to_device(jobs, abi.OBMC_JOB_DTYPE)
    t_mv = api.to_device(mv_array, np.int16) if mv_array is not None and len(mv_array) else None
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_neighbour_device(ctx, bit_depth, ss_x, ss_y, plane, refs, t_blocks, max(1, len(blocks)), t_jobs, n, t_above, t_left, t_status, mv_array=t_mv,
                         n_mvs=len(mv_array) if t_mv is not None else 0, strip_samples=len(above))
    ctx.sync()
    return {"above": api.to_host(t_above, dt), "left": api.to_host(t_left, dt), "status": api.to_host(t_status, count=n + spare_jobs),
            "planes": [api.to_host(t, dt, p.shape) for t, (p, _, _) in zip(t_planes, planes)]}


def run_blend_hip(ctx, bit_depth, ss_x, ss_y, plane, blocks, jobs, above, left, dst, spare_jobs=0, fill=0):
    """svt_hip_obmc_blend_batch on host arrays.  dst: the prediction plane [rows][stride] as it is before the call.  Returns {"dst", "status", "above",
    "left"} after the call."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    t_above, t_left, t_dst = (api.to_device(a, dt) for a in (above, left, dst))
    t_status = api.filled(n + spare_jobs, fill)
    t_blocks, t_jobs = api.records_to_device(blocks, abi.OBMC_BLOCK_DTYPE), api.records_to_device(jobs, abi.OBMC_JOB_DTYPE)
    torch.cuda.current_stream().synchronize()
    run_blend_device(ctx, bit_depth, ss_x, ss_y, plane, t_blocks, max(1, len(blocks)), t_jobs, n, t_above, t_left, t_dst, dst.shape[1], t_status,
                     strip_samples=len(above), dst_samples=dst.size)
    ctx.sync()
    return {"dst": api.to_host(t_dst, dt, dst.shape), "status": api.to_host(t_status, count=n + spare_jobs), "above": api.to_host(t_above, dt),
            "left": api.to_host(t_left, dt)}


def run_target_hip(ctx, strip_bit_depth, blocks, jobs, above, left, src, out_values, spare_jobs=0, fill=0):
    """svt_hip_obmc_target_batch on host arrays.  src: the 8-bit source luma plane [rows][stride] from its sample (0, 0); wsrc and mask hold
    out_values int32 each and start as the byte `fill`.  Returns {"wsrc", "mask", "status"} after the call."""
    import torch
    dt = api.sample_dtype(strip_bit_depth)
    n = len(jobs)
    t_above, t_left = api.to_device(above, dt), api.to_device(left, dt)
    t_src = api.to_device(src, np.uint8)
    t_wsrc, t_mask = (api.filled(max(1, out_values) * 4, fill) for _ in range(2))
    t_status = api.filled(n + spare_jobs, fill)
    t_blocks, t_jobs = api.records_to_device(blocks, abi.OBMC_BLOCK_DTYPE), api.records_to_device(jobs, abi.OBMC_JOB_DTYPE)
    torch.cuda.current_stream().synchronize()
    run_target_device(ctx, strip_bit_depth, t_blocks, max(1, len(blocks)), t_jobs, n, t_above, t_left, t_src, src.shape[1], t_wsrc, t_mask, t_status,
                      strip_samples=len(above), src_samples=src.size, out_values=out_values)
    ctx.sync()
    return {"wsrc": api.to_host(t_wsrc, np.int32, count=out_values), "mask": api.to_host(t_mask, np.int32, count=out_values),
            "status": api.to_host(t_status, count=n + spare_jobs)}


def check_search_desc(d):
    api.check_desc("svt_hip_obmc_search_check_desc", d)


MV_CENTRE = 1 << 14  # the cost tables hold the entries [-16384, 16384]; the descriptor points at the centre


def run_search_device(ctx, params, ref, ref_stride, wsrc, mask, jobs, n_jobs, best_mv, results, status, tables=None, ref_samples=None, target_values=None):
    """Enqueues svt_hip_obmc_search_batch on the context stream, without waiting.  params: refine_level, fpel_search_diag, fpel_search_range,
    approx_inter_rate, allow_hp, sadpb, error_per_bit; ref: the 8-bit reference plane's buffer; wsrc / mask: what svt_hip_obmc_target_batch wrote;
    tables: device tensors (mvjcost int32[4], row and column tables int32[32769]) or None with approx_inter_rate; best_mv: int16 (row, col) pairs."""
    d = abi.ObmcSearchDesc(ref_bit_depth=8, n_jobs=n_jobs, ref_stride=ref_stride, ref=ref.data_ptr(),
                           ref_samples=ref.numel() * ref.element_size() if ref_samples is None else ref_samples, wsrc=wsrc.data_ptr(), mask=mask.data_ptr(),
                           target_values=min(wsrc.numel() * wsrc.element_size(), mask.numel() * mask.element_size()) // 4 if target_values is None else target_values,
                           jobs=jobs.data_ptr(), best_mv=best_mv.data_ptr(), results=results.data_ptr(), status=status.data_ptr(), **params)
    if tables is not None:
        d.mvjcost = tables[0].data_ptr()
        d.mvcost[0], d.mvcost[1] = tables[1].data_ptr() + 4 * MV_CENTRE, tables[2].data_ptr() + 4 * MV_CENTRE
    ctx.check(api.lib().svt_hip_obmc_search_batch(ctx._h, C.byref(d)), "svt_hip_obmc_search_batch")
    return d


def run_search_hip(ctx, params, ref, wsrc, mask, jobs, tables=None, spare_jobs=0, fill=0):
    """svt_hip_obmc_search_batch on host arrays.  ref: the 8-bit reference plane [rows][stride]; wsrc / mask: int32 arrays; tables: (mvjcost, row table,
    column table) int32 arrays or None.  Returns {"best_mv" [n + spare_jobs][2], "results" abi.OBMC_SEARCH_RESULT_DTYPE, "status"}; all start as `fill`."""
    import torch
    n = len(jobs)
    t_ref, t_wsrc, t_mask = api.to_device(ref, np.uint8), api.to_device(wsrc, np.int32), api.to_device(mask, np.int32)
    t_jobs = api.records_to_device(jobs, abi.OBMC_SEARCH_JOB_DTYPE)
    t_tab = [api.to_device(t, np.int32) for t in tables] if tables is not None else None
    rec = np.dtype(abi.OBMC_SEARCH_RESULT_DTYPE).itemsize
    t_mv, t_res, t_st = (api.filled((n + spare_jobs) * k, fill) for k in (4, rec, 1))
    torch.cuda.current_stream().synchronize()
    run_search_device(ctx, params, t_ref, ref.shape[1], t_wsrc, t_mask, t_jobs, n, t_mv, t_res, t_st, tables=t_tab, ref_samples=ref.size, target_values=len(wsrc))
    ctx.sync()
    return {"best_mv": api.to_host(t_mv, np.int16, (-1, 2), count=(n + spare_jobs) * 2), "results": api.to_host(t_res, abi.OBMC_SEARCH_RESULT_DTYPE, count=n + spare_jobs),
            "status": api.to_host(t_st, count=n + spare_jobs)}
