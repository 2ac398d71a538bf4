"""Host-side helpers of the masked prediction entries (include/svt_hip_mask.h): svt_hip_masked_pred_batch, svt_hip_interintra_blend_batch and
svt_hip_mask_search_batch as runners on device buffers (the links between the prediction planes, the searches' result array and
rd.enqueue_hip's prediction plane) and on host arrays, and the library's wedge tables.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api
from .api import ptr as _ptr, samples as _samples

WEDGE_SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (8, 32), (32, 8)]  # (width, height), the order of the sign-flip table


def check_pred_desc(d):
    """svt_hip_masked_pred_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_masked_pred_check_desc", d)


def check_blend_desc(d):
    api.check_desc("svt_hip_interintra_blend_check_desc", d)


def check_search_desc(d):
    api.check_desc("svt_hip_mask_search_check_desc", d)


def wedge_tables():
    """the library's host copies: the twelve primaries [2][6][64][64] (sign, direction) and the sign-flip table [9][16] (WEDGE_SIZES' order)"""
    L = api.lib()
    L.svt_hip_wedge_primaries.restype = C.POINTER(C.c_uint8 * (12 * 4096))
    L.svt_hip_wedge_signflip.restype = C.POINTER(C.c_uint8 * (9 * 16))
    return (np.array(L.svt_hip_wedge_primaries().contents, np.uint8).reshape(2, 6, 64, 64), np.array(L.svt_hip_wedge_signflip().contents, np.uint8).reshape(9, 16))


def run_masked_pred_device(ctx, bit_depth, ss_x, ss_y, plane, refs, dst, dst_stride, jobs, n_jobs, status, mv_array=None, n_mvs=0, results=None, n_results=0,
                           mask_buf=None, dst_samples=None):
    """Enqueues svt_hip_masked_pred_batch on the context stream, without waiting.  refs: a list of abi.InterPredRef (pred.plane_ref); dst / jobs /
    status / mv_array / results / mask_buf are device tensors: jobs abi.MASKED_PRED_JOB_DTYPE records, results abi.MASK_SEARCH_RESULT_DTYPE records
    such as svt_hip_mask_search_batch's, mask_buf bytes."""
    if len(refs) > abi.INTER_PRED_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.INTER_PRED_MAX_REFS}")
    d = abi.MaskedPredDesc(bit_depth=bit_depth, ss_x=ss_x, ss_y=ss_y, n_refs=len(refs), n_jobs=n_jobs, dst=dst.data_ptr(), dst_stride=dst_stride, plane=plane,
                           dst_samples=_samples(dst, bit_depth) if dst_samples is None else dst_samples, jobs=jobs.data_ptr(), mv_array=_ptr(mv_array),
                           n_mvs=n_mvs, n_results=n_results, results=_ptr(results), mask_buf=_ptr(mask_buf),
                           mask_bytes=mask_buf.numel() * mask_buf.element_size() if mask_buf is not None else 0, status=status.data_ptr())
    for i, r in enumerate(refs):
        d.refs[i] = r
    ctx.check(api.lib().svt_hip_masked_pred_batch(ctx._h, C.byref(d)), "svt_hip_masked_pred_batch")
    return d


def run_interintra_blend_device(ctx, bit_depth, intra, intra_stride, inter, inter_stride, dst, dst_stride, jobs, n_jobs, status, results=None, n_results=0):
    """Enqueues svt_hip_interintra_blend_batch on the context stream, without waiting; dst may be the inter tensor itself."""
    d = abi.InterIntraDesc(bit_depth=bit_depth, n_jobs=n_jobs, intra=intra.data_ptr(), inter=inter.data_ptr(), dst=dst.data_ptr(), intra_stride=intra_stride,
                           inter_stride=inter_stride, dst_stride=dst_stride, n_results=n_results, intra_samples=_samples(intra, bit_depth),
                           inter_samples=_samples(inter, bit_depth), dst_samples=_samples(dst, bit_depth), jobs=jobs.data_ptr(), results=_ptr(results),
                           status=status.data_ptr())
    ctx.check(api.lib().svt_hip_interintra_blend_batch(ctx._h, C.byref(d)), "svt_hip_interintra_blend_batch")
    return d


def run_mask_search_device(ctx, bit_depth, mult, src, src_stride, pred0, pred0_stride, pred1, pred1_stride, intra, intra_stride, jobs, n_jobs, results, status):
    """Enqueues svt_hip_mask_search_batch on the context stream, without waiting; pred0 / intra may be None."""
    d = abi.MaskSearchDesc(bit_depth=bit_depth, pred0_to_pred1_mult=mult, n_jobs=n_jobs, src=src.data_ptr(), pred0=_ptr(pred0), pred1=pred1.data_ptr(),
                           intra=_ptr(intra), src_stride=src_stride, pred0_stride=pred0_stride, pred1_stride=pred1_stride, intra_stride=intra_stride,
                           src_samples=_samples(src, bit_depth), pred0_samples=_samples(pred0, bit_depth) if pred0 is not None else 0,
                           pred1_samples=_samples(pred1, bit_depth), intra_samples=_samples(intra, bit_depth) if intra is not None else 0,
                           jobs=jobs.data_ptr(), results=results.data_ptr(), status=status.data_ptr())
    ctx.check(api.lib().svt_hip_mask_search_batch(ctx._h, C.byref(d)), "svt_hip_mask_search_batch")
    return d


def run_masked_pred_hip(ctx, bit_depth, ss_x, ss_y, plane, planes, jobs, dst_shape, dst_stride=None, mv_array=None, results=None, mask_buf=None, spare_jobs=0,
                        fill=0):
    """svt_hip_masked_pred_batch on host arrays.  planes: a list of (padded plane, org_x, org_y); jobs: abi.MASKED_PRED_JOB_DTYPE; mask_buf: the bytes
    the mask buffer starts with (uint8 array) or None for no buffer.  Returns {"dst", "status", "mask_buf", "planes"} as they are after the call
    (dst and the spare status slots start as the byte `fill`)."""
    import torch
    from . import pred
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    rows, cols = dst_shape
    dst_stride = cols if dst_stride is None else dst_stride
    t_planes = [api.to_device(p, dt) for p, _, _ in planes]
    refs = [pred.plane_ref(t, p.shape[1], ox, oy, p.shape[1], p.shape[0]) for t, (p, ox, oy) in zip(t_planes, planes)]
    t_dst = api.filled(rows * dst_stride * np.dtype(dt).itemsize, fill)
    t_status = api.filled(n + spare_jobs, fill)
    t_jobs = api.records_to_device(jobs, abi.MASKED_PRED_JOB_DTYPE)
    t_mv = api.to_device(mv_array, np.int16) if mv_array is not None and len(mv_array) else None
    t_res = api.to_device(results, abi.MASK_SEARCH_RESULT_DTYPE) if results is not None and len(results) else None
    t_mask = api.to_device(mask_buf, np.uint8) if mask_buf is not None else None
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_masked_pred_device(ctx, bit_depth, ss_x, ss_y, plane, refs, t_dst, dst_stride, t_jobs, n, t_status, mv_array=t_mv,
                           n_mvs=len(mv_array) if t_mv is not None else 0, results=t_res, n_results=len(results) if t_res is not None else 0, mask_buf=t_mask,
                           dst_samples=rows * dst_stride)
    ctx.sync()
    return {"dst": api.to_host(t_dst, dt, (rows, dst_stride)), "status": api.to_host(t_status, count=n + spare_jobs),
            "mask_buf": api.to_host(t_mask) if t_mask is not None else None,
            "planes": [api.to_host(t, dt, p.shape) for t, (p, _, _) in zip(t_planes, planes)]}


def run_interintra_blend_hip(ctx, bit_depth, intra, inter, jobs, dst_shape=None, results=None, spare_jobs=0, fill=0):
    """svt_hip_interintra_blend_batch on host arrays.  intra / inter: planes [rows][stride]; dst_shape None: the destination is the inter plane
    itself (in place), else a plane of that shape filled with `fill`.  Returns {"dst", "status", "intra", "inter"} after the call."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    t_intra, t_inter = api.to_device(intra, dt), api.to_device(inter, dt)
    in_place = dst_shape is None
    dst_shape = inter.shape if in_place else dst_shape
    t_dst = t_inter if in_place else api.filled(dst_shape[0] * dst_shape[1] * np.dtype(dt).itemsize, fill)
    t_status = api.filled(n + spare_jobs, fill)
    t_jobs = api.records_to_device(jobs, abi.INTERINTRA_JOB_DTYPE)
    t_res = api.to_device(results, abi.MASK_SEARCH_RESULT_DTYPE) if results is not None and len(results) else None
    torch.cuda.current_stream().synchronize()
    run_interintra_blend_device(ctx, bit_depth, t_intra, intra.shape[1], t_inter, inter.shape[1], t_dst, dst_shape[1], t_jobs, n, t_status, results=t_res,
                                n_results=len(results) if t_res is not None else 0)
    ctx.sync()
    return {"dst": api.to_host(t_dst, dt, dst_shape), "status": api.to_host(t_status, count=n + spare_jobs),
            "intra": api.to_host(t_intra, dt, intra.shape), "inter": api.to_host(t_inter, dt, inter.shape)}


def run_mask_search_hip(ctx, bit_depth, mult, src, pred0, pred1, intra, jobs, spare_jobs=0, fill=0):
    """svt_hip_mask_search_batch on host arrays.  src / pred0 / pred1 / intra: planes [rows][stride] (pred0 / intra may be None).  Returns
    {"results": abi.MASK_SEARCH_RESULT_DTYPE [n + spare_jobs] (they start as the byte `fill`), "status"} after the call."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    up = lambda a: api.to_device(a, dt) if a is not None else None
    t_src, t_p0, t_p1, t_in = up(src), up(pred0), up(pred1), up(intra)
    t_jobs = api.records_to_device(jobs, abi.MASK_SEARCH_JOB_DTYPE)
    rec = np.dtype(abi.MASK_SEARCH_RESULT_DTYPE).itemsize
    t_res, t_status = api.filled((n + spare_jobs) * rec, fill), api.filled(n + spare_jobs, fill)
    torch.cuda.current_stream().synchronize()
    run_mask_search_device(ctx, bit_depth, mult, t_src, src.shape[1], t_p0, pred0.shape[1] if pred0 is not None else 0, t_p1, pred1.shape[1], t_in,
                           intra.shape[1] if intra is not None else 0, t_jobs, n, t_res, t_status)
    ctx.sync()
    return {"results": api.to_host(t_res, abi.MASK_SEARCH_RESULT_DTYPE, count=n + spare_jobs), "status": api.to_host(t_status, count=n + spare_jobs)}
