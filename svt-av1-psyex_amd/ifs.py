"""Host-side helpers of the interpolation-filter search (svt_hip_ifs_batch) and of the step that hands its filters on
(svt_hip_ifs_scatter_filters): runners on device buffers and on host arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api
from .pred import plane_ref

PARAMS = ("enable_dual_filter", "subsampled_distortion", "skip_sse_rd_model", "spy_rd", "quantizer", "lambda_", "smooth_bias_pct", "psy_rd")


def check_desc(d):
    """svt_hip_ifs_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_ifs_check_desc", d)


def model_tables():
    """the three tables of model_rd_norm as the library holds them: int32 [3][104] = rate_tab_q10, dist_tab_q10, xsq_iq_q10"""
    L = api.lib()
    L.svt_hip_ifs_model_table.restype = C.POINTER(C.c_int32)
    return np.array([np.ctypeslib.as_array(L.svt_hip_ifs_model_table(k), (abi.IFS_MODEL_ENTRIES,)) for k in range(3)], np.int32)


def run_ifs_device(ctx, bit_depth, refs, src, src_stride, jobs, n_jobs, fac_bits, results, status, params, dst=None, dst_stride=0, mv_array=None, n_mvs=0,
                   rd=None, sse=None, src_samples=None, dst_samples=None):
    """Enqueues svt_hip_ifs_batch on the context stream, without waiting.  refs: a list of abi.InterPredRef (pred.plane_ref); every other array is a
    device tensor: src the source luma plane, jobs abi.IFS_JOB_DTYPE records, fac_bits int32 [16][3], results abi.IFS_RESULT_DTYPE records, status one
    byte per job, dst the prediction plane or None (search only), rd / sse uint64 [n_jobs][9] or None.  params: a dict of PARAMS."""
    sample_bytes = 2 if bit_depth > 8 else 1
    ptr = lambda t: t.data_ptr() if t is not None else None
    samples = lambda t: t.numel() * t.element_size() // sample_bytes
    d = abi.IfsDesc(bit_depth=bit_depth, n_refs=len(refs), n_jobs=n_jobs, n_mvs=n_mvs, src=src.data_ptr(), src_stride=src_stride, dst_stride=dst_stride,
                    src_samples=samples(src) if src_samples is None else src_samples, dst=ptr(dst),
                    dst_samples=(samples(dst) if dst is not None else 0) if dst_samples is None else dst_samples, jobs=jobs.data_ptr(), mv_array=ptr(mv_array),
                    switchable_interp_fac_bits=fac_bits.data_ptr(), results=results.data_ptr(), rd=ptr(rd), sse=ptr(sse), status=status.data_ptr())
    for k in PARAMS:
        setattr(d, k, params.get(k, 0))
    if len(refs) > abi.INTER_PRED_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.INTER_PRED_MAX_REFS}")
    for i, r in enumerate(refs):
        d.refs[i] = r
    ctx.check(api.lib().svt_hip_ifs_batch(ctx._h, C.byref(d)), "svt_hip_ifs_batch")
    return d


def run_scatter_device(ctx, patches, n_patches, results, result_status, n_results, records, n_records, record_stride, filter_x_offset, status):
    """Enqueues svt_hip_ifs_scatter_filters on the context stream, without waiting; all arrays are device tensors."""
    d = abi.IfsScatterDesc(n_patches=n_patches, n_results=n_results, n_records=n_records, record_stride=record_stride, filter_x_offset=filter_x_offset,
                           patches=patches.data_ptr(), results=results.data_ptr(), result_status=result_status.data_ptr(), base=records.data_ptr(),
                           status=status.data_ptr())
    ctx.check(api.lib().svt_hip_ifs_scatter_filters(ctx._h, C.byref(d)), "svt_hip_ifs_scatter_filters")
    return d


def run_ifs_hip(ctx, bit_depth, planes, src, jobs, fac_bits, params, dst_shape=None, dst_stride=None, mv_array=None, spare_jobs=0, fill=0, want_arrays=True):
    """svt_hip_ifs_batch on host arrays.  planes: a list of (padded plane [H][W], org_x, org_y); src: the source plane [H][W]; jobs: abi.IFS_JOB_DTYPE;
    fac_bits: int32 [16][3]; dst_shape: (rows, columns) of the destination plane or None for dst == NULL.  Every output starts as the byte `fill`.
    Returns {"results", "status", "rd", "sse", "dst"} as they are after the call (dst None without a destination)."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    t_planes = [api.to_device(p, dt) for p, _, _ in planes]
    refs = [plane_ref(t, p.shape[1], ox, oy, p.shape[1], p.shape[0]) for t, (p, ox, oy) in zip(t_planes, planes)]
    t_src = api.to_device(src, dt)
    t_dst = None
    if dst_shape is not None:
        rows, cols = dst_shape
        dst_stride = cols if dst_stride is None else dst_stride
        t_dst = torch.full((rows * dst_stride * np.dtype(dt).itemsize,), fill, dtype=torch.uint8, device="cuda")
    slots = max(1, n + spare_jobs)
    full = lambda nbytes: torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
    t_status, t_res = full(slots), full(slots * np.dtype(abi.IFS_RESULT_DTYPE).itemsize)
    t_rd, t_sse = (full(slots * 72), full(slots * 72)) if want_arrays else (None, None)
    t_jobs = api.records_to_device(jobs, abi.IFS_JOB_DTYPE)
    t_fac = api.to_device(fac_bits, np.int32)
    t_mv = api.to_device(mv_array, np.int16) if mv_array is not None and len(mv_array) else None
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_ifs_device(ctx, bit_depth, refs, t_src, src.shape[1], t_jobs, n, t_fac, t_res, t_status, params, dst=t_dst, dst_stride=dst_stride or 0, mv_array=t_mv,
                   n_mvs=len(mv_array) if t_mv is not None else 0, rd=t_rd, sse=t_sse)
    ctx.sync()
    out = {"results": api.to_host(t_res, abi.IFS_RESULT_DTYPE), "status": api.to_host(t_status),
           "dst": api.to_host(t_dst, dt, (rows, dst_stride)) if t_dst is not None else None}
    out["rd"], out["sse"] = (api.to_host(t, np.uint64, (slots, 9)) if t is not None else None for t in (t_rd, t_sse))
    return out


def run_scatter_hip(ctx, patches, results, result_status, records, filter_x_offset, fill=0):
    """svt_hip_ifs_scatter_filters on host arrays.  records: a structured array (its itemsize is the record stride).  Returns (records after the
    call, status [n_patches])."""
    import torch
    n = len(patches)
    t_pat = api.records_to_device(patches, abi.IFS_PATCH_DTYPE)
    t_res, t_rs, t_rec = api.to_device(results, abi.IFS_RESULT_DTYPE), api.to_device(result_status, np.uint8), api.to_device(records)
    t_status = api.filled(n, fill)
    torch.cuda.current_stream().synchronize()
    run_scatter_device(ctx, t_pat, n, t_res, t_rs, len(results), t_rec, len(records), records.dtype.itemsize, filter_x_offset, t_status)
    ctx.sync()
    return api.to_host(t_rec, records.dtype), api.to_host(t_status, count=n)
