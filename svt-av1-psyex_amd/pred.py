"""Host-side helpers of the inter prediction entry (svt_hip_inter_pred_batch): a runner on device buffers (the link between the motion searches'
best_mv and rd.enqueue_hip's prediction plane) and one on host arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api


def plane_ref(tensor, stride, org_x, org_y, width, height):
    """abi.InterPredRef of a padded plane held by a device tensor: `width` x `height` are the padded plane's, (org_x, org_y) the picture's first sample in it"""
    return abi.InterPredRef(plane=tensor.data_ptr(), stride=stride, org_x=org_x, org_y=org_y, width=width, height=height)


def check_desc(d):
    """svt_hip_inter_pred_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_inter_pred_check_desc", d)


def run_inter_pred_device(ctx, bit_depth, ss_x, ss_y, refs, dst, dst_stride, jobs, n_jobs, status, mv_array=None, n_mvs=0, dst_samples=None):
    """Enqueues svt_hip_inter_pred_batch on the context stream, without waiting.  refs: a list of abi.InterPredRef (plane_ref); dst / jobs / status
    / mv_array are device tensors: dst the prediction plane (uint8, or uint16 at 10 bits, as bytes or samples), jobs abi.INTER_PRED_JOB_DTYPE records,
    status one byte per job, mv_array int16 (row, col) pairs such as svt_hip_md_subpel_batch's best_mv.  dst_samples: the samples dst holds (default:
    all of the tensor)."""
    sample_bytes = 2 if bit_depth > 8 else 1
    if dst_samples is None:
        dst_samples = dst.numel() * dst.element_size() // sample_bytes
    d = abi.InterPredDesc(bit_depth=bit_depth, ss_x=ss_x, ss_y=ss_y, n_refs=len(refs), n_jobs=n_jobs, dst=dst.data_ptr(), dst_stride=dst_stride,
                          dst_samples=dst_samples, jobs=jobs.data_ptr(), mv_array=mv_array.data_ptr() if mv_array is not None else None, n_mvs=n_mvs,
                          status=status.data_ptr())
    if len(refs) > abi.INTER_PRED_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.INTER_PRED_MAX_REFS}")
    for i, r in enumerate(refs):
        d.refs[i] = r
    ctx.check(api.lib().svt_hip_inter_pred_batch(ctx._h, C.byref(d)), "svt_hip_inter_pred_batch")
    return d


def run_inter_pred_hip(ctx, bit_depth, ss_x, ss_y, planes, jobs, dst_shape, dst_stride=None, mv_array=None, spare_jobs=0, fill=0):
    """svt_hip_inter_pred_batch on host arrays.  planes: a list of (padded plane [H][W] uint8 / uint16, org_x, org_y); jobs:
    abi.INTER_PRED_JOB_DTYPE; dst_shape: (rows, columns) of the destination plane, dst_stride its pitch in samples (default: columns); mv_array:
    int16 [n][2] or None.  Returns {"dst": [rows][dst_stride] as it is after the call (it starts as the byte `fill`), "status": [n + spare_jobs]
    (the spare slots start as `fill`), "planes": the reference planes read back}."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    rows, cols = dst_shape
    dst_stride = cols if dst_stride is None else dst_stride
    t_planes = [api.to_device(p, dt) for p, _, _ in planes]
    refs = [plane_ref(t, p.shape[1], ox, oy, p.shape[1], p.shape[0]) for t, (p, ox, oy) in zip(t_planes, planes)]
    t_dst = torch.full((rows * dst_stride * np.dtype(dt).itemsize,), fill, dtype=torch.uint8, device="cuda")
    t_status = api.filled(n + spare_jobs, fill)
    t_jobs = api.records_to_device(jobs, abi.INTER_PRED_JOB_DTYPE)
    t_mv = api.to_device(mv_array, np.int16) if mv_array is not None and len(mv_array) else None
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_inter_pred_device(ctx, bit_depth, ss_x, ss_y, refs, t_dst, dst_stride, t_jobs, n, t_status, mv_array=t_mv,
                          n_mvs=len(mv_array) if t_mv is not None else 0, dst_samples=rows * dst_stride)
    ctx.sync()
    return {"dst": api.to_host(t_dst, dt, (rows, dst_stride)), "status": api.to_host(t_status, count=n + spare_jobs),
            "planes": [api.to_host(t, dt, p.shape) for t, (p, _, _) in zip(t_planes, planes)]}
