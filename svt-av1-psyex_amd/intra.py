"""Host-side helpers of the intra prediction entry (svt_hip_intra_pred_batch): a runner on device buffers (it writes the prediction plane
rd.enqueue_hip reads) and one on host arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api


def check_desc(d):
    """svt_hip_intra_pred_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_intra_pred_check_desc", d)


def run_intra_pred_device(ctx, bit_depth, disable_edge_filter, nbr, nbr_stride, nbr_width, nbr_height, dst, dst_stride, jobs, n_jobs, status, dst_samples=None):
    """Enqueues svt_hip_intra_pred_batch on the context stream, without waiting.  nbr / dst / jobs / status are device tensors: nbr the neighbour
    plane and dst the prediction plane (uint8, or uint16 at 10 bits, as bytes or samples), jobs abi.INTRA_PRED_JOB_DTYPE records, status one byte
    per job.  dst_samples: the samples dst holds (default: all of the tensor)."""
    sample_bytes = 2 if bit_depth > 8 else 1
    if dst_samples is None:
        dst_samples = dst.numel() * dst.element_size() // sample_bytes
    d = abi.IntraPredDesc(bit_depth=bit_depth, disable_edge_filter=int(bool(disable_edge_filter)), n_jobs=n_jobs, nbr=nbr.data_ptr(), nbr_stride=nbr_stride,
                          nbr_width=nbr_width, nbr_height=nbr_height, dst=dst.data_ptr(), dst_stride=dst_stride, dst_samples=dst_samples,
                          jobs=jobs.data_ptr(), status=status.data_ptr())
    ctx.check(api.lib().svt_hip_intra_pred_batch(ctx._h, C.byref(d)), "svt_hip_intra_pred_batch")
    return d


def run_intra_pred_hip(ctx, bit_depth, disable_edge_filter, nbr, jobs, dst_shape, dst_stride=None, spare_jobs=0, fill=0, nbr_size=None):
    """svt_hip_intra_pred_batch on host arrays.  nbr: the neighbour plane [H][stride] uint8 / uint16; nbr_size: (width, height) the kernel may read
    (default: the whole array); jobs: abi.INTRA_PRED_JOB_DTYPE; dst_shape: (rows, columns) of the destination plane, dst_stride its pitch in
    samples (default: columns).  Returns {"dst": [rows][dst_stride] as it is after the call (it starts as the byte `fill`), "status":
    [n + spare_jobs] (the spare slots start as `fill`), "nbr": the neighbour plane read back}."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    rows, cols = dst_shape
    dst_stride = cols if dst_stride is None else dst_stride
    nbr = np.ascontiguousarray(nbr, dtype=dt)
    width, height = (nbr.shape[1], nbr.shape[0]) if nbr_size is None else nbr_size
    t_nbr = api.to_device(nbr)
    t_dst = torch.full((rows * dst_stride * np.dtype(dt).itemsize,), fill, dtype=torch.uint8, device="cuda")
    t_status = api.filled(n + spare_jobs, fill)
    t_jobs = api.records_to_device(jobs, abi.INTRA_PRED_JOB_DTYPE)
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_intra_pred_device(ctx, bit_depth, disable_edge_filter, t_nbr, nbr.shape[1], width, height, t_dst, dst_stride, t_jobs, n, t_status,
                          dst_samples=rows * dst_stride)
    ctx.sync()
    return {"dst": api.to_host(t_dst, dt, (rows, dst_stride)), "status": api.to_host(t_status, count=n + spare_jobs),
            "nbr": api.to_host(t_nbr, dt, nbr.shape)}
