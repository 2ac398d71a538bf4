"""Host-side helpers of the warped-motion entries (svt_hip_warp_pred_batch, svt_hip_warp_model_batch, svt_hip_wm_refine_batch): runners on device buffers (the fit reads
the MV array a motion search wrote, the prediction reads the fit's model array and writes the plane rd.enqueue_hip's descriptor reads) and on host
arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api


def plane_ref(tensor, stride, org_x, org_y, width, height, rows):
    """abi.WarpRef of a padded plane held by a device tensor: `width` x `height` are the PICTURE's on this plane, (org_x, org_y) its first sample in the
    plane, `rows` the rows the plane holds"""
    return abi.WarpRef(plane=tensor.data_ptr(), stride=stride, org_x=org_x, org_y=org_y, width=width, height=height, rows=rows)


def check_desc(d):
    """svt_hip_warp_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_warp_check_desc", d)


def pred_desc(bit_depth, ss_x, ss_y, refs, dst, dst_stride, dst_samples, jobs, n_jobs, status, models=None, n_models=0):
    """SvtHipWarpPredDesc from addresses (ints) and a list of abi.WarpRef"""
    if len(refs) > abi.WARP_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.WARP_MAX_REFS}")
    d = abi.WarpPredDesc(bit_depth=bit_depth, ss_x=ss_x, ss_y=ss_y, n_refs=len(refs), n_jobs=n_jobs, dst=dst, dst_stride=dst_stride, dst_samples=dst_samples,
                         jobs=jobs, models=models, n_models=n_models, status=status)
    for i, r in enumerate(refs):
        d.refs[i] = r
    return d


def run_warp_pred_device(ctx, bit_depth, ss_x, ss_y, refs, dst, dst_stride, jobs, n_jobs, status, models=None, n_models=0, dst_samples=None):
    """Enqueues svt_hip_warp_pred_batch on the context stream, without waiting.  refs: a list of abi.WarpRef (plane_ref); dst / jobs / status / models
    are device tensors: dst the prediction plane (uint8, or uint16 at 10 bits, as bytes or samples), jobs abi.WARP_PRED_JOB_DTYPE records, status one
    byte per job, models abi.WARP_MODEL_DTYPE records such as run_warp_model_device wrote.  dst_samples: the samples dst holds (default: all)."""
    sample_bytes = 2 if bit_depth > 8 else 1
    if dst_samples is None:
        dst_samples = dst.numel() * dst.element_size() // sample_bytes
    d = pred_desc(bit_depth, ss_x, ss_y, refs, dst.data_ptr(), dst_stride, dst_samples, jobs.data_ptr(), n_jobs, status.data_ptr(),
                  models.data_ptr() if models is not None else None, n_models)
    ctx.check(api.lib().svt_hip_warp_pred_batch(ctx._h, C.byref(d)), "svt_hip_warp_pred_batch")
    return d


def run_warp_model_device(ctx, jobs, n_jobs, models, status, shut_approx=0, lower_band_th=0, upper_band_th=0, mv_array=None, n_mvs=0):
    """Enqueues svt_hip_warp_model_batch on the context stream, without waiting.  jobs (abi.WARP_MODEL_JOB_DTYPE), models (abi.WARP_MODEL_DTYPE, written),
    status and mv_array (int16 (row, col) pairs such as svt_hip_md_subpel_batch's best_mv) are device tensors."""
    d = abi.WarpModelDesc(n_jobs=n_jobs, shut_approx=int(bool(shut_approx)), lower_band_th=lower_band_th, upper_band_th=upper_band_th, n_mvs=n_mvs,
                          jobs=jobs.data_ptr(), mv_array=mv_array.data_ptr() if mv_array is not None else None, models=models.data_ptr(),
                          status=status.data_ptr())
    ctx.check(api.lib().svt_hip_warp_model_batch(ctx._h, C.byref(d)), "svt_hip_warp_model_batch")
    return d


def run_warp_pred_hip(ctx, bit_depth, ss_x, ss_y, planes, jobs, dst_shape, dst_stride=None, models=None, spare_jobs=0, fill=0):
    """svt_hip_warp_pred_batch on host arrays.  planes: a list of (padded plane [rows][stride] uint8 / uint16, org_x, org_y, picture width, picture
    height); jobs: abi.WARP_PRED_JOB_DTYPE; dst_shape: (rows, columns) of the destination plane, dst_stride its pitch in samples (default: columns);
    models: abi.WARP_MODEL_DTYPE records or None.  Returns {"dst": [rows][dst_stride] as it is after the call (it starts as the byte `fill`), "status":
    [n + spare_jobs] (the spare slots start as `fill`), "planes": the reference planes read back}."""
    import torch
    dt = api.sample_dtype(bit_depth)
    n = len(jobs)
    rows, cols = dst_shape
    dst_stride = cols if dst_stride is None else dst_stride
    t_planes = [api.to_device(p[0], dt) for p in planes]
    refs = [plane_ref(t, p.shape[1], ox, oy, pw, ph, p.shape[0]) for t, (p, ox, oy, pw, ph) in zip(t_planes, planes)]
    t_dst = torch.full((rows * dst_stride * np.dtype(dt).itemsize,), fill, dtype=torch.uint8, device="cuda")
    t_status = api.filled(n + spare_jobs, fill)
    t_jobs = api.records_to_device(jobs, abi.WARP_PRED_JOB_DTYPE)
    t_models = api.to_device(models, abi.WARP_MODEL_DTYPE) if models is not None and len(models) else None
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_warp_pred_device(ctx, bit_depth, ss_x, ss_y, refs, t_dst, dst_stride, t_jobs, n, t_status, models=t_models,
                         n_models=len(models) if t_models is not None else 0, dst_samples=rows * dst_stride)
    ctx.sync()
    return {"dst": api.to_host(t_dst, dt, (rows, dst_stride)), "status": api.to_host(t_status, count=n + spare_jobs),
            "planes": [api.to_host(t, dt, p[0].shape) for t, p in zip(t_planes, planes)]}


def run_warp_model_hip(ctx, jobs, shut_approx=0, lower_band_th=0, upper_band_th=0, mv_array=None, spare_jobs=0, fill=0):
    """svt_hip_warp_model_batch on host arrays.  jobs: abi.WARP_MODEL_JOB_DTYPE; mv_array: int16 [n][2] or None.  Returns {"models": abi.WARP_MODEL_DTYPE
    [n + spare_jobs], "status": [n + spare_jobs]}; both start as the byte `fill`."""
    import torch
    n = len(jobs)
    size = np.dtype(abi.WARP_MODEL_DTYPE).itemsize
    t_jobs = api.records_to_device(jobs, abi.WARP_MODEL_JOB_DTYPE)
    t_models = api.filled(max(1, n + spare_jobs) * size, fill)
    t_status = api.filled(n + spare_jobs, fill)
    t_mv = api.to_device(mv_array, np.int16) if mv_array is not None and len(mv_array) else None
    torch.cuda.current_stream().synchronize()
    run_warp_model_device(ctx, t_jobs, n, t_models, t_status, shut_approx, lower_band_th, upper_band_th, t_mv, len(mv_array) if t_mv is not None else 0)
    ctx.sync()
    return {"models": api.to_host(t_models, abi.WARP_MODEL_DTYPE, count=n + spare_jobs), "status": api.to_host(t_status, count=n + spare_jobs)}


MV_CENTRE = 1 << 14  # the cost tables hold indices -16384 .. 16384; the descriptor points at their centre entries
REFINE_OUT_DTYPES = {"best_mv": "<i2", "best_cost": "<i4", "n_checked": "<u4", "status": "u1"}


def refine_desc(n_jobs, settings, refs, src, src_stride, src_samples, jobs, outs, mv_array=None, n_mvs=0, cost_tables=None, waves_per_job=0):
    """SvtHipWmRefineDesc from addresses.  settings: a mapping with iterations, refine_diag, mv_prec_shift, shut_approx, lower_band_th, upper_band_th,
    approx_inter_rate, error_per_bit; outs: addresses by the names of REFINE_OUT_DTYPES; cost_tables: the addresses of (mvjcost, the first entry of the
    row table, of the column table) or None."""
    if len(refs) > abi.WARP_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.WARP_MAX_REFS}")
    d = abi.WmRefineDesc(n_jobs=n_jobs, n_refs=len(refs), waves_per_job=waves_per_job, src=src, src_stride=src_stride, src_samples=src_samples, jobs=jobs,
                         mv_array=mv_array, n_mvs=n_mvs, **{k: int(v) for k, v in settings.items()}, **outs)
    for i, r in enumerate(refs):
        d.refs[i] = r
    if cost_tables is not None:
        d.mvjcost = cost_tables[0]
        d.mvcost[0], d.mvcost[1] = cost_tables[1] + 4 * MV_CENTRE, cost_tables[2] + 4 * MV_CENTRE
    return d


def check_refine_desc(d):
    """svt_hip_wm_refine_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_wm_refine_check_desc", d)


def run_wm_refine_device(ctx, settings, refs, src, src_stride, jobs, n_jobs, mv_array=None, n_mvs=0, cost_tables=None, waves_per_job=0, spare=0, fill=0,
                         outs=None):
    """Enqueues svt_hip_wm_refine_batch on the context stream and returns the outputs as device byte tensors by name, without waiting.  src / jobs /
    mv_array and the three cost_tables (mvjcost int32 [4], the row and the column table int32 [32769]) are device tensors; every output has `spare`
    slots past its length and starts as the byte `fill` (or is taken from `outs`)."""
    import torch
    if outs is None:
        outs = {name: torch.full(((n_jobs + spare) * (2 if name == "best_mv" else 1) * np.dtype(dt).itemsize,), fill, dtype=torch.uint8, device="cuda")
                for name, dt in REFINE_OUT_DTYPES.items()}
        torch.cuda.current_stream().synchronize()  # the fills ran on torch's stream
    d = refine_desc(n_jobs, settings, refs, src.data_ptr(), src_stride, src.numel() * src.element_size(), jobs.data_ptr(),
                    {k: t.data_ptr() for k, t in outs.items()}, mv_array.data_ptr() if mv_array is not None else None, n_mvs,
                    [t.data_ptr() for t in cost_tables] if cost_tables is not None else None, waves_per_job)
    ctx.check(api.lib().svt_hip_wm_refine_batch(ctx._h, C.byref(d)), "svt_hip_wm_refine_batch")
    return outs


def run_wm_refine_hip(ctx, settings, planes, src, jobs, mv_array=None, cost_tables=None, waves_per_job=0, spare=0, fill=0):
    """svt_hip_wm_refine_batch on host arrays.  planes as in run_warp_pred_hip (8-bit); src: the source plane [rows][stride] uint8; jobs:
    abi.WM_REFINE_JOB_DTYPE; cost_tables: (mvjcost, row table, column table) int32 arrays or None.  Returns the outputs by name, each [n + spare]
    (best_mv [n + spare][2]), and "planes" / "src" read back."""
    n = len(jobs)
    t_planes = [api.to_device(p[0], np.uint8) for p in planes]
    refs = [plane_ref(t, p.shape[1], ox, oy, pw, ph, p.shape[0]) for t, (p, ox, oy, pw, ph) in zip(t_planes, planes)]
    t_src = api.to_device(src, np.uint8)
    t_jobs = api.records_to_device(jobs, abi.WM_REFINE_JOB_DTYPE)
    t_mv = api.to_device(mv_array, np.int16) if mv_array is not None and len(mv_array) else None
    t_cost = [api.to_device(t, np.int32) for t in cost_tables] if cost_tables is not None else None
    outs = run_wm_refine_device(ctx, settings, refs, t_src, src.shape[1], t_jobs, n, t_mv, len(mv_array) if t_mv is not None else 0, t_cost, waves_per_job,
                                spare, fill)
    ctx.sync()
    out = {name: api.to_host(t, REFINE_OUT_DTYPES[name]) for name, t in outs.items()}
    out["best_mv"] = out["best_mv"].reshape(-1, 2)
    out["planes"] = [api.to_host(t, shape=p[0].shape) for t, p in zip(t_planes, planes)]
    out["src"] = api.to_host(t_src, shape=src.shape)
    return out


def tables():
    """the library's host copies of the 193 x 8 filter table (int16) and of the 257 divisor multipliers (uint16)"""
    L = api.lib()
    L.svt_hip_warp_filter_table.restype = C.POINTER(C.c_int16 * (193 * 8))
    L.svt_hip_warp_div_lut.restype = C.POINTER(C.c_uint16 * 257)
    return (np.array(L.svt_hip_warp_filter_table().contents, np.int16).reshape(193, 8), np.array(L.svt_hip_warp_div_lut().contents, np.uint16))
