"""Host-side helpers of the chroma-from-luma entries (svt_hip_cfl_pred_batch, svt_hip_cfl_pick_alpha_batch): runners on device buffers (the
prediction writes the plane rd.enqueue_hip's descriptor reads; the pick reads what rate.run_rate_device wrote) and on host arrays.  torch is
plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api

ALPHAS_FULL = list(range(-16, 17))  # the alpha search's list: slot k is alpha_q3 = k - 16


def check_desc(d):
    """svt_hip_cfl_pred_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_cfl_pred_check_desc", d)


def pred_desc(bit_depth, width, height, alphas, luma, luma_stride, luma_width, luma_height, planes, slot_stride, jobs, n_jobs, status, ac=None):
    """SvtHipCflPredDesc from addresses: luma / jobs / status / ac are addresses (ints), planes two mappings with dc, dc_stride, dc_samples, dst,
    dst_stride, dst_samples."""
    if len(alphas) > abi.CFL_SLOTS:
        raise ValueError(f"{len(alphas)} alphas: the descriptor holds {abi.CFL_SLOTS}")
    d = abi.CflPredDesc(bit_depth=bit_depth, width=width, height=height, n_alpha=len(alphas), n_jobs=n_jobs, luma=luma, luma_stride=luma_stride,
                        luma_width=luma_width, luma_height=luma_height, slot_stride=slot_stride, jobs=jobs, status=status, ac=ac)
    for k, a in enumerate(alphas):
        d.alpha_q3[k] = int(a)
    for p in range(2):
        for name, _ in abi.CflPlane._fields_:
            setattr(d.plane[p], name, planes[p][name])
    return d


def run_cfl_pred_device(ctx, bit_depth, width, height, alphas, luma, luma_stride, luma_width, luma_height, dc, dc_stride, dst, dst_stride, slot_stride,
                        jobs, n_jobs, status, ac=None, dc_samples=None, dst_samples=None, dst_first=0):
    """Enqueues svt_hip_cfl_pred_batch on the context stream, without waiting.  luma / jobs / status / ac and the two dc and two dst are device
    tensors (uint8, or uint16 at 10 bits, as bytes or samples); jobs are abi.CFL_PRED_JOB_DTYPE records.  dc_samples / dst_samples: the samples
    each plane holds (default: all of the tensor behind dst_first); dst_first: the sample of each dst tensor the destination begins at."""
    sb = 2 if bit_depth > 8 else 1
    samples = lambda t: t.numel() * t.element_size() // sb
    planes = [dict(dc=dc[p].data_ptr(), dc_stride=dc_stride, dc_samples=samples(dc[p]) if dc_samples is None else dc_samples,
                   dst=dst[p].data_ptr() + dst_first * sb, dst_stride=dst_stride,
                   dst_samples=samples(dst[p]) - dst_first if dst_samples is None else dst_samples) for p in range(2)]
    d = pred_desc(bit_depth, width, height, alphas, luma.data_ptr(), luma_stride, luma_width, luma_height, planes, slot_stride, jobs.data_ptr(), n_jobs,
                  status.data_ptr(), ac.data_ptr() if ac is not None else None)
    ctx.check(api.lib().svt_hip_cfl_pred_batch(ctx._h, C.byref(d)), "svt_hip_cfl_pred_batch")
    return d


def run_cfl_pred_hip(ctx, bit_depth, width, height, alphas, luma, dc, jobs, dst_samples, dst_stride, slot_stride, want_ac=False, spare_jobs=0, fill=0,
                     guard=0, luma_size=None):
    """svt_hip_cfl_pred_batch on host arrays.  luma: the luma plane [rows][stride] uint8 / uint16; luma_size: (width, height) the kernel may read
    (default: the whole array); dc: the two DC planes [rows][stride] (one stride); jobs: abi.CFL_PRED_JOB_DTYPE; each destination holds dst_samples
    samples between two bands of `guard` samples.  Returns {"dst": the two destinations with their bands, as they are after the call (they start
    as the byte `fill`), "status": [n + spare_jobs], "ac": [n + spare_jobs][H][W] int16 or None, "luma" / "dc": the inputs read back}."""
    import torch
    dt = api.sample_dtype(bit_depth)
    sb = np.dtype(dt).itemsize
    n = len(jobs)
    luma = np.ascontiguousarray(luma, dtype=dt)
    dc = [np.ascontiguousarray(a, dtype=dt) for a in dc]
    lw, lh = (luma.shape[1], luma.shape[0]) if luma_size is None else luma_size
    t_luma, t_dc = api.to_device(luma), [api.to_device(a) for a in dc]
    t_dst = [torch.full(((dst_samples + 2 * guard) * sb,), fill, dtype=torch.uint8, device="cuda") for _ in range(2)]
    t_status = api.filled(n + spare_jobs, fill)
    t_ac = api.filled(max(1, n + spare_jobs) * width * height * 2, fill) if want_ac else None
    t_jobs = api.records_to_device(jobs, abi.CFL_PRED_JOB_DTYPE)
    torch.cuda.current_stream().synchronize()  # the fills and copies above ran on torch's stream; the context stream is not waited for
    run_cfl_pred_device(ctx, bit_depth, width, height, alphas, t_luma, luma.shape[1], lw, lh, t_dc, dc[0].shape[1], t_dst, dst_stride, slot_stride, t_jobs,
                        n, t_status, t_ac, dst_samples=dst_samples, dst_first=guard)
    ctx.sync()
    return {"dst": [api.to_host(t, dt) for t in t_dst], "status": api.to_host(t_status, count=n + spare_jobs),
            "ac": api.to_host(t_ac, np.int16, (-1, height, width))[:n + spare_jobs] if want_ac else None,
            "luma": api.to_host(t_luma, dt, luma.shape), "dc": [api.to_host(t, dt, a.shape) for t, a in zip(t_dc, dc)]}


PICK_OUT_DTYPES = {"best_rd": "<u8", "cfl_alpha_idx": "u1", "cfl_alpha_signs": "u1", "status": "u1"}


def run_pick_device(ctx, n_blocks, bits, dist, mode_bits, alpha_fac_bits, lam, itr_th, n_mag=16, dist_stride=1, spare=0, fill=0):
    """Enqueues svt_hip_cfl_pick_alpha_batch on the context stream and returns the outputs as device byte tensors by name, without waiting.
    bits / dist / mode_bits / alpha_fac_bits are device tensors: bits and dist [n_blocks][2][33] uint64 (rate.run_rate_device's outs["bits"] and,
    with dist_stride = 2, rd's outs["dist_coeff"] in place), mode_bits int32 [n_blocks], alpha_fac_bits int32 [8][2][16].  Every output has `spare`
    slots past its length and starts as the byte `fill`."""
    import torch
    outs = {name: torch.full(((n_blocks + spare) * np.dtype(dt).itemsize,), fill, dtype=torch.uint8, device="cuda") for name, dt in PICK_OUT_DTYPES.items()}
    d = abi.CflPickDesc(n_blocks=n_blocks, lambda_=int(lam), itr_th=itr_th, n_mag=n_mag, dist_stride=dist_stride, bits=bits.data_ptr(), dist=dist.data_ptr(),
                        mode_bits=mode_bits.data_ptr(), alpha_fac_bits=alpha_fac_bits.data_ptr())
    for name, t in outs.items():
        setattr(d, name, t.data_ptr())
    torch.cuda.current_stream().synchronize()  # the fills above ran on torch's stream
    ctx.check(api.lib().svt_hip_cfl_pick_alpha_batch(ctx._h, C.byref(d)), "svt_hip_cfl_pick_alpha_batch")
    return outs


def download_pick(outs):
    """run_pick_device's outputs as numpy arrays (after ctx.sync())"""
    return {name: api.to_host(t, PICK_OUT_DTYPES[name]) for name, t in outs.items()}


def run_pick_hip(ctx, bits, dist, mode_bits, alpha_fac_bits, lam, itr_th, n_mag=16, spare=0, fill=0):
    """svt_hip_cfl_pick_alpha_batch on host arrays: bits / dist uint64 [n][2][33], mode_bits int32 [n], alpha_fac_bits int32 [8][2][16]."""
    n = len(mode_bits)
    bits, dist = np.ascontiguousarray(bits, np.uint64), np.ascontiguousarray(dist, np.uint64)
    if bits.size != n * 2 * abi.CFL_SLOTS or dist.size != bits.size or np.asarray(alpha_fac_bits).size != 8 * 2 * 16:
        raise ValueError(f"{n} blocks: bits holds {bits.size}, dist {dist.size}, alpha_fac_bits {np.asarray(alpha_fac_bits).size}")
    ins = [api.records_to_device(a, dt) for a, dt in ((bits, np.uint64), (dist, np.uint64), (mode_bits, np.int32), (alpha_fac_bits, np.int32))]  # held until the stream has run
    outs = run_pick_device(ctx, n, *ins, lam, itr_th, n_mag, 1, spare, fill)
    ctx.sync()
    return download_pick(outs)
