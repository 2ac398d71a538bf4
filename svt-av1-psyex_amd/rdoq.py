"""Host-side helpers of the RDOQ entry (svt_hip_rdoq_batch): a runner on device buffers (the link between rd.enqueue_hip and
rate.run_rate_device) and one on host arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api, rate

CONTROLS = ("sharpness", "eob_fast_inter", "eob_fast_intra", "eob_th", "eob_fast_th")
RDOQ_OUT_DTYPES = {"status": "u1", "dist_coeff": "<u8", "cul_level": "u1"}


def run_rdoq_device(ctx, tables, tx_size, plane, jobs, n_jobs, quant_rows, n_quant_rows, coeff, qcoeff, dqcoeff, eob, lam, sharpness=0, eob_fast_inter=0,
                    eob_fast_intra=0, eob_th=255, eob_fast_th=255, iqmatrix=None, fallback=None, dist_coeff=None, outputs=("status", "dist_coeff", "cul_level"),
                    spare_jobs=0, fill=0):
    """Enqueues svt_hip_rdoq_batch on the context stream, without waiting.  tables / jobs / quant_rows / coeff / qcoeff / dqcoeff / eob are device
    tensors (rate.upload_tables; rd.enqueue_hip's outs of a quant_kind 1 batch): qcoeff, dqcoeff and eob are rewritten in place.  fallback: the
    (qcoeff, dqcoeff, eob) device tensors of the same jobs' quant_kind 0 batch, or None.  dist_coeff: a device tensor to renew in place (the RD
    batch's own), else a new one is made when `outputs` asks for it.  Returns the optional outputs as device byte tensors by name, each with
    `spare_jobs` slots past its length and starting as the byte `fill`."""
    import torch
    sizes = {"status": 1, "dist_coeff": 16, "cul_level": 1}
    outs = {name: torch.full(((n_jobs + spare_jobs) * sizes[name],), fill, dtype=torch.uint8, device="cuda") for name in outputs
            if not (name == "dist_coeff" and dist_coeff is not None)}
    if dist_coeff is not None:
        outs["dist_coeff"] = dist_coeff
    d = abi.RdoqDesc(tx_size=tx_size, plane_type=plane, sharpness=sharpness, eob_fast_inter=eob_fast_inter, eob_fast_intra=eob_fast_intra, eob_th=eob_th,
                     eob_fast_th=eob_fast_th, n_jobs=n_jobs, lambda_=int(lam), jobs=jobs.data_ptr(), tables=tables.data_ptr(),
                     quant_rows=quant_rows.data_ptr(), n_quant_rows=n_quant_rows, iqmatrix=iqmatrix.data_ptr() if iqmatrix is not None else None,
                     coeff=coeff.data_ptr(), qcoeff=qcoeff.data_ptr(), dqcoeff=dqcoeff.data_ptr(), eob=eob.data_ptr())
    for name, t in outs.items():
        setattr(d, name, t.data_ptr())
    if fallback is not None:
        d.qcoeff_b, d.dqcoeff_b, d.eob_b = (t.data_ptr() for t in fallback)
    torch.cuda.current_stream().synchronize()  # the fills above ran on torch's stream; the context stream is not waited for
    ctx.check(api.lib().svt_hip_rdoq_batch(ctx._h, C.byref(d)), "svt_hip_rdoq_batch")
    return outs


def download(outs):
    """run_rdoq_device's outputs as numpy arrays (after ctx.sync())"""
    return {name: api.to_host(t, RDOQ_OUT_DTYPES[name]) for name, t in outs.items()}


def run_rdoq_hip(ctx, tables, tx_size, plane, jobs, quant_rows, coeff, qcoeff, dqcoeff, eob, lam, iqmatrix=None, fallback=None, spare_jobs=0, fill=0,
                 outputs=("status", "dist_coeff", "cul_level"), **controls):
    """svt_hip_rdoq_batch on host arrays: jobs (abi.RDOQ_JOB_DTYPE), quant_rows (abi.QUANT_ROW_DTYPE), coeff / qcoeff / dqcoeff int32
    [n][min(W,32) * min(H,32)], eob uint16 [n]; fallback = (qcoeff_b, dqcoeff_b, eob_b) or None; controls: CONTROLS.  tables: rate.upload_tables'
    tensor, or the host tables.  Returns {"coeff", "qcoeff", "dqcoeff", "eob"} as they are after the call plus the optional outputs, every array
    with its `spare_jobs` slots (the inputs' spare slots start as `fill`)."""
    unknown = set(controls) - set(CONTROLS)
    if unknown:
        raise ValueError(f"unknown RDOQ controls {sorted(unknown)}")
    n = len(jobs)
    npk = min(abi.TX_W[tx_size], 32) * min(abi.TX_H[tx_size], 32) if tx_size < len(abi.TX_W) else 0

    def padded(a, dtype, per_job):
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        if a.size != n * per_job:
            raise ValueError(f"{n} jobs of {per_job} elements: an array holds {a.size}")
        t = api.filled(max(1, (n + spare_jobs) * per_job) * a.itemsize, fill)  # an empty batch still passes pointers
        t[:a.nbytes] = api.to_device(a)
        return t
    if not hasattr(tables, "data_ptr"):
        tables = rate.upload_tables(tables)
    pad = np.zeros(1, np.uint64)
    t_jobs = api.to_device(np.ascontiguousarray(jobs, dtype=abi.RDOQ_JOB_DTYPE) if n else pad)
    t_rows = api.to_device(quant_rows, abi.QUANT_ROW_DTYPE)
    t_iqm = api.to_device(iqmatrix, np.uint8) if iqmatrix is not None else None
    t_c, t_q, t_dq, t_eob = padded(coeff, np.int32, npk), padded(qcoeff, np.int32, npk), padded(dqcoeff, np.int32, npk), padded(eob, np.uint16, 1)
    t_fb = (padded(fallback[0], np.int32, npk), padded(fallback[1], np.int32, npk), padded(fallback[2], np.uint16, 1)) if fallback is not None else None
    outs = run_rdoq_device(ctx, tables, tx_size, plane, t_jobs, n, t_rows, len(quant_rows), t_c, t_q, t_dq, t_eob, lam, iqmatrix=t_iqm, fallback=t_fb,
                           outputs=outputs, spare_jobs=spare_jobs, fill=fill, **controls)
    ctx.sync()
    res = download(outs)
    slots = n + spare_jobs
    for name, t in (("coeff", t_c), ("qcoeff", t_q), ("dqcoeff", t_dq)):
        res[name] = api.to_host(t, np.int32, (slots, npk), count=slots * npk)
    res["eob"] = api.to_host(t_eob, np.uint16, count=slots)
    if "dist_coeff" in res:
        res["dist_coeff"] = res["dist_coeff"].reshape(-1, 2)
    return res
