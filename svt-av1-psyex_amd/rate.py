"""Host-side helpers of the coefficient-rate entry (svt_hip_coeff_rate_batch): table upload, a runner on host arrays and one on device
buffers (the chain behind rd.enqueue_hip).  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api


def tables_bytes(tables):
    """SvtHipRateTables as bytes from the four members of MdRateEstimationContext it mirrors: `tables` is a mapping or an object with
    coeff_fac_bits, eob_frac_bits, intra_tx_type_fac_bits and inter_tx_type_fac_bits as int32 arrays of abi.RATE_TABLE_SHAPES' sizes."""
    out = []
    for name, shape in abi.RATE_TABLE_SHAPES:
        a = np.ascontiguousarray(tables[name] if isinstance(tables, dict) else getattr(tables, name), np.int32)
        if a.size != int(np.prod(shape)):
            raise ValueError(f"{name}: {a.size} values, SvtHipRateTables holds {int(np.prod(shape))}")
        out.append(a.tobytes())
    raw = b"".join(out)
    assert len(raw) == C.sizeof(abi.RateTables)
    return raw


def upload_tables(tables):
    """the rate tables in device memory (a torch byte tensor; pass it as `tables` to the runners, once per picture)"""
    import torch
    return torch.frombuffer(bytearray(tables_bytes(tables)), dtype=torch.uint8).cuda()


def run_rate_device(ctx, tables, tx_size, plane, jobs, n_jobs, qcoeff, eob, reduced_tx_set=0, coeff_rate_est_lvl=1, mds_fast_coeff_est_level=1,
                    mds_subres_step=0, lam=None, dist=None, dist_stride=1, group_start=None, n_groups=0, spare_jobs=0, fill=0):
    """Enqueues svt_hip_coeff_rate_batch on the context stream and returns the outputs as device byte tensors by name, without waiting.
    tables / jobs / qcoeff / eob / dist / group_start are device tensors (upload_tables; rd.enqueue_hip's outs["qcoeff"], outs["eob"] and, with
    dist_stride = 2, outs["dist_coeff"]).  lam: lambda; with it and dist -> "rd_cost"; with group_start (n_groups + 1 uint32) -> "best_job",
    "best_cost".  Every output has `spare_jobs` slots past its length and starts as the byte `fill`."""
    import torch
    new = lambda count, size: torch.full(((count + spare_jobs) * size,), fill, dtype=torch.uint8, device="cuda")
    outs = {"bits": new(n_jobs, 8)}
    d = abi.CoeffRateDesc(tx_size=tx_size, plane_type=plane, reduced_tx_set=reduced_tx_set, coeff_rate_est_lvl=coeff_rate_est_lvl,
                          mds_fast_coeff_est_level=mds_fast_coeff_est_level, mds_subres_step=mds_subres_step, n_jobs=n_jobs,
                          jobs=jobs.data_ptr(), tables=tables.data_ptr(), qcoeff=qcoeff.data_ptr(), eob=eob.data_ptr(), bits=outs["bits"].data_ptr())
    if lam is not None:
        outs["rd_cost"] = new(n_jobs, 8)
        d.lambda_, d.dist_stride, d.dist, d.rd_cost = int(lam), dist_stride, dist.data_ptr() if dist is not None else None, outs["rd_cost"].data_ptr()
    if group_start is not None:
        outs["best_job"], outs["best_cost"] = new(n_groups, 4), new(n_groups, 8)
        d.n_groups, d.group_start, d.best_job, d.best_cost = n_groups, group_start.data_ptr(), outs["best_job"].data_ptr(), outs["best_cost"].data_ptr()
    torch.cuda.current_stream().synchronize()  # the fills above ran on torch's stream; the context stream is not waited for
    ctx.check(api.lib().svt_hip_coeff_rate_batch(ctx._h, C.byref(d)), "svt_hip_coeff_rate_batch")
    return outs


RATE_OUT_DTYPES = {"bits": "<u8", "rd_cost": "<u8", "best_job": "<u4", "best_cost": "<u8"}


def download(outs):
    """run_rate_device's outputs as numpy arrays (after ctx.sync())"""
    return {name: api.to_host(t, RATE_OUT_DTYPES[name]) for name, t in outs.items()}


def run_rate_hip(ctx, tables, tx_size, plane, jobs, qcoeff, eob, reduced_tx_set=0, coeff_rate_est_lvl=1, mds_fast_coeff_est_level=1,
                 mds_subres_step=0, lam=None, dist=None, group_start=None, spare_jobs=0, fill=0):
    """svt_hip_coeff_rate_batch on host arrays: jobs (abi.RATE_JOB_DTYPE), qcoeff int32 [n][min(W,32) * min(H,32)], eob uint16 [n], optional
    lam + dist (uint64 [n]) and group_start (uint32 [n_groups + 1]).  tables: upload_tables' tensor, or the host tables.  Returns
    {"bits", "rd_cost", "best_job", "best_cost"} (those asked for) as numpy arrays, each with its `spare_jobs` slots."""
    n = len(jobs)
    npk = min(abi.TX_W[tx_size], 32) * min(abi.TX_H[tx_size], 32) if tx_size < len(abi.TX_W) else 0
    qcoeff = np.ascontiguousarray(qcoeff, np.int32)
    if qcoeff.size != n * npk or len(eob) != n:
        raise ValueError(f"{n} jobs of {npk} coefficients: qcoeff holds {qcoeff.size}, eob {len(eob)}")
    if not hasattr(tables, "data_ptr"):
        tables = upload_tables(tables)
    pad = np.zeros(1, np.uint64)  # an empty batch still passes pointers
    t_jobs = api.to_device(np.ascontiguousarray(jobs, dtype=abi.RATE_JOB_DTYPE) if n else pad)
    t_q, t_eob = api.to_device(qcoeff if n else pad), api.to_device(np.ascontiguousarray(eob, np.uint16) if n else pad)
    t_dist = api.to_device(dist, np.uint64) if dist is not None else None
    t_gs = api.to_device(group_start, np.uint32) if group_start is not None else None
    outs = run_rate_device(ctx, tables, tx_size, plane, t_jobs, n, t_q, t_eob, reduced_tx_set, coeff_rate_est_lvl, mds_fast_coeff_est_level,
                           mds_subres_step, lam, t_dist, 1, t_gs, len(group_start) - 1 if group_start is not None else 0, spare_jobs, fill)
    ctx.sync()
    return download(outs)
