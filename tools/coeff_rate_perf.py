#!/usr/bin/env python3
"""Times svt_hip_coeff_rate_batch beside svt_hip_rd_batch on the RD job sets of bench.py: one 2160p 10-bit picture tiled with 16x16, 32x32 and 64x64 blocks.

Per size: the RD batch (quantizer rows of bench.py, qcoeff requested, no reconstruction), then the rate batch on the qcoeff / eob / dist_coeff
buffers the RD batch left on the device, with the RD cost and groups of 16 candidates (one winner per group).  HIP events around each launch
on the context stream, 5 warm-up launches, median of --reps.  Also printed: the bytes that no longer cross PCIe -- the qcoeff array against
8 (bits), 16 (bits + rd_cost) bytes per job or 12 bytes per block of 16 candidates -- and the rate kernel's read rate (4 bytes per
coefficient) against the 8.0 TB/s HBM spec peak.  The tables are the default-probability tables of tests/golden/coeff_rate.npz; the
results are compared with the restatement of tests/coeff_rate_cases.py on a sample of the jobs.  Prints one JSON line per size (and, with
--out, writes the figures as JSON)."""
import ctypes as C
import statistics

import numpy as np

import perf_common

perf_common.repo_paths()
import coeff_rate_cases as cr  # noqa: E402
from svt_av1_psyex_amd import abi, api, rate, rd  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s: the MI355X's HBM3E spec peak
W, H = 3840, 2160
GROUP = 16


def median_min(ms):
    return statistics.median(ms), min(ms)


def main():
    a = perf_common.arguments(__doc__, 30)
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(5)
    src = rng.integers(0, 1024, (H, W)).astype(np.uint16)
    pred = np.clip(src.astype(np.int32) + rng.integers(-64, 65, src.shape), 0, 1023).astype(np.uint16)
    z = np.load(cr.GOLDEN)
    T = cr.Tables.from_golden(z, 1)
    t_tab = rate.upload_tables(T)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_src, t_pred, t_rows = dev(src), dev(pred), dev(np.stack([rd.quant_row_from_step(140, 176)]))
    results = []
    for ts in (2, 3, 4):
        jobs = rd.grid_jobs(W, H, W, ts)
        n = len(jobs)
        npk = min(abi.TX_W[ts], 32) * min(abi.TX_H[ts], 32)
        t_jobs = dev(jobs)
        outs = {name: torch.zeros(n * k * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for name, dt, k in abi.RD_OUT_FIELDS}
        outs["qcoeff"] = torch.zeros(n * npk * 4, dtype=torch.uint8, device="cuda")
        d = abi.RdBatchDesc(bit_depth=10, quant_kind=0, tx_size=ts, n_jobs=n, src_stride=W, pred_stride=W, src=t_src.data_ptr(), pred=t_pred.data_ptr(),
                            recon=None, jobs=t_jobs.data_ptr(), quant_rows=t_rows.data_ptr(), n_quant_rows=1)
        for name, t in outs.items():
            setattr(d, name, t.data_ptr())
        rjobs = np.zeros(n, abi.RATE_JOB_DTYPE)
        rjobs["txb_skip_ctx"], rjobs["dc_sign_ctx"], rjobs["is_inter"] = np.arange(n) % 13, np.arange(n) % 3, 1
        group_start = np.append(np.arange(0, n, GROUP), n).astype(np.uint32)
        n_groups = len(group_start) - 1
        t_rjobs, t_gs = dev(rjobs), dev(group_start)
        t_bits, t_cost = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        t_bj, t_bc = torch.zeros(n_groups, dtype=torch.int32, device="cuda"), torch.zeros(n_groups, dtype=torch.int64, device="cuda")
        r = abi.CoeffRateDesc(tx_size=ts, plane_type=0, coeff_rate_est_lvl=1, mds_fast_coeff_est_level=1, n_jobs=n, n_groups=n_groups, jobs=t_rjobs.data_ptr(),
                              tables=t_tab.data_ptr(), qcoeff=outs["qcoeff"].data_ptr(), eob=outs["eob"].data_ptr(), bits=t_bits.data_ptr(), lambda_=41000,
                              dist_stride=2, dist=outs["dist_coeff"].data_ptr(), rd_cost=t_cost.data_ptr(), group_start=t_gs.data_ptr(),
                              best_job=t_bj.data_ptr(), best_cost=t_bc.data_ptr())
        torch.cuda.synchronize()
        rd_ms, rd_min = median_min(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_rd_batch(ctx._h, C.byref(d)), "svt_hip_rd_batch")))
        rate_ms, rate_min = median_min(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_coeff_rate_batch(ctx._h, C.byref(r)), "svt_hip_coeff_rate_batch")))
        # a sample of the jobs against the restatement
        eob = outs["eob"].cpu().numpy().view(np.uint16)
        q = outs["qcoeff"].cpu().numpy().view(np.int32).reshape(n, npk)
        bits = t_bits.cpu().numpy().view(np.uint64)
        pick = np.linspace(0, n - 1, 64).astype(int)
        case = {"tx_size": ts, "plane": 0, "reduced": 0, "jobs": rjobs[pick], "qcoeff": q[pick], "eob": eob[pick]}
        _, want = cr.run_case(T, case, variants=[(1, 0)])
        if not np.array_equal(bits[pick], want[0]):
            raise SystemExit(f"tx_size {ts}: the device's bits differ from the restatement")
        res = dict(tx=f"{abi.TX_W[ts]}x{abi.TX_H[ts]}", jobs=n, coeffs_per_job=npk, mean_eob=round(float(eob.mean()), 1), rd_ms_median=round(rd_ms, 4),
                   rd_ms_min=round(rd_min, 4), rate_ms_median=round(rate_ms, 4), rate_ms_min=round(rate_min, 4), rate_over_rd=round(rate_ms / rd_ms, 3),
                   rate_gb_per_s=round(n * npk * 4 / rate_ms / 1e6, 1), rate_hbm_peak_share=round(n * npk * 4 / rate_ms / 1e-3 / HBM_PEAK, 4),
                   qcoeff_bytes=n * npk * 4, bits_bytes=n * 8, bits_and_cost_bytes=n * 16, winner_bytes=n_groups * 12)
        results.append(res)
        perf_common.emit(res)
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
