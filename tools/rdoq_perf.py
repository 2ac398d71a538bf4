#!/usr/bin/env python3
"""Times svt_hip_rdoq_batch beside svt_hip_rd_batch and svt_hip_coeff_rate_batch on the RD job sets of bench.py: one 2160p 10-bit picture tiled with 16x16, 32x32 and 64x64 blocks.

Per size: the RD batch with the "fp" quantizer (quantizer rows of bench.py; coeff, qcoeff and dqcoeff requested, no reconstruction), then RDOQ in
place on the buffers the RD batch left on the device (level-1 controls: no gate, no fast mode; dist_coeff renewed, cul_level and status written),
then the rate batch on the optimised qcoeff / eob / dist_coeff.  RDOQ rewrites its inputs, so every timed launch starts from a device-side copy of
the RD batch's qcoeff / dqcoeff / eob made outside the timed interval.  HIP events around each launch on the context stream, 5 warm-up launches,
median of --reps.  Also printed: the bytes RDOQ on the host would move in the middle of the chain -- coeff, qcoeff and dqcoeff down (12 bytes per
coefficient) and qcoeff and dqcoeff up again (8 bytes per coefficient), eob both ways -- against the HIP-event time.  The tables are the
default-probability tables of tests/golden/coeff_rate.npz; the results are compared with the restatement of tests/rdoq_cases.py on a sample of
the jobs.  Prints one JSON line per size (and, with --out, writes the figures as JSON)."""
import ctypes as C
import statistics

import numpy as np

import perf_common

perf_common.repo_paths()
import coeff_rate_cases as cr  # noqa: E402
import rdoq_cases as rq  # noqa: E402
from svt_av1_psyex_amd import abi, api, rate, rd  # noqa: E402

W, H = 3840, 2160
GROUP = 16
LAMBDA = 41000


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
    T = cr.Tables.from_golden(np.load(cr.GOLDEN), 1)
    t_tab = rate.upload_tables(T)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    rows = np.stack([rd.quant_row_from_step(140, 176)])
    t_src, t_pred, t_rows = dev(src), dev(pred), dev(rows)
    results = []
    for ts in (2, 3, 4):
        jobs = rd.grid_jobs(W, H, W, ts)
        n = len(jobs)
        npk = min(abi.TX_W[ts], 32) * min(abi.TX_H[ts], 32)
        t_jobs = dev(jobs)
        outs = {name: torch.zeros(n * k * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for name, dt, k in abi.RD_OUT_FIELDS}
        for name in ("coeff", "qcoeff", "dqcoeff"):
            outs[name] = torch.zeros(n * npk * 4, dtype=torch.uint8, device="cuda")
        d = abi.RdBatchDesc(bit_depth=10, quant_kind=1, tx_size=ts, n_jobs=n, src_stride=W, pred_stride=W, src=t_src.data_ptr(), pred=t_pred.data_ptr(),
                            recon=None, jobs=t_jobs.data_ptr(), quant_rows=t_rows.data_ptr(), n_quant_rows=1)
        for name, t in outs.items():
            setattr(d, name, t.data_ptr())
        qjobs = np.zeros(n, abi.RDOQ_JOB_DTYPE)
        qjobs["txb_skip_ctx"], qjobs["dc_sign_ctx"], qjobs["is_inter"] = np.arange(n) % 13, np.arange(n) % 3, 1
        rjobs = np.zeros(n, abi.RATE_JOB_DTYPE)
        rjobs["txb_skip_ctx"], rjobs["dc_sign_ctx"], rjobs["is_inter"] = qjobs["txb_skip_ctx"], qjobs["dc_sign_ctx"], 1
        group_start = np.append(np.arange(0, n, GROUP), n).astype(np.uint32)
        n_groups = len(group_start) - 1
        t_qjobs, t_rjobs, t_gs = dev(qjobs), dev(rjobs), dev(group_start)
        t_status, t_cul = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        t_bits, t_cost = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        t_bj, t_bc = torch.zeros(n_groups, dtype=torch.int32, device="cuda"), torch.zeros(n_groups, dtype=torch.int64, device="cuda")
        o = abi.RdoqDesc(tx_size=ts, plane_type=0, eob_th=255, eob_fast_th=255, n_jobs=n, lambda_=LAMBDA, jobs=t_qjobs.data_ptr(), tables=t_tab.data_ptr(),
                         quant_rows=t_rows.data_ptr(), n_quant_rows=1, coeff=outs["coeff"].data_ptr(), qcoeff=outs["qcoeff"].data_ptr(),
                         dqcoeff=outs["dqcoeff"].data_ptr(), eob=outs["eob"].data_ptr(), status=t_status.data_ptr(), dist_coeff=outs["dist_coeff"].data_ptr(),
                         cul_level=t_cul.data_ptr())
        r = abi.CoeffRateDesc(tx_size=ts, plane_type=0, coeff_rate_est_lvl=1, mds_fast_coeff_est_level=1, n_jobs=n, n_groups=n_groups, jobs=t_rjobs.data_ptr(),
                              tables=t_tab.data_ptr(), qcoeff=outs["qcoeff"].data_ptr(), eob=outs["eob"].data_ptr(), bits=t_bits.data_ptr(), lambda_=LAMBDA,
                              dist_stride=2, dist=outs["dist_coeff"].data_ptr(), rd_cost=t_cost.data_ptr(), group_start=t_gs.data_ptr(),
                              best_job=t_bj.data_ptr(), best_cost=t_bc.data_ptr())
        torch.cuda.synchronize()
        rd_ms, rd_min = median_min(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_rd_batch(ctx._h, C.byref(d)), "svt_hip_rd_batch")))
        keep = {name: outs[name].clone() for name in ("qcoeff", "dqcoeff", "eob", "dist_coeff")}  # the RD batch's own: every RDOQ launch starts here
        torch.cuda.synchronize()

        def restore():
            for name, t in keep.items():
                outs[name].copy_(t)
        # the batch works in place: every round puts the inputs back first, between events of its own that are not reported
        rounds = [("restore", restore), ("rdoq", lambda: ctx.check(L.svt_hip_rdoq_batch(ctx._h, C.byref(o)), "svt_hip_rdoq_batch"))]
        rdoq_ms, rdoq_min = median_min(perf_common.timed_rounds(ctx, ext, a.reps, rounds)["rdoq"])
        rate_ms, rate_min = median_min(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_coeff_rate_batch(ctx._h, C.byref(r)), "svt_hip_coeff_rate_batch")))
        # a sample of the jobs against the restatement
        pick = np.linspace(0, n - 1, 48).astype(int)
        view = lambda t, dt, k: t.cpu().numpy().view(dt).reshape(n, k)[pick]
        case = dict(tx_size=ts, plane=0, jobs=qjobs[pick], coeff=view(outs["coeff"], np.int32, npk), quant_rows=rows, iqmatrix=None, lam=LAMBDA, sharpness=0,
                    eob_fast_inter=0, eob_fast_intra=0, eob_th=255, eob_fast_th=255)
        inp = {"qcoeff": view(keep["qcoeff"], np.int32, npk), "dqcoeff": view(keep["dqcoeff"], np.int32, npk), "eob": view(keep["eob"], np.uint16, 1).reshape(-1)}
        want = rq.run_case(T, case, inp, False)
        got_q, got_eob = view(outs["qcoeff"], np.int32, npk), view(outs["eob"], np.uint16, 1).reshape(-1)
        if not (np.array_equal(got_q, want["qcoeff"]) and np.array_equal(got_eob, want["eob"]) and np.array_equal(view(outs["dqcoeff"], np.int32, npk), want["dqcoeff"])
                and np.array_equal(view(outs["dist_coeff"], np.uint64, 2), want["dist_coeff"]) and np.array_equal(t_cul.cpu().numpy()[pick], want["cul_level"])):
            raise SystemExit(f"tx_size {ts}: the device's RDOQ results differ from the restatement")
        eob_in, eob_out = keep["eob"].cpu().numpy().view(np.uint16), outs["eob"].cpu().numpy().view(np.uint16)
        res = dict(tx=f"{abi.TX_W[ts]}x{abi.TX_H[ts]}", jobs=n, coeffs_per_job=npk, mean_eob_in=round(float(eob_in.mean()), 1), mean_eob_out=round(float(eob_out.mean()), 1),
                   sample_jobs_changed=int(np.count_nonzero((got_q != inp["qcoeff"]).any(axis=1))), rd_ms_median=round(rd_ms, 4), rd_ms_min=round(rd_min, 4),
                   rdoq_ms_median=round(rdoq_ms, 4), rdoq_ms_min=round(rdoq_min, 4), rate_ms_median=round(rate_ms, 4), rate_ms_min=round(rate_min, 4),
                   rdoq_over_rd=round(rdoq_ms / rd_ms, 3), download_bytes=n * (npk * 12 + 2), upload_bytes=n * (npk * 8 + 2))
        results.append(res)
        perf_common.emit(res)
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
