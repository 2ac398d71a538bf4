#!/usr/bin/env python3
"""Times the warped-motion entries on one 2160p picture, beside the translational predictor and a device-to-device copy.

Per block size (8x8, 16x16, 32x32, 64x64; one size per batch, the luma plane tiled with it):
  svt_hip_warp_pred_batch    10-bit luma, single reference, every job its own AFFINE model; and the averaged compound of two references
  svt_hip_inter_pred_batch   the yardstick that exists without this feature: the same block list, single reference, EIGHTTAP_REGULAR on both axes
                             with a fractional MV on both (the 8-tap 2-D path)
  device_to_device_copy      torch's copy_ of as many bytes as the prediction batch writes, on the same stream
and once: svt_hip_warp_model_batch on one fit per 8x8 block, and svt_hip_wm_refine_batch (8-bit luma, 16x16 and 64x64 blocks) at 8 iterations without
diagonals and at 16 with, each with one wave and with four waves per job.  HIP events around each launch on the context stream, 5 warm-up launches,
the median of --reps with the quartiles, minimum and maximum.  A sample of the jobs of every warp batch is compared with the restatement of
tests/warp_cases.py.  Prints one JSON line per measurement (and, with --out, writes them as JSON)."""
import ctypes as C

import numpy as np

import perf_common

perf_common.repo_paths()
import warp_cases as wc  # noqa: E402
from svt_av1_psyex_amd import abi, api, pred, warp  # noqa: E402

LW, LH, PAD = 3840, 2160, 80


def ms_fields(ms):
    return {f"ms_{k}": round(v, 4) for k, v in perf_common.quartiles(ms).items()}


def grid(size):
    ys, xs = np.meshgrid(np.arange(0, LH - size + 1, size), np.arange(0, LW - size + 1, size), indexing="ij")
    return xs.ravel(), ys.ravel()


def random_models(rng, n):
    """n AFFINE models near the identity that svt_get_shear_params accepts, a few dozen distinct ones repeated"""
    pool = [wc.random_model(rng, LW, LH, 1500, wc.AFFINE, span=3) for _ in range(64)]
    return wc.pack_jobs(pool, wc.MODEL_DTYPE)[np.arange(n) % 64]


def warp_jobs(size, models, compound):
    xs, ys = grid(size)
    jobs = np.zeros(len(xs), abi.WARP_PRED_JOB_DTYPE)
    jobs["dst_offset"] = (ys * LW + xs).astype(np.uint32)
    jobs["p_col"], jobs["p_row"], jobs["width"], jobs["height"] = xs, ys, size, size
    jobs["ref"][:, 0], jobs["ref"][:, 1] = 0, (1 if compound else abi.WARP_NO_REF)
    jobs["model"][:, 0] = models[:len(xs)]
    jobs["model"][:, 1] = models[:len(xs)][::-1]
    return jobs


def inter_jobs(size):
    xs, ys = grid(size)
    jobs = np.zeros(len(xs), abi.INTER_PRED_JOB_DTYPE)
    jobs["dst_offset"] = (ys * LW + xs).astype(np.uint32)
    jobs["org_x"], jobs["org_y"], jobs["width"], jobs["height"] = xs, ys, size, size
    jobs["ref"][:, 0], jobs["ref"][:, 1] = 0, abi.INTER_PRED_NO_REF
    jobs["mv"][:, 0, 0], jobs["mv"][:, 0, 1] = 13, -11  # (row, col) in 1/8: fractional on both axes
    jobs["mb_to_left_edge"], jobs["mb_to_right_edge"] = -(xs * 8), (LW - xs - size) * 8
    jobs["mb_to_top_edge"], jobs["mb_to_bottom_edge"] = -(ys * 8), (LH - ys - size) * 8
    return jobs


def main():
    a = perf_common.arguments(__doc__, 30)
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    rng = np.random.default_rng(12)
    planes = [rng.integers(0, 1024, (LH + 2 * PAD, LW + 2 * PAD)).astype(np.uint16) for _ in range(2)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    t_planes = [dev(p) for p in planes]
    stride, rows = LW + 2 * PAD, LH + 2 * PAD
    wrefs = [warp.plane_ref(t, stride, PAD, PAD, LW, LH, rows) for t in t_planes]
    irefs = [pred.plane_ref(t, stride, PAD, PAD, stride, rows) for t in t_planes]
    t_dst = torch.zeros(LW * LH * 2, dtype=torch.uint8, device="cuda")
    results = []

    def report(**kw):
        perf_common.emit(kw)
        results.append(kw)

    for size in (8, 16, 32, 64):
        n = len(grid(size)[0])
        models = random_models(rng, n)
        t_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        medians = {}
        for what in ("warp_single", "warp_compound", "inter_pred"):
            if what == "inter_pred":
                jobs = inter_jobs(size)
                t_jobs = dev(jobs)
                torch.cuda.synchronize()
                d = pred.run_inter_pred_device(ctx, 10, 0, 0, irefs[:1], t_dst, LW, t_jobs, n, t_status)
                t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_inter_pred_batch(ctx._h, C.byref(d)), "svt_hip_inter_pred_batch")))
            else:
                jobs = warp_jobs(size, models, what == "warp_compound")
                t_jobs = dev(jobs)
                torch.cuda.synchronize()
                d = warp.run_warp_pred_device(ctx, 10, 0, 0, wrefs, t_dst, LW, t_jobs, n, t_status)
                t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_warp_pred_batch(ctx._h, C.byref(d)), "svt_hip_warp_pred_batch")))
                got = t_dst.cpu().numpy().view(np.uint16).reshape(LH, LW)
                b = dict(bit_depth=10, ss_x=0, ss_y=0, planes=[(p, PAD, PAD, LW, LH) for p in planes], dst_shape=(LH, LW), dst_stride=LW)
                for i in np.linspace(0, n - 1, 6).astype(int):  # a sample of the jobs against the restatement
                    st, ms = wc.job_status(b, jobs[i])
                    x, y = int(jobs[i]["p_col"]), int(jobs[i]["p_row"])
                    if st != 0 or not np.array_equal(got[y:y + size, x:x + size], wc.warp_block(b, jobs[i], ms)):
                        raise SystemExit(f"{what} {size}x{size}: job {i} differs from the restatement")
            if t_status.cpu().numpy().any():
                raise SystemExit(f"{what} {size}x{size}: a job reported a status other than 0")
            medians[what] = t["ms_median"]
            report(entry=what, block=size, jobs=n, **t, ns_per_sample=round(t["ms_median"] * 1e6 / (n * size * size), 4))
        wr_b = n * size * size * 2
        t_from, t_to = torch.zeros(wr_b, dtype=torch.uint8, device="cuda"), torch.zeros(wr_b, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(ext):
            c = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: t_to.copy_(t_from)))
        report(entry="device_to_device_copy", block=size, bytes=wr_b, **c)
        report(block=size, warp_over_inter_pred=round(medians["warp_single"] / medians["inter_pred"], 2),
               compound_over_single=round(medians["warp_compound"] / medians["warp_single"], 2), warp_over_copy=round(medians["warp_single"] / c["ms_median"], 2))
        del t_from, t_to

    # the fit: one job per 8x8 block of the picture
    xs, ys = grid(8)
    n = len(xs)
    pool = [wc.model_job(rng, 16, 16, 3 + k % 6, ("calm", "mild", "mixed")[k % 3]) for k in range(96)]
    mjobs = wc.pack_jobs(pool, wc.MODEL_JOB_DTYPE)[np.arange(n) % 96]
    mjobs["blk_org_x"], mjobs["blk_org_y"] = xs, ys
    t_mjobs, t_models = dev(mjobs), torch.zeros(n * np.dtype(abi.WARP_MODEL_DTYPE).itemsize, dtype=torch.uint8, device="cuda")
    t_mstatus = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dm = warp.run_warp_model_device(ctx, t_mjobs, n, t_models, t_mstatus, 0, 0, 65535)
    t = ms_fields(perf_common.timed(ctx, ext, a.reps, lambda: ctx.check(L.svt_hip_warp_model_batch(ctx._h, C.byref(dm)), "svt_hip_warp_model_batch")))
    got = t_models.cpu().numpy().view(abi.WARP_MODEL_DTYPE)
    for i in np.linspace(0, n - 1, 50).astype(int):
        if got[i].tobytes() != wc.fit_model(mjobs[i], (int(mjobs[i]["mv"][0]), int(mjobs[i]["mv"][1])), 0, 0, 65535).tobytes():
            raise SystemExit(f"fit {i} differs from the restatement")
    report(entry="svt_hip_warp_model_batch", jobs=n, **t, ns_per_fit=round(t["ms_median"] * 1e6 / n, 2), valid=int(got["valid"].sum()))

    # the refinement: 8-bit luma, the source the reference displaced by (1, -2) samples
    ref8 = (planes[0] >> 2).astype(np.uint8)
    src8 = np.ascontiguousarray(ref8[PAD + 1:PAD + 1 + LH, PAD - 2:PAD - 2 + LW])
    t_ref8, t_src8 = dev(ref8), dev(src8)
    rrefs = [warp.plane_ref(t_ref8, stride, PAD, PAD, LW, LH, rows)]
    tables = wc.cost_tables(rng)
    t_cost = [dev(x) for x in tables]
    for size in (16, 64):
        xs, ys = grid(size)
        n = len(xs)
        pool = [wc.refine_job(rng, 0, 0, size, size, LW, 3 + k % 6, ("calm", "mild", "mixed")[k % 3], (8, -16), (5, -12)) for k in range(96)]
        rjobs = wc.pack_jobs(pool, wc.REFINE_JOB_DTYPE)[np.arange(n) % 96]
        rjobs["blk_org_x"], rjobs["blk_org_y"], rjobs["src_offset"] = xs, ys, (ys * LW + xs).astype(np.uint32)
        t_rjobs = dev(rjobs)
        for iters, diag in ((8, 0), (16, 1)):
            settings = dict(iterations=iters, refine_diag=diag, mv_prec_shift=1, shut_approx=0, lower_band_th=0, upper_band_th=65535, approx_inter_rate=0,
                            error_per_bit=60)
            first = None
            for waves in (1, 4):
                outs = {k: torch.zeros(n * (2 if k == "best_mv" else 1) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
                        for k, dt in warp.REFINE_OUT_DTYPES.items()}
                dsc = warp.refine_desc(n, settings, rrefs, t_src8.data_ptr(), LW, LW * LH, t_rjobs.data_ptr(), {k: v.data_ptr() for k, v in outs.items()}, None, 0,
                                       [x.data_ptr() for x in t_cost], waves)
                torch.cuda.synchronize()
                t = ms_fields(perf_common.timed(ctx, ext, max(5, a.reps // 3), lambda: ctx.check(L.svt_hip_wm_refine_batch(ctx._h, C.byref(dsc)), "svt_hip_wm_refine_batch")))
                got = {k: v.cpu().numpy().view(warp.REFINE_OUT_DTYPES[k]) for k, v in outs.items()}
                if got["status"].any():
                    raise SystemExit("a refinement reported a status other than 0")
                if first is None:
                    first = got
                    b = dict(settings=settings, planes=[(ref8, PAD, PAD, LW, LH)], src=src8, mv_array=None, cost_tables=tables)
                    for i in np.linspace(0, n - 1, 3).astype(int):
                        mv, cost, tot, _ = wc.refine(b, rjobs[i])
                        if (tuple(got["best_mv"].reshape(-1, 2)[i]), int(got["best_cost"][i]), int(got["n_checked"][i])) != (mv, cost, tot):
                            raise SystemExit(f"refinement {i} differs from the restatement")
                elif any(not np.array_equal(first[k], got[k]) for k in got):
                    raise SystemExit("one wave and four waves per job disagree")
                report(entry="svt_hip_wm_refine_batch", block=size, jobs=n, iterations=iters, refine_diag=diag, waves_per_job=waves, **t,
                       positions_per_job=round(float(got["n_checked"].mean()), 1), us_per_job=round(t["ms_median"] * 1e3 / n, 3))
    ctx.close()
    perf_common.write_json(a.out, results)


if __name__ == "__main__":
    main()
