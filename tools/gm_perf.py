#!/usr/bin/env python3
"""Times the global-motion entries on one picture's work.

  svt_hip_gm_refine_batch          5 refinements, one model type per batch (as compute_global_motion's model loop asks), on the full plane of a
                                   2160p picture with the chess pattern (gm level 3's shape) with 2 and with 4 jobs (references), and at 1920x1080 -- a
                                   1080p picture, and the quarter plane of the 2160p one -- with and without the pattern; and with 0 refinements (the picture SAD, the
                                   first evaluation and two decision launches), so that the cost of a round is the difference over 30 rounds
  svt_hip_gm_correspondence_batch  the 2160p picture, MV_8x8 and MV_16x16, two pairs, on synthetic ME results
HIP events around each batch on the context stream, 5 warm-up batches, the median of --reps (default 20) with the quartiles, minimum and maximum.  Every
job must end with status 0 and two runs must give the same bytes.  Prints one JSON line per measurement (and, with --out, writes them as text)."""
import json

import numpy as np

import perf_common

perf_common.repo_paths()
import gm_cases as gc  # noqa: E402
from svt_av1_psyex_amd import abi, api, gm, warp  # noqa: E402


def ms_fields(ms):
    return {f"ms_{k}": round(v, 4) for k, v in perf_common.quartiles(ms).items()}


def refine_case(ctx, ext, reps, w, h, chess, n_jobs, wmtype, n_refinements):
    import torch
    src, planes = gc.pictures(7, w, h, pad=16)
    planes = (planes[:2] * 2)[:n_jobs]  # the moved and the turned picture in turn
    start = {gc.TRANSLATION: gc.T_NEAR, gc.ROTZOOM: gc.R_NEAR, gc.AFFINE: gc.A_NEAR}[wmtype]
    jobs = np.zeros(n_jobs, abi.GM_REFINE_JOB_DTYPE)
    for i in range(n_jobs):
        jobs[i] = gc.job(start, wmtype, i, params_cost=300)
    t_planes = [api.to_device(p[0]) for p in [src] + planes]
    refs = [warp.plane_ref(t, p[0].shape[1], p[1], p[2], p[3], p[4], p[0].shape[0]) for t, p in zip(t_planes, [src] + planes)]
    t_jobs = api.to_device(jobs)
    sizes = {k: np.dtype(dt).itemsize for k, dt in gm.REFINE_OUT_DTYPES.items()}
    outs = {k: torch.zeros((n_jobs * sz,), dtype=torch.uint8, device="cuda") for k, sz in sizes.items()}
    work = torch.empty((gm.work_bytes(n_jobs),), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = gm.refine_desc(refs[0], refs[1:], n_refinements, chess, 0, t_jobs.data_ptr(), n_jobs, work.data_ptr(), {k: t.data_ptr() for k, t in outs.items()})
    import ctypes as C

    def launch():
        ctx.check(api.lib().svt_hip_gm_refine_batch(ctx._h, C.byref(d)), "svt_hip_gm_refine_batch")
    launch()
    ctx.sync()
    first = {k: t.cpu().numpy().copy() for k, t in outs.items()}
    assert not first["status"].any(), first["status"]
    r = ms_fields(perf_common.timed(ctx, ext, reps, launch))
    assert all(np.array_equal(first[k], t.cpu().numpy()) for k, t in outs.items()), "two runs differ"
    best, sad = first["best_error"].view("<i8"), first["pic_sad"].view("<u4")
    r.update(what="gm_refine", picture=f"{w}x{h}", chess=chess, jobs=n_jobs, wmtype=wmtype, refinements=n_refinements, launches=3 + 2 * (6 * n_refinements + 1),
             error_over_pic_sad=[round(float(b) / float(s), 3) for b, s in zip(best, sad)])
    return r


def corr_case(ctx, ext, reps, w, h, method):
    rng = np.random.default_rng(5)
    nb, n_pu, mc, mr = ((w + 63) // 64) * ((h + 63) // 64), 85, 3, 2
    pic = {"aligned_width": w, "aligned_height": h, "enable_me_8x8": 1, "enable_me_16x16": 1, "max_cand": mc, "max_refs": mr, "max_l0": 1}
    cands = np.array([gc.cand_byte(0), gc.cand_byte(1, ref1_list=1), gc.cand_byte(2, ref1_list=1)], np.uint8)
    arrays = {"total_me_candidate_index": rng.integers(0, mc + 1, (nb, n_pu)).astype(np.uint8), "me_candidate_array": np.tile(cands, (nb, n_pu)),
              "me_mv_array": rng.integers(0, 1 << 32, (nb, n_pu * mr), dtype=np.uint64).astype(np.uint32), "rc_me_distortion": rng.integers(0, 1 << 20, (nb, 1)).astype(np.uint32),
              "stationary_block_present_sb": rng.integers(0, 2, (nb, 1)).astype(np.uint8), "rc_me_allow_gm": rng.integers(0, 2, (nb, 1)).astype(np.uint8)}
    me, keep = abi.MeResults(), []
    for name in gm.ME_ARRAYS:
        keep.append(api.to_device(arrays[name]))
        setattr(me, name, keep[-1].data_ptr())
    pairs = [(0, 0), (1, 0)]
    outs = gm.run_gm_correspondence_device(ctx, pic, method, 0, pairs, me)
    ctx.sync()
    cap = outs["corr"].shape[1]
    d = gm.corr_desc(pic, method, 0, pairs, cap, me, outs["corr"].data_ptr(), outs["count"].data_ptr(), outs["sums"].data_ptr())
    import ctypes as C
    r = ms_fields(perf_common.timed(ctx, ext, reps, lambda: ctx.check(api.lib().svt_hip_gm_correspondence_batch(ctx._h, C.byref(d)), "svt_hip_gm_correspondence_batch")))
    r.update(what="gm_correspondence", picture=f"{w}x{h}", method=method, pairs=len(pairs), blocks=cap, kept=outs["count"].cpu().numpy().tolist())
    return r


def main():
    import torch
    a = perf_common.arguments(__doc__, 20)
    ctx = api.Context()
    ext = torch.cuda.ExternalStream(ctx.stream)
    rows = []
    plan = [(3840, 2160, 1, 2, gc.ROTZOOM, 5), (3840, 2160, 1, 4, gc.ROTZOOM, 5), (3840, 2160, 1, 2, gc.ROTZOOM, 0), (3840, 2160, 1, 2, gc.TRANSLATION, 5),
            (3840, 2160, 1, 2, gc.AFFINE, 5), (1920, 1080, 1, 2, gc.ROTZOOM, 5), (1920, 1080, 1, 2, gc.ROTZOOM, 0), (1920, 1080, 0, 2, gc.ROTZOOM, 5),
            (1920, 1080, 0, 2, gc.ROTZOOM, 0)]
    for w, h, chess, n, t, nr in plan:
        rows.append(refine_case(ctx, ext, a.reps, w, h, chess, n, t, nr))
        perf_common.emit(rows[-1])
    for method in (gc.MV_8x8, gc.MV_16x16):
        rows.append(corr_case(ctx, ext, a.reps, 3840, 2160, method))
        perf_common.emit(rows[-1])
    ctx.close()
    perf_common.write_lines(a.out, [json.dumps(r) for r in rows])


if __name__ == "__main__":
    main()
