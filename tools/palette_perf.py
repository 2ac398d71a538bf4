#!/usr/bin/env python3
"""Times svt_hip_palette_search_batch and svt_hip_palette_pred_batch on a 1920x1088 luma plane tiled with 8x8, 16x16, 32x32 and 64x64 blocks, 8-bit and
10-bit, with 3, 8, 32 and 64 colours per block.

Every block holds exactly that many values, drawn per block and spread over its samples at random (the hardest map for the context model: no
runs), with a cache of six colours of which two are one step from a block value; dominant_color_step 1, the map cost on, no color_maps.  The
prediction batch that follows predicts every candidate the search kept (the job list is built from one read of the results before the timed
rounds; a host that enqueues all 14 slots blindly pays for the refusals as well: not measured).  There is no earlier device path to compare with.
HIP events around each launch on the context stream, 5 warm-up rounds, --reps timed ones, the two launches in alternation: median, quartiles,
minimum, maximum, and the median per job.  Three blocks of every search batch are compared with the restatement of tests/palette_cases.py after
the timed launches.  Prints a table (and, with --out, writes it)."""

import numpy as np

import perf_common

perf_common.repo_paths()
import palette_cases as pc  # noqa: E402
from svt_av1_psyex_amd import abi, api, palette  # noqa: E402

W, H = 1920, 1088


def make_plane(rng, bd, size, k):
    """(plane, jobs): every size x size block with exactly k values of its own"""
    by, bx = H // size, W // size
    n = by * bx
    vals = np.argsort(rng.random((n, 1 << bd)), axis=1)[:, :k]
    idx = rng.integers(0, k, (n, size * size))
    idx[:, :k] = np.arange(k)  # every value at least once
    idx = rng.permuted(idx, axis=1)
    blocks = np.take_along_axis(vals, idx, axis=1).reshape(by, bx, size, size)
    plane = blocks.transpose(0, 2, 1, 3).reshape(H, W).astype(np.uint16 if bd > 8 else np.uint8)
    jobs = np.zeros(n, abi.PALETTE_JOB_DTYPE)
    ys, xs = np.divmod(np.arange(n), bx)
    jobs["src_offset"], jobs["width"], jobs["height"], jobs["rows"], jobs["cols"] = ys * size * W + xs * size, size, size, size, size
    jobs["bsize_ctx"], jobs["mode_ctx"], jobs["n_cache"] = (size * size).bit_length() - 7, np.arange(n) % 3, 6
    cache = np.sort(np.concatenate([np.clip(vals[:, :2] + 1, 0, (1 << bd) - 1), rng.integers(0, 1 << bd, (n, 4))], axis=1), axis=1)
    jobs["color_cache"][:, :6] = cache
    return plane, jobs


def main():
    a = perf_common.arguments(__doc__, 20, "also write the table to this file")
    import torch
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    tables = pc.cost_tables(17)
    t_tab = [dev(tables[k]) for k in ("ycolor", "ysize", "ymode")]
    lines = [f"{'what':<32}{'bits':>5}{'block':>6}{'colours':>8}{'jobs':>8}{'median ms':>11}{'q1':>9}{'q3':>9}{'min':>9}{'max':>9}{'us / job':>10}"]
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        params = dict(pc.PARAMS, cost_bit_depth=bd)
        for size in (8, 16, 32, 64):
            for k in (3, 8, 32, 64):
                rng = np.random.default_rng(1000 * bd + 10 * size + k)
                plane, jobs = make_plane(rng, bd, size, k)
                n = len(jobs)
                t_src, t_jobs = dev(plane), dev(jobs)
                t_res = torch.zeros(n * np.dtype(abi.PALETTE_RESULT_DTYPE).itemsize, dtype=torch.uint8, device="cuda")
                t_st = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")  # a job that never ran would show
                t_dst = torch.zeros(pc.MAX_CANDS * size * size * plane.itemsize * 64, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()

                def search():
                    palette.run_search_device(ctx, bd, t_src, W, t_jobs, n, t_tab, t_res, t_st, params)

                search()
                ctx.sync()
                res = t_res.cpu().numpy().view(abi.PALETTE_RESULT_DTYPE)
                # every kept candidate's prediction; the destinations cycle through a buffer of 64 x 14 blocks (the stores are what is timed)
                pj = np.array([(i, q, ((i % 64) * pc.MAX_CANDS + q) * size * size, 0) for i in range(n) for q in range(int(res[i]["n_cands"]))], abi.PALETTE_PRED_JOB_DTYPE)
                m = len(pj)
                t_pj, t_pst = dev(pj), torch.full((max(1, m),), 0xA5 if m else 0, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()

                def predict():
                    palette.run_pred_device(ctx, bd, t_src, W, t_dst, size, t_jobs, t_res, t_st, n, t_pj, m, t_pst)

                ms = perf_common.timed_rounds(ctx, ext, a.reps, [("svt_hip_palette_search_batch", search), ("svt_hip_palette_pred_batch", predict)])
                t = {k: perf_common.quartiles(v) for k, v in ms.items()}
                if t_st.cpu().numpy().any() or t_pst.cpu().numpy().any():
                    raise SystemExit(f"{bd} {size} {k}: a job reported a status other than 0")
                for what, r in t.items():
                    count = n if what.endswith("search_batch") else m
                    lines.append(f"{what:<32}{bd:>5}{size:>6}{k:>8}{count:>8}{r['median']:>11.4f}{r['q1']:>9.4f}{r['q3']:>9.4f}{r['min']:>9.4f}{r['max']:>9.4f}"
                                 f"{r['median'] * 1e3 / count:>10.3f}")
                    print(lines[-1], flush=True)
                res = t_res.cpu().numpy().view(abi.PALETTE_RESULT_DTYPE)
                for i in np.linspace(0, n - 1, 3).astype(int):
                    want = pc.result_records([pc.restate_job(plane, bd, jobs[i], params, tables)], 0)[0]
                    got = res[i].copy()
                    got["cands"][int(got["n_cands"]):] = want["cands"][int(got["n_cands"]):]  # the records past n_cands are not the kernel's
                    if got.tobytes() != want.tobytes():
                        raise SystemExit(f"{bd} {size} {k}: block {i} differs from the restatement")
    ctx.close()
    perf_common.write_lines(a.out, lines)


if __name__ == "__main__":
    main()
