#!/usr/bin/env python3
"""Times svt_hip_ifs_batch on a 2160p luma plane tiled with 16x16, 32x32 and 64x64 blocks, 8-bit and 10-bit, psy on and off.

Every block is a single-reference candidate with the MV (13, -11) / 8: both phases non-zero, so all nine pairs are distinct predictions on the
8-tap 2-D path; dual filter on, the Laplacian model on, subsampled distortion off, the winner's luma written to the prediction plane.  The
yardstick, which exists without this feature, is the same search composed from the entries the library already had: nine launches of
svt_hip_inter_pred_batch (one per pair, into one prediction plane), each followed by a launch of svt_hip_block_stats_batch for the SSE (and the psy
distortion when psy is on) of every block -- 18 launches, and the cost and the choice still to be made on the host.  Both are measured in the same
process, a fused launch and a composed search in alternation: HIP events around each on the context stream, 5 warm-up rounds, --reps timed ones:
median, quartiles, minimum, maximum.  Four blocks of every fused batch are compared with the restatement of tests/ifs_cases.py after the timed
launches, and the composed search's SSE / psy columns of those blocks with the same restatement.  Prints a table (and, with --out, writes it)."""
import ctypes as C

import numpy as np

import perf_common

perf_common.repo_paths()
import ifs_cases as ic  # noqa: E402
from svt_av1_psyex_amd import abi, api, ifs, pred  # noqa: E402

W, H, PAD = 3840, 2160, 160
MV = (13, -11)


def make_jobs(size):
    ys, xs = np.meshgrid(np.arange(0, H - size + 1, size), np.arange(0, W - size + 1, size), indexing="ij")
    n = ys.size
    j = np.zeros(n, abi.IFS_JOB_DTYPE)
    p = j["pred"]
    p["dst_offset"], p["org_x"], p["org_y"], p["width"], p["height"] = ys.ravel() * W + xs.ravel(), xs.ravel(), ys.ravel(), size, size
    p["ref"][:, 1], p["mv"][:, 0] = abi.INTER_PRED_NO_REF, MV
    p["mb_to_left_edge"], p["mb_to_right_edge"] = -(xs.ravel() * 8), (W - size - xs.ravel()) * 8
    p["mb_to_top_edge"], p["mb_to_bottom_edge"] = -(ys.ravel() * 8), (H - size - ys.ravel()) * 8
    j["src_offset"] = p["dst_offset"]
    j["pred_ctx"][:, 0], j["pred_ctx"][:, 1] = np.arange(n) % 4, 8 + (np.arange(n) // 4) % 4
    s = np.zeros(n, abi.BLOCK_JOB_DTYPE)
    s["src_offset"], s["ref_offset"], s["width"], s["height"] = p["dst_offset"], p["dst_offset"], size, size
    return j, s


def main():
    a = perf_common.arguments(__doc__, 30, "also write the table to this file")
    import torch
    L = api.lib()
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    fac = ic.fac_table("random")
    t_fac = dev(fac)
    lines = [f"{'what':<44}{'bits':>5}{'psy':>5}{'block':>6}{'jobs':>8}{'median':>9}{'q1':>9}{'q3':>9}{'min':>9}{'max':>9}{'ns / sample':>13}"]
    ratios = []
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        rng = np.random.default_rng(16 + bd)
        plane = rng.integers(0, 1 << bd, (H + 2 * PAD, W + 2 * PAD)).astype(dt)
        # the source: the reference half a sample away plus noise, so that the costs differ between the pairs
        src = np.clip((plane[PAD + 1:PAD + 1 + H, PAD - 1:PAD - 1 + W].astype(np.int32) + plane[PAD + 2:PAD + 2 + H, PAD - 2:PAD - 2 + W]) // 2
                      + rng.integers(-6, 7, (H, W)), 0, (1 << bd) - 1).astype(dt)
        t_plane, t_src = dev(plane), dev(src)
        refs = [pred.plane_ref(t_plane, W + 2 * PAD, PAD, PAD, W + 2 * PAD, H + 2 * PAD)]
        t_dst, t_tmp = (torch.zeros(H * W * plane.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
        for psy in (0.0, 1.35):
            params = dict(ic.PARAMS, psy_rd=psy, quantizer=400 << (bd - 8))
            for size in (16, 32, 64):
                jobs, sjobs = make_jobs(size)
                n = len(jobs)
                t_jobs, t_sjobs = dev(jobs), dev(sjobs)
                pj = []
                for yf, xf in ic.FILTER_SETS:
                    q = jobs["pred"].copy()
                    q["filter_y"], q["filter_x"] = yf, xf
                    pj.append(dev(q))
                t_res, t_st = torch.zeros(n * 24, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
                t_rd, t_sse = (torch.zeros(n * 72, dtype=torch.uint8, device="cuda") for _ in range(2))
                c_sse, c_psy = (torch.zeros(9 * n * 8, dtype=torch.uint8, device="cuda") for _ in range(2))
                descs = []
                for k in range(9):
                    d = abi.BlockStatsDesc(bit_depth=bd, n_jobs=n, src_stride=W, ref_stride=W, src=t_src.data_ptr(), ref=t_tmp.data_ptr(), jobs=t_sjobs.data_ptr(),
                                           sse=c_sse.data_ptr() + 8 * n * k)
                    if psy > 0:
                        d.psy_rd, d.psy_dist = psy, c_psy.data_ptr() + 8 * n * k
                    descs.append(d)
                torch.cuda.synchronize()

                def fused():
                    ifs.run_ifs_device(ctx, bd, refs, t_src, W, t_jobs, n, t_fac, t_res, t_st, params, dst=t_dst, dst_stride=W, rd=t_rd, sse=t_sse)

                def composed():
                    for k in range(9):
                        pred.run_inter_pred_device(ctx, bd, 0, 0, refs, t_tmp, W, pj[k], n, t_st)
                        ctx.check(L.svt_hip_block_stats_batch(ctx._h, C.byref(descs[k])), "svt_hip_block_stats_batch")

                ms = perf_common.timed_rounds(ctx, ext, a.reps, [("svt_hip_ifs_batch", fused), ("9 x (inter_pred + block_stats)", composed)])
                t = {k: perf_common.quartiles(v) for k, v in ms.items()}
                if t_st.cpu().numpy().any():
                    raise SystemExit(f"{bd} {size}: a job reported a status other than 0")
                for what, r in t.items():
                    lines.append(f"{what:<44}{bd:>5}{'on' if psy else 'off':>5}{size:>6}{n:>8}{r['median']:>9.4f}{r['q1']:>9.4f}{r['q3']:>9.4f}{r['min']:>9.4f}{r['max']:>9.4f}"
                                 f"{r['median'] * 1e6 / (n * size * size):>13.4f}")
                    print(lines[-1], flush=True)
                ratios.append(f"{bd}-bit psy {'on' if psy else 'off'} {size}x{size} {t['svt_hip_ifs_batch']['median'] / t['9 x (inter_pred + block_stats)']['median']:.2f}")
                # a sample of the blocks against the restatement
                res = t_res.cpu().numpy().view(abi.IFS_RESULT_DTYPE)
                rd, sse = (x.cpu().numpy().view(np.uint64).reshape(n, 9) for x in (t_rd, t_sse))
                got = t_dst.cpu().numpy().view(dt).reshape(H, W)
                cs, cp = (x.cpu().numpy().view(np.uint64).reshape(9, n) for x in (c_sse, c_psy))
                for i in np.linspace(0, n - 1, 4).astype(int):
                    want = ic.restate_job([(plane, PAD, PAD)], src, bd, jobs[i], params, fac)
                    y, x = divmod(int(jobs[i]["src_offset"]), W)
                    ok = (np.array_equal(rd[i], want["rd"]) and np.array_equal(sse[i], want["sse"]) and int(res[i]["winner"]) == want["winner"]
                          and int(res[i]["best_rd"]) == want["best_rd"] and np.array_equal(got[y:y + size, x:x + size], want["pred"]))
                    if not ok:
                        raise SystemExit(f"{bd} {size}: block {i} of the fused batch differs from the restatement")
                    if not np.array_equal(cs[:, i] + (cp[:, i] if psy else 0), want["sse"]):
                        raise SystemExit(f"{bd} {size}: block {i} of the composed search differs from the restatement")
    lines += ["", "fused / composed (medians):"] + ["   " + "   ".join(ratios[k:k + 3]) for k in range(0, len(ratios), 3)]
    print("\n".join(lines[-6:]), flush=True)
    ctx.close()
    perf_common.write_lines(a.out, lines)


if __name__ == "__main__":
    main()
