#!/usr/bin/env python3
"""Times svt_hip_tpl_group over whole TPL groups: 2160p (synth 32) and 1080p (synth 16) windows of 8 and 16 pictures, dispense + synthesize +
r0beta in one call, and the synthesize + r0beta stages alone on the dispensed grids.

The pictures are tests/tpl_group_cases.dispensed_window (tpl_dispenser_cases.make_case pictures, level 4, an I picture first, each picture's TPL
recon the next one's reference, the last picture tpl_valid_pic = 0).  HIP events around each call on the context stream, 2 warm-up calls, median
of --reps, ms per group.  The split into dispense / synthesize / r0beta comes from a kernel trace of the same command
(rocprofv3 --kernel-trace --stats -- python tools/tpl_group_perf.py: tpl_*_kernel of tpl_kernel.hip, tpl_synth_kernel, tpl_r0beta_kernel).
Prints one line per window and stage set (and, with --out, writes the figures as JSON)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "tests")]
from svt_av1_psyex_amd import abi, api, tpl  # noqa: E402
import tpl_group_cases as gc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the figures as JSON to this file")
    a = ap.parse_args()
    import torch
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    results = []
    for (W, H, synth) in ((3840, 2160, 32), (1920, 1080, 16)):
        for n in (8, 16):
            win = gc.dispensed_window(500, W, H, n=n, synth=synth, distinct=False)
            nb, ns = gc.n_beta(win), gc.n_scaling(win)
            t = tpl.upload_window(win, nb, ns)
            torch.cuda.synchronize()
            for what, stages in (("dispense+synthesize+r0beta", gc.STAGES_ALL), ("synthesize+r0beta", gc.STAGES_SYNTH_R0)):
                ms = []
                for i in range(2 + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ext)
                    ctx.check(tpl.enqueue_group(ctx, win, t, stages, nb, ns), "svt_hip_tpl_group")
                    e1.record(ext)
                    e1.synchronize()
                    if i >= 2:
                        ms.append(e0.elapsed_time(e1))
                r = dict(picture=f"{W}x{H}", synth=synth, pictures=n, stages=what, ms=round(statistics.median(ms), 4))
                print(f"{r['picture']} synth {synth} {n:2d} pictures {what:27s}: {r['ms']:.3f} ms / group", flush=True)
                results.append(r)
            del t
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
