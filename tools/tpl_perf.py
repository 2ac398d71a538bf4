#!/usr/bin/env python3
"""Times svt_hip_tpl_dispense (levels 4 / 5) on one 2160p and one 1080p picture: an inter picture with intra enabled, the same picture with
intra disabled (disable_intra_pred), and an I picture (every block through the one-workgroup intra wavefront).

The pictures are the seeded cases of tests/tpl_dispenser_cases.py (level 4: 16x16 blocks, synth 16; level 5: 32x32 blocks, subsample_tx 2,
synth 32).  HIP events around each dispense on the context stream, 3 warm-up dispenses, median of --reps, ms per picture.  The split into
the source, inter-recon, intra-wavefront, padding and grid kernels comes from a kernel trace of the same command
(rocprofv3 --kernel-trace --stats -- python tools/tpl_perf.py).  Prints one line per variant (and, with --out, writes the figures as JSON)."""
import argparse
import json
import os
import statistics
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"),
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests")]
from svt_av1_psyex_amd import api, tpl  # noqa: E402
from tpl_dispenser_cases import PAD, make_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the figures as JSON to this file")
    a = ap.parse_args()
    import torch
    ctx = api.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    results = []
    for (W, H) in ((3840, 2160), (1920, 1080)):
        for level, sub, synth in ((0, 0, 16), (1, 2, 32)):
            for what, kw in (("inter, intra on", {}), ("inter, intra off", dict(disable_intra_pred=1)), ("I picture", dict(slice_is_i=1))):
                c = make_case(7, W, H, level=level, sub=sub, synth=synth, **kw)
                t = tpl.upload_case(c)
                torch.cuda.synchronize()
                ms = []
                for i in range(3 + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ext)
                    tpl.dispense_dev(ctx, c, t, PAD)
                    e1.record(ext)
                    e1.synchronize()
                    if i >= 3:
                        ms.append(e0.elapsed_time(e1))
                r = dict(picture=f"{W}x{H}", level=4 if level == 0 else 5, synth=synth, kind=what, ms=round(statistics.median(ms), 4))
                print(f"{r['picture']} level {r['level']} synth {synth} {what:17s}: {r['ms']:.3f} ms / picture")
                results.append(r)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
