"""What the tools/*_perf.py timing tools share: the path preamble, --reps / --out, event timing on the context stream and the quartiles.

A tool keeps what is its own: the workload, the comparisons with the restatements, and the keys and rounding of the lines it prints (the text
files under profiles/ were made from those lines).  quartiles() is pure and checked by tests/test_tools_common.py; the rest needs a GPU."""
import argparse
import json
import os
import statistics
import sys


def repo_paths(*more):
    """Puts the repository's root, its tests/ and the directories `more` of it in front of sys.path; returns the root."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root] + [os.path.join(root, d) for d in ("tests",) + more]
    return root


def arguments(doc, reps, out_help="also write the figures as JSON to this file"):
    """--reps (default `reps`) and --out, parsed; the description is the first line of `doc`."""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--out", default=None, help=out_help)
    return ap.parse_args()


def emit(row):
    """One measurement as one JSON line."""
    print(json.dumps(row), flush=True)


def write_json(path, results):
    """--out for the tools that print JSON lines: all of them as one JSON list; nothing without a path."""
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)


def write_lines(path, lines):
    """--out for the tools that print a table: the lines as they were printed; nothing without a path."""
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed_rounds(ctx, ext, reps, launches, warmup=5):
    """{name: [ms, ...]} of `launches`, a list of (name, callable): `warmup` rounds, then `reps` timed ones.  A round runs every launch once, in the
    given order, each between two events of its own on the context stream (`ext`: that stream as torch's), and waits for its end event."""
    import torch
    ms = {name: [] for name, _ in launches}
    with torch.cuda.stream(ext):
        for _ in range(warmup):
            for _, launch in launches:
                launch()
        ctx.sync()
        for _ in range(reps):
            for name, launch in launches:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
    ctx.sync()
    return ms


def timed(ctx, ext, reps, launch, warmup=5):
    """[ms, ...] of one launch: timed_rounds with that launch alone."""
    return timed_rounds(ctx, ext, reps, [("", launch)], warmup)[""]


def quartiles(ms):
    """median, q1, q3, min and max of a list of times (the quartiles as statistics.quantiles gives them: exclusive method)."""
    q = statistics.quantiles(ms, n=4)
    return dict(median=statistics.median(ms), q1=q[0], q3=q[2], min=min(ms), max=max(ms))
