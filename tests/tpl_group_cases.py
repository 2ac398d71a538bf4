"""A readable restatement of the second half of tpl_mc_flow (Source/Lib/Codec/src_ops_process.c:1783-1956) and of what rate control
reads from it: tpl_mc_flow_synthesizer (:1571-1584, tpl_model_update{,_b} :1480-1565), svt_aom_generate_r0beta (:1585-1677) and
generate_lambda_scaling_factor (:176-223), in C's int64 semantics (wrapping multiply, truncating division; Python floats are IEEE
doubles).  Where the reference is undefined the device's definition is restated: a cell with recrf_dist == 0 propagates nothing; a cell
whose reference resolves to its own frame propagates nothing (only intra cells, which add zero, do that in the reference).

Also the seeded windows shared by the CPU and GPU tests.  A window is a dict: the group geometry, and per frame (decode order) the
picture number, tpl_valid_pic, base_rdmult, the TplStats grid (abi.TPL_STATS_DTYPE, a few canary cells past the reference's
allocation) and the r0 value the frame's r0 holds before stage 3.  The synthetic grids hold what result_model_store can produce: all
four dist / rate fields >= 1 and recrf >= srcrf; their MVs are not multiples of 8 and reach off the picture on every side."""
import hashlib
import os

import numpy as np

from svt_av1_psyex_amd import abi

M64 = 1 << 64
RDDIV_BITS, AV1_PROB_COST_SHIFT = 7, 9
CANARY = 4  # cells past the reference's allocation, filled with CANARY_BYTE
CANARY_BYTE = 0xA5
STAGES_SYNTH_R0 = abi.TPL_STAGE_SYNTHESIZE | abi.TPL_STAGE_R0BETA
STAGES_ALL = abi.TPL_STAGE_DISPENSE | STAGES_SYNTH_R0


def s64(v):
    v &= M64 - 1
    return v - M64 if v >> 63 else v


def tdiv(a, b):
    """C's int64 division (truncation toward zero); b == -1 wraps like the device's."""
    q = abs(a) // abs(b)
    return s64(q if (a < 0) == (b < 0) else -q)


def rdcost(rm, r, d):  # RDCOST (Codec/rd_cost.h:37-39)
    return s64((s64(s64(r * rm) + ((1 << AV1_PROB_COST_SHIFT) >> 1)) >> AV1_PROB_COST_SHIFT) + s64(d << RDDIV_BITS))


def mv_rawpel(x):  # GET_MV_RAWPEL (block_structures.h:41)
    return (x + 3 + (1 if x >= 0 else 0)) >> 3


def round_floor(x, b):  # :1440-1448
    return -(1 + (-x - 1) // b) if x < 0 else x // b


def overlap_area(gr, gc, rr, rc, block, b):  # get_overlap_area (:1411-1438)
    w = rc + b - gc if block & 1 else gc + b - rc
    h = rr + b - gr if block >> 1 else gr + b - rr
    return w * h


def cdiv(a, b):
    return (a + b - 1) // b


def geometry(win):
    s = win["synth"]
    shift = 2 if s == 16 else 3
    aw, ah, W, H = win["aligned_width"], win["aligned_height"], win["width"], win["height"]
    return dict(s=s, shift=shift, n=1 << shift, mi_rows=ah >> 2, mi_cols=aw >> 2, stride_a=(((aw + 15) // 16) << 2) >> shift,
                mi_cols_sr=((W + 15) // 16) << 2, mi_rows_u=((H + 15) // 16) << 2, alloc=cdiv(W, s) * cdiv(H, s),
                dispenser_stride=cdiv(aw, s), cells=max(cdiv(W, s) * cdiv(H, s), cdiv(aw, s) * cdiv(ah, s)))


def stride_alias(win):
    """synth 32 with ceil(aligned_width / 16) odd: the synthesizer's row stride is one cell shorter than the dispenser's."""
    g = geometry(win)
    return g["stride_a"] != g["dispenser_stride"]


def n_beta(win):
    return cdiv(win["aligned_width"], win["sb_size"]) * cdiv(win["aligned_height"], win["sb_size"])


def n_scaling(win):
    g = geometry(win)
    return cdiv(g["mi_cols_sr"], g["n"]) * cdiv(g["mi_rows"], g["n"])


# ---------------------------------------------------------------------------------------------------------------------------
def synthesize(win, grids, stats=None):
    """tpl_mc_flow_synthesizer for f = n-1 .. 0 with tpl_valid_pic, on copies of `grids`; returns them.  stats (a dict) counts what
    the walk met: clipped quadrants, out-of-window references, negative reference positions, skipped cells."""
    g = geometry(win)
    S, shift, stride = g["s"], g["shift"], g["stride_a"]
    pix_num = S * S
    frames = win["frames"]
    pocs = [f["poc"] for f in frames]
    cols = {k: [grid[k].tolist() for grid in grids] for k in ("srcrf_dist", "recrf_dist", "srcrf_rate", "recrf_rate", "mc_dep_rate",
                                                             "mc_dep_dist", "mv_row", "mv_col", "ref_frame_poc")}
    st = stats if stats is not None else {}
    for k in ("clipped", "outside", "negative", "self", "zero_recrf", "propagated", "aliased"):
        st.setdefault(k, 0)
    for f in reversed(range(len(frames))):
        if not frames[f]["valid"]:
            continue
        for mi_row in range(0, g["mi_rows"], g["n"]):
            for mi_col in range(0, g["mi_cols"], g["n"]):
                idx = (mi_row >> shift) * stride + (mi_col >> shift)
                if (mi_col >> shift) == cdiv(g["mi_cols"], g["n"]) - 1 and stride < g["dispenser_stride"]:
                    st["aliased"] += 1
                poc = cols["ref_frame_poc"][f][idx]
                i = pocs.index(poc) if poc in pocs else None  # the FIRST frame of the window with that picture number
                if i is None:
                    st["outside"] += 1
                    continue
                recrf, srcrf = cols["recrf_dist"][f][idx], cols["srcrf_dist"][f][idx]
                if i == f:
                    st["self"] += 1
                    continue
                if recrf == 0:
                    st["zero_recrf"] += 1
                    continue
                ref_r = mi_row * 4 + mv_rawpel(cols["mv_row"][f][idx])
                ref_c = mi_col * 4 + mv_rawpel(cols["mv_col"][f][idx])
                if ref_r < 0 or ref_c < 0:
                    st["negative"] += 1
                base_r, base_c = round_floor(ref_r, S) * S, round_floor(ref_c, S) * S
                cur_dep = s64(recrf - srcrf)
                mc_dep = tdiv(s64(cols["mc_dep_dist"][f][idx] * cur_dep), recrf)
                dist = s64(cur_dep + mc_dep)
                rate = s64(cols["recrf_rate"][f][idx] - cols["srcrf_rate"][f][idx])
                for block in range(4):
                    gr, gc = base_r + S * (block >> 1), base_c + S * (block & 1)
                    if not (0 <= gr < g["mi_rows"] * 4 and 0 <= gc < g["mi_cols"] * 4):  # the reference frame's aligned size
                        st["clipped"] += 1
                        continue
                    area = overlap_area(gr, gc, ref_r, ref_c, block, S)
                    t = (gr // S) * stride + gc // S
                    cols["mc_dep_dist"][i][t] = s64(cols["mc_dep_dist"][i][t] + tdiv(s64(dist * area), pix_num))
                    cols["mc_dep_rate"][i][t] = s64(cols["mc_dep_rate"][i][t] + tdiv(s64(rate * area), pix_num))
                    st["propagated"] += 1
    out = [grid.copy() for grid in grids]
    for f, grid in enumerate(out):
        grid["mc_dep_dist"] = np.array(cols["mc_dep_dist"][f], np.int64)
        grid["mc_dep_rate"] = np.array(cols["mc_dep_rate"][f], np.int64)
    return out


def r0beta(win, grid, base_rdmult, r0_in, stats=None):
    """svt_aom_generate_r0beta + generate_lambda_scaling_factor of one frame: (r0, tpl_is_valid, beta[], scaling[])."""
    g = geometry(win)
    shift, step, mi_cols_sr = g["shift"], g["n"], g["mi_cols_sr"]
    stride = mi_cols_sr >> shift
    rec = grid["recrf_dist"].tolist()
    delta = [rdcost(base_rdmult, r, d) for r, d in zip(grid["mc_dep_rate"].tolist(), grid["mc_dep_dist"].tolist())]
    rsum = dsum = count = max_dist = 0
    for row in range(0, g["mi_rows"], step):
        for col in range(0, mi_cols_sr, step):
            i = (row >> shift) * stride + (col >> shift)
            rsum, dsum, count = s64(rsum + rec[i]), s64(dsum + delta[i]), count + 1
            max_dist = max(max_dist, delta[i])
    cost = s64(s64(rsum << RDDIV_BITS) + dsum)
    r0, valid, outlier = r0_in, 0, False
    if cost != 0:
        r0 = float(s64(rsum << RDDIV_BITS)) / float(cost)
        if max_dist > s64(tdiv(dsum, count) * 100) and max_dist > tdiv(s64(dsum * 9), 10):
            r0, outlier = 1.0, True
        valid = 1
    if stats is not None:
        stats.update(cost=cost, outlier=outlier)
    num_cols, num_rows = cdiv(mi_cols_sr, step), cdiv(g["mi_rows"], step)
    scaling = []
    for row in range(num_rows):
        for col in range(num_cols):
            i = row * stride + col
            sf = 1.2
            if cost and rec[i] > 0:
                num = s64(rec[i] << RDDIV_BITS)
                sf += (float(num) / float(s64(num + delta[i]))) / r0
            scaling.append(sf)
    sb = win["sb_size"]
    sb_mi, sb_w, sb_h = sb >> 2, cdiv(win["aligned_width"], sb), cdiv(win["aligned_height"], sb)
    beta = []
    for sy in range(sb_h):
        for sx in range(sb_w):
            mi_row, mi_col = sy * sb >> 2, sx * sb >> 2
            rs = ds = 0
            for row in range(mi_row, mi_row + sb_mi, step):
                for col in range(mi_col, mi_col + sb_mi, step):
                    if row >= g["mi_rows_u"] or col >= mi_cols_sr:
                        continue
                    i = (row >> shift) * stride + (col >> shift)
                    rs, ds = s64(rs + rec[i]), s64(ds + delta[i])
            b = 1.0
            if rs > 0:
                num = s64(rs << RDDIV_BITS)
                b = r0 / (float(num) / float(s64(num + ds)))
            beta.append(b)
    return r0, valid, np.array(beta, np.float64), np.array(scaling, np.float64)


def restate(win, stages=STAGES_SYNTH_R0, grids=None):
    """The stages on a window whose grids are already dispensed (`grids`, default the window's): (grids, [(r0, valid, beta, scaling)
    per frame that supplies outputs, else None])."""
    grids = [f["grid"] for f in win["frames"]] if grids is None else grids
    if stages & abi.TPL_STAGE_SYNTHESIZE:
        grids = synthesize(win, grids)
    outs = [None] * len(grids)
    if stages & abi.TPL_STAGE_R0BETA:
        outs = [r0beta(win, grids[i], f["base_rdmult"], f["r0"]) if f["outputs"] else None for i, f in enumerate(win["frames"])]
    return grids, outs


# ---------------------------------------------------------------------------------------------------------------------------
def synthetic_window(seed, W, H, synth=16, sb=64, pocs=(16, 8, 4, 12), valid=None, aw=None, ah=None, outside=(999, 1), kind="synth",
                     intra_frac=0.2, mv_cells=3, outputs=None):
    """Seeded grids as a dispenser would leave them (mc_dep fields 0), except kind "outlier" (one cell carries most of the propagation)
    and "cost_zero" (mc_dep_dist summing to minus the recrf_dist sum: mc_dep_cost_base == 0), which are inputs of stage 3 alone."""
    rng = np.random.default_rng(seed)
    aw = aw or (W + 7) & ~7
    ah = ah or (H + 7) & ~7
    n = len(pocs)
    win = dict(width=W, height=H, aligned_width=aw, aligned_height=ah, synth=synth, sb_size=sb, frames=[], seed=seed, kind=kind)
    g = geometry(win)
    alloc = g["cells"]  # the reference's allocation, or the dispenser's grid when the aligned size reaches a further synth cell
    for f in range(n):
        grid = np.zeros(alloc + CANARY, abi.TPL_STATS_DTYPE)
        grid.view(np.uint8).reshape(len(grid), -1)[alloc:] = CANARY_BYTE
        c = grid[:alloc]
        src = rng.integers(1, 1 << 22, alloc)
        c["srcrf_dist"] = src
        c["recrf_dist"] = src + rng.integers(0, 1 << 22, alloc)
        sr = rng.integers(1, 1 << 12, alloc)
        c["srcrf_rate"] = sr
        c["recrf_rate"] = sr + rng.integers(0, 1 << 12, alloc)
        amp = 8 * mv_cells * synth  # off the picture on every side
        c["mv_row"] = rng.integers(-amp, amp + 1, alloc)
        c["mv_col"] = rng.integers(-amp, amp + 1, alloc)
        others = [p for i, p in enumerate(pocs) if i != f and p != pocs[f]] + list(outside)
        c["ref_frame_poc"] = rng.choice(others, alloc)
        intra = rng.random(alloc) < intra_frac  # intra cells: ref_frame_poc 0, no MV, recrf == srcrf, equal rates
        c["ref_frame_poc"][intra] = 0
        c["mv_row"][intra] = c["mv_col"][intra] = 0
        c["recrf_dist"][intra] = c["srcrf_dist"][intra]
        c["recrf_rate"][intra] = c["srcrf_rate"][intra]
        if pocs[f] == 0:  # an inter cell of picture 0 must not name picture 0 (that is only intra)
            assert 0 not in others
        if kind == "outlier":
            c["mc_dep_rate"] = 0
            c["mc_dep_dist"] = rng.integers(0, 4, alloc)
            c["mc_dep_dist"][int(rng.integers(0, alloc))] = 1 << 40
        elif kind == "cost_zero":
            c["mc_dep_rate"] = 0
            e = rng.integers(-1000, 1001, alloc)
            e[-1] -= e.sum()
            c["mc_dep_dist"] = -c["recrf_dist"] + e
        win["frames"].append(dict(poc=int(pocs[f]), valid=1 if valid is None else int(valid[f]), base_rdmult=int(rng.integers(40, 4000)),
                                  grid=grid, r0=0.5 + 0.125 * f, outputs=1 if outputs is None else int(outputs[f])))
    win["stages"] = abi.TPL_STAGE_R0BETA if kind in ("outlier", "cost_zero") else STAGES_SYNTH_R0
    return win


def dispensed_window(seed=320, W=136, H=104, n=4, synth=16, distinct=True):
    """A group for the dispenser stage: tpl_dispenser_cases.make_case pictures 0 .. n-1 in decode order, an I picture first, each
    later picture's list-0 reference the picture before it (its TPL recon the recon-path reference: the sliding window), the last
    picture tpl_valid_pic = 0.  Every block is at least half inside, so no cell stays unwritten (picture 0 is in the window).  With
    distinct False the inter pictures share the planes of one case (a timing window)."""
    from tpl_dispenser_cases import make_case
    win = dict(width=W, height=H, aligned_width=(W + 7) & ~7, aligned_height=(H + 7) & ~7, synth=synth, sb_size=64, frames=[], seed=seed,
               kind="dispensed", stages=STAGES_ALL)
    rng = np.random.default_rng(seed)
    for i in range(n):
        if distinct or i < 2:
            c = make_case(seed + 1 + i, W, H, level=0, sub=0, synth=synth, n_refs=(1, 0))
        else:
            c = dict(win["frames"][1]["case"], refs={k: dict(v) for k, v in win["frames"][1]["case"]["refs"].items()})
        if i == 0:
            c["slice_is_i"] = c["tpl_slice_is_i"] = 1
        else:
            c["refs"][(0, 0)]["poc"] = i - 1
        win["frames"].append(dict(poc=i, valid=int(i < n - 1), base_rdmult=int(rng.integers(40, 4000)), grid=c["tpl_stats"], r0=0.25 * (i + 1),
                                  outputs=1, case=c))
    return win


def restate_dispensed(win, recon_of=None):
    """Stage 1 restated: (grids, recon planes) of a dispensed_window; recon_of(frame index, case) -> the recon-path reference plane
    of the NEXT picture (default: this restatement's)."""
    from tpl_dispenser_cases import restate as restate_dispense
    g = geometry(win)
    grids, recons, prev = [], [], None
    for i, f in enumerate(win["frames"]):
        c = dict(f["case"])
        c["tpl_stats"] = f["grid"].copy()
        c["tpl_stats"][:g["alloc"]].view(np.uint8)[:] = 0  # :1841-1845
        if prev is not None:
            c["refs"] = {k: dict(v) for k, v in c["refs"].items()}
            c["refs"][(0, 0)]["recon"] = prev
        if f["valid"]:
            grid, _, rec = restate_dispense(c)
        else:
            grid, rec = c["tpl_stats"], c["recon"]
        grids.append(grid)
        recons.append(rec)
        prev = rec if recon_of is None else recon_of(i, c)
    return grids, recons


def chained_cases(win, recons):
    """The window's dispenser cases with each picture's list-0 recon-path reference set to the previous picture's TPL recon."""
    out = []
    for i, f in enumerate(win["frames"]):
        c = dict(f["case"])
        if i:
            c["refs"] = {k: dict(v) for k, v in c["refs"].items()}
            c["refs"][(0, 0)]["recon"] = recons[i - 1]
        out.append(c)
    return out


def window_checksum(win):
    """sha256 over every input of a window: geometry, and per frame its number, flags, base_rdmult, r0 and grid (and the dispenser
    case's arrays for a dispensed window)."""
    from tpl_dispenser_cases import input_checksum
    h = hashlib.sha256()
    h.update(np.array([win["width"], win["height"], win["aligned_width"], win["aligned_height"], win["synth"], win["sb_size"], win["stages"]],
                      np.int64).tobytes())
    for f in win["frames"]:
        h.update(np.array([f["poc"], f["valid"], f["base_rdmult"], f["outputs"]], np.int64).tobytes())
        h.update(np.array([f["r0"]], np.float64).tobytes())
        h.update(np.ascontiguousarray(f["grid"]).view(np.uint8).tobytes())
        if "case" in f:
            h.update(input_checksum(f["case"]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------------------
# The reference fixture (tools/gen_tpl_group_golden.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tpl_group.npz")
FIXTURE_WINDOWS = [
    ("s16_sb64", dict(seed=300, W=200, H=136, synth=16, sb=64, pocs=(24, 16, 20, 18, 22))),
    ("s16_sb128_partial", dict(seed=301, W=196, H=130, aw=200, ah=136, synth=16, sb=128, pocs=(8, 4, 6, 5, 7))),
    ("s32_odd_sb64", dict(seed=302, W=200, H=136, synth=32, sb=64, pocs=(40, 32, 36, 34, 38))),    # ceil(200 / 16) = 13: stride alias
    ("s32_even_sb128", dict(seed=303, W=256, H=144, synth=32, sb=128, pocs=(48, 40, 44, 42))),     # ceil(256 / 16) = 16
    ("s32_odd_720", dict(seed=304, W=720, H=104, synth=32, sb=64, pocs=(64, 56, 60))),             # 45 columns of 16, as 720x1280
    ("picture0_in_window", dict(seed=305, W=136, H=104, synth=16, sb=64, pocs=(0, 8, 4, 2, 6), outside=(999,))),
    ("invalid_frame_dup_poc", dict(seed=306, W=152, H=88, synth=16, sb=128, pocs=(32, 24, 28, 24), valid=(1, 1, 0, 1))),
    ("s32_partial_aligned", dict(seed=307, W=226, H=142, aw=232, ah=144, synth=32, sb=128, pocs=(72, 64, 68))),
    ("aligned_past_picture", dict(seed=310, W=184, H=120, aw=208, ah=136, synth=16, sb=64, pocs=(96, 92, 94))),  # quadrants in [W, aw)
    ("outlier_r0", dict(seed=308, W=200, H=136, synth=16, sb=64, pocs=(80, 76), kind="outlier")),
    ("cost_base_zero", dict(seed=309, W=200, H=136, synth=16, sb=64, pocs=(88, 84), kind="cost_zero")),  # every cell read once
]


def fixture_windows():
    """(name, window) of the fixture in order; the last is the dispensed group."""
    for name, kw in FIXTURE_WINDOWS:
        yield name, synthetic_window(**kw)
    yield "dispensed_group", dispensed_window()


def load_fixture():
    z = np.load(GOLDEN)
    out = []
    for i, (name, win) in enumerate(fixture_windows()):
        assert str(z[f"name_{i}"]) == name
        np.testing.assert_array_equal(z[f"checksum_{i}"], window_checksum(win), err_msg=f"{name}: the inputs changed")
        out.append((name, win, {k[:-len(f"_{i}")]: z[k] for k in z.files if k.endswith(f"_{i}") and not k.startswith(("name_", "checksum_"))}))
    return out


def outputs_record(win, grids, outs, full_grids=False):
    """What the fixture stores of a window's result: the propagated fields per frame (the whole grids when stage 1 ran), r0 /
    tpl_is_valid / beta / scaling as uint64 bits (frames without outputs: r0 NaN bits, valid 255, empty beta / scaling)."""
    rec = {}
    if full_grids:
        rec["grids"] = np.stack(grids)
    else:
        rec["mc_dep_dist"] = np.stack([g["mc_dep_dist"] for g in grids])
        rec["mc_dep_rate"] = np.stack([g["mc_dep_rate"] for g in grids])
    if win["stages"] & abi.TPL_STAGE_R0BETA:
        nb, ns = n_beta(win), n_scaling(win)
        r0 = np.full(len(grids), np.nan)
        valid = np.full(len(grids), 255, np.uint8)
        beta = np.zeros((len(grids), nb))
        scaling = np.zeros((len(grids), ns))
        for i, o in enumerate(outs):
            if o is not None:
                r0[i], valid[i], beta[i], scaling[i] = o
        rec.update(r0=r0.view(np.uint64), tpl_is_valid=valid, beta=beta.view(np.uint64), scaling=scaling.view(np.uint64))
    return rec
