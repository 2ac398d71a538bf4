"""CPU: the TPL group's restatement against the reference fixture (tests/golden/tpl_group.npz, tools/gen_tpl_group_golden.py), the regimes
the windows reach, and the group C-ABI (descriptor sizes, host-side validation)."""
import ctypes as C

import numpy as np
import pytest

from svt_av1_psyex_amd import abi, api, tpl
import tpl_group_cases as gc

FIXTURE = gc.load_fixture()
NAMES = [n for n, _, _ in FIXTURE]


def result(win):
    """The restatement of a fixture window, in the fixture's record layout, and the synthesizer's / r0beta's walk statistics."""
    st, r0st = {}, []
    if win["kind"] == "dispensed":
        grids, _ = gc.restate_dispensed(win)
    else:
        grids = [f["grid"] for f in win["frames"]]
    if win["stages"] & abi.TPL_STAGE_SYNTHESIZE:
        grids = gc.synthesize(win, grids, st)
    outs = []
    for f, g in zip(win["frames"], grids):
        s = {}
        outs.append(gc.r0beta(win, g, f["base_rdmult"], f["r0"], s) if win["stages"] & abi.TPL_STAGE_R0BETA and f["outputs"] else None)
        r0st.append(s)
    return gc.outputs_record(win, grids, outs, full_grids=win["kind"] == "dispensed"), st, r0st


RESULTS = {n: result(w) for n, w, _ in FIXTURE}


@pytest.mark.parametrize("i", range(len(FIXTURE)), ids=NAMES)
def test_restatement_equals_the_reference_fixture(i):
    name, win, want = FIXTURE[i]
    got = RESULTS[name][0]
    assert sorted(got) == sorted(want), name
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")


def test_fixture_windows_reach_their_regimes():
    wins = {n: w for n, w, _ in FIXTURE}
    st = {n: RESULTS[n][1] for n in NAMES}
    synth_windows = [n for n in NAMES if wins[n]["stages"] & abi.TPL_STAGE_SYNTHESIZE and wins[n]["kind"] != "dispensed"]
    for n in synth_windows:  # quadrants clipped at the aligned picture, positions left of / above it, references outside the window
        assert st[n]["clipped"] > 0 and st[n]["negative"] > 0 and st[n]["outside"] > 0 and st[n]["propagated"] > 0, n
        w = wins[n]
        S = w["synth"]
        for f in w["frames"]:
            c = f["grid"][:gc.geometry(w)["alloc"]]
            assert (c["mv_row"] % 8 != 0).any() and (c["mv_col"] % 8 != 0).any(), n
            # off the picture on every side
            g = gc.geometry(w)
            cols = g["dispenser_stride"]
            x = (np.arange(len(c)) % cols) * S + (c["mv_col"] >> 3)
            y = (np.arange(len(c)) // cols) * S + (c["mv_row"] >> 3)
            assert (x < 0).any() and (y < 0).any() and (x + S > w["aligned_width"]).any() and (y + S > w["aligned_height"]).any(), n
            assert (c["recrf_dist"] >= c["srcrf_dist"]).all() and (c["srcrf_dist"] >= 1).all() and (c["srcrf_rate"] >= 1).all()
            assert (c["recrf_rate"] >= c["srcrf_rate"]).all()
    assert {wins[n]["synth"] for n in synth_windows} == {16, 32} and {wins[n]["sb_size"] for n in synth_windows} == {64, 128}
    # synth 32 with ceil(w / 16) odd (the stride alias) and even
    assert st["s32_odd_sb64"]["aliased"] > 0 and st["s32_odd_720"]["aliased"] > 0 and gc.stride_alias(wins["s32_odd_720"])
    assert not gc.stride_alias(wins["s32_even_sb128"])
    for n in ("s16_sb128_partial", "s32_partial_aligned"):  # partial last rows / columns, aligned size above the picture size
        w = wins[n]
        assert w["width"] % w["synth"] and w["height"] % w["synth"] and w["aligned_width"] > w["width"]
    w = wins["aligned_past_picture"]  # a synth cell lies between the picture and the aligned size: the quadrant bound is the aligned one
    assert w["aligned_width"] // w["synth"] > (w["width"] - 1) // w["synth"] and w["aligned_height"] // w["synth"] > (w["height"] - 1) // w["synth"]
    assert st["picture0_in_window"]["self"] > 0  # picture 0's intra cells name picture 0
    w = wins["picture0_in_window"]
    assert w["frames"][0]["poc"] == 0 and any((f["grid"]["ref_frame_poc"] == 0).any() for f in w["frames"][1:])
    w = wins["invalid_frame_dup_poc"]
    assert [f["valid"] for f in w["frames"]].count(0) == 1 and len({f["poc"] for f in w["frames"]}) < len(w["frames"])
    assert any(s.get("outlier") for s in RESULTS["outlier_r0"][2])
    assert all(s["cost"] == 0 for s in RESULTS["cost_base_zero"][2])
    assert all(not s.get("outlier") for n in synth_windows for s in RESULTS[n][2])
    d = wins["dispensed_group"]
    assert d["frames"][0]["case"]["slice_is_i"] and [f["valid"] for f in d["frames"]] == [1, 1, 1, 0]


def test_group_desc_sizes_match_ctypes():
    assert tpl.group_desc_size() == C.sizeof(abi.TplGroupDesc)
    assert tpl.group_frame_size() == C.sizeof(abi.TplGroupFrame)


def fake_group(win, stages=gc.STAGES_SYNTH_R0, n_beta=None, n_scaling=None):
    """A group descriptor of a window with host addresses as stand-ins: svt_hip_tpl_group_check_desc reads no cell."""
    nb, ns = n_beta or gc.n_beta(win), n_scaling or gc.n_scaling(win)
    keep = []
    grids, outs = [], []
    for f in win["frames"]:
        g = f["grid"].copy()
        bufs = (np.zeros(1), np.zeros(1, np.uint8), np.zeros(nb), np.zeros(ns))
        keep += [g, *bufs]
        grids.append((g.ctypes.data, len(g)))
        outs.append((bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, nb, bufs[3].ctypes.data, ns))
    d = tpl.make_group_desc(win, stages, grids, outs)
    d._host = keep
    return d


@pytest.mark.parametrize("i", range(len(FIXTURE) - 1), ids=NAMES[:-1])
def test_group_check_desc_accepts_the_windows(i):
    tpl.group_check_desc(fake_group(FIXTURE[i][1]))


def test_group_check_desc_accepts_the_dispensed_group():
    from test_tpl_dispenser import fake_desc
    win = FIXTURE[-1][1]
    d = fake_group(win, gc.STAGES_ALL)
    disp = []
    for i, f in enumerate(win["frames"]):
        t = fake_desc(f["case"])
        t.tpl_stats = d.frames[i].tpl_stats
        disp.append(t)
        d.frames[i].dispense = C.pointer(t)
    d._disp = disp
    tpl.group_check_desc(d)
    disp[1].tpl_stats = d.frames[2].tpl_stats  # a dispenser descriptor naming another frame's grid
    with pytest.raises(api.SvtHipError):
        tpl.group_check_desc(d)
    disp[1].tpl_stats = d.frames[1].tpl_stats
    disp[1].compute_rate = 1  # the embedded descriptor is checked too
    with pytest.raises(api.SvtHipError):
        tpl.group_check_desc(d)
    disp[1].compute_rate = 0
    d.frames[1].dispense = None  # a valid frame without a dispenser descriptor
    with pytest.raises(api.SvtHipError):
        tpl.group_check_desc(d)


BAD_FIELDS = [("compute_rate", 1), ("synth_blk_size", 8), ("synth_blk_size", 64), ("superres_denom", 16), ("superres_denom", 0), ("sb_size", 32),
              ("sb_size", 0), ("n_frames", 0), ("n_frames", 513), ("stages", 0), ("stages", 8), ("aligned_width", 100), ("width", 0)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_group_check_desc_refuses(field, value):
    d = fake_group(FIXTURE[0][1])
    setattr(d, field, value)
    with pytest.raises(api.SvtHipError):
        tpl.group_check_desc(d)


@pytest.mark.parametrize("what", ["null_grid", "short_grid", "short_beta", "short_scaling", "partial_outputs", "shared_grid", "null_frames",
                                  "short_grid_r0beta_alias"])
def test_group_check_desc_refuses_frames(what):
    win = FIXTURE[2][1] if what == "short_grid_r0beta_alias" else FIXTURE[0][1]
    d = fake_group(win)
    f = d.frames[1]
    alloc = gc.geometry(win)["alloc"]
    if what == "null_grid":
        f.tpl_stats = None
    elif what == "short_grid":
        f.n_tpl_stats = alloc - 1
    elif what == "short_beta":
        f.n_beta = gc.n_beta(win) - 1
    elif what == "short_scaling":
        f.n_scaling = gc.n_scaling(win) - 1
    elif what == "partial_outputs":
        f.r0 = None
    elif what == "shared_grid":
        f.tpl_stats = d.frames[0].tpl_stats + 64
    elif what == "null_frames":
        d.frames = None
    else:  # synth 32, stride alias: the reference's allocation is what every stage reads; one cell less is refused
        f.n_tpl_stats = alloc - 1
    with pytest.raises(api.SvtHipError):
        tpl.group_check_desc(d)


def test_stage3_alone_needs_no_disjoint_grids():
    """r0beta alone only reads the grids: frames sharing one (RC asking twice) are accepted."""
    d = fake_group(FIXTURE[0][1], abi.TPL_STAGE_R0BETA)
    d.frames[1].tpl_stats = d.frames[0].tpl_stats
    tpl.group_check_desc(d)
    d.stages = abi.TPL_STAGE_SYNTHESIZE
    with pytest.raises(api.SvtHipError):
        tpl.group_check_desc(d)
