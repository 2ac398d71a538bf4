"""GPU: svt_hip_tpl_group against the reference fixture (tests/golden/tpl_group.npz) and the restatement of tests/tpl_group_cases.py, bit
for bit: every field of every grid cell, canary cells past the grids, r0 / tpl_is_valid / beta / scaling as bits and the entries past them."""
import ctypes as C

import numpy as np
import pytest

from svt_av1_psyex_amd import abi, api, tpl
import tpl_group_cases as gc

pytestmark = pytest.mark.gpu
FILL64 = np.frombuffer(bytes([tpl.OUT_FILL]) * 8, np.uint64)[0]


def run(ctx, win, stages=None):
    return tpl.run_group_hip(ctx, win, win["stages"] if stages is None else stages, gc.n_beta(win), gc.n_scaling(win))


def assert_group(win, got, grids, outs, what):
    """got: run()'s frames; grids: the expected grids (canaries included); outs: per frame None or (r0, valid, beta, scaling)."""
    nb, ns = gc.n_beta(win), gc.n_scaling(win)
    for i, (g, r0, valid, beta, scaling, _) in enumerate(got):
        w = grids[i]
        for k in w.dtype.names:
            np.testing.assert_array_equal(g[k], w[k], err_msg=f"{what}: frame {i}: {k}")
        assert g.tobytes() == w.tobytes(), f"{what}: frame {i}: grid bytes"
        o = outs[i]
        if o is None:
            assert r0 == win["frames"][i]["r0"] and valid == tpl.OUT_FILL and (beta == FILL64).all() and (scaling == FILL64).all(), what
            continue
        assert np.float64(r0).view(np.uint64) == np.float64(o[0]).view(np.uint64), f"{what}: frame {i}: r0 {r0} != {o[0]}"
        assert valid == o[1], f"{what}: frame {i}: tpl_is_valid"
        np.testing.assert_array_equal(beta[:nb], np.asarray(o[2], np.float64).view(np.uint64), err_msg=f"{what}: frame {i}: beta")
        np.testing.assert_array_equal(scaling[:ns], np.asarray(o[3], np.float64).view(np.uint64), err_msg=f"{what}: frame {i}: scaling")
        assert (beta[nb:] == FILL64).all() and (scaling[ns:] == FILL64).all(), f"{what}: frame {i}: written past beta / scaling"


def from_fixture(win, rec, grids_in):
    """The expected (grids, outs) of a window from its fixture record."""
    if "grids" in rec:
        grids = list(rec["grids"])
    else:
        grids = [g.copy() for g in grids_in]
        for i, g in enumerate(grids):
            g["mc_dep_dist"], g["mc_dep_rate"] = rec["mc_dep_dist"][i], rec["mc_dep_rate"][i]
    outs = [None] * len(grids)
    if "r0" in rec:
        for i, f in enumerate(win["frames"]):
            if f["outputs"]:
                outs[i] = (rec["r0"][i].view(np.float64), int(rec["tpl_is_valid"][i]), rec["beta"][i].view(np.float64), rec["scaling"][i].view(np.float64))
    return grids, outs


FIXTURE = gc.load_fixture()


@pytest.mark.parametrize("i", range(len(FIXTURE) - 1), ids=[n for n, _, _ in FIXTURE[:-1]])
def test_group_vs_reference_fixture(hip_ctx, i):
    name, win, rec = FIXTURE[i]
    grids, outs = from_fixture(win, rec, [f["grid"] for f in win["frames"]])
    got = run(hip_ctx, win)
    assert_group(win, got, grids, outs, name)
    assert_group(win, got, *gc.restate(win, win["stages"]), name + " (restatement)")


def test_dispensed_group_vs_fixture_and_restatement(hip_ctx):
    """Stage 1 + 2 + 3 in one call: the reference's grids and outputs, and the TPL recon planes of the dispenser's restatement."""
    name, win, rec = FIXTURE[-1]
    assert name == "dispensed_group"
    got = run(hip_ctx, win)
    grids, outs = from_fixture(win, rec, None)
    assert_group(win, got, grids, outs, name)
    d_grids, recons = gc.restate_dispensed(win)
    assert_group(win, got, *gc.restate(win, win["stages"], d_grids), name + " (restatement)")
    for i, f in enumerate(win["frames"]):
        want = recons[i]
        np.testing.assert_array_equal(got[i][5].reshape(want.shape), want, err_msg=f"frame {i}: recon")


@pytest.mark.parametrize("W,H,synth,sb", [(720, 1280, 32, 64), (1920, 1080, 16, 128), (3840, 2160, 32, 128)])
def test_large_windows_vs_restatement(hip_ctx, W, H, synth, sb):
    win = gc.synthetic_window(400 + W, W, H, synth=synth, sb=sb, pocs=(64, 32, 16, 8, 24, 48, 40, 56), mv_cells=2)
    if W == 720:
        assert gc.stride_alias(win)
    assert_group(win, run(hip_ctx, win), *gc.restate(win, win["stages"]), f"{W}x{H}")


def test_zero_recrf_cells_propagate_nothing(hip_ctx):
    """The reference's undefined case: cells the dispenser did not write (recrf_dist 0, ref_frame_poc 0) with picture 0 in the window."""
    win = gc.synthetic_window(450, 200, 136, synth=16, pocs=(0, 8, 4, 2), outside=(999,))
    rng = np.random.default_rng(451)
    for f in win["frames"]:
        c = f["grid"][:gc.geometry(win)["alloc"]]
        z = rng.random(len(c)) < 0.2
        for k in ("srcrf_dist", "recrf_dist", "srcrf_rate", "recrf_rate"):
            c[k][z] = 0
        c["ref_frame_poc"][z] = 0
        c["mv_row"][z] = rng.integers(-100, 100, z.sum())
        c["mc_dep_dist"][z] = rng.integers(1, 1000, z.sum())  # would be divided by recrf_dist 0
    st = {}
    gc.synthesize(win, [f["grid"] for f in win["frames"]], st)
    assert st["zero_recrf"] > 0
    assert_group(win, run(hip_ctx, win), *gc.restate(win, win["stages"]), "recrf_dist 0")


def test_cost_base_zero_leaves_r0(hip_ctx):
    name, win, rec = next(x for x in FIXTURE if x[0] == "cost_base_zero")
    got = run(hip_ctx, win)
    for i, f in enumerate(win["frames"]):
        assert got[i][2] == 0 and got[i][1] == f["r0"], f"frame {i}: tpl_is_valid {got[i][2]}, r0 {got[i][1]}"


def test_synthesizer_twice_gives_identical_grids(hip_ctx):
    win = gc.synthetic_window(460, 1920, 1080, synth=16, sb=128, pocs=(32, 16, 8, 24))
    a = run(hip_ctx, win, abi.TPL_STAGE_SYNTHESIZE)
    b = run(hip_ctx, win, abi.TPL_STAGE_SYNTHESIZE)
    for i in range(len(a)):
        assert a[i][0].tobytes() == b[i][0].tobytes(), i


def test_stage3_alone_after_synthesis(hip_ctx):
    """RC's later call: r0beta on its own, on grids the synthesizer left on the device, equals the one-call group."""
    import torch
    win = FIXTURE[0][1]
    nb, ns = gc.n_beta(win), gc.n_scaling(win)
    t = tpl.upload_window(win, nb, ns)
    torch.cuda.synchronize()
    hip_ctx.check(tpl.enqueue_group(hip_ctx, win, t, abi.TPL_STAGE_SYNTHESIZE, nb, ns), "synthesize")
    for i in range(len(win["frames"])):
        one = dict(win, frames=[win["frames"][i]])
        hip_ctx.check(tpl.enqueue_group(hip_ctx, one, dict(frames=[t["frames"][i]]), abi.TPL_STAGE_R0BETA, nb, ns), "r0beta")
    hip_ctx.sync()
    assert_group(win, tpl.download_window(t), *gc.restate(win, win["stages"]), "stage 3 alone")


@pytest.mark.parametrize("field,value", [("compute_rate", 1), ("synth_blk_size", 8), ("superres_denom", 16), ("sb_size", 32), ("n_frames", 0)])
def test_refused_descriptor_writes_nothing(hip_ctx, field, value):
    import torch
    win = FIXTURE[-1][1]  # the dispensed group: stage 1 would write the grids and the recon planes
    nb, ns = gc.n_beta(win), gc.n_scaling(win)
    t = tpl.upload_window(win, nb, ns)
    torch.cuda.synchronize()
    before = tpl.download_window(t)
    rc = tpl.enqueue_group(hip_ctx, win, t, gc.STAGES_ALL, nb, ns, over=lambda d: setattr(d, field, value))
    assert rc == 2  # SVT_HIP_ERR_BAD_PARAM
    hip_ctx.sync()
    after = tpl.download_window(t)
    for x, y in zip(before, after):
        assert x[0].tobytes() == y[0].tobytes() and x[1] == y[1] and x[2] == y[2] and (x[3] == y[3]).all() and (x[4] == y[4]).all()
        assert (x[5] == y[5]).all()


def test_refused_embedded_dispenser_descriptor_writes_nothing(hip_ctx):
    import torch
    win = FIXTURE[-1][1]
    nb, ns = gc.n_beta(win), gc.n_scaling(win)
    t = tpl.upload_window(win, nb, ns)
    torch.cuda.synchronize()
    before = tpl.download_window(t)

    def spoil(d):  # the LAST frame that is dispensed: every frame is checked before the first launch
        d.frames[2].dispense.contents.compute_rate = 1
    assert tpl.enqueue_group(hip_ctx, win, t, gc.STAGES_ALL, nb, ns, over=spoil) == 2
    hip_ctx.sync()
    for x, y in zip(before, tpl.download_window(t)):
        assert x[0].tobytes() == y[0].tobytes() and (x[5] == y[5]).all() and x[1] == y[1]
