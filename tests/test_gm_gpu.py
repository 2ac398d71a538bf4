"""GPU: svt_hip_gm_refine_batch and svt_hip_gm_correspondence_batch on the MI355X, every comparison exact -- against the restatements
(tests/gm_cases.py) and the reference's own results (golden/gm.npz): every picture size with the chess pattern on and off, 0, 1 and 5 refinements,
the three model types, batches of 1, 2 and 5 jobs that end at different rounds, the error of every evaluation; the correspondences of the four
methods, three PU counts and three shifts.  Outputs start as the byte 0xA5 with spare slots and are compared whole; planes are checked unchanged.
Two chains: the correspondences of an asynchronous ME launch's device-resident results, and a refined ROTZOOM model through
svt_hip_warp_pred_batch."""
import numpy as np
import pytest

import gm_cases as gc
import warp_cases as wc
from svt_av1_psyex_amd import abi, api, gm, warp

pytestmark = pytest.mark.gpu

FILL = gc.FILL
SPARE = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(gc.GOLDEN)


def run_refine(ctx, b):
    out = gm.run_gm_refine_hip(ctx, b["src"], b["planes"], b["n_refinements"], b["chess_refn"], b["rfn_early_exit"], b["jobs"], spare=SPARE, fill=FILL)
    n = len(b["jobs"])
    for k in ("models", "best_error", "pic_sad", "status", "round_error"):
        assert len(out[k]) == n + SPARE and np.all(out[k][n:].view(np.uint8) == FILL), f"spare {k} slots written"
    assert np.array_equal(out["src"], b["src"][0]) and all(np.array_equal(g, p[0]) for g, p in zip(out["planes"], b["planes"])), "a plane changed"
    return {k: out[k][:n] for k in ("models", "best_error", "pic_sad", "status", "round_error")}


@pytest.mark.parametrize("name", gc.batch_names())
def test_refine_batch_equals_the_restatement_and_the_reference(hip_ctx, golden, name):
    """device == restatement on every byte of every output (so what an undefined job leaves untouched is still 0xA5) == the fixture"""
    b = gc.batch(name)
    want, _ = gc.restated(name)
    got = run_refine(hip_ctx, b)
    for k in ("status", "pic_sad", "round_error", "best_error"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k].tolist(), want[k].tolist())
    assert got["models"].tobytes() == want["models"].tobytes(), (name, got["models"], want["models"])
    for key, mine in gc.fixture_arrays(name, got).items():
        assert np.array_equal(mine, golden[key]), key


def test_a_batch_run_twice_gives_identical_bytes(hip_ctx):
    b = gc.batch("mixed_72x44")
    first, second = run_refine(hip_ctx, b), run_refine(hip_ctx, b)
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)


def test_round_error_is_optional(hip_ctx):
    b = gc.batch("one_72x44")
    out = gm.run_gm_refine_hip(hip_ctx, b["src"], b["planes"], b["n_refinements"], b["chess_refn"], b["rfn_early_exit"], b["jobs"], with_round_error=False)
    want, _ = gc.restated("one_72x44")
    assert "round_error" not in out and np.array_equal(out["best_error"], want["best_error"]) and out["models"].tobytes() == want["models"].tobytes()


@pytest.mark.parametrize("name", list(gc.CORR_CASES))
def test_correspondence_batch_equals_the_restatement_and_the_reference(hip_ctx, golden, name):
    c, want = gc.corr_case(name), gc.restated_corr(name)
    got = gm.run_gm_correspondence_hip(hip_ctx, c["pic"], c["method"], c["shift"], c["pairs"], c["arrays"], cap=c["cap"], spare=SPARE, fill=FILL)
    n = len(c["pairs"])
    assert np.all(got["corr"][n:].view(np.uint8) == FILL) and np.all(got["count"][n:].view(np.uint8) == FILL) and np.all(got["sums"][3:].view(np.uint8) == FILL)
    assert np.array_equal(got["count"][:n], want["count"]) and np.array_equal(got["corr"][:n], want["corr"]) and np.array_equal(got["sums"][:3], want["sums"])
    for key, mine in gc.corr_fixture_arrays(name, {"corr": got["corr"][:n], "count": got["count"][:n]}).items():
        assert np.array_equal(mine, golden[key]), key
    again = gm.run_gm_correspondence_hip(hip_ctx, c["pic"], c["method"], c["shift"], c["pairs"], c["arrays"], cap=c["cap"], spare=SPARE, fill=FILL)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_the_sums_alone(hip_ctx):
    c, want = gc.corr_case("m16_b"), gc.restated_corr("m16_b")
    got = gm.run_gm_correspondence_hip(hip_ctx, c["pic"], c["method"], c["shift"], [], c["arrays"], cap=c["cap"], fill=FILL)
    assert np.array_equal(got["sums"], want["sums"]) and np.all(got["corr"].view(np.uint8) == FILL)


def test_correspondences_of_an_asynchronous_me_launch(hip_ctx):
    """the correspondence batch behind svt_hip_me_picture_async on the same stream, reading the result arrays where the launch left them"""
    import torch
    from me_cases import MeCase
    mc = MeCase(352, 288, enc_mode=6)
    cur, refs = hip_ctx.upload(mc.cur), {k: hip_ctx.upload(v) for k, v in mc.refs.items()}
    d = mc.desc
    n_pu, nb = abi.n_pu(d.enable_me_16x16, d.enable_me_8x8), ((d.aligned_width + 63) // 64) * ((d.aligned_height + 63) // 64)
    res, bufs = abi.MeResults(), {}
    for name, dt, cnt in abi.RESULT_FIELDS:
        bufs[name] = torch.zeros(nb * cnt(n_pu, d.max_refs, d.max_cand) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
        setattr(res, name, bufs[name].data_ptr())
    torch.cuda.synchronize()
    pairs = sorted(mc.refs)
    hip_ctx.me_picture_async(mc.cfg, d, cur, refs, res)
    outs = {m: gm.run_gm_correspondence_device(hip_ctx, d, m, s, pairs, res, fill=FILL) for m, s in ((gc.MV_16x16, 0), (gc.MV_8x8, 1))}
    hip_ctx.sync()
    arrays = {name: bufs[name].cpu().numpy().view(dt).reshape(nb, -1) for name, dt, _ in abi.RESULT_FIELDS if name in gc.ME_ARRAYS}
    pic = {k: getattr(d, k) for k in ("aligned_width", "aligned_height", "enable_me_8x8", "enable_me_16x16", "max_cand", "max_refs", "max_l0")}
    for (m, s), got in zip(((gc.MV_16x16, 0), (gc.MV_8x8, 1)), outs.values()):
        want = gc.restate_corr({"pic": pic, "arrays": arrays, "method": m, "shift": s, "pairs": pairs, "cap": (1 << (2 * m)) * nb})
        assert want["count"].sum() > 0
        assert np.array_equal(got["count"].cpu().numpy().view(np.uint32), want["count"]) and np.array_equal(got["corr"].cpu().numpy(), want["corr"])
        assert np.array_equal(got["sums"].cpu().numpy().view(np.uint32), want["sums"])
    for p in [cur] + list(refs.values()):
        p.free()


def test_a_refined_rotzoom_model_through_the_warp_prediction(hip_ctx):
    """svt_hip_warp_pred_batch takes the refine batch's model array with SVT_HIP_WARP_MODEL0_FROM_ARRAY, on the same stream, with no host look at it"""
    import torch
    b = gc.batch("one_72x44")
    want_model = gc.restated("one_72x44")[0]["models"]
    assert int(want_model[0]["wmtype"]) == gc.ROTZOOM and int(want_model[0]["valid"]) == 1
    ref = b["planes"][1]
    t_planes = [api.to_device(p[0]) for p in [b["src"], ref]]
    refs = [warp.plane_ref(t, p[0].shape[1], p[1], p[2], p[3], p[4], p[0].shape[0]) for t, p in zip(t_planes, [b["src"], ref])]
    jobs = b["jobs"].copy()
    jobs["ref"] = 0
    outs, work = gm.run_gm_refine_device(hip_ctx, refs[0], refs[1:], b["n_refinements"], b["chess_refn"], b["rfn_early_exit"], api.to_device(jobs), 1, fill=FILL)
    pj = wc.pack_jobs([wc.pred_job(y * 64 + x, x, y, w, h, [0], [], flags=wc.MODEL0_FROM_ARRAY, model_index=(0, 0)) for x, y, w, h in ((0, 0, 32, 32), (40, 8, 16, 32), (56, 32, 8, 8))],
                      wc.PRED_JOB_DTYPE)
    dst = torch.full((64 * 64,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(pj),), FILL, dtype=torch.uint8, device="cuda")
    t_jobs = api.to_device(pj)
    torch.cuda.current_stream().synchronize()
    warp.run_warp_pred_device(hip_ctx, 8, 0, 0, refs[1:], dst, 64, t_jobs, len(pj), status, models=outs["models"], n_models=1)
    hip_ctx.sync()
    del work
    assert outs["models"].cpu().numpy().view(abi.WARP_MODEL_DTYPE)[:1].tobytes() == want_model.tobytes()
    bw = {"bit_depth": 8, "ss_x": 0, "ss_y": 0, "planes": [ref], "jobs": pj, "dst_shape": (64, 64), "dst_stride": 64, "models": want_model}
    want, want_status, _ = wc.restate_pred(bw)
    assert np.all(want_status == wc.ST_OK) and np.array_equal(status.cpu().numpy(), want_status)
    assert np.array_equal(dst.cpu().numpy().reshape(64, 64), want)
