"""GPU: svt_hip_cfl_pred_batch and svt_hip_cfl_pick_alpha_batch on the MI355X, every comparison exact -- against the reference's own results
(golden/cfl.npz) and the restatement (tests/cfl_cases.py): every size in both depths with the extreme blocks first and last in a wave and a partial
last wave, the AC output, origins and pitches that leave no access aligned, alpha lists of 1, 2 and 33 unordered entries, undefined jobs between
good ones, a luma plane allocated exactly, rejected descriptors, and the alpha search on the CPU test's case list.  Both destinations sit between
guard bands, and they, the spare status and AC slots and the inputs are compared whole."""
import ctypes as C

import numpy as np
import pytest

import cfl_cases as cc
from svt_av1_psyex_amd import abi, api, cfl

pytestmark = pytest.mark.gpu

FILL = 0xA5
SPARE = 3
GUARD = 96


@pytest.fixture(scope="module")
def golden():
    return np.load(cc.GOLDEN)


def run(ctx, b, jobs=None, want_ac=True):
    """the batch (or `jobs` of it) on destinations, a status array and an AC array pre-filled with 0xA5: checks that the spare slots and the
    inputs are as they were; returns (the two destinations with their guard bands, status, ac)"""
    jobs = b["jobs"] if jobs is None else jobs
    out = cfl.run_cfl_pred_hip(ctx, b["bit_depth"], b["width"], b["height"], b["alphas"], b["luma"], b["dc"], jobs, b["dst_samples"], b["dst_stride"],
                               b["slot_stride"], want_ac=want_ac, spare_jobs=SPARE, fill=FILL, guard=GUARD, luma_size=b["luma_size"])
    n = len(jobs)
    assert len(out["status"]) == n + SPARE and np.all(out["status"][n:] == FILL), "spare status slots written"
    assert np.array_equal(out["luma"], b["luma"]) and all(np.array_equal(g, w) for g, w in zip(out["dc"], b["dc"])), "an input plane changed"
    if want_ac:
        assert np.all(out["ac"][n:].view(np.uint8) == FILL), "spare AC slots written"
    else:
        assert out["ac"] is None
    return out["dst"], out["status"][:n], out["ac"][:n] if want_ac else None


def check(ctx, golden, name, want_ac=True):
    """device == restatement on every sample of both destinations and their guard bands (so every sample outside the jobs' slots is still 0xA5)
    == the fixture"""
    b = cc.batch(name)
    preds, acs, _ = cc.restated(name)
    dst, status, ac = run(ctx, b, want_ac=want_ac)
    assert np.all(status == cc.ST_OK), name
    got = [cc.blocks_of(b, dst, j, GUARD) for j in b["jobs"]]
    bad = [i for i, (g, w) in enumerate(zip(got, preds)) if not np.array_equal(g, w)]
    assert not bad, (name, bad[:8], [b["kinds"][i] for i in bad[:8]])
    for p, (g, w) in enumerate(zip(dst, cc.expected_dst(b, preds, FILL, GUARD))):
        assert np.array_equal(g, w), f"{name}: plane {p}: a sample outside the jobs' slots was written"
    if want_ac:
        assert np.array_equal(ac, np.stack(acs)), name
    assert np.array_equal(cc.batch_crcs(got, ac if want_ac else acs), golden[f"crc_{name}"]), name


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", cc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_size_every_alpha_extreme_blocks_at_the_ends_of_a_wave(hip_ctx, golden, size, bd):
    check(hip_ctx, golden, f"size_{size[0]}x{size[1]}_{bd}")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", cc.GEOMETRY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_origins_and_pitches_without_the_ac_output(hip_ctx, golden, size, bd):
    """no luma load, DC load or store is aligned; the luma plane is narrower than its array and the grid's last jobs end on its last column and
    row; the AC is not asked for"""
    check(hip_ctx, golden, f"geometry_{size[0]}x{size[1]}_{bd}", want_ac=False)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", list(cc.ALPHA_LISTS))
def test_alpha_lists_of_1_2_and_33_unordered(hip_ctx, golden, kind, bd):
    for size in ("8x8", "4x16"):
        check(hip_ctx, golden, f"alist_{kind}_{size}_{bd}")


def test_sample_blocks_equal_the_fixture(hip_ctx, golden):
    for kp, ka, name, i in cc.sample_jobs()[::5]:
        b = cc.batch(name)
        j = b["jobs"][i:i + 1]
        dst, status, ac = run(hip_ctx, b, j)
        assert status[0] == cc.ST_OK
        assert np.array_equal(cc.blocks_of(b, dst, j[0], GUARD)[:, cc.sample_slots()], golden[kp]), kp
        assert np.array_equal(ac[0], golden[ka]), ka


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(4, 4), (8, 8), (16, 16), (32, 32), (4, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_undefined_jobs_report_0xff_write_nothing_else_and_leave_their_neighbours(hip_ctx, size, bd):
    b, bad = cc.undefined_batch(bd, *size)
    defined = [cc.job_defined(b, j) for j in b["jobs"]]
    assert [i for i, ok in enumerate(defined) if not ok] == bad
    dst, status, ac = run(hip_ctx, b)
    assert np.array_equal(status, np.where(defined, cc.ST_OK, cc.ST_UNDEFINED))
    preds, acs, _ = cc.restate_batch(b, defined)
    # both destinations whole: the good jobs exact, the undefined jobs' slots, the guard bands and everything else still 0xA5
    for g, w in zip(dst, cc.expected_dst(b, preds, FILL, GUARD)):
        assert np.array_equal(g, w)
    for i, ok in enumerate(defined):
        assert np.array_equal(ac[i], acs[i]) if ok else np.all(ac[i].view(np.uint8) == FILL), i


@pytest.mark.parametrize("n,name", [(1, "size_4x4_8"), (15, "size_4x4_10"), (17, "size_4x4_8"), (65, "size_4x4_10"), (3, "size_8x8_8"), (5, "size_8x8_10"),
                                    (1, "size_16x16_10"), (5, "size_16x16_8"), (1, "size_32x32_8"), (2, "size_16x32_10")])
def test_job_counts_that_leave_lanes_waves_and_workgroups_empty(hip_ctx, n, name):
    b = cc.batch(name)
    jobs = b["jobs"][2:2 + n]
    preds, acs, _ = cc.restated(name)
    dst, status, ac = run(hip_ctx, b, jobs)
    assert np.all(status == cc.ST_OK)
    for g, w in zip(dst, cc.expected_dst(dict(b, jobs=jobs), preds[2:2 + n], FILL, GUARD)):
        assert np.array_equal(g, w)
    assert np.array_equal(ac, np.stack(acs[2:2 + n]))


def test_no_jobs_enqueue_nothing(hip_ctx):
    b = cc.batch("size_8x8_8")
    dst, status, ac = run(hip_ctx, b, b["jobs"][:0])
    assert all(np.all(g == FILL) for g in dst) and len(status) == 0


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(8, 8), (16, 4), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_jobs_in_the_corners_of_a_luma_plane_allocated_exactly(hip_ctx, size, bd):
    """the luma buffer holds the plane and not one byte more, its stride is its width, and the four jobs sit in its corners: the kernel's address
    rule (a lane loads the 8 x 2 samples under its four chroma samples) keeps every load inside"""
    w, h = size
    b = cc.make_batch(f"corners_{w}x{h}_{bd}", bd, w, h, cc.ALPHAS_FULL, ["noise", "rows", "checker", "noise"], 2, 8100 + w + h + bd, dense=True)
    assert b["luma"].shape == (4 * h, 4 * w) and {(int(j["luma_x"]), int(j["luma_y"])) for j in b["jobs"]} == {(0, 0), (2 * w, 0), (0, 2 * h), (2 * w, 2 * h)}
    preds, acs, _ = cc.restate_batch(b)
    dst, status, ac = run(hip_ctx, b)
    assert np.all(status == cc.ST_OK)
    for g, want in zip(dst, cc.expected_dst(b, preds, FILL, GUARD)):
        assert np.array_equal(g, want)
    assert np.array_equal(ac, np.stack(acs))


@pytest.mark.parametrize("bad", ["bit_depth_12", "width_12", "height_64", "n_alpha_0", "n_alpha_34", "alpha_17", "zero_luma_stride", "zero_slot_stride", "no_luma",
                                 "no_status", "no_dc1", "no_dst0", "zero_dst_stride1", "dst0_inside_luma", "dst0_inside_dc1"])
def test_rejected_descriptor_returns_non_zero_and_leaves_the_buffers_as_filled(hip_ctx, bad):
    import torch
    fill = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    bufs = {"luma": fill(2 * 256 * 144), "dc0": fill(2 * 128 * 72), "dc1": fill(2 * 128 * 72), "dst0": fill(2 * 33 * 128 * 72), "dst1": fill(2 * 33 * 128 * 72),
            "jobs": fill(24 * 6), "status": fill(6)}
    planes = [dict(dc=bufs[f"dc{q}"].data_ptr(), dc_stride=128, dc_samples=128 * 72, dst=bufs[f"dst{q}"].data_ptr(), dst_stride=128, dst_samples=33 * 128 * 72)
              for q in range(2)]
    d = cfl.pred_desc(10, 8, 8, cc.ALPHAS_FULL, bufs["luma"].data_ptr(), 256, 208, 144, planes, 128 * 72, bufs["jobs"].data_ptr(), 6, bufs["status"].data_ptr())
    cc.spoil_desc(d, bad)
    torch.cuda.synchronize()
    assert api.lib().svt_hip_cfl_pred_batch(hip_ctx._h, C.byref(d)) == 2
    assert b"svt_hip_cfl_pred_check_desc" in api.lib().svt_hip_last_error(None)
    hip_ctx.sync()
    for name, t in bufs.items():
        assert bool(torch.all(t == FILL)), name


# ---- the alpha search ----
def pick_tables():
    cases = cc.pick_cases()
    return (np.stack([c["bits"] for c in cases]), np.stack([c["dist"] for c in cases]), np.array([c["mode_bits"] for c in cases], np.int32))


def test_pick_equals_the_restatement_and_the_reference_case_by_case(hip_ctx, golden):
    """every case of the CPU test under its own lambda, itr_th, n_mag and alpha rates"""
    ref = golden["pick_ref"]
    for c, r, want in zip(cc.pick_cases(), cc.pick_results(), ref):
        got = cfl.run_pick_hip(hip_ctx, c["bits"][None], c["dist"][None], [c["mode_bits"]], c["fac"], c["lam"], c["itr_th"], c["n_mag"], spare=SPARE, fill=FILL)
        assert (int(got["best_rd"][0]), int(got["cfl_alpha_idx"][0]), int(got["cfl_alpha_signs"][0]), int(got["status"][0])) == \
            (r["best_rd"], r["idx"], r["signs"], r["status"]), c["name"]
        if r["status"] == 0:
            assert (int(got["best_rd"][0]), int(got["cfl_alpha_idx"][0]), int(got["cfl_alpha_signs"][0])) == tuple(int(v) for v in want[:3]), c["name"]
        for name, a in got.items():
            assert np.all(a[1:].view(np.uint8) == FILL), (c["name"], name)


@pytest.mark.parametrize("shared", [0, 9, 12, 40, 47, 78, 84, 91])
def test_pick_batches_of_every_table_under_one_cases_shared_values(hip_ctx, shared):
    """one launch over all the tables (two workgroups, the second partial), lambda / itr_th / n_mag / alpha rates those of one case; one block's
    Cr alpha-zero entry is UINT64_MAX: status 0xFF, MAX_MODE_COST, 0, 0, its neighbours as they were"""
    cases = cc.pick_cases()
    s = cases[shared]
    bits, dist, mode_bits = pick_tables()
    undefined = 66
    bits = bits.copy()
    bits[undefined][1][16] = cc.U64_MAX
    assert 64 < len(cases) < 128
    want = [cc.pick_alpha(b, d, s["fac"], int(m), s["lam"], s["itr_th"], s["n_mag"]) for b, d, m in zip(bits, dist, mode_bits)]
    got = cfl.run_pick_hip(hip_ctx, bits, dist, mode_bits, s["fac"], s["lam"], s["itr_th"], s["n_mag"], spare=SPARE, fill=FILL)
    n = len(cases)
    for key, name in (("best_rd", "best_rd"), ("idx", "cfl_alpha_idx"), ("signs", "cfl_alpha_signs"), ("status", "status")):
        assert [int(v) for v in got[name][:n]] == [w[key] for w in want], name
        assert np.all(got[name][n:].view(np.uint8) == FILL), name
    assert (want[undefined]["status"], want[undefined]["best_rd"]) == (cc.PICK_UNDEFINED, cc.MAX_MODE_COST)
    assert {w["status"] for w in want} >= ({0, cc.PICK_UNDEFINED} if s["n_mag"] == 16 else {cc.PICK_TRUNCATED, cc.PICK_UNDEFINED})


def test_pick_with_no_blocks_enqueues_nothing(hip_ctx):
    c = cc.pick_cases()[0]
    got = cfl.run_pick_hip(hip_ctx, np.zeros((0, 2, 33), np.uint64), np.zeros((0, 2, 33), np.uint64), np.zeros(0, np.int32), c["fac"], c["lam"], 1, spare=SPARE,
                           fill=FILL)
    assert all(np.all(a.view(np.uint8) == FILL) for a in got.values())
