"""CPU: the restatement of the chroma-from-luma prediction and of the alpha search (tests/cfl_cases.py) against the reference's own results
(golden/cfl.npz: svt_cfl_luma_subsampling_420_*_c, svt_subtract_average_c, svt_cfl_predict_*_c and md_cfl_rd_pick_alpha itself, driven by
tools/gen_cfl_golden.py), the coverage conditions recomputed from the restatement, the struct lay-outs of abi.py against the library's, and
svt_hip_cfl_pred_check_desc (validation needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import cfl_cases as cc
from abi_mirror import check_layout
from batch_entry_cases import good_cfl_pick_desc, good_cfl_pred_desc as good_desc
from svt_av1_psyex_amd import abi, api, cfl

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(cc.GOLDEN)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", ["size", "geometry", "alist"])
def test_restatement_equals_the_reference_on_every_job(golden, group, bd):
    names = [n for n in cc.batch_names() if n.startswith(group) and cc.batch(n)["bit_depth"] == bd]
    assert names
    for name in names:
        b = cc.batch(name)
        preds, acs, _ = cc.restated(name)
        assert all(cc.job_defined(b, j) for j in b["jobs"]), name
        assert np.array_equal(cc.batch_crcs(preds, acs), golden[f"crc_{name}"]), name


def test_the_fixture_holds_exactly_the_generators_keys(golden):
    keys = {f"crc_{n}" for n in cc.batch_names()} | {k for kp, ka, _, _ in cc.sample_jobs() for k in (kp, ka)} | {"pick_ref"}
    assert set(golden.files) == keys
    for name in cc.batch_names():
        assert len(golden[f"crc_{name}"]) == len(cc.batch(name)["jobs"]), name
    assert golden["pick_ref"].shape == (len(cc.pick_cases()), 5)


def test_sample_blocks_equal_the_reference_sample_by_sample(golden):
    """one whole block per size and depth, so that a mismatch can be looked at"""
    seen = set()
    for kp, ka, name, i in cc.sample_jobs():
        b = cc.batch(name)
        preds, acs, _ = cc.restated(name)
        assert np.array_equal(preds[i][:, cc.sample_slots()], golden[kp]), kp
        assert np.array_equal(acs[i], golden[ka]) and golden[ka].dtype == np.int16, ka
        assert golden[kp].shape == (2, 3, b["height"], b["width"])
        seen.add((b["bit_depth"], b["width"], b["height"]))
    assert seen == {(bd, w, h) for bd in (8, 10) for w, h in cc.SIZES}


def test_coverage_conditions_hold_on_the_restatement():
    """in both depths: clipping at 0 and at the maximum, alpha * ac on a tie (32 mod 64) of either sign, sum + round off a multiple of W * H and an
    average with a remainder of exactly one half, flat luma at 0 and at the maximum, the 2x2 checkerboard, alternating rows (|AC| = 4 * max), every
    alpha, all 16 sizes, and per size a luma extent that ends on the plane's last row and column with the stride equal to the width"""
    records = cc.all_records()
    assert cc.coverage_missing(records) == []
    assert len(records) > 4000
    assert cc.coverage_missing(records[:300]) != []  # the check can fail: a truncated case list misses sizes


def test_the_cases_are_what_the_issue_lists():
    for bd in (8, 10):
        for w, h in cc.SIZES:
            b = cc.batch(f"size_{w}x{h}_{bd}")
            jpw, n = cc.jobs_per_wave(w, h), len(b["jobs"])
            assert b["alphas"] == list(range(-16, 17)) and (jpw == 1 or n % jpw != 0)  # a partial last wave
            assert n % (4 * jpw) != 0  # a partial last workgroup
            assert set(cc.EXTREME_KINDS) <= {b["kinds"][i] for i in range(n) if i % jpw == 0}  # first in a wave
            assert set(cc.EXTREME_KINDS) <= {b["kinds"][i] for i in range(n) if i % jpw == jpw - 1}  # and last
            assert b["luma"].shape[1] == b["luma_size"][0]
        for w, h in cc.GEOMETRY_SIZES:
            g = cc.batch(f"geometry_{w}x{h}_{bd}")
            assert g["luma_size"][0] < g["luma"].shape[1] and any(int(j["luma_x"]) & 1 for j in g["jobs"]) and any(int(j["luma_y"]) & 1 for j in g["jobs"])
            assert any(int(j["dst_offset"][0]) % 4 for j in g["jobs"]) and any(int(j["dc_offset"][1]) % 4 for j in g["jobs"]) and g["dst_stride"] % 4
        assert [len(cc.batch(f"alist_{k}_8x8_{bd}")["alphas"]) for k in cc.ALPHA_LISTS] == [1, 2, 33]
    assert sorted(cc.UNORDERED_33) == list(range(-16, 17)) and cc.UNORDERED_33 != sorted(cc.UNORDERED_33)
    assert len(set(cc.batch_names())) == len(cc.batch_names())


def test_struct_layouts_match_the_library():
    check_layout("svt_hip_cfl_layout", (abi.CflPredDesc, abi.CflPredJob, abi.CflPlane, abi.CflPickDesc), multiple_of_8=True)
    dt = np.dtype(abi.CFL_PRED_JOB_DTYPE)
    assert dt.itemsize == C.sizeof(abi.CflPredJob) and abi.CFL_PRED_JOB_DTYPE == cc.JOB_DTYPE
    for name, *_ in abi.CflPredJob._fields_:
        assert dt.fields[name][1] == getattr(abi.CflPredJob, name).offset, name
    assert (abi.CFL_OK, abi.CFL_UNDEFINED, abi.CFL_SLOTS, abi.CFL_MAX_MODE_COST) == (cc.ST_OK, cc.ST_UNDEFINED, cc.SLOTS, cc.MAX_MODE_COST)
    assert (abi.CFL_PICK_TRUNCATED, abi.CFL_PICK_UNDEFINED) == (cc.PICK_TRUNCATED, cc.PICK_UNDEFINED)
    assert cfl.ALPHAS_FULL == cc.ALPHAS_FULL


def test_check_desc_accepts_a_good_descriptor():
    for bd in (8, 10):
        for n_alpha in (1, 33):
            cfl.check_desc(good_desc(bd, n_alpha))
    for w in cc.SIDES:
        for h in cc.SIDES:
            d = good_desc()
            d.width, d.height = w, h
            cfl.check_desc(d)
    d = good_desc()
    d.ac = None
    cfl.check_desc(d)
    d = good_desc()
    d.plane[0].dst = d.luma + ((d.luma_height - 1) * d.luma_stride + d.luma_width) * 2  # the destination begins where the luma plane ends
    cfl.check_desc(d)
    d = good_desc()
    d.plane[1].dst = d.plane[0].dc - 2 * d.plane[1].dst_samples  # and ends where a DC plane begins
    cfl.check_desc(d)
    d = good_desc()
    d.plane[1].dc = d.plane[0].dc  # the two DC planes may be one
    cfl.check_desc(d)


BAD = ["null_desc", "no_luma", "no_jobs", "no_status", "no_dc0", "no_dc1", "no_dst0", "no_dst1", "bit_depth_12", "bit_depth_0", "bit_depth_9", "width_0", "width_2",
       "width_12", "width_64", "height_0", "height_6", "height_64", "n_alpha_0", "n_alpha_34", "alpha_17", "alpha_-17", "alpha_127", "zero_luma_stride",
       "stride_below_width", "zero_luma_width", "zero_luma_height", "zero_slot_stride", "zero_dc_stride0", "zero_dc_stride1", "zero_dst_stride0",
       "zero_dst_stride1", "zero_dc_samples1", "zero_dst_samples0", "ac_unaligned", "dst0_inside_luma", "dst1_ends_in_luma", "luma_ends_in_dst0",
       "dst0_inside_dc0", "dst0_inside_dc1", "dst1_inside_dc0"]


@pytest.mark.parametrize("bad", BAD)
def test_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    if bad == "null_desc":
        assert L.svt_hip_cfl_pred_check_desc(None) == BAD_PARAM
    else:
        d = cc.spoil_desc(good_desc(), bad)
        assert L.svt_hip_cfl_pred_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_cfl_pred_check_desc"):
            cfl.check_desc(d)
    assert b"svt_hip_cfl_pred_check_desc" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("bad", ["null_ctx", "null_desc", "bit_depth_12", "width_12", "n_alpha_34", "alpha_17", "no_status", "dst0_inside_dc1"])
def test_batch_rejects_a_bad_descriptor_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_desc()
    if bad == "null_ctx":
        assert L.svt_hip_cfl_pred_batch(None, C.byref(d)) == BAD_PARAM
    elif bad == "null_desc":
        assert L.svt_hip_cfl_pred_batch(ctx, None) == BAD_PARAM
    else:
        assert L.svt_hip_cfl_pred_batch(ctx, C.byref(cc.spoil_desc(d, bad))) == BAD_PARAM
    assert b"svt_hip_cfl_pred" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("bad", ["null_ctx", "null_desc", "no_bits", "no_dist", "no_mode_bits", "no_alpha_fac_bits", "no_best_rd", "no_cfl_alpha_idx",
                                 "no_cfl_alpha_signs", "no_status", "itr_th_17", "n_mag_0", "n_mag_17"])
def test_pick_rejects_a_bad_descriptor_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)
    d = good_cfl_pick_desc()
    if bad == "null_ctx":
        assert L.svt_hip_cfl_pick_alpha_batch(None, C.byref(d)) == BAD_PARAM
    elif bad == "null_desc":
        assert L.svt_hip_cfl_pick_alpha_batch(ctx, None) == BAD_PARAM
    else:
        if bad.startswith("no_"):
            setattr(d, bad[3:], None)
        else:
            name, _, v = bad.rpartition("_")
            setattr(d, name, int(v))
        assert L.svt_hip_cfl_pick_alpha_batch(ctx, C.byref(d)) == BAD_PARAM
    assert b"svt_hip_cfl_pick_alpha_batch" in L.svt_hip_last_error(None)


def test_job_defined_names_every_undefined_kind():
    for bd in (8, 10):
        for w, h in ((4, 4), (8, 8), (16, 16), (32, 32), (4, 16)):
            b, bad = cc.undefined_batch(bd, w, h)
            assert [i for i, j in enumerate(b["jobs"]) if not cc.job_defined(b, j)] == bad and len(bad) == 11


# ---- the alpha search ----
def test_pick_restatement_equals_md_cfl_rd_pick_alpha(golden):
    """best_rd, cfl_alpha_idx, cfl_alpha_signs and the slots evaluated, on every case; a case cut to n_mag < 16 magnitudes equals the reference on
    the whole table unless its truncation bit says that the reference would have gone on"""
    ref = golden["pick_ref"]
    truncated = 0
    for c, r, want in zip(cc.pick_cases(), cc.pick_results(), ref):
        assert r["status"] in (0, cc.PICK_TRUNCATED), c["name"]
        if r["status"] == cc.PICK_TRUNCATED:
            assert c["n_mag"] < 16, c["name"]
            truncated += 1
            continue
        assert (r["best_rd"], r["idx"], r["signs"], r["evals"][0], r["evals"][1]) == tuple(int(v) for v in want), c["name"]
        if not r["found"]:
            assert (r["best_rd"], r["idx"], r["signs"]) == (cc.MAX_MODE_COST, 0, 0)
    assert truncated >= 4


def test_pick_coverage_conditions_hold():
    """every joint sign as the winner, both itr_th values, a break at c = itr_th + 1, a run to c = 15, ties (the first wins), a block with no pair,
    n_mag < 16 with and without the truncation bit"""
    cases, results = cc.pick_cases(), cc.pick_results()
    assert cc.pick_coverage_missing(cases, results) == []
    assert cc.pick_coverage_missing(cases[:6], results[:6]) != []  # the check can fail
    flat = {c["name"]: r for c, r in zip(cases, results)}["flat_th1"]
    assert (flat["idx"], flat["signs"]) == (0, 2)  # one cost everywhere: c = 0 in both planes, and the first pair in the reference's order
    assert {c["itr_th"] for c in cases} == {1, 2}


def test_pick_truncation_bit_means_the_reference_would_have_gone_on():
    """a truncated replay reads no slot beyond its magnitudes, and the reference on the whole table read at least one of them"""
    for c, r, want in zip(cc.pick_cases(), cc.pick_results(), np.load(cc.GOLDEN)["pick_ref"]):
        if c["n_mag"] == 16:
            continue
        allowed = sum(1 << k for k in range(16 - c["n_mag"], 17 + c["n_mag"]))
        assert r["evals"][0] & ~allowed == 0 and r["evals"][1] & ~allowed == 0, c["name"]
        beyond = (int(want[3]) | int(want[4])) & ~allowed
        assert (r["status"] == cc.PICK_TRUNCATED) == (beyond != 0), c["name"]


def test_pick_reports_an_undefined_bits_entry():
    c = cc.pick_cases()[0]
    bits = c["bits"].copy()
    bits[1][16] = cc.U64_MAX
    r = cc.pick_alpha(bits, c["dist"], c["fac"], c["mode_bits"], c["lam"], c["itr_th"])
    assert (r["status"], r["best_rd"], r["idx"], r["signs"]) == (cc.PICK_UNDEFINED, cc.MAX_MODE_COST, 0, 0)
    bits = c["bits"].copy()
    bits[0][0] = cc.U64_MAX  # a slot this replay does not read
    r = cc.pick_alpha(bits, c["dist"], c["fac"], c["mode_bits"], c["lam"], c["itr_th"])
    assert r["status"] == 0 and not (r["evals"][0] & 1)
