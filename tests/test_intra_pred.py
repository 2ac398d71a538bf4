"""CPU: the restatement of the intra prediction (tests/intra_pred_cases.py) against the reference's own build_intra_predictors /
build_intra_predictors_high results (golden/intra_pred.npz), the coverage conditions recomputed from the restatement, the independence of
filter-intra's anti-diagonals, the struct lay-outs of abi.py against the library's, and svt_hip_intra_pred_check_desc (validation needs no
GPU)."""
import ctypes as C

import numpy as np
import pytest

import intra_pred_cases as ic
from abi_mirror import check_layout
from batch_entry_cases import good_intra_pred_desc as good_desc
from svt_av1_psyex_amd import abi, api, intra

BAD_PARAM = 2
GROUPS = ["nondir", "dir", "fi", "extreme", "geometry"]


@pytest.fixture(scope="module")
def golden():
    return np.load(ic.GOLDEN)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", GROUPS)
def test_restatement_equals_the_reference_on_every_job(golden, group, bd):
    names = [n for n in ic.batch_names() if n.startswith(group) and ic.batch(n)["bit_depth"] == bd]
    assert names
    for name in names:
        blocks, events = ic.restated(name)
        assert all(e["inside"] for e in events), name  # no read leaves the neighbour plane
        assert np.array_equal(ic.batch_crcs(blocks), golden[f"crc_{name}"]), name


def test_the_fixture_holds_every_batch_and_nothing_else(golden):
    keys = {f"crc_{n}" for n in ic.batch_names()} | {k for k, _, _ in ic.sample_jobs()}
    assert set(golden.files) == keys
    for name in ic.batch_names():
        assert len(golden[f"crc_{name}"]) == len(ic.batch(name)["jobs"]), name


def test_sample_blocks_equal_the_reference_sample_by_sample(golden):
    """one full block per mode family x depth, so that a mismatch can be looked at"""
    seen = set()
    for key, name, i in ic.sample_jobs():
        b = ic.batch(name)
        assert np.array_equal(ic.restated(name)[0][i], golden[key]), key
        j = b["jobs"][i]
        seen.add((b["bit_depth"], int(j["mode"]), int(j["filter_intra_mode"]) != ic.NO_FI))
    assert {(bd, m, False) for bd in (8, 10) for m in range(13)} | {(bd, 0, True) for bd in (8, 10)} == seen
    assert 26 <= len(ic.sample_jobs()) <= 34


def all_records():
    records = []
    for name in ic.batch_names():
        b = ic.batch(name)
        records += [(b["bit_depth"], j, e) for j, e in zip(b["jobs"], ic.restated(name)[1])]
    return records


def test_coverage_conditions_hold_on_the_restatement():
    """each zone with upsampling off and on per side, strengths 0..3 for both filt_types, the corner filter run and skipped, zone 1's fill past
    max_base_x, zone 2 using both edges in one row, the four DC variants, every early-fill value in both depths, replication on each of the four
    edge parts and beyond what 4x16 / 16x4 / 16x64 / 64x16 can be given, PAETH's three candidates, filter-intra clipping both ways in both depths"""
    records = all_records()
    assert ic.coverage_missing(records) == []
    assert len(records) > 50000
    assert ic.coverage_missing(records[:200]) != []  # the check can fail


def test_zone3_cannot_run_past_max_base():
    """why the coverage list has no fill for zone 3: with its largest dy (angle 212) the last sample's base stays below bw + bh - 1"""
    dy = max(ic.DERIV[270 - a] for m in (ic.H_PRED, ic.D203_PRED) for a in (ic.MODE_TO_ANGLE[m] + 3 * d for d in range(-3, 4)) if a > 180)
    assert dy == 40
    for tx in range(ic.N_TX):
        w, h = ic.TX_W[tx], ic.TX_H[tx]
        for up in (0, 1):
            assert ((w * dy) >> (6 - up)) + ((h - 1) << up) < ((w + h - 1) << up)


def test_the_cases_are_what_the_issue_lists():
    for bd in (8, 10):
        b = ic.batch(f"nondir_{bd}")  # group 1
        for tx in range(ic.N_TX):
            w, h = ic.TX_W[tx], ic.TX_H[tx]
            js = [j for j in b["jobs"] if j["tx_size"] == tx]
            assert {int(j["mode"]) for j in js} == set(ic.NON_DIRECTIONAL)
            assert {int(j["n_top_px"]) for j in js} == {0, w} | ({w // 2} if w >= 8 else set())
            assert {int(j["n_left_px"]) for j in js} == {0, h} | ({h // 2} if h >= 8 else set())
            assert {int(j["n_topright_px"]) for j in js if j["n_top_px"] == w} == {0, w // 2, w}
            assert {int(j["n_bottomleft_px"]) for j in js if j["n_left_px"] == h} == {0, h // 2, h}
        for tx in range(ic.N_TX):  # group 2
            for ef in (0, 1):
                d = ic.batch(f"dir_tx{tx}_{bd}_ef{ef}")
                assert d["disable_edge_filter"] == 1 - ef
                combos = {(int(j["mode"]), int(j["angle_delta"]), int(j["filt_type"])) for j in d["jobs"]}
                assert len(combos) == 56 * 2 and len(d["jobs"]) == 56 * 2 * 5
        f = ic.batch(f"fi_{bd}")  # group 3
        assert {(int(j["filter_intra_mode"]), int(j["tx_size"])) for j in f["jobs"]} == {(m, tx) for m in range(5) for tx in ic.FI_SIZES}
        assert len(ic.FI_SIZES) == 14 and len(f["jobs"]) == 5 * 14 * 4
        for kind in ic.EXTREME_KINDS:  # group 4
            e = ic.batch(f"extreme_{kind}_{bd}")
            assert {int(j["mode"]) for j in e["jobs"]} == set(range(13)) and {int(j["filter_intra_mode"]) for j in e["jobs"]} == set(range(6))
        for stride in (204, 203):  # group 5
            g = ic.batch(f"geometry_{bd}_stride{stride}")
            assert {int(j["dst_offset"]) % stride % 16 for j in g["jobs"]} == {0, 4, 8, 12}
            assert any(j["nbr_x"] & 1 for j in g["jobs"])
            corners = {(int(j["nbr_x"]) == 0, int(j["nbr_y"]) == 0) for j in g["jobs"] if int(j["nbr_x"]) in (0, ic.NBR_W - ic.TX_W[j["tx_size"]])
                       and int(j["nbr_y"]) in (0, ic.NBR_H - ic.TX_H[j["tx_size"]])}
            assert len(corners) == 4
    assert len(set(ic.batch_names())) == len(ic.batch_names())


@pytest.mark.parametrize("tx", ic.FI_SIZES)
def test_filter_intra_anti_diagonals_are_independent(tx):
    """the kernel computes all sub-blocks of one R + C from the tile as it was before that diagonal: equal to the reference's serial order"""
    w, h = ic.TX_W[tx], ic.TX_H[tx]
    rng = np.random.default_rng(500 + tx)
    for bd in (8, 10):
        mx = (1 << bd) - 1
        for fim in range(5):
            above, left, corner = rng.integers(0, mx + 1, w), rng.integers(0, mx + 1, h), int(rng.integers(0, mx + 1))
            serial = ic.filter_intra_block(above, left, corner, w, h, fim, mx)[0]
            assert np.array_equal(ic.filter_intra_block(above, left, corner, w, h, fim, mx, by_diagonals=True)[0], serial)
    assert max(min(h // 2, w // 4, d + 1) for d in range(h // 2 + w // 4 - 1)) <= 8  # at most 8 sub-blocks of 8 lanes on a diagonal


def test_struct_layouts_match_the_library():
    check_layout("svt_hip_intra_pred_layout", (abi.IntraPredDesc, abi.IntraPredJob), multiple_of_8=True)
    dt = np.dtype(abi.INTRA_PRED_JOB_DTYPE)
    assert dt.itemsize == C.sizeof(abi.IntraPredJob) and abi.INTRA_PRED_JOB_DTYPE == ic.JOB_DTYPE
    for name, *_ in abi.IntraPredJob._fields_:
        assert dt.fields[name][1] == getattr(abi.IntraPredJob, name).offset, name
    assert (abi.INTRA_PRED_OK, abi.INTRA_PRED_UNDEFINED, abi.INTRA_PRED_NO_FILTER_INTRA) == (ic.ST_OK, ic.ST_UNDEFINED, ic.NO_FI)
    assert (list(abi.TX_W), list(abi.TX_H)) == (ic.TX_W, ic.TX_H)


def test_check_desc_accepts_a_good_descriptor():
    intra.check_desc(good_desc())
    intra.check_desc(good_desc(8))
    d = good_desc()
    d.dst = d.nbr + ((d.nbr_height - 1) * d.nbr_stride + d.nbr_width) * 2  # the destination begins where the neighbour plane ends
    intra.check_desc(d)
    d = good_desc()
    d.dst = d.nbr - 2 * d.dst_samples  # and ends where it begins
    intra.check_desc(d)


BAD = ["null_desc", "no_nbr", "no_dst", "no_jobs", "no_status", "bit_depth_12", "bit_depth_0", "bit_depth_9", "zero_stride", "stride_below_width", "zero_width",
       "zero_height", "zero_dst_stride", "zero_dst_samples", "dst_inside_nbr", "dst_ends_in_nbr", "nbr_ends_in_dst"]


@pytest.mark.parametrize("bad", BAD)
def test_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    if bad == "null_desc":
        assert L.svt_hip_intra_pred_check_desc(None) == BAD_PARAM
    else:
        d = ic.spoil_desc(good_desc(), bad)
        assert L.svt_hip_intra_pred_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_intra_pred_check_desc"):
            intra.check_desc(d)
    assert b"svt_hip_intra_pred_check_desc" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("bad", ["null_ctx", "null_desc", "bit_depth_12", "zero_stride", "no_status", "dst_inside_nbr"])
def test_batch_rejects_a_bad_descriptor_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_desc()
    if bad == "null_ctx":
        assert L.svt_hip_intra_pred_batch(None, C.byref(d)) == BAD_PARAM
    elif bad == "null_desc":
        assert L.svt_hip_intra_pred_batch(ctx, None) == BAD_PARAM
    else:
        assert L.svt_hip_intra_pred_batch(ctx, C.byref(ic.spoil_desc(d, bad))) == BAD_PARAM
    assert b"svt_hip_intra_pred" in L.svt_hip_last_error(None)


def test_job_defined_names_every_undefined_kind():
    for bd in (8, 10):
        b, bad = ic.undefined_batch(bd)
        n = b["dst_shape"][0] * b["dst_stride"]
        defined = [ic.job_defined(j, ic.NBR_W, ic.NBR_H, n, b["dst_stride"]) for j in b["jobs"]]
        assert [i for i, ok in enumerate(defined) if not ok] == bad and len(bad) == 22
