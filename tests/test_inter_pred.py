"""CPU: the restatement of the inter prediction (tests/inter_pred_cases.py) against the reference's own svt_aom_enc_make_inter_predictor results
(golden/inter_pred.npz), the coverage conditions recomputed from the restatement, the struct lay-outs of abi.py against the library's, and
svt_hip_inter_pred_check_desc (validation needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
from abi_mirror import check_layout
from batch_entry_cases import good_inter_pred_desc as good_desc
from svt_av1_psyex_amd import abi, api, pred

BAD_PARAM = 2
GROUPS = ["sizes", "sweep", "compound", "clamp", "extremes", "geometry"]


@pytest.fixture(scope="module")
def golden():
    return np.load(ip.GOLDEN)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", GROUPS)
def test_restatement_equals_the_reference_on_every_job(golden, group, bd):
    names = [n for n in ip.batch_names() if n.startswith(group) and ip.batch(n)["bit_depth"] == bd]
    assert names
    for name in names:
        blocks, events = ip.restated(name)
        assert all(e["inside"] for e in events), name  # the reference is defined on every job: no read leaves the padded plane
        assert np.array_equal(ip.batch_crcs(name, blocks), golden[f"crc_{name}"]), name


def test_the_fixture_holds_every_batch_and_nothing_else(golden):
    keys = {f"crc_{n}" for n in ip.batch_names()} | {k for k, _, _ in ip.sample_jobs()}
    assert set(golden.files) == keys
    for name in ip.batch_names():
        assert len(golden[f"crc_{name}"]) == (16 if name.startswith("sweep") else len(ip.batch(name)["jobs"])), name


def test_sample_blocks_equal_the_reference_sample_by_sample(golden):
    """one full block per variant x mode x depth, so that a mismatch can be looked at"""
    seen = set()
    for key, name, i in ip.sample_jobs():
        b = ip.batch(name)
        blocks, events = ip.restated(name)
        assert np.array_equal(blocks[i], golden[key]), key
        comp = int(b["jobs"][i]["ref"][1]) != ip.NO_REF
        seen.add((b["bit_depth"], events[i]["refs"][0][0], (1 + int(b["jobs"][i]["comp_mode"])) if comp else 0))
    assert seen == {(bd, v, m) for bd in (8, 10) for v in range(4) for m in range(3)}


def test_coverage_conditions_hold_on_the_restatement():
    """each of the 16 convolve functions runs, the clamp moves the MV on each side and leaves it alone, the 4-tap tables serve x alone, y alone
    and both, the output clips at 0 and at the maximum in both depths, res is negative in the 2-D single path"""
    records = []
    for name in ip.batch_names():
        b = ip.batch(name)
        records += [(b["bit_depth"], j, e) for j, e in zip(b["jobs"], ip.restated(name)[1])]
    assert ip.coverage_missing(records) == []
    assert len(records) > 40000
    assert ip.coverage_missing(records[:24]) != []  # the check can fail


def test_the_cases_are_what_the_issue_lists():
    names = ip.batch_names()
    for bd in (8, 10):
        for w, h in ip.BLOCK_SIZES:  # group 1: every size x variant x mode
            b = ip.batch(f"sizes_{w}x{h}_{bd}_ss0")
            ev = ip.restated(b["name"])[1]
            got = {(e["refs"][0][0], 0 if j["ref"][1] == ip.NO_REF else 1 + int(j["comp_mode"])) for j, e in zip(b["jobs"], ev)}
            assert got == {(v, m) for v in range(4) for m in range(3)}, b["name"]
            assert len({(int(j["filter_x"]), int(j["filter_y"])) for j in b["jobs"]}) > 4
        for w, h in ip.SWEEP_SIZES:  # group 2: 256 phases x 16 filter pairs
            b = ip.batch(f"sweep_{w}x{h}_{bd}")
            got = {(int(j["filter_x"]), int(j["filter_y"]), int(j["mv"][0][0]) & 15, int(j["mv"][0][1]) & 15) for j in b["jobs"]}
            assert len(got) == 4096 == len(b["jobs"]) and b["ss"] == 1
        c = ip.batch(f"compound_{bd}")  # group 3
        ev = ip.restated(c["name"])[1]
        dw = [j for j in c["jobs"] if j["comp_mode"] == 1]
        assert {(int(j["fwd_offset"]), int(j["bck_offset"])) for j in dw if j["ref"][0] == j["ref"][1]} == set(ip.DIST_PAIRS)
        assert {(int(j["fwd_offset"]), int(j["bck_offset"])) for j in dw if j["ref"][0] != j["ref"][1]} == set(ip.DIST_PAIRS)
        for cm in (0, 1):
            assert {(e["refs"][0][0], e["refs"][1][0]) for j, e in zip(c["jobs"], ev) if j["comp_mode"] == cm} == {(a, b) for a in range(4) for b in range(4)}
        for ss in (0, 1):  # group 4
            b = ip.batch(f"clamp_{bd}_ss{ss}")
            pw, ph, _ = ip.plane_dims(ss)
            corners = {(int(j["org_x"]) in (0, pw - int(j["width"])), int(j["org_y"]) in (0, ph - int(j["height"]))) for j in b["jobs"]}
            assert {(True, True), (True, False), (False, True)} <= corners
            moved = np.array([e["refs"][0][1] for e in ip.restated(b["name"])[1]])
            assert moved.any(axis=0).all() and (~moved).any(axis=0).all()
        e = ip.batch(f"extremes_{bd}")  # group 5
        assert [k for k, _ in e["planes"]] == ["zero", "max", "checker"] and set(e["jobs"]["filter_x"]) == {2} == set(e["jobs"]["filter_y"])
        for stride in (204, 203):  # group 6
            g = ip.batch(f"geometry_{bd}_stride{stride}")
            assert g["dst_stride"] % 16 and {int(j["dst_offset"]) % g["dst_stride"] % 16 for j in g["jobs"]} == {0, 4, 8, 12}
    assert len(names) == len(set(names))


def test_struct_layouts_match_the_library():
    check_layout("svt_hip_inter_pred_layout", (abi.InterPredDesc, abi.InterPredJob, abi.InterPredRef), multiple_of_8=True)
    dt = np.dtype(abi.INTER_PRED_JOB_DTYPE)
    assert dt.itemsize == C.sizeof(abi.InterPredJob) and abi.INTER_PRED_JOB_DTYPE == ip.JOB_DTYPE
    for name, *_ in abi.InterPredJob._fields_:
        assert dt.fields[name][1] == getattr(abi.InterPredJob, name).offset, name
    assert (abi.INTER_PRED_NO_REF, abi.INTER_PRED_MV0_FROM_ARRAY, abi.INTER_PRED_MV1_FROM_ARRAY) == (ip.NO_REF, ip.MV0_FROM_ARRAY, ip.MV1_FROM_ARRAY)
    assert (abi.INTER_PRED_OK, abi.INTER_PRED_UNDEFINED) == (ip.ST_OK, ip.ST_UNDEFINED)


def test_check_desc_accepts_a_good_descriptor():
    pred.check_desc(good_desc())
    pred.check_desc(good_desc(8))
    d = good_desc()
    d.bit_depth, d.ss_x, d.ss_y, d.mv_array, d.n_mvs = 8, 0, 0, 0x1000, 7
    pred.check_desc(d)


BAD = ["null_desc", "no_dst", "no_jobs", "no_status", "bit_depth_12", "bit_depth_0", "bit_depth_9", "ss_x_2", "ss_y_2", "n_refs_9", "n_refs_0", "null_plane",
       "zero_stride", "stride_below_width", "zero_width", "org_outside", "zero_dst_stride", "zero_dst_samples", "n_mvs_without_mv_array"]


@pytest.mark.parametrize("bad", BAD)
def test_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    if bad == "null_desc":
        assert L.svt_hip_inter_pred_check_desc(None) == BAD_PARAM
    else:
        d = ip.spoil_desc(good_desc(), bad)
        assert L.svt_hip_inter_pred_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_inter_pred_check_desc"):
            pred.check_desc(d)
    assert b"svt_hip_inter_pred_check_desc" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("bad", ["null_ctx", "null_desc", "bit_depth_12", "n_refs_9", "zero_stride", "no_status"])
def test_batch_rejects_a_bad_descriptor_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_desc()
    if bad == "null_ctx":
        assert L.svt_hip_inter_pred_batch(None, C.byref(d)) == BAD_PARAM
    elif bad == "null_desc":
        assert L.svt_hip_inter_pred_batch(ctx, None) == BAD_PARAM
    else:
        assert L.svt_hip_inter_pred_batch(ctx, C.byref(ip.spoil_desc(d, bad))) == BAD_PARAM
    assert b"svt_hip_inter_pred" in L.svt_hip_last_error(None)


def test_job_defined_names_every_undefined_kind():
    for bd in (8, 10):
        b, bad = ip.undefined_batch(bd)
        n = b["dst_shape"][0] * b["dst_stride"]
        defined = [ip.job_defined(j, len(b["planes"]), b["mv_array"], n, b["dst_stride"]) for j in b["jobs"]]
        assert [i for i, ok in enumerate(defined) if not ok] == bad and len(bad) == 24
