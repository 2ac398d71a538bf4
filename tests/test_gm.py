"""CPU: the restatements of the global-motion refinement and of the MV correspondences (tests/gm_cases.py) against the reference's own results
(golden/gm.npz: svt_av1_refine_integerized_param and correspondence_from_mvs themselves, driven by tools/gen_gm_golden.py), the coverage conditions
recomputed from the restatements, the struct lay-outs of abi.py against the library's, the two descriptor validations and the empty batch (they need
no GPU)."""
import ctypes as C

import numpy as np
import pytest

import gm_cases as gc
from abi_mirror import check_layout
from svt_av1_psyex_amd import abi, api, gm

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(gc.GOLDEN)


# ---- the restatements against the fixture ----
@pytest.mark.parametrize("name", gc.batch_names())
def test_refinement_restatement_equals_the_reference_on_every_output(golden, name):
    """the final matrix, its shear parameters, wmtype and valid, best_error, pic_sad, status and the error of every evaluation"""
    for key, mine in gc.fixture_arrays(name, gc.restated(name)[0]).items():
        assert mine.dtype == golden[key].dtype and np.array_equal(mine, golden[key]), key


@pytest.mark.parametrize("name", list(gc.CORR_CASES))
def test_correspondence_restatement_equals_the_reference(golden, name):
    for key, mine in gc.corr_fixture_arrays(name, gc.restated_corr(name)).items():
        assert mine.dtype == golden[key].dtype and np.array_equal(mine, golden[key]), key


def test_the_fixture_holds_exactly_the_generators_keys(golden):
    keys = {k for n in gc.batch_names() for k in gc.fixture_arrays(n, gc.restated(n)[0])} | {k for n in gc.CORR_CASES for k in gc.corr_fixture_arrays(n, gc.restated_corr(n))}
    assert set(golden.files) == keys


def test_a_changed_sample_changes_the_restatement():
    """the comparison can fail: one source sample off by one changes the first error"""
    b = dict(gc.batch("raw_32x32_0"))
    want = gc.restated("raw_32x32_0")[0]["round_error"][0, 0]
    plane, ox, oy, pw, ph = b["src"]
    plane = plane.copy()
    plane[oy + 5, ox + 7] ^= 1
    b["src"] = (plane, ox, oy, pw, ph)
    assert gc.restate_refine(b)["round_error"][0, 0] in (want - 1, want + 1)


# ---- coverage ----
def test_refinement_coverage_conditions_hold():
    """left / right / right after left accepted, right equal to left, nothing accepted, both clamps, both refusals, a refusal behind a warp, the ROTZOOM
    stale shear deciding a kept parameter, both ends of rfn_early_exit, best_frame_error below the first error, pic_sad 0, a final wmtype other than the
    job's, a chess block row without a block, tiles straddling both edges; every picture size with chess on and off"""
    assert gc.coverage_missing() == []
    assert gc.coverage_missing(["raw_32x32_0"]) != []  # the check can fail
    s = list(gc.BATCHES.values())
    assert {v[1] for v in s} == set(gc.SIZES) and {v[3] for v in s} >= {0, 1, 5} and {len(v[5]) for v in s} >= {1, 2, 5}
    assert {int(j["wmtype"]) for v in s for j in v[5]} >= {1, 2, 3}
    assert any(len({int(j["ref"]) for j in v[5]}) > 1 and len({int(j["wmtype"]) for j in v[5]}) > 1 for v in s)


def test_correspondence_coverage_conditions_hold():
    """a pair no candidate names, a negative pos + mv, the aligned size cutting a column and a row of blocks, bi-predictive candidates passed over, both
    folds of the PU index; the four methods, the three PU counts, the three shifts, P and B"""
    assert gc.corr_coverage_missing() == []
    assert gc.corr_coverage_missing(["m64_p"]) != []
    s = list(gc.CORR_CASES.values())
    assert {v[1] for v in s} == {0, 1, 2, 3} and {v[2] for v in s} == {0, 1, 2} and {gc.n_pu_of(*v[3]) for v in s} == {85, 21, 5} and {v[4] for v in s} == {"P", "B"}


# ---- lay-outs ----
MIRRORS = (abi.GmRefineDesc, abi.GmRefineJob, abi.GmCorrDesc, abi.GmPair)


def test_struct_layouts_match_the_library():
    check_layout("svt_hip_gm_layout", MIRRORS)
    dt = np.dtype(abi.GM_REFINE_JOB_DTYPE)
    assert dt.itemsize == C.sizeof(abi.GmRefineJob) and abi.GM_REFINE_JOB_DTYPE == gc.REFINE_JOB_DTYPE
    for name, *_ in abi.GmRefineJob._fields_:
        assert dt.fields[name][1] == getattr(abi.GmRefineJob, name).offset, name
    assert C.sizeof(abi.GmRefineDesc) % 8 == 0 and C.sizeof(abi.GmRefineJob) % 8 == 0 and C.sizeof(abi.GmCorrDesc) % 8 == 0
    assert (abi.GM_OK, abi.GM_IDENTICAL, abi.GM_UNDEFINED) == (gc.ST_OK, gc.ST_IDENTICAL, gc.ST_UNDEFINED) == (0, 1, 0xFF)
    assert (abi.GM_IDENTITY, abi.GM_TRANSLATION, abi.GM_ROTZOOM, abi.GM_AFFINE) == (gc.IDENTITY, gc.TRANSLATION, gc.ROTZOOM, gc.AFFINE)
    assert (abi.GM_ROTZOOM, abi.GM_AFFINE) == (abi.WARP_ROTZOOM, abi.WARP_AFFINE) and abi.GM_ROUND_ERRORS == gc.N_ERRORS == 1 + 2 * 5 * 6
    assert abi.GM_NO_FRAME_ERROR == gc.INT64_MAX and abi.WARP_MODEL_DTYPE == gc.MODEL_DTYPE
    assert gm.work_bytes(0) < gm.work_bytes(1) < gm.work_bytes(5) and gm.work_bytes(5) - gm.work_bytes(4) == gm.work_bytes(1) - gm.work_bytes(0)


# ---- svt_hip_gm_refine_check_desc ----
def plane(stride=144, org_x=8, org_y=8, width=128, height=96, rows=112):
    return abi.WarpRef(plane=0x1000, stride=stride, org_x=org_x, org_y=org_y, width=width, height=height, rows=rows)


def good_refine_desc(n_refs=2, n_jobs=3):
    d = abi.GmRefineDesc(n_jobs=n_jobs, n_refs=n_refs, n_refinements=5, chess_refn=1, rfn_early_exit=1, src=plane(), jobs=0x2000, work=0x3000, models=0x4000,
                         best_error=0x5000, pic_sad=0x6000, status=0x7000, round_error=0x8000)
    for i in range(n_refs):
        d.refs[i] = plane()
    return d


def spoil(d, bad):
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith(("ref_", "src_")):
        who, name, v = bad.split("_")
        setattr(d.refs[1] if who == "ref" else d.src, name, None if name == "plane" else int(v))
    else:
        name, _, v = bad.rpartition("_")
        setattr(d, name, int(v))
    return d


def test_refine_check_desc_accepts_a_good_descriptor():
    for n_refs in (1, 8):
        gm.check_refine_desc(good_refine_desc(n_refs))
    d = good_refine_desc()
    d.round_error, d.n_refinements, d.n_jobs = None, 0, 0
    gm.check_refine_desc(d)
    d = good_refine_desc()
    d.refs[0].org_x, d.refs[0].org_y = 16, 16  # the picture ends on the plane's last column and row
    gm.check_refine_desc(d)


REFINE_BAD = ["null_desc", "no_jobs", "no_work", "no_models", "no_best_error", "no_pic_sad", "no_status", "work_12292", "n_jobs_65536", "n_refs_0", "n_refs_9", "n_refinements_6",
              "ref_plane_0", "ref_stride_0", "ref_width_0", "ref_height_0", "ref_rows_103", "ref_stride_135", "src_plane_0", "src_rows_103", "src_stride_135",
              "ref_width_126", "ref_height_94", "src_width_126"]


@pytest.mark.parametrize("bad", REFINE_BAD)
def test_refine_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    if bad == "null_desc":
        assert L.svt_hip_gm_refine_check_desc(None) == BAD_PARAM and L.svt_hip_gm_refine_batch(ctx, None) == BAD_PARAM
    else:
        d = spoil(good_refine_desc(), bad)
        assert L.svt_hip_gm_refine_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_gm_refine_check_desc"):
            gm.check_refine_desc(d)
        assert L.svt_hip_gm_refine_batch(ctx, C.byref(d)) == BAD_PARAM
    assert b"svt_hip_gm_refine" in L.svt_hip_last_error(None)


def test_an_empty_refine_batch_returns_0_and_touches_nothing():
    L = api.lib()
    d = good_refine_desc(n_jobs=0)
    assert L.svt_hip_gm_refine_batch(C.create_string_buffer(8192), C.byref(d)) == 0
    assert L.svt_hip_gm_refine_batch(None, C.byref(d)) == BAD_PARAM


# ---- svt_hip_gm_corr_check_desc ----
def good_corr_desc(e16=1, e8=1, method=3):
    me = abi.MeResults()
    for i, name in enumerate(gm.ME_ARRAYS):
        setattr(me, name, 0x1000 * (i + 1))
    pic = {"aligned_width": 168, "aligned_height": 104, "enable_me_8x8": e8, "enable_me_16x16": e16, "max_cand": 9, "max_refs": 4, "max_l0": 2}
    return gm.corr_desc(pic, method, 1, [(0, 0), (0, 1), (1, 0), (1, 1)], (1 << (2 * method)) * 6, me, 0x9000, 0xA000, 0xB000)


def test_corr_check_desc_accepts_a_good_descriptor():
    for e16, e8 in ((1, 1), (1, 0), (0, 0)):
        for method in range(4):
            gm.check_corr_desc(good_corr_desc(e16, e8, method))
    d = good_corr_desc()
    d.n_pairs, d.corr, d.count, d.cap = 0, None, None, 0  # the sums alone
    gm.check_corr_desc(d)


CORR_BAD = ["null_desc", "no_corr", "no_count", "no_sums", "me_total_me_candidate_index", "me_me_candidate_array", "me_me_mv_array", "me_rc_me_distortion",
            "me_stationary_block_present_sb", "me_rc_me_allow_gm", "aligned_width_0", "aligned_height_0", "method_4", "shift_3", "n_pairs_9", "n_pu_21", "n_pu_84",
            "enable_me_16x16_0", "max_cand_0", "max_refs_0", "cap_383", "pair_list_2", "pair_ref_2"]


@pytest.mark.parametrize("bad", CORR_BAD)
def test_corr_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)
    if bad == "null_desc":
        assert L.svt_hip_gm_corr_check_desc(None) == BAD_PARAM and L.svt_hip_gm_correspondence_batch(ctx, None) == BAD_PARAM
    else:
        d = good_corr_desc()
        if bad.startswith("me_"):
            setattr(d.me, bad[3:], None)
        elif bad.startswith("pair_"):
            setattr(d.pairs[3], bad.split("_")[1], int(bad.split("_")[2]))  # list 2; reference 2 of list 1: MV slot 4 of 4
        else:
            spoil(d, bad)
        assert L.svt_hip_gm_corr_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_gm_corr_check_desc"):
            gm.check_corr_desc(d)
        assert L.svt_hip_gm_correspondence_batch(ctx, C.byref(d)) == BAD_PARAM
    assert b"svt_hip_gm_corr" in L.svt_hip_last_error(None)
    assert L.svt_hip_gm_correspondence_batch(None, C.byref(good_corr_desc())) == BAD_PARAM
