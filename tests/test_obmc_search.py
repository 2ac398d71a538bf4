"""CPU: the restatement of the OBMC motion search (tests/obmc_search_cases.py) against the reference's own results (golden/obmc.npz: every output of
every job of single_motion_search and the two av1me.c functions), the conditions of the planted inputs recomputed from the restatement, the struct
lay-outs of abi.py against the library's, and svt_hip_obmc_search_check_desc."""
import ctypes as C

import numpy as np
import pytest

import obmc_cases as oc
import obmc_search_cases as sc
from abi_mirror import check_layout
from batch_entry_cases import good_obmc_search_desc as good_desc
from svt_av1_psyex_amd import abi, api, obmc

BAD_PARAM = 2
FIELDS = ("fullpel_value", "besterr", "distortion", "sse1", "rate_mv")


@pytest.fixture(scope="module")
def golden():
    return np.load(oc.GOLDEN)


@pytest.mark.parametrize("level", range(5))
def test_grid_restatement_equals_the_reference_on_every_job(golden, level):
    names = [n for n, b in sc.batches().items() if n.startswith("grid") and b["params"]["refine_level"] == level]
    assert len(names) == 16
    for name in names:
        mv, res, _ = sc.restated(name)
        assert np.array_equal(mv, golden[f"searchmv_{name}"]), name
        assert np.array_equal(np.array([[r[k] for k in FIELDS] for r in res], np.int64), golden[f"search_{name}"]), name


def test_planted_restatement_equals_the_reference_and_meets_its_conditions(golden):
    for name in sc.planted_batches():
        mv, res, _ = sc.restated(name)
        assert np.array_equal(mv, golden[f"searchmv_{name}"]), name
        assert np.array_equal(np.array([[r[k] for k in FIELDS] for r in res], np.int64), golden[f"search_{name}"]), name
    # the generator asserts the same on the reference's results, which the restatement equals on every output of every job
    assert sc.planted_missing() == []


def test_the_search_cases_are_what_the_issue_lists(golden):
    grid = {tuple(b["params"][k] for k in ("refine_level", "approx_inter_rate", "fpel_search_diag", "fpel_search_range", "allow_hp"))
            for n, b in sc.batches().items() if n.startswith("grid")}
    assert grid == {(l, r, d, s, hp) for l in range(5) for r in (0, 1) for d in (0, 1) for s in (8, 16) for hp in (0, 1)}
    assert sc.SIZES == [(8, 8), (16, 8), (32, 32), (64, 64)]
    for n, b in sc.batches().items():
        if n.startswith("grid"):
            assert [(int(j["width"]), int(j["height"])) for j in b["jobs"]] == sc.SIZES
    assert {k[7:] for k in golden.files if k.startswith("search_")} == set(sc.batches()) == {k[9:] for k in golden.files if k.startswith("searchmv_")}
    # levels 2 and 4 start the sub-pel search from start_mv >> 3 and never run the full-pel one
    for n in ("grid_2_0_0_8_1", "grid_4_1_1_16_0"):
        res, ev = sc.restated(n)[1:]
        assert not res["fullpel_value"].any() and all(e["fp_stop"] is None for e in ev)
    # without allow_hp the third round does not run: every MV is even
    assert not (sc.restated("grid_0_0_0_8_0")[0] & 1).any() and (sc.restated("grid_0_0_0_8_1")[0] & 1).any()


def test_every_search_read_lies_inside_the_plane_and_the_guard_is_tight():
    """restate_job asserts for every job that what it read lies inside what the per-job guard proved; here: inside the padded plane too, and some job
    reads the guard's first row, first column, last row and last column (range + 5 before the co-located block, range + 5 after): no slack either way"""
    at_guard = np.zeros(4, int)
    for name, b in sc.batches().items():
        shape = sc.ref_plane(b["ref"]).shape
        for e in sc.restated(name)[2]:
            assert e["reads"][0] >= 0 and e["reads"][1] >= 0 and e["reads"][2] < shape[0] and e["reads"][3] < shape[1], name
            at_guard += np.array(e["reads_at_guard"])
    assert at_guard.all(), at_guard
    # the jobs of the undefined batch that start or end exactly at the buffer are defined and read nothing outside it
    b, bad = sc.undefined_batch()
    ref, tables = sc.ref_plane(b["ref"]), sc.cost_tables()
    for kind in ("ref_before_by_one", "ref_after_by_one"):
        j = b["jobs"][bad[kind] - 2]
        e = sc.restate_job(b["params"], ref, b["wsrc"], b["mask"], j, tables)[2]
        assert e["reads"][0] >= 0 and e["reads"][2] < ref.shape[0]


def test_struct_layouts_match_the_library():
    structs = (abi.ObmcNeighbourDesc, abi.ObmcBlendDesc, abi.ObmcTargetDesc, abi.ObmcBlock, abi.ObmcNeighbour, abi.ObmcJob, abi.ObmcSearchDesc, abi.ObmcSearchJob,
               abi.ObmcSearchResult)
    check_layout("svt_hip_obmc_layout", structs, only=(6, 7, 8), multiple_of_8=True)  # 0 .. 5: tests/test_obmc.py
    for dtype, t, mine in ((abi.OBMC_SEARCH_JOB_DTYPE, abi.ObmcSearchJob, sc.JOB_DTYPE), (abi.OBMC_SEARCH_RESULT_DTYPE, abi.ObmcSearchResult, sc.RESULT_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(t) and np.dtype(mine) == dt
        for name, *_ in t._fields_:
            off = getattr(t, name).offset
            assert dt.fields[name][1] == off, name


def test_check_desc_accepts_good_descriptors():
    obmc.check_search_desc(good_desc())
    obmc.check_search_desc(good_desc(1))  # the light rate forms read no table


BAD = ["no_ref", "no_wsrc", "no_mask", "no_jobs", "no_best_mv", "no_results", "no_status", "no_mvjcost", "no_mvcost", "ref_bit_depth_10", "ref_bit_depth_0",
       "refine_level_5", "fpel_search_range_65", "zero_ref_stride", "zero_ref_samples", "zero_target_values"]


@pytest.mark.parametrize("bad", BAD)
def test_check_desc_and_batch_refuse_with_an_error_text(bad):
    L = api.lib()
    d = good_desc()
    if bad == "no_mvcost":
        d.mvcost[1] = None
    elif bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith("zero_"):
        assert hasattr(type(d), bad[5:])
        setattr(d, bad[5:], 0)
    else:
        name, v = bad.rsplit("_", 1)
        assert hasattr(type(d), name)
        setattr(d, name, int(v))
    assert L.svt_hip_obmc_search_check_desc(C.byref(d)) == BAD_PARAM
    assert b"svt_hip_obmc_search_check_desc" in L.svt_hip_last_error(None)
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    assert L.svt_hip_obmc_search_batch(ctx, C.byref(d)) == BAD_PARAM
    assert L.svt_hip_obmc_search_check_desc(None) == BAD_PARAM and L.svt_hip_obmc_search_batch(None, None) == BAD_PARAM


def test_job_defined_names_every_undefined_kind():
    b, bad = sc.undefined_batch()
    ref, tables = sc.ref_plane(b["ref"]), sc.cost_tables()
    undefined = [i for i, j in enumerate(b["jobs"]) if sc.restate_job(b["params"], ref, b["wsrc"], b["mask"], j, tables) is None]
    assert undefined == sorted(bad.values()) and list(bad) == sc.UNDEFINED_KINDS
