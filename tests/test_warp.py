"""CPU: the restatements of the warped-motion prediction, of the local-warp fit and of the MV refinement (tests/warp_cases.py) against the
reference's own results (golden/warp.npz: svt_av1_warp_plane over the _c kernels, svt_aom_select_samples, svt_find_projection and
svt_aom_wm_motion_refinement itself, driven by tools/gen_warp_golden.py), the filter and divisor tables, the coverage conditions recomputed from the
restatements, the struct lay-outs of abi.py against the library's, and the two descriptor validations (they need no GPU)."""
import ctypes as C

import numpy as np
import pytest

import warp_cases as wc
from abi_mirror import check_layout
from batch_entry_cases import good_warp_model_desc, good_warp_pred_desc as good_desc, good_wm_refine_desc as good_refine_desc
from svt_av1_psyex_amd import abi, api, warp

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(wc.GOLDEN)


# ---- the tables ----
def test_every_filter_row_sums_to_128_and_the_table_is_the_references(golden):
    filt, _ = warp.tables()
    assert filt.shape == (193, 8) and filt.dtype == np.int16
    assert np.all(filt.sum(1) == 128)
    assert np.array_equal(filt[192], filt[191]) and list(filt[0]) == [0, 0, 127, 1, 0, 0, 0, 0] and list(filt[64]) == [0, 0, 0, 127, 1, 0, 0, 0]
    assert wc.table_crc(filt, "<i2") == int(golden["filter_crc"][0])
    broken = filt.copy()
    broken[100, 3] += 1
    assert wc.table_crc(broken, "<i2") != int(golden["filter_crc"][0])  # the check can fail


def test_divisor_table_is_round_2_22_over_256_plus_i(golden):
    _, lut = warp.tables()
    want = np.array([round((1 << 22) / (256 + i)) for i in range(257)])
    assert all(abs((1 << 22) / (256 + i) - int((1 << 22) / (256 + i)) - 0.5) > 1e-9 for i in range(257))  # no tie: round() is unambiguous
    assert np.array_equal(lut, want) and np.array_equal(wc.div_lut(), want)
    assert (int(lut[0]), int(lut[256])) == (16384, 8192)
    assert wc.table_crc(lut, "<u2") == int(golden["div_lut_crc"][0])


# ---- the restatements against the fixture ----
@pytest.mark.parametrize("name", wc.batch_names())
def test_prediction_restatement_equals_the_reference_on_every_job(golden, name):
    b = wc.batch(name)
    _, status, blocks, _ = wc.restated(name)
    assert np.all(status == wc.ST_OK), name
    crcs = np.array([wc.block_crc(blocks[i]) for i in range(len(b["jobs"]))], np.uint32)
    assert np.array_equal(crcs, golden[f"crc_{name}"]), name


def test_sample_blocks_equal_the_reference_sample_by_sample(golden):
    """one whole block per size and depth, so that a mismatch can be looked at"""
    seen = set()
    for key, name, i in wc.sample_jobs():
        j = wc.batch(name)["jobs"][i]
        assert np.array_equal(wc.restated(name)[2][i], golden[key]) and golden[key].dtype == np.uint16, key
        assert golden[key].shape == (int(j["height"]), int(j["width"]))
        seen.add((wc.batch(name)["bit_depth"], int(j["width"]), int(j["height"])))
    assert seen == {(bd, w, h) for bd in (8, 10) for w, h in wc.SIZES} and len(wc.SIZES) == 17


@pytest.mark.parametrize("name", list(wc.MODEL_BATCHES))
def test_fit_restatement_equals_the_reference(golden, name):
    models, status, _ = wc.restated_models(name)
    assert np.all(status == wc.ST_OK)
    assert np.array_equal(wc.models_crc(models, status), golden[f"fit_{name}"])
    invalid = models[models["valid"] == 0]
    assert len(invalid) and not invalid["wmmat"].any() and not any(invalid[k].any() for k in ("alpha", "beta", "gamma", "delta"))  # defined: zero
    assert np.all(models["wmtype"] == wc.AFFINE)


@pytest.mark.parametrize("name", list(wc.REFINE_BATCHES))
def test_refinement_restatement_equals_svt_aom_wm_motion_refinement(golden, name):
    """the best MV, the positions tested (tot_checked_pos = the calls of svt_aom_warped_motion_parameters) and the positions warped"""
    want, _ = wc.restated_refine(name)
    ref = golden[f"refine_{name}"]
    assert np.all(want["status"] == wc.ST_OK)
    assert np.array_equal(want["best_mv"], ref[:, :2]) and np.array_equal(want["n_checked"], ref[:, 2]) and np.array_equal(want["n_valid"], ref[:, 3])
    assert np.array_equal(want["best_cost"] == wc.INT_MAX, ref[:, 3] == 0)


def test_the_fixture_holds_exactly_the_generators_keys(golden):
    keys = ({f"crc_{n}" for n in wc.batch_names()} | {k for k, _, _ in wc.sample_jobs()} | {f"fit_{n}" for n in wc.MODEL_BATCHES}
            | {f"refine_{n}" for n in wc.REFINE_BATCHES} | {"filter_crc", "div_lut_crc"})
    assert set(golden.files) == keys


# ---- coverage ----
def test_prediction_coverage_conditions_hold():
    """filter index 0 and 192 in each direction, all shears zero, a shear of each sign, tiles wholly outside and across each edge, a picture that is
    no multiple of 8, a negative projection on a sub-sampled plane, ROTZOOM and AFFINE, every quant_dist pair"""
    assert wc.pred_coverage_missing() == []


def test_fit_coverage_conditions_hold():
    """n_samples 1 .. 8, a sample dropped by LS_MV_MAX, det == 0, shear refused, each band test, each clamp, none / all / a mixed set kept by
    svt_aom_select_samples, thresh at 16 and at 112.  wmmat[2] <= 0 and shift < 0 are unreachable: see warp_cases.model_coverage_missing"""
    assert wc.model_coverage_missing() == []
    assert wc.model_coverage_missing(["open"]) != []  # the check can fail: without the band tests none fires


def test_refinement_coverage_conditions_hold():
    """a stop because the centre did not move, a run out of iterations, a skip by mv_record and one by prev_mv, an invalid fit in mid-search, a job
    with no valid position, a tie resolved by the strict <; both cost forms, both precisions, diagonals on and off, 1, 8 and 16 iterations"""
    assert wc.refine_coverage_missing() == []
    assert wc.refine_coverage_missing(["one"]) != []
    s = [dict(zip(wc.SETTING_KEYS, v)) for v in wc.REFINE_BATCHES.values()]
    assert {x["iterations"] for x in s} == {1, 8, 16} and {x["refine_diag"] for x in s} == {0, 1} and {x["mv_prec_shift"] for x in s} == {0, 1}
    assert {x["approx_inter_rate"] for x in s} == {0, 1}
    sizes = {(int(j["bwidth"]), int(j["bheight"])) for n in wc.REFINE_BATCHES for j in wc.refine_batch(n)["jobs"]}
    assert {(8, 8), (16, 16), (32, 16), (64, 64)} <= sizes


def test_the_rate_forms():
    tables = wc.cost_tables(np.random.default_rng(3))
    assert wc.mv_err_cost_light((5, -3), (1, 4)) == 1296 + 50 * (4 + 7)
    jc, tr, tc = tables
    bits = int(jc[3]) + int(tr[wc.MV_CENTRE + 4]) + int(tc[wc.MV_CENTRE - 7])
    assert wc.mv_err_cost((5, -3), (1, 4), tables, 77) == (bits * 77 + (1 << 13)) >> 14


# ---- lay-outs ----
MIRRORS = (abi.WarpPredDesc, abi.WarpPredJob, abi.WarpRef, abi.WarpModel, abi.WarpModelDesc, abi.WarpModelJob, abi.WmRefineDesc, abi.WmRefineJob)


def test_struct_layouts_match_the_library():
    check_layout("svt_hip_warp_layout", MIRRORS, multiple_of_8=True)
    for dtype, mirror, own in ((abi.WARP_MODEL_DTYPE, abi.WarpModel, wc.MODEL_DTYPE), (abi.WARP_PRED_JOB_DTYPE, abi.WarpPredJob, wc.PRED_JOB_DTYPE),
                               (abi.WARP_MODEL_JOB_DTYPE, abi.WarpModelJob, wc.MODEL_JOB_DTYPE), (abi.WM_REFINE_JOB_DTYPE, abi.WmRefineJob, wc.REFINE_JOB_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(mirror) and dtype == own
        for name, *_ in mirror._fields_:
            assert dt.fields[name][1] == getattr(mirror, name).offset, name
    assert (abi.WARP_OK, abi.WARP_NO_MODEL, abi.WARP_UNDEFINED) == (wc.ST_OK, wc.ST_NO_MODEL, wc.ST_UNDEFINED) == (0, 0xFE, 0xFF)
    assert (abi.WARP_ROTZOOM, abi.WARP_AFFINE, abi.WARP_NO_REF, abi.WM_NO_COST) == (wc.ROTZOOM, wc.AFFINE, wc.NO_REF, wc.INT_MAX)
    assert (abi.WARP_MODEL0_FROM_ARRAY, abi.WARP_MODEL1_FROM_ARRAY, abi.WARP_MV_FROM_ARRAY, abi.WM_START_FROM_ARRAY) == (1, 2, 1, 1)


# ---- svt_hip_warp_check_desc ----
def spoil(d, bad):
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad.startswith("ref_"):
        _, name, v = bad.split("_")
        setattr(d.refs[1], name, None if name == "plane" else int(v))
    else:
        name, _, v = bad.rpartition("_")
        setattr(d, name, int(v))
    return d


def test_check_desc_accepts_a_good_descriptor():
    for bd in (8, 10):
        for n_refs in (1, 8):
            warp.check_desc(good_desc(bd, n_refs))
    d = good_desc()
    d.ss_x = d.ss_y = 1
    d.models, d.n_models = None, 0
    warp.check_desc(d)
    d = good_desc()
    d.refs[0].org_x, d.refs[0].org_y = 32, 16  # the picture ends on the plane's last column and row
    warp.check_desc(d)


BAD = ["null_desc", "no_dst", "no_jobs", "no_status", "bit_depth_12", "bit_depth_0", "bit_depth_9", "ss_x_2", "ss_y_2", "n_refs_0", "n_refs_9", "ref_plane_0",
       "ref_stride_0", "ref_width_0", "ref_height_0", "ref_width_145", "ref_height_105", "ref_rows_103", "ref_stride_143", "dst_stride_0", "dst_samples_0",
       "no_models"]


@pytest.mark.parametrize("bad", BAD)
def test_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    if bad == "null_desc":
        assert L.svt_hip_warp_check_desc(None) == BAD_PARAM
    else:
        d = spoil(good_desc(), bad)
        assert L.svt_hip_warp_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_warp_check_desc"):
            warp.check_desc(d)
    assert b"svt_hip_warp_check_desc" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("bad", ["null_ctx", "null_desc", "bit_depth_12", "ss_x_2", "n_refs_9", "ref_rows_103", "no_status", "no_models"])
def test_pred_batch_rejects_a_bad_descriptor_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_desc()
    if bad == "null_ctx":
        assert L.svt_hip_warp_pred_batch(None, C.byref(d)) == BAD_PARAM
    elif bad == "null_desc":
        assert L.svt_hip_warp_pred_batch(ctx, None) == BAD_PARAM
    else:
        assert L.svt_hip_warp_pred_batch(ctx, C.byref(spoil(d, bad))) == BAD_PARAM
    assert b"svt_hip_warp" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("bad", ["null_ctx", "null_desc", "no_jobs", "no_models", "no_status", "no_mv_array"])
def test_model_batch_rejects_a_bad_descriptor_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)
    d = good_warp_model_desc()
    if bad == "null_ctx":
        assert L.svt_hip_warp_model_batch(None, C.byref(d)) == BAD_PARAM
    elif bad == "null_desc":
        assert L.svt_hip_warp_model_batch(ctx, None) == BAD_PARAM
    else:
        assert L.svt_hip_warp_model_batch(ctx, C.byref(spoil(d, bad))) == BAD_PARAM
    assert b"svt_hip_warp_model_batch" in L.svt_hip_last_error(None)


# ---- svt_hip_wm_refine_check_desc ----
def test_refine_check_desc_accepts_a_good_descriptor():
    warp.check_refine_desc(good_refine_desc())
    warp.check_refine_desc(good_refine_desc(light=1))  # no cost table is needed
    for it in (1, 16):
        for waves in (0, 1, 4):
            d = good_refine_desc()
            d.iterations, d.waves_per_job, d.error_per_bit = it, waves, 0
            warp.check_refine_desc(d)


REFINE_BAD = ["null_desc", "no_src", "no_jobs", "no_best_mv", "no_best_cost", "no_n_checked", "no_status", "iterations_0", "iterations_17", "mv_prec_shift_2",
              "waves_per_job_2", "waves_per_job_8", "n_refs_0", "n_refs_9", "src_stride_0", "src_samples_0", "no_mv_array", "error_per_bit_-1", "no_mvjcost",
              "rows_100"]


@pytest.mark.parametrize("bad", REFINE_BAD)
def test_refine_check_desc_refuses_with_an_error_text(bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)
    if bad == "null_desc":
        assert L.svt_hip_wm_refine_check_desc(None) == BAD_PARAM and L.svt_hip_wm_refine_batch(ctx, None) == BAD_PARAM
    else:
        d = good_refine_desc()
        if bad == "rows_100":
            d.refs[0].rows = 100  # the picture ends below the plane
        else:
            spoil(d, bad)
        assert L.svt_hip_wm_refine_check_desc(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match="svt_hip_wm_refine_check_desc"):
            warp.check_refine_desc(d)
        assert L.svt_hip_wm_refine_batch(ctx, C.byref(d)) == BAD_PARAM  # validation comes first, and a rejected call enqueues nothing
    assert b"svt_hip_wm_refine" in L.svt_hip_last_error(None)


def test_job_status_names_every_undefined_kind():
    for bd in (8, 10):
        b, expect = wc.undefined_batch(bd)
        _, status, _ = wc.restate_pred(b)
        assert {i for i, s in enumerate(status) if s != wc.ST_OK} == set(expect) and len(expect) == 19
