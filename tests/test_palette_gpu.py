"""GPU: svt_hip_palette_search_batch and svt_hip_palette_pred_batch against the restatement of tests/palette_cases.py (which golden/palette.npz pins
on the reference job by job), bit for bit.  Every buffer a launch writes starts as the byte 0xA5 and is compared whole, so a byte outside a job's
outputs must come back untouched; the per-job refusals run in a batch that also holds valid jobs.  No tolerance: every output is an integer.

The shapes are the smallest at which the kernels can go wrong: 4x16 and 16x4 (narrower than a map word's row in any other path), 8x8 (one pass of
the wave over the samples), 8x16 (two), 16x16 cropped to 8 rows and to 8 columns, 64x64 with 64 colours (the whole LDS slice, n = 4096 in the
random pick of an empty cluster) -- all among the batches of the case list."""
import numpy as np
import pytest

import palette_cases as pc
from svt_av1_psyex_amd import api, palette

pytestmark = pytest.mark.gpu
FILL = 0xA5


def launch(ctx, b, jobs=None, with_maps=True, pred=True, pred_maps=True, spare=2):
    jobs = b["jobs"] if jobs is None else jobs
    t = b["tables"]
    pj, dst_samples, pmap = pc.pred_jobs(jobs) if pred else (None, 0, 0)
    got = palette.run_palette_hip(ctx, b["bit_depth"], b["src"], jobs, (t["ycolor"], t["ysize"], t["ymode"]), b["params"], map_bytes=b["map_bytes"] if with_maps else 0,
                                  pred_jobs=pj, dst_samples=dst_samples, dst_stride=pc.DST_STRIDE, pred_map_bytes=pmap if pred_maps else 0, spare_jobs=spare, fill=FILL)
    return got, pj, dst_samples, pmap


def check(got, b, jobs, results, pj, dst_samples, pmap, defined=None, with_maps=True, pred_maps=True):
    """every output of the two launches against `results`; jobs that are not `defined` left every byte of theirs as it was"""
    n = len(jobs)
    defined = np.ones(n, bool) if defined is None else defined
    assert np.array_equal(got["status"][:n], np.where(defined, pc.ST_OK, pc.ST_UNDEFINED)) and np.all(got["status"][n:] == FILL)
    rec = pc.result_records(results, FILL, defined)
    for i in range(n):
        assert got["results"][i].tobytes() == rec[i].tobytes(), (i, got["results"][i]["n_colors"], got["results"][i]["n_cands"], results[i]["n_cands"])
    assert np.all(got["results"][n:].view(np.uint8) == FILL)
    if with_maps:
        want = pc.expected_maps(jobs, results, b["map_bytes"], FILL, defined)
        assert np.array_equal(got["color_maps"], want), np.flatnonzero(got["color_maps"] != want)[:4].tolist()
    else:
        assert got["color_maps"] is None
    if pj is not None:
        dst, cmap, status = pc.expected_pred(b["bit_depth"], results, pj, dst_samples, pmap, FILL, defined)
        assert np.array_equal(got["pred_status"], status), np.flatnonzero(got["pred_status"] != status)[:4].tolist()
        assert np.array_equal(got["dst"].reshape(dst.shape), dst), np.argwhere(got["dst"].reshape(dst.shape) != dst)[:4].tolist()
        if pred_maps:
            assert np.array_equal(got["pred_map"], cmap)
            if with_maps:  # the prediction's map is the search's, byte for byte
                for p, st in zip(pj, status):
                    if st == pc.ST_OK:
                        j = jobs[int(p["search_index"])]
                        wh = int(j["width"]) * int(j["height"])
                        o = int(j["map_offset"]) + int(p["cand_index"]) * wh
                        assert np.array_equal(got["pred_map"][int(p["map_offset"]):int(p["map_offset"]) + wh], got["color_maps"][o:o + wh])


@pytest.mark.parametrize("name", pc.batch_names())
def test_every_output_equals_the_restatement_bit_for_bit(hip_ctx, name):
    """the search with color_maps, then a prediction for every one of the 14 slots of every job: those past n_cands get 0xFF and write nothing"""
    b = pc.batch(name)
    got, pj, dst_samples, pmap = launch(hip_ctx, b)
    res = pc.restated(name)
    assert any(r["n_cands"] for r in res) and len(pj) == pc.MAX_CANDS * len(res)
    check(got, b, b["jobs"], res, pj, dst_samples, pmap)


@pytest.mark.parametrize("name", ["crop_8", "colors_10"])
def test_without_the_optional_maps(hip_ctx, name):
    """color_maps == NULL and color_map == NULL: the same results and samples"""
    b = pc.batch(name)
    got, pj, dst_samples, pmap = launch(hip_ctx, b, with_maps=False, pred_maps=False)
    check(got, b, b["jobs"], pc.restated(name), pj, dst_samples, pmap, with_maps=False, pred_maps=False)
    got, pj, dst_samples, pmap = launch(hip_ctx, b, with_maps=False, pred_maps=True)  # the prediction writes the winner's map though the search kept none
    check(got, b, b["jobs"], pc.restated(name), pj, dst_samples, pmap, with_maps=False, pred_maps=True)


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_write_their_status_and_nothing_else(hip_ctx, bd):
    b, bad = pc.undefined_batch(bd)
    jobs = b["jobs"]
    defined = np.array([pc.job_defined(j, bd, pc.STRIDE, b["src"].size, b["map_bytes"]) for j in jobs])
    assert sorted(np.flatnonzero(~defined)) == bad
    empty = {"n_colors": 0, "n_cands": 0, "cands": []}
    results = [pc.restate_job(b["src"], bd, j, b["params"], b["tables"]) if ok else empty for j, ok in zip(jobs, defined)]
    assert sum(r["n_cands"] for r in results) > 20
    got, pj, dst_samples, pmap = launch(hip_ctx, b, jobs=jobs)
    check(got, b, jobs, results, pj, dst_samples, pmap, defined=defined)
    # without color_maps the map offset is not looked at: that job is defined
    defined2 = np.array([pc.job_defined(j, bd, pc.STRIDE, b["src"].size) for j in jobs])
    assert defined2.sum() == defined.sum() + 1
    got, _, _, _ = launch(hip_ctx, b, jobs=jobs, with_maps=False, pred=False)
    assert np.array_equal(got["status"][:len(jobs)], np.where(defined2, pc.ST_OK, pc.ST_UNDEFINED))


def test_undefined_prediction_jobs(hip_ctx):
    """a search index out of range, a destination and a map that leave their buffers, among valid ones"""
    b = pc.batch("step2_8")
    res = pc.restated("step2_8")
    pj, dst_samples, pmap = pc.pred_jobs(b["jobs"], res)
    want_dst, want_map, want_st = pc.expected_pred(8, res, pj, dst_samples, pmap, FILL)
    assert np.all(want_st == pc.ST_OK) and len(pj) > 20
    pj = pj.copy()
    for i, (k, v) in enumerate([("search_index", len(res)), ("search_index", 0xFFFFFFFF), ("dst_offset", dst_samples - 20), ("map_offset", pmap - 3), ("cand_index", 0xFFFFFFFF)]):
        pj[3 * i + 1][k] = v
    bad = np.zeros(len(pj), bool)
    bad[1:14:3] = True
    keep = [p for p, x in zip(pj, bad) if not x]
    want_dst, want_map, _ = pc.expected_pred(8, res, np.array(keep, pc.PRED_JOB_DTYPE), dst_samples, pmap, FILL)
    t = b["tables"]
    got = palette.run_palette_hip(hip_ctx, 8, b["src"], b["jobs"], (t["ycolor"], t["ysize"], t["ymode"]), b["params"], pred_jobs=pj, dst_samples=dst_samples,
                                  dst_stride=pc.DST_STRIDE, pred_map_bytes=pmap, fill=FILL)
    assert np.array_equal(got["pred_status"], np.where(bad, pc.ST_UNDEFINED, pc.ST_OK))
    assert np.array_equal(got["dst"].reshape(want_dst.shape), want_dst) and np.array_equal(got["pred_map"], want_map)


def test_an_empty_batch_and_a_refused_descriptor_enqueue_nothing(hip_ctx):
    b = dict(pc.batch("step2_10"))
    n = len(b["jobs"])
    got, _, _, _ = launch(hip_ctx, b, jobs=b["jobs"][:0], pred=False, spare=n)
    assert np.all(got["status"] == FILL) and np.all(got["color_maps"] == FILL) and np.all(got["results"].view(np.uint8) == FILL)
    b["params"] = dict(b["params"], dominant_color_step=3)
    with pytest.raises(api.SvtHipError, match="dominant_color_step"):
        launch(hip_ctx, b, pred=False)
