"""GPU: svt_hip_warp_pred_batch and svt_hip_warp_model_batch on the MI355X, every comparison exact -- against the reference's own results
(golden/warp.npz) and the restatements (tests/warp_cases.py): every size in both depths, single, averaged and distance-weighted, on the full and on
the sub-sampled plane; tiles outside and across every edge of pictures that are no multiples of 8; both ends of the filter table; job counts that
leave waves and workgroups empty; every undefined kind and the no-model status between good jobs; the fits with the MV given and taken from an
array.  Destinations, model arrays and status arrays start as the byte 0xA5 with spare slots and are compared whole; reference planes are checked
unchanged."""
import numpy as np
import pytest

import warp_cases as wc
from svt_av1_psyex_amd import warp

pytestmark = pytest.mark.gpu

FILL = wc.FILL
SPARE = 3


@pytest.fixture(scope="module")
def golden():
    return np.load(wc.GOLDEN)


def run_pred(ctx, b):
    out = warp.run_warp_pred_hip(ctx, b["bit_depth"], b["ss_x"], b["ss_y"], b["planes"], b["jobs"], b["dst_shape"], b["dst_stride"], models=b.get("models"),
                                 spare_jobs=SPARE, fill=FILL)
    n = len(b["jobs"])
    assert len(out["status"]) == n + SPARE and np.all(out["status"][n:] == FILL), "spare status slots written"
    assert all(np.array_equal(g, p[0]) for g, p in zip(out["planes"], b["planes"])), "a reference plane changed"
    return out["dst"], out["status"][:n]


def block_of(b, dst, j):
    flat, w, h = dst.reshape(-1), int(j["width"]), int(j["height"])
    return np.stack([flat[int(j["dst_offset"]) + r * b["dst_stride"]:int(j["dst_offset"]) + r * b["dst_stride"] + w] for r in range(h)])


def check_pred(ctx, golden, name):
    """device == restatement on every sample of the destination (so every sample outside the jobs' blocks is still 0xA5) == the fixture"""
    b = wc.batch(name)
    want, want_status, _, _ = wc.restated(name)
    dst, status = run_pred(ctx, b)
    assert np.array_equal(status, want_status) and np.all(status == wc.ST_OK), name
    bad = [i for i, j in enumerate(b["jobs"]) if not np.array_equal(block_of(b, dst, j), block_of(b, want, j))]
    assert not bad, (name, bad[:8])
    assert np.array_equal(dst, want), f"{name}: a sample outside the jobs' blocks was written"
    crcs = np.array([wc.block_crc(block_of(b, dst, j)) for j in b["jobs"]], np.uint32)
    assert np.array_equal(crcs, golden[f"crc_{name}"]), name


@pytest.mark.parametrize("ss", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
def test_every_size_single_average_and_distance_weighted(hip_ctx, golden, bd, ss):
    check_pred(hip_ctx, golden, f"size_{bd}_{ss}")


@pytest.mark.parametrize("pic", ["40x24", "37x21"])
@pytest.mark.parametrize("bd", [8, 10])
def test_tiles_outside_and_across_every_edge(hip_ctx, golden, bd, pic):
    check_pred(hip_ctx, golden, f"edge_{bd}_{pic}")


@pytest.mark.parametrize("bd", [8, 10])
def test_both_ends_of_the_filter_table(hip_ctx, golden, bd):
    check_pred(hip_ctx, golden, f"ends_{bd}")


@pytest.mark.parametrize("bd", [8, 10])
def test_one_128x128_block(hip_ctx, golden, bd):
    check_pred(hip_ctx, golden, f"big_{bd}")
    key = f"block_{bd}_128x128"
    assert np.array_equal(wc.restated(f"big_{bd}")[2][0], golden[key])


@pytest.mark.parametrize("n", wc.COUNTS)
def test_job_counts_around_a_wave_and_a_workgroup(hip_ctx, golden, n):
    check_pred(hip_ctx, golden, f"count_{n}")


def test_no_jobs_enqueue_nothing(hip_ctx):
    b = dict(wc.batch("count_1"))
    b["jobs"] = b["jobs"][:0]
    dst, status = run_pred(hip_ctx, b)
    assert np.all(dst.view(np.uint8) == FILL) and len(status) == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_and_jobs_without_a_model_write_their_status_alone(hip_ctx, bd):
    b, expect = wc.undefined_batch(bd)
    want, want_status, _ = wc.restate_pred(b)
    assert {i: int(want_status[i]) for i in expect} == expect and set(expect.values()) == {wc.ST_UNDEFINED, wc.ST_NO_MODEL}
    assert all(int(s) == wc.ST_OK for i, s in enumerate(want_status) if i not in expect)
    dst, status = run_pred(hip_ctx, b)
    assert np.array_equal(status, want_status)
    assert np.array_equal(dst, want)  # the neighbours' blocks are right, the refused jobs' slots are still 0xA5


def test_models_from_the_array_equal_models_in_the_job(hip_ctx):
    """the same jobs with their models moved into an array and named by index, the second reference's too"""
    b = dict(wc.batch("size_8_1"))
    want, want_status, _, _ = wc.restated("size_8_1")
    jobs, models = b["jobs"].copy(), []
    for j in jobs:
        for r in range(2 if int(j["ref"][1]) != wc.NO_REF else 1):
            m = j["model"][r].copy()
            m["valid"] = 1
            j["model_index"][r] = len(models)
            j["flags"] |= (wc.MODEL0_FROM_ARRAY, wc.MODEL1_FROM_ARRAY)[r]
            j["model"][r] = np.zeros((), wc.MODEL_DTYPE)
            models.append(m)
    b["jobs"], b["models"] = jobs, wc.pack_jobs(models, wc.MODEL_DTYPE)
    dst, status = run_pred(hip_ctx, b)
    assert np.all(status == wc.ST_OK) and np.array_equal(dst, want)


# ---- the fit ----
def run_models(ctx, b, jobs=None):
    jobs = b["jobs"] if jobs is None else jobs
    out = warp.run_warp_model_hip(ctx, jobs, b["shut_approx"], b["lower_band_th"], b["upper_band_th"], mv_array=b["mv_array"], spare_jobs=SPARE, fill=FILL)
    n = len(jobs)
    assert np.all(out["status"][n:] == FILL) and np.all(out["models"][n:].view(np.uint8) == FILL), "spare slots written"
    return out["models"][:n], out["status"][:n]


@pytest.mark.parametrize("name", list(wc.MODEL_BATCHES))
def test_fits_equal_the_reference(hip_ctx, golden, name):
    b = wc.model_batch(name)
    want, want_status, _ = wc.restated_models(name)
    models, status = run_models(hip_ctx, b)
    assert np.array_equal(status, want_status) and np.all(status == wc.ST_OK)
    bad = [i for i in range(len(want)) if models[i].tobytes() != want[i].tobytes()]
    assert not bad, (name, bad[:8], models[bad[:2]], want[bad[:2]])
    assert np.array_equal(wc.models_crc(models, status), golden[f"fit_{name}"])


@pytest.mark.parametrize("n", [1, 64, 65])
def test_fit_job_counts(hip_ctx, n):
    b = wc.model_batch("m6")
    want, _, _ = wc.restated_models("m6")
    models, status = run_models(hip_ctx, b, b["jobs"][:n])
    assert np.all(status == wc.ST_OK) and models.tobytes() == want[:n].tobytes()


def test_undefined_fits_write_their_status_alone(hip_ctx):
    b = dict(wc.model_batch("m6"))
    jobs = b["jobs"][:12].copy()
    jobs[1]["bwidth"] = 4
    jobs[3]["bwidth"], jobs[3]["bheight"] = 128, 32
    jobs[5]["n_samples"] = 9
    jobs[7]["flags"], jobs[7]["mv_index"] = wc.MV_FROM_ARRAY, len(b["mv_array"])  # one past the array
    jobs[9]["flags"], jobs[9]["mv_index"] = wc.MV_FROM_ARRAY, len(b["mv_array"]) - 1
    b["jobs"] = jobs
    want, want_status = wc.restate_models(b)
    assert [int(s) for s in want_status] == [0, 255, 0, 255, 0, 255, 0, 255, 0, 0, 0, 0]
    models, status = run_models(hip_ctx, b)
    assert np.array_equal(status, want_status) and models.tobytes() == want.tobytes()  # an undefined job's record is still 0xA5
    b["mv_array"] = None  # no array at all: every job that names it is undefined
    want, want_status = wc.restate_models(b)
    assert int(want_status[9]) == wc.ST_UNDEFINED
    models, status = run_models(hip_ctx, b)
    assert np.array_equal(status, want_status) and models.tobytes() == want.tobytes()


# ---- the refinement ----
REFINE_OUTS = ("best_mv", "best_cost", "n_checked", "status")


def run_refine(ctx, b, jobs=None, waves=0):
    jobs = b["jobs"] if jobs is None else jobs
    out = warp.run_wm_refine_hip(ctx, b["settings"], b["planes"], b["src"], jobs, mv_array=b["mv_array"], cost_tables=b["cost_tables"], waves_per_job=waves,
                                 spare=SPARE, fill=FILL)
    n = len(jobs)
    for k in REFINE_OUTS:
        assert np.all(out[k][n:].view(np.uint8) == FILL), f"spare {k} slots written"
    assert all(np.array_equal(g, p[0]) for g, p in zip(out["planes"], b["planes"])) and np.array_equal(out["src"], b["src"]), "an input plane changed"
    return {k: out[k][:n] for k in REFINE_OUTS}


@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("name", list(wc.REFINE_BATCHES))
def test_refinement_equals_the_reference(hip_ctx, golden, name, waves):
    """blocks 8x8, 16x16, 32x16 (and a 64x64) on a 96x64 picture; 1, 8 and 16 iterations, diagonals on and off, both precisions, both rates; the
    workgroup form and the one-wave form give the same"""
    b = wc.refine_batch(name)
    want, _ = wc.restated_refine(name)
    got = run_refine(hip_ctx, b, waves=waves)
    for k in REFINE_OUTS:
        assert np.array_equal(got[k], want[k]), (name, k, got[k].tolist(), want[k].tolist())
    ref = golden[f"refine_{name}"]
    assert np.array_equal(got["best_mv"], ref[:, :2]) and np.array_equal(got["n_checked"], ref[:, 2].astype(np.uint32))
    none = want["n_valid"] == 0
    assert np.all(got["best_cost"][none] == wc.INT_MAX) and np.all(got["best_cost"][~none] != wc.INT_MAX)


def test_undefined_refinements_write_their_status_alone(hip_ctx):
    b = dict(wc.refine_batch("light"))
    jobs = b["jobs"][:10].copy()
    jobs[1]["bwidth"] = 4
    jobs[2]["n_samples"] = 9
    jobs[4]["ref"] = 2
    jobs[5]["flags"], jobs[5]["mv_index"] = wc.WM_START_FROM_ARRAY, len(b["mv_array"])
    jobs[7]["src_offset"] = b["src"].size - (int(jobs[7]["bheight"]) - 1) * b["src"].shape[1] - int(jobs[7]["bwidth"]) + 1  # ends one sample past the plane
    b["jobs"] = jobs
    want = wc.restate_refine(b)
    assert [int(s) for s in want["status"]] == [0, 255, 255, 0, 255, 255, 0, 255, 0, 0]
    got = run_refine(hip_ctx, b)
    for k in REFINE_OUTS:
        assert np.array_equal(got[k], want[k]), k  # an undefined job's slots are still 0xA5
