"""GPU: svt_hip_wm_refine_batch, svt_hip_warp_model_batch and svt_hip_warp_pred_batch on the cases of tests/warp_edge_cases.py, every comparison
exact -- against the restatements of tests/warp_cases.py and against the reference's own results (golden/warp_edges.npz): refinements of every
block size with waves_per_job 0, 1 and 4, sums of differences whose square leaves 32 bits and the two limits of the variance (best_cost compared
too), blocks at every edge of a picture that is no multiple of 8 against eight reference planes, records of more than 64 positions, MVs that wrap;
fits at block origins up to 65532 with clamped translations; a 128x128 compound and eight references in the prediction.  Outputs start as the
byte 0xA5 with spare slots and are compared whole; input planes are checked unchanged."""
import numpy as np
import pytest

import warp_cases as wc
import warp_edge_cases as ec
from svt_av1_psyex_amd import warp

pytestmark = pytest.mark.gpu

FILL = wc.FILL
SPARE = 3
REFINE_OUTS = ("best_mv", "best_cost", "n_checked", "status")


@pytest.fixture(scope="module")
def golden():
    return np.load(ec.GOLDEN)


def run_refine(ctx, b, waves):
    jobs = b["jobs"]
    out = warp.run_wm_refine_hip(ctx, b["settings"], b["planes"], b["src"], jobs, mv_array=b["mv_array"], cost_tables=b["cost_tables"], waves_per_job=waves,
                                 spare=SPARE, fill=FILL)
    n = len(jobs)
    for k in REFINE_OUTS:
        assert np.all(out[k][n:].view(np.uint8) == FILL), f"spare {k} slots written"
    assert all(np.array_equal(g, p[0]) for g, p in zip(out["planes"], b["planes"])) and np.array_equal(out["src"], b["src"]), "an input plane changed"
    return {k: out[k][:n] for k in REFINE_OUTS}


@pytest.mark.parametrize("waves", ec.WAVES)
@pytest.mark.parametrize("name", list(ec.REFINE_EDGE_BATCHES))
def test_refinement_equals_the_restatement_and_the_reference(hip_ctx, golden, name, waves):
    """best MV, best cost, the positions tested and the status of every job; the one-wave form, the four-wave form and the default agree because
    each equals the restatement"""
    b = ec.refine_edge_batch(name)
    want, _, _ = ec.restated_refine_edge(name)
    got = run_refine(hip_ctx, b, waves)
    for k in REFINE_OUTS:
        bad = [i for i in range(len(b["jobs"])) if not np.array_equal(got[k][i], want[k][i])]
        assert not bad, (name, waves, k, bad[:8], [(got[k][i].tolist(), want[k][i].tolist()) for i in bad[:4]])
    ref = golden[f"refine_{name}"]
    assert np.array_equal(got["best_mv"], ref[:, :2]) and np.array_equal(got["n_checked"], ref[:, 2].astype(np.uint32))
    assert np.array_equal(got["best_cost"] == wc.INT_MAX, ref[:, 3] == 0)


def test_fits_far_from_the_origin_equal_the_reference(hip_ctx, golden):
    b = ec.far_batch()
    want, want_status, _ = ec.restated_far()
    out = warp.run_warp_model_hip(hip_ctx, b["jobs"], b["shut_approx"], b["lower_band_th"], b["upper_band_th"], mv_array=b["mv_array"], spare_jobs=SPARE, fill=FILL)
    n = len(b["jobs"])
    assert np.all(out["status"][n:] == FILL) and np.all(out["models"][n:].view(np.uint8) == FILL), "spare slots written"
    models, status = out["models"][:n], out["status"][:n]
    assert np.array_equal(status, want_status) and np.all(status == wc.ST_OK)
    bad = [i for i in range(n) if models[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], models[bad[:2]], want[bad[:2]])
    assert np.array_equal(wc.models_crc(models, status), golden["fit_far"])


def block_of(b, dst, j):
    flat, w, h = dst.reshape(-1), int(j["width"]), int(j["height"])
    return np.stack([flat[int(j["dst_offset"]) + r * b["dst_stride"]:int(j["dst_offset"]) + r * b["dst_stride"] + w] for r in range(h)])


@pytest.mark.parametrize("name", ec.pred_edge_names())
def test_compound_128x128_and_eight_references(hip_ctx, golden, name):
    b = ec.pred_edge_batch(name)
    want, want_status, _ = ec.restated_pred_edge(name)
    out = warp.run_warp_pred_hip(hip_ctx, b["bit_depth"], b["ss_x"], b["ss_y"], b["planes"], b["jobs"], b["dst_shape"], b["dst_stride"], models=b.get("models"),
                                 spare_jobs=SPARE, fill=FILL)
    n = len(b["jobs"])
    assert len(out["status"]) == n + SPARE and np.all(out["status"][n:] == FILL), "spare status slots written"
    assert all(np.array_equal(g, p[0]) for g, p in zip(out["planes"], b["planes"])), "a reference plane changed"
    dst, status = out["dst"], out["status"][:n]
    assert np.array_equal(status, want_status) and np.all(status == wc.ST_OK), name
    bad = [i for i, j in enumerate(b["jobs"]) if not np.array_equal(block_of(b, dst, j), block_of(b, want, j))]
    assert not bad, (name, bad[:8])
    assert np.array_equal(dst, want), f"{name}: a sample outside the jobs' blocks was written"
    crcs = np.array([wc.block_crc(block_of(b, dst, j)) for j in b["jobs"]], np.uint32)
    assert np.array_equal(crcs, golden[f"crc_{name}"]), name
