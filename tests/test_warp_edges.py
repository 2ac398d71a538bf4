"""CPU: the cases of tests/warp_edge_cases.py.  The restatements of tests/warp_cases.py equal the reference's own results on every new batch
(golden/warp_edges.npz, written by tools/gen_warp_golden.py through svt_aom_wm_motion_refinement, svt_find_projection and svt_av1_warp_plane), the
batches reach the conditions they exist for (warp_edge_cases.edge_coverage_missing, computed from the restatements' traces), and their inputs stay
where the reference is defined."""
import numpy as np
import pytest

import warp_cases as wc
import warp_edge_cases as ec


@pytest.fixture(scope="module")
def golden():
    return np.load(ec.GOLDEN)


@pytest.mark.parametrize("name", list(ec.REFINE_EDGE_BATCHES))
def test_refinement_restatement_equals_the_reference_on_the_edge_batches(golden, name):
    want, _, _ = ec.restated_refine_edge(name)
    ref = golden[f"refine_{name}"]
    assert np.all(want["status"] == wc.ST_OK) and len(ref) == len(ec.refine_edge_batch(name)["jobs"])
    assert np.array_equal(want["best_mv"], ref[:, :2]) and np.array_equal(want["n_checked"], ref[:, 2]) and np.array_equal(want["n_valid"], ref[:, 3])
    assert np.array_equal(want["best_cost"] == wc.INT_MAX, ref[:, 3] == 0)


def test_fit_restatement_equals_the_reference_on_the_far_batch(golden):
    models, status, _ = ec.restated_far()
    assert np.all(status == wc.ST_OK) and np.array_equal(wc.models_crc(models, status), golden["fit_far"])
    assert 0 < int(models["valid"].sum()) < len(models)


@pytest.mark.parametrize("name", ec.pred_edge_names())
def test_prediction_restatement_equals_the_reference_on_the_edge_batches(golden, name):
    b = ec.pred_edge_batch(name)
    _, status, blocks = ec.restated_pred_edge(name)
    assert np.all(status == wc.ST_OK)
    assert np.array_equal(np.array([wc.block_crc(blocks[i]) for i in range(len(b["jobs"]))], np.uint32), golden[f"crc_{name}"])


def test_the_fixture_holds_exactly_the_generators_keys(golden):
    assert set(golden.files) == {f"refine_{n}" for n in ec.REFINE_EDGE_BATCHES} | {"fit_far"} | {f"crc_{n}" for n in ec.pred_edge_names()}


def test_edge_coverage_conditions_hold():
    """every size with 5 costed warps and a best MV off its start, with and without diagonals, in both precisions; |sum| past 46341 and past 65536
    with either sign in at least three sizes, the two limits of the variance, a limit job with a unique winner that is not the first position;
    tiles of costed warps outside and across every edge, every reference index 0 .. 7, a source offset that is not the block origin's; a record
    of more than 64 positions and a skip because of an entry at index >= 64; a recorded wrap in each direction; the translation clamps of the
    fit, valid fits at a clamped translation; a 128x128 compound, eight references"""
    for k, v in ec.refine_edge_stats().items():  # the counts the conditions are judged on: shown with -s, and when the assertion fails
        print(f"  {k}: {v}")
    print(f"  far: {ec.far_stats()}")
    assert ec.edge_coverage_missing() == []


def test_the_conditions_can_fail():
    """the same judgements on batches that do not meet them"""
    logs = []
    wc.restate_refine(wc.refine_batch("m6"), None, logs)
    sums = [abs(t) for log in logs for _, _, t, _ in log["costed"]]
    assert sums and max(sums) < ec.INT32_SQUARE  # the earlier batch never squares a sum that leaves int32
    assert max(max(log["record_hits"], default=-1) for log in logs) < ec.RECORD_SCAN and not any(log["wrapped"] for log in logs)
    # the int32 judgement of the fit's intermediates: an origin of 20 bits, which no uint16 field holds, wraps the translation
    trace = set()
    wc.find_affine_int(1, [8, 8] + [0] * 14, [9, 9] + [0] * 14, 8, 8, 0, 0, 1 << 18, 1 << 18, trace)
    assert "int32_left" in trace


def test_settings_and_sizes_of_the_edge_batches():
    s = {n: dict(zip(wc.SETTING_KEYS, v)) for n, v in ec.REFINE_EDGE_BATCHES.items()}
    assert {(s[n]["refine_diag"], s[n]["mv_prec_shift"]) for n in s if n.startswith("sizes")} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for n in ("walk_0", "walk_1"):
        assert (s[n]["iterations"], s[n]["refine_diag"], s[n]["approx_inter_rate"], s[n]["shut_approx"]) == (16, 1, 1, 1)
    assert (s["walk_0"]["mv_prec_shift"], s["walk_1"]["mv_prec_shift"]) == (0, 1)
    assert all(s[n]["approx_inter_rate"] == 1 for n in ("wrap_0", "wrap_1"))  # the entropy rate is not defined on a wrapped difference's table index
    for n in s:
        if n.startswith("sizes"):
            b = ec.refine_edge_batch(n)
            assert {(int(j["bwidth"]), int(j["bheight"])) for j in b["jobs"]} == set(wc.SIZES)
            assert b["planes"][0][3:] == (160, 136) and {(int(j["blk_org_x"]), int(j["blk_org_y"])) for j in b["jobs"] if int(j["bwidth"]) == int(j["bheight"]) == 128} == {(32, 8), (0, 4)}
    assert {(int(j["bwidth"]), int(j["bheight"])) for j in ec.refine_edge_batch("bias")["jobs"]} == set(ec.BIAS_SIZES)


def test_the_walk_records_84_positions_and_ends_on_the_iteration_limit():
    for name in ("walk_0", "walk_1"):
        out, traces, _ = ec.restated_refine_edge(name)
        assert 9 + 15 * 5 == 84 and int(out["n_checked"].max()) == 84
        assert all("stop_iterations" in t for t, n in zip(traces, out["n_checked"]) if n == 84)
        b = ec.refine_edge_batch(name)
        step = 1 << b["settings"]["mv_prec_shift"]
        moved = {(int(mv[0]) - int(j["start_mv"][0]), int(mv[1]) - int(j["start_mv"][1])) for j, mv, n in zip(b["jobs"], out["best_mv"], out["n_checked"]) if n == 84}
        # towards (40, 40) and towards (-40, -40), one diagonal step per round (a job some of whose fits are invalid may end a step beside)
        assert {(16 * step, 16 * step), (-16 * step, -16 * step)} <= moved


def test_geometry_inputs_are_as_described():
    b = ec.refine_edge_batch("geometry")
    assert b["src"].shape[1] == 117 > 100 and len(b["planes"]) == 8
    assert len({p[0].shape[1] for p in b["planes"]}) == 8 and len({(p[1], p[2]) for p in b["planes"]}) == 8  # eight strides, eight origins
    assert all(p[3:] == (100, 70) for p in b["planes"])
    at = {(int(j["blk_org_x"]) == 0, int(j["blk_org_x"]) + int(j["bwidth"]) == 100, int(j["blk_org_y"]) == 0, int(j["blk_org_y"]) + int(j["bheight"]) == 70) for j in b["jobs"]}
    for want in ((1, 0, 1, 0), (0, 1, 1, 0), (1, 0, 0, 1), (0, 1, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        assert tuple(bool(v) for v in want) in at, want  # the four corners, the four edges
    inside = [(3 + int(j["blk_org_y"])) * 117 + 5 + int(j["blk_org_x"]) == int(j["src_offset"]) for j in b["jobs"]]
    assert all(inside[:-1]) and not inside[-1]


def test_inputs_stay_where_the_reference_is_defined():
    """block origins and MVs fit the reference's uint16 / int16 fields as they are (nothing relies on a wrap of an input), every block and its
    source samples lie inside their planes, no 32-bit intermediate of the fit wraps on the far batch, and the wrap batches cost with the light rate
    alone"""
    for name in ec.REFINE_EDGE_BATCHES:
        b = ec.refine_edge_batch(name)
        stride = b["src"].shape[1]
        for j in b["jobs"]:
            pw, ph = b["planes"][int(j["ref"])][3:]
            assert int(j["blk_org_x"]) + int(j["bwidth"]) <= pw and int(j["blk_org_y"]) + int(j["bheight"]) <= ph
            assert int(j["src_offset"]) % stride + int(j["bwidth"]) <= stride
            assert int(j["src_offset"]) + (int(j["bheight"]) - 1) * stride + int(j["bwidth"]) <= b["src"].size
            assert 1 <= int(j["n_samples"]) <= 8
    for name in ("wrap_0", "wrap_1"):
        b = ec.refine_edge_batch(name)
        step = 1 << b["settings"]["mv_prec_shift"]
        starts = {(k, int(j["start_mv"][k])) for j in b["jobs"] for k in range(2) if abs(int(j["start_mv"][k])) > 30000}
        assert starts == {(0, ec.I16_MAX - step + 1), (0, ec.I16_MIN + step - 1), (1, ec.I16_MAX - step + 1), (1, ec.I16_MIN + step - 1)}
    b = ec.far_batch()
    _, _, traces = ec.restated_far()
    assert not any("int32_left" in t for t in traces)
    assert len(b["jobs"]) == 142 and max(int(j["blk_org_x"]) for j in b["jobs"]) == 65532 == max(int(j["blk_org_y"]) for j in b["jobs"])
    near = sum(1 for j in b["jobs"][:130] if max(abs(int(j["mv"][0])), abs(int(j["mv"][1]))) > 32000)
    assert 40 <= near <= 46  # a third of the 130
