"""GPU parity: svt_hip_md_fullpel_batch / svt_hip_md_subpel_batch (csrc/md_search_kernel.hip) against the oracle and against the committed
outputs of the reference's own md_full_pel_search chains and svt_av1_find_best_sub_pixel_tree_pruned (tests/golden/md_search.npz)."""
import os

import numpy as np
import pytest

import md_search_cases as mc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_search.npz")


@pytest.mark.parametrize("gi", range(len(mc.FULLPEL_GRID)))
def test_fullpel_chain(hip_ctx, oracle, gi):
    dist, psad, ctype = mc.FULLPEL_GRID[gi]
    rng = np.random.default_rng(100 + dist * 10 + psad * 3 + ctype)
    src, refp = mc.planes(7 + dist)
    tables = mc.cost_tables(rng)
    rounds = mc.fullpel_chain(rng, 40, dist, psad)
    want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, 37, tables)
    got = mc.run_fullpel_hip(hip_ctx, src, refp, rounds, ctype, 37, tables)
    z = np.load(GOLDEN)
    for r, ((cw, mw), (cg, mg)) in enumerate(zip(want, got)):
        np.testing.assert_array_equal(cg, cw, err_msg=f"round {r} cost vs oracle")
        np.testing.assert_array_equal(mg, mw, err_msg=f"round {r} mv vs oracle")
        np.testing.assert_array_equal(cg, z[f"fp_cost_{gi}"][r], err_msg=f"round {r} cost vs reference fixture")
        np.testing.assert_array_equal(mg, z[f"fp_mv_{gi}"][r], err_msg=f"round {r} mv vs reference fixture")


@pytest.mark.parametrize("si", range(len(mc.SUBPEL_SETTINGS)))
def test_subpel_tree_searches(hip_ctx, oracle, si):
    rng = np.random.default_rng(300 + si)
    src, refp = mc.planes(11 + si)
    tables = mc.cost_tables(rng)
    jobs = mc.subpel_jobs(rng, 60)
    want = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 41, 36, tables)
    got = mc.run_subpel_hip(hip_ctx, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 41, 36, tables)
    z = np.load(GOLDEN)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} vs oracle")
        np.testing.assert_array_equal(got[k], z[f"sp_{k}_{si}"], err_msg=f"{k} vs reference fixture")


def test_many_blocks_random_settings(hip_ctx, oracle):
    """a larger randomized sweep: 600 sub-pel jobs per setting with other seeds, full-pel chains of 300 blocks"""
    for si in range(len(mc.SUBPEL_SETTINGS)):
        rng = np.random.default_rng(900 + si)
        src, refp = mc.planes(40 + si)
        tables = mc.cost_tables(rng)
        jobs = mc.subpel_jobs(rng, 600)
        want = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 23 + si, 20 + 7 * si, tables)
        got = mc.run_subpel_hip(hip_ctx, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 23 + si, 20 + 7 * si, tables)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} setting {si}")
    for gi, (dist, psad, ctype) in enumerate(mc.FULLPEL_GRID):
        rng = np.random.default_rng(1200 + gi)
        src, refp = mc.planes(60 + gi)
        tables = mc.cost_tables(rng)
        rounds = mc.fullpel_chain(rng, 300, dist, psad)
        want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, 19 + gi, tables)
        got = mc.run_fullpel_hip(hip_ctx, src, refp, rounds, ctype, 19 + gi, tables)
        for r, ((cw, mw), (cg, mg)) in enumerate(zip(want, got)):
            np.testing.assert_array_equal(cg, cw, err_msg=f"grid {gi} round {r} cost")
            np.testing.assert_array_equal(mg, mw, err_msg=f"grid {gi} round {r} mv")


# ---------------------------------------------------------------------------------------------------------------------------------------
# Plane edges, ties, every MV cost mode, odd strides, chains without the host, the chaining contract (tests/golden/md_search_edges.npz).
# tests/test_md_search.py proves on the CPU that these inputs reach the search-area adjustment and really tie.
# ---------------------------------------------------------------------------------------------------------------------------------------
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_search_edges.npz")
N_EDGE = len(mc.FULLPEL_EDGE_GRID)


def assert_traces_equal(got, want, what):
    assert len(got) == len(want)
    for r, ((cg, mg), (cw, mw)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(cg, cw, err_msg=f"{what} round {r} cost")
        np.testing.assert_array_equal(mg, mw, err_msg=f"{what} round {r} mv")


@pytest.mark.parametrize("chain,key", [("edge", "fe"), ("std", "fc")])
@pytest.mark.parametrize("ci", range(N_EDGE))
def test_fullpel_edges_and_ties(hip_ctx, oracle, ci, chain, key):
    src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci, chain)
    want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, epb, tables)
    got = mc.run_fullpel_hip(hip_ctx, src, refp, rounds, ctype, epb, tables)
    assert_traces_equal(got, want, f"{mc.FULLPEL_EDGE_GRID[ci]} {chain} vs oracle")
    z = np.load(EDGES)
    np.testing.assert_array_equal(np.stack([c for c, _ in got]), z[f"{key}_cost"][ci], err_msg="cost vs reference fixture")
    np.testing.assert_array_equal(np.stack([m for _, m in got]), z[f"{key}_mv"][ci], err_msg="mv vs reference fixture")


def check_subpel_group(hip_ctx, oracle, kind, si, far, key):
    grid = mc.SUBPEL_FAR_GRID if far else mc.SUBPEL_TIE_GRID
    c0 = grid.index((kind, si, 0))
    z = np.load(EDGES)
    for ci in range(c0, c0 + 6):
        src, refp, tables, jobs, setting = mc.subpel_edge_case(ci, far)
        want = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        got = mc.run_subpel_hip(hip_ctx, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{grid[ci]} {k} vs oracle")
            np.testing.assert_array_equal(got[k], z[f"{key}_{k}"][ci], err_msg=f"{grid[ci]} {k} vs reference fixture")


@pytest.mark.parametrize("kind,si", [(kind, si) for kind, si, ctype in mc.SUBPEL_TIE_GRID if ctype == 0])
def test_subpel_every_cost_type(hip_ctx, oracle, kind, si):
    check_subpel_group(hip_ctx, oracle, kind, si, False, "st")


@pytest.mark.parametrize("kind,si", [(kind, si) for kind, si, ctype in mc.SUBPEL_FAR_GRID if ctype == 0])
def test_subpel_far_jobs_every_cost_type(hip_ctx, oracle, kind, si):
    check_subpel_group(hip_ctx, oracle, kind, si, True, "sf")


@pytest.mark.parametrize("ci", [0, 3, 10, 13, 18, 23, 27, 28])
def test_fullpel_chain_without_the_host(hip_ctx, oracle, ci):
    """every round enqueued back to back on the context stream, one sync at the end: the same final costs and vectors as with a sync and a copy
    after every round, and as the oracle's"""
    for chain in ("edge", "std"):
        src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci, chain)
        want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, epb, tables)
        synced = mc.run_fullpel_hip(hip_ctx, src, refp, rounds, ctype, epb, tables)
        queued = mc.run_fullpel_hip(hip_ctx, src, refp, rounds, ctype, epb, tables, sync_each=False)
        assert len(queued) == 1
        assert_traces_equal(queued, synced[-1:], f"{ci} {chain} queued vs synced")
        assert_traces_equal(queued, want[-1:], f"{ci} {chain} queued vs oracle")


@pytest.mark.parametrize("ci", range(0, N_EDGE, 3))
def test_fullpel_strided_planes(hip_ctx, oracle, ci):
    """source and reference as views into wider arrays whose strides (354, 514) are not multiples of 4: lane_sad's dword reads at odd addresses"""
    for chain in ("edge", "std"):
        src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci, chain)
        s, r = mc.strided(src, 1), mc.strided(refp, 2)
        assert s.strides[0] % 4 and r.strides[0] % 4
        rounds = [mc.restride(j, s.strides[0]) for j in rounds]
        want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, s, r, rounds, ctype, epb, tables)
        got = mc.run_fullpel_hip(hip_ctx, s, r, rounds, ctype, epb, tables)
        assert_traces_equal(got, want, f"strided {ci} {chain}")
        if chain == "std" or not (mc.FULLPEL_EDGE_GRID[ci][1] == 0 and mc.FULLPEL_EDGE_GRID[ci][2] == 1):
            # (the rounded-up wide form reads a few columns past the plane's row: there the parent's bytes differ from the tight plane's next row)
            z = np.load(EDGES)
            key = "fe" if chain == "edge" else "fc"
            np.testing.assert_array_equal(np.stack([c for c, _ in got]), z[f"{key}_cost"][ci], err_msg="cost vs reference fixture")
            np.testing.assert_array_equal(np.stack([m for _, m in got]), z[f"{key}_mv"][ci], err_msg="mv vs reference fixture")


@pytest.mark.parametrize("far", [False, True])
def test_subpel_strided_planes(hip_ctx, oracle, far):
    grid = mc.SUBPEL_FAR_GRID if far else mc.SUBPEL_TIE_GRID
    z = np.load(EDGES)
    for ci in range(0, len(grid), 5):
        src, refp, tables, jobs, setting = mc.subpel_edge_case(ci, far)
        s, r = mc.strided(src, 1), mc.strided(refp, 2)
        jobs = mc.restride(jobs, s.strides[0], r.strides[0])
        want = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, s, r, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        got = mc.run_subpel_hip(hip_ctx, s, r, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"strided {grid[ci]} {k} vs oracle")
            np.testing.assert_array_equal(got[k], z[f"{'sf' if far else 'st'}_{k}"][ci], err_msg=f"strided {grid[ci]} {k} vs reference fixture")


def test_subpel_without_center_err(hip_ctx, oracle):
    """center_err is optional: with a null pointer the other four outputs are what they were"""
    for far, ci in ((False, 7), (False, 100), (True, 40), (True, 77)):
        src, refp, tables, jobs, setting = mc.subpel_edge_case(ci, far)
        want = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        got = mc.run_subpel_hip(hip_ctx, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables, center_err=False)
        assert sorted(got) == ["best_mv", "besterr", "distortion", "sse"]
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"far={far} {ci} {k}")


def test_chain_from_out_of_range_is_ignored(hip_ctx, oracle):
    """Both chain flags with chain_from = -1 = the same job with the flags clear.  One sentinel entry lies in front of the base pointers
    handed to the descriptor, so that even an unguarded read of index -1 would stay inside the allocation -- and would bring the sentinel,
    not the job's own fields."""
    src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(1)
    plain = rounds[0]
    want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, [plain], ctype, epb, tables)
    assert_traces_equal(mc.run_fullpel_hip(hip_ctx, src, refp, [plain], ctype, epb, tables, guard=True), want, "flags clear")
    flagged = plain.copy()
    flagged["flags"] |= mc.abi.FP_CENTRE_FROM_CHAIN | mc.abi.FP_BEST_FROM_CHAIN
    flagged["chain_from"] = -1
    assert_traces_equal(mc.run_fullpel_hip(hip_ctx, src, refp, [flagged], ctype, epb, tables, guard=True), want, "chain_from -1")


@pytest.mark.parametrize("dist,psad,ctype", [(0, 1, 0), (1, 0, 4), (0, 0, 4)])
def test_fullpel_mixed_batch(hip_ctx, oracle, dist, psad, ctype):
    """2000 jobs per batch, two chained rounds: every block size, the four contents by quadrant, edge and interior blocks side by side -- nothing
    of a job's state may reach the workgroup next to it"""
    rng = np.random.default_rng([1500, dist, psad, ctype])
    src, refp = mc.mixed_planes(31)
    tables = mc.cost_tables(rng)
    rounds = mc.mixed_fullpel_rounds(rng, 1000, dist, psad)
    want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, mc.EDGE_EPB[ctype], tables)
    got = mc.run_fullpel_hip(hip_ctx, src, refp, rounds, ctype, mc.EDGE_EPB[ctype], tables)
    assert_traces_equal(got, want, "mixed batch")
    assert len({tuple(m) for m in want[-1][1]}) > 200


@pytest.mark.parametrize("si,ctype", [(1, 1), (3, 4), (6, 0), (8, 3)])
def test_subpel_mixed_batch(hip_ctx, oracle, si, ctype):
    """2000 jobs in one batch: interior and far / corner jobs, every block size, the four contents by quadrant"""
    rng = np.random.default_rng([1600, si, ctype])
    src, refp = mc.mixed_planes(32)
    tables = mc.cost_tables(rng)
    jobs = np.concatenate([mc.subpel_jobs(rng, 1000), mc.subpel_far_jobs(rng, 1000)])
    jobs = jobs[rng.permutation(len(jobs))]
    setting = mc.with_cost_type(mc.SUBPEL_SETTINGS[si], ctype)
    want = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
    got = mc.run_subpel_hip(hip_ctx, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if setting[1] < 3:
        assert (want["best_mv"] % 8 != 0).any()
