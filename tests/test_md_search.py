"""CPU: the mode-decision side motion search (include/svt_hip_md_search.h).  The oracle's restatement (oracle/md_search_oracle.c) against the
REFERENCE's own md_full_pel_search and svt_av1_find_best_sub_pixel_tree_pruned (oracle/ref_harness_md.c, build container), and against the
committed outputs of the reference (tests/golden/md_search.npz) everywhere."""
import os

import numpy as np
import pytest

import md_search_cases as mc
import pyoracle
from svt_av1_psyex_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_search.npz")


def test_struct_sizes(oracle):
    oracle.orc_sizeof_md_search.restype = __import__("ctypes").c_size_t
    import ctypes as C
    assert oracle.orc_sizeof_md_search(0) == abi.FULLPEL_JOB_DTYPE.itemsize and oracle.orc_sizeof_md_search(1) == C.sizeof(abi.FullpelBatchDesc)
    assert oracle.orc_sizeof_md_search(2) == abi.SUBPEL_JOB_DTYPE.itemsize and oracle.orc_sizeof_md_search(3) == C.sizeof(abi.SubpelBatchDesc)


@pytest.mark.parametrize("dist,psad,ctype", mc.FULLPEL_GRID)
def test_fullpel_chain_oracle_equals_reference(oracle, ref, dist, psad, ctype):
    rng = np.random.default_rng(100 + dist * 10 + psad * 3 + ctype)
    src, refp = mc.planes(7 + dist)
    tables = mc.cost_tables(rng)
    rounds = mc.fullpel_chain(rng, 40, dist, psad)
    a = mc.run_fullpel_cpu(ref.ref_md_fullpel_batch, src, refp, rounds, ctype, 37, tables)
    b = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, 37, tables)
    for r, ((ca, ma), (cb, mb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ca, cb, err_msg=f"round {r} cost")
        np.testing.assert_array_equal(ma, mb, err_msg=f"round {r} mv")
    assert len({tuple(m) for m in a[-1][1]}) > 10  # the chains really moved


@pytest.mark.parametrize("si", range(len(mc.SUBPEL_SETTINGS)))
def test_subpel_tree_searches_oracle_equals_reference(oracle, ref, si):
    rng = np.random.default_rng(300 + si)
    src, refp = mc.planes(11 + si)
    tables = mc.cost_tables(rng)
    jobs = mc.subpel_jobs(rng, 60)
    a = mc.run_subpel_cpu(ref.ref_md_subpel_batch, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 41, 36, tables)
    b = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 41, 36, tables)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    if mc.SUBPEL_SETTINGS[si][1] < 3:
        assert (a["best_mv"] % 8 != 0).any()  # some searches ended on a fractional position


def test_oracle_vs_golden(oracle):
    z = np.load(GOLDEN)
    for gi, (dist, psad, ctype) in enumerate(mc.FULLPEL_GRID):
        rng = np.random.default_rng(100 + dist * 10 + psad * 3 + ctype)
        src, refp = mc.planes(7 + dist)
        tables = mc.cost_tables(rng)
        rounds = mc.fullpel_chain(rng, 40, dist, psad)
        got = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, 37, tables)
        np.testing.assert_array_equal(np.stack([c for c, _ in got]), z[f"fp_cost_{gi}"])
        np.testing.assert_array_equal(np.stack([m for _, m in got]), z[f"fp_mv_{gi}"])
    for si in range(len(mc.SUBPEL_SETTINGS)):
        rng = np.random.default_rng(300 + si)
        src, refp = mc.planes(11 + si)
        tables = mc.cost_tables(rng)
        jobs = mc.subpel_jobs(rng, 60)
        got = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, mc.SUBPEL_SETTINGS[si], 41, 36, tables)
        for k in got:
            np.testing.assert_array_equal(got[k], z[f"sp_{k}_{si}"], err_msg=f"{k} {si}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# Plane edges, ties, every MV cost mode, odd strides, the chaining contract (tests/golden/md_search_edges.npz)
# ---------------------------------------------------------------------------------------------------------------------------------------
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_search_edges.npz")
N_EDGE = len(mc.FULLPEL_EDGE_GRID)


def assert_traces_equal(a, b, what):
    assert len(a) == len(b)
    for r, ((ca, ma), (cb, mb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ca, cb, err_msg=f"{what} round {r} cost")
        np.testing.assert_array_equal(ma, mb, err_msg=f"{what} round {r} mv")


def test_edge_chain_reaches_the_search_area_adjustment(oracle):
    """The inputs prove their own coverage, from the job fields and the four comparisons restated in md_search_cases.adjusted_area (nothing here
    comes from a kernel's output): shares of the 1536 round-0 edge jobs that the adjustment moves, empties, and pushes under the wide form's 8
    columns; and, with the oracle's chained centres, that the sparse-level skip rule fires in round 1."""
    n = adjusted = empty = wide_after = lost_wide = skipped = 0
    sides = [0] * 4
    for ci in range(N_EDGE):
        src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci)
        for j in rounds[0]:
            a = mc.adjusted_area(j, j["mvx"], j["mvy"])
            n += 1
            adjusted += any(a["sides"]) and not a["empty"]
            empty += a["empty"]
            for k in range(4):
                sides[k] += a["sides"][k]
            wide_after += any(a["sides"]) and a["wide"] and not a["empty"]
            lost_wide += a["wide_before"] and not a["wide"] and not a["empty"]
        centres = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds[:1], ctype, epb, tables)[0][1]
        for j, (cx, cy) in zip(rounds[1], centres):
            plain = j.copy()
            plain["flags"] = int(j["flags"]) & (0xFF ^ abi.FP_SPRS_LEV0_DONE)
            skipped += len(mc.visited_positions(j, cx, cy)) < len(mc.visited_positions(plain, cx, cy))
    print(f"edge jobs {n}: adjusted and non-empty {adjusted}, empty {empty}, sides {sides}, wide after an adjustment {wide_after}, lost the wide form {lost_wide}, "
          f"round-1 jobs with skipped positions {skipped}")
    assert adjusted >= 0.20 * n
    assert all(s >= 0.10 * n for s in sides)
    assert 0.05 * n <= empty <= 0.35 * n
    assert wide_after >= 20
    assert lost_wide >= 10
    assert skipped >= 0.20 * n


def test_tie_content_really_ties():
    """On the tie contents, among the round-0 edge jobs that bring no best of their own (0xFFFFFFFF), at least half have two or more visited
    positions at the winning cost (plain numpy distortion + the MV rate restated in md_search_cases): the visiting order decides them.  And on
    `flat` with MV_COST_OPT some areas of several positions have a single winner, so the rate decides too."""
    jobs = tied = flat_opt_unique = 0
    for ci, (kind, dist, psad, ctype) in enumerate(mc.FULLPEL_EDGE_GRID):
        if kind == "noise":
            continue
        src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci)
        for j in rounds[0]:
            if int(j["best_cost"]) != 0xFFFFFFFF:
                continue
            costs = mc.position_costs(src, refp, j, j["mvx"], j["mvy"], ctype, epb, tables)
            jobs += 1
            at_min = costs.count(min(costs)) if costs else 0
            tied += at_min >= 2
            flat_opt_unique += kind == "flat" and ctype == 4 and len(costs) >= 2 and at_min == 1
    print(f"tie-content jobs without an incoming best {jobs}: tied at the winning cost {tied}; flat / MV_COST_OPT with a single winner {flat_opt_unique}")
    assert 2 * tied >= jobs
    assert flat_opt_unique >= 5


def test_position_costs_restatement_matches_oracle(oracle):
    """the numpy restatement behind the tie count is itself right: first minimum in visiting order = the oracle's round-0 winner"""
    for ci in range(0, N_EDGE, 3):
        src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci)
        cost, mv = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds[:1], ctype, epb, tables)[0]
        for i, j in enumerate(rounds[0]):
            costs = mc.position_costs(src, refp, j, j["mvx"], j["mvy"], ctype, epb, tables)
            if costs and min(costs) < int(j["best_cost"]):
                px, py = mc.visited_positions(j, j["mvx"], j["mvy"])[costs.index(min(costs))]
                assert (int(cost[i]), int(mv[i][0]), int(mv[i][1])) == (min(costs), int(j["mvx"]) + 8 * px, int(j["mvy"]) + 8 * py), (ci, i)
            else:
                assert (int(cost[i]), int(mv[i][0]), int(mv[i][1])) == (int(j["best_cost"]), -1, -1), (ci, i)


@pytest.mark.parametrize("chain", ["edge", "std"])
@pytest.mark.parametrize("ci", range(N_EDGE))
def test_fullpel_edges_and_ties_oracle_equals_reference(oracle, ref, ci, chain):
    src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci, chain)
    a = mc.run_fullpel_cpu(ref.ref_md_fullpel_batch, src, refp, rounds, ctype, epb, tables)
    b = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, epb, tables)
    assert_traces_equal(a, b, f"{mc.FULLPEL_EDGE_GRID[ci]} {chain}")


def subpel_groups(grid):
    """(kind, setting index) of every run of six cost types in a sub-pel grid"""
    return [(kind, si) for kind, si, ctype in grid if ctype == 0]


def check_subpel_group(oracle, ref, kind, si, far):
    grid = mc.SUBPEL_FAR_GRID if far else mc.SUBPEL_TIE_GRID
    c0 = grid.index((kind, si, 0))
    for ci in range(c0, c0 + 6):
        assert grid[ci] == (kind, si, ci - c0)
        src, refp, tables, jobs, setting = mc.subpel_edge_case(ci, far)
        a = mc.run_subpel_cpu(ref.ref_md_subpel_batch, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        b = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{grid[ci]} {k}")
        if kind == "noise" and setting[1] < 3:
            assert (a["best_mv"] % 8 != 0).any(), grid[ci]  # some searches ended on a fractional position, in every cost mode


@pytest.mark.parametrize("kind,si", subpel_groups(mc.SUBPEL_TIE_GRID))
def test_subpel_every_cost_type_oracle_equals_reference(oracle, ref, kind, si):
    check_subpel_group(oracle, ref, kind, si, False)


@pytest.mark.parametrize("kind,si", subpel_groups(mc.SUBPEL_FAR_GRID))
def test_subpel_far_jobs_every_cost_type_oracle_equals_reference(oracle, ref, kind, si):
    check_subpel_group(oracle, ref, kind, si, True)


def test_oracle_vs_edges_golden(oracle):
    z = np.load(EDGES)
    for chain, key in (("edge", "fe"), ("std", "fc")):
        for ci in range(N_EDGE):
            src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci, chain)
            got = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, rounds, ctype, epb, tables)
            np.testing.assert_array_equal(np.stack([c for c, _ in got]), z[f"{key}_cost"][ci], err_msg=f"{chain} {ci}")
            np.testing.assert_array_equal(np.stack([m for _, m in got]), z[f"{key}_mv"][ci], err_msg=f"{chain} {ci}")
    for far, key in ((False, "st"), (True, "sf")):
        for ci in range(len(mc.SUBPEL_FAR_GRID if far else mc.SUBPEL_TIE_GRID)):
            src, refp, tables, jobs, setting = mc.subpel_edge_case(ci, far)
            got = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
            for k in got:
                np.testing.assert_array_equal(got[k], z[f"{key}_{k}"][ci], err_msg=f"far={far} {ci} {k}")


def strided_fullpel(ci, chain="edge"):
    src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(ci, chain)
    s, r = mc.strided(src, 1), mc.strided(refp, 2)
    return s, r, tables, [mc.restride(j, s.strides[0]) for j in rounds], ctype, epb


def strided_subpel(ci, far=True):
    src, refp, tables, jobs, setting = mc.subpel_edge_case(ci, far)
    s, r = mc.strided(src, 1), mc.strided(refp, 2)
    return s, r, tables, mc.restride(jobs, s.strides[0], r.strides[0]), setting


def test_strided_planes_oracle_equals_reference(oracle, ref):
    """planes as views into wider arrays, the strides (354 and 514) not multiples of 4: the reference and the oracle on the views"""
    for ci in range(0, N_EDGE, 5):
        for chain in ("edge", "std"):
            s, r, tables, rounds, ctype, epb = strided_fullpel(ci, chain)
            assert s.strides[0] % 4 and r.strides[0] % 4 and not s.flags.c_contiguous
            a = mc.run_fullpel_cpu(ref.ref_md_fullpel_batch, s, r, rounds, ctype, epb, tables)
            b = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, s, r, rounds, ctype, epb, tables)
            assert_traces_equal(a, b, f"strided {ci} {chain}")
    for ci in range(0, len(mc.SUBPEL_FAR_GRID), 7):
        s, r, tables, jobs, setting = strided_subpel(ci)
        a = mc.run_subpel_cpu(ref.ref_md_subpel_batch, s, r, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        b = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, s, r, jobs, setting, mc.SUBPEL_EPB, mc.SUBPEL_QP, tables)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"strided sub-pel {ci} {k}")


def test_chain_from_out_of_range_is_ignored(oracle):
    """both chain flags with chain_from = -1 (or >= n_jobs) = the same job with the flags clear"""
    src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(1)
    plain = rounds[0]
    want = mc.run_fullpel_cpu(oracle.orc_md_fullpel_batch, src, refp, [plain], ctype, epb, tables)
    for bad in (-1, len(plain), 2 ** 31 - 1, -2 ** 31):
        flagged = plain.copy()
        flagged["flags"] |= abi.FP_CENTRE_FROM_CHAIN | abi.FP_BEST_FROM_CHAIN
        flagged["chain_from"] = bad
        n = len(plain)  # the output arrays lie inside larger ones: a read of index -1 or n would stay in them, and would bring other values
        cost, mv = np.full(n + 2, 0x1234, np.uint32), np.full((n + 2, 2), 77, np.int16)
        d = mc.fullpel_desc(src, refp, flagged, ctype, epb, tables, cost[1:-1], mv[1:-1])
        assert oracle.orc_md_fullpel_batch(__import__("ctypes").byref(d)) == 0
        np.testing.assert_array_equal(cost[1:-1], want[0][0])
        np.testing.assert_array_equal(mv[1:-1], want[0][1])


def test_oracle_rejects_a_chain_to_another_index(oracle):
    """jobs of a batch run concurrently on the device: the oracle refuses what would race there, so that no test can pin it"""
    import ctypes as C
    src, refp, tables, rounds, ctype, epb = mc.fullpel_edge_case(1)
    n = len(rounds[0])
    for flag in (abi.FP_CENTRE_FROM_CHAIN, abi.FP_BEST_FROM_CHAIN):
        jobs = rounds[0].copy()
        jobs["flags"][5] |= flag
        jobs["chain_from"][5] = 4
        cost, mv = np.zeros(n, np.uint32), np.zeros((n, 2), np.int16)
        assert oracle.orc_md_fullpel_batch(C.byref(mc.fullpel_desc(src, refp, jobs, ctype, epb, tables, cost, mv))) != 0
        jobs["chain_from"][5] = 5  # its own slot: accepted
        assert oracle.orc_md_fullpel_batch(C.byref(mc.fullpel_desc(src, refp, jobs, ctype, epb, tables, cost, mv))) == 0
