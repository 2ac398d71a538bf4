"""GPU: svt_hip_coeff_rate_batch and svt_hip_rdoq_batch past one trip of their capped grid, every comparison exact.  Both kernels launch at most
2048 workgroups of four waves and let every wave walk its share of the packs in a loop; a wave takes a second pack only past 8192 packs, which
no other test reaches.  Here the cap is lowered to one and two workgroups (Context.set_lvmap_max_grid), so that the fixture cases and orders
built to carry state from one job into the next (tests/lvmap_trip_cases.py) run at several trips, and batches of production size run under the
default cap.  Every test proves through svt_hip_lvmap_plan that its batch is multi-trip and prints the trip count; every output array is
pre-filled with 0xA5 and followed by spare slots (the helpers of test_rdoq_gpu.py and test_coeff_rate_gpu.py)."""
import numpy as np
import pytest

import coeff_rate_cases as cr
import lvmap_trip_cases as lt
import rdoq_cases as rq
import test_coeff_rate_gpu as cg
import test_rdoq_gpu as rg
from svt_av1_psyex_amd import api, rate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev_tables(hip_ctx):
    return [rate.upload_tables(T) for T in rq.shared()["tables"]]


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def rate_cases(golden):
    return cr.cases_from_arrays(golden)


def trips(tx_size, n_jobs, max_grid, what, single=False):
    """the trips of a batch by svt_hip_lvmap_plan, printed; more than one unless the launch is the declared single-trip one"""
    p = api.lvmap_plan(tx_size, n_jobs, max_grid)
    assert p == lt.plan(tx_size, n_jobs, max_grid)
    t = lt.trips_of(p)
    print(f"{what}: tx_size {tx_size}, {n_jobs} jobs in {p[1]} packs, {p[0]} workgroups: {t} trips")
    assert (p[1] > p[0] * lt.K_WAVES and t > 1) != single
    return t


def capped(ctx, max_grid, launch):
    """launch() (which waits for its batch) under the cap max_grid; the context is shared, so the default comes back whatever happens"""
    ctx.set_lvmap_max_grid(max_grid)
    try:
        return launch()
    finally:
        ctx.set_lvmap_max_grid(0)


def compare_rdoq(got, want, n, what):
    """rg.compare, by whole arrays where they agree (the large batches have tens of thousands of jobs)"""
    if not all(np.array_equal(got[name], want[name][:n]) for name in ("status", "eob", "qcoeff", "dqcoeff")):
        rg.compare(got, want, n, what)  # names the jobs
    w = want["written"][:n]
    assert np.array_equal(got["dist_coeff"][w], want["dist_coeff"][:n][w]) and np.array_equal(got["cul_level"][w], want["cul_level"][:n][w]), what
    assert np.all(got["dist_coeff"][~w].view(np.uint8) == rg.FILL) and np.all(got["cul_level"][~w] == rg.FILL), what


# ---- a. every fixture case under a cap of one and of two workgroups ------------------------------------------------------------------------
@pytest.mark.parametrize("tx_size", range(cr.N_TX_SIZES))
def test_rdoq_fixture_cases_do_not_change_a_byte_under_a_cap_of_one_and_two_workgroups(hip_ctx, dev_tables, tx_size):
    """every variant of the size with the fallback arrays, against the restatement and the reference's own results; a case too short for three
    trips under one workgroup (the 25 jobs of TX_4X4 are seven packs) runs repeated"""
    ran = 0
    for k, c0 in enumerate(rq.shared()["cases"]):
        if c0["tx_size"] != tx_size:
            continue
        inp0, want0, _ = rq.restated(k)
        n0 = len(c0["jobs"])
        idx = lt.tiled(n0, lt.repeats_for_three_trips(tx_size, n0) * n0, tx_size, 1)
        n = len(idx)
        assert idx.max() == n0 - 1 and (lt.plan(tx_size, n)[2] == 1 or n % lt.plan(tx_size, n)[2])  # the whole case; a wave's last group has no job
        c, inp, want, ref = lt.take(c0, idx, lt.RDOQ_JOB_KEYS), lt.take(inp0, idx), lt.take(want0, idx), c0["ref"]
        name = rq.VARIANTS[c0["variant"]][0]
        for max_grid in lt.GRIDS:
            assert trips(tx_size, n, max_grid, f"rdoq {name}") >= (3 if max_grid == 1 else 2)
            got = capped(hip_ctx, max_grid, lambda: rg.run(hip_ctx, dev_tables[c["table"]], c, inp, n))
            rg.compare(got, want, n, (name, max_grid))
            assert np.array_equal(got["qcoeff"], ref["qcoeff"][idx]) and np.array_equal(got["eob"], ref["eob"][idx]), (name, max_grid)
            assert np.array_equal(got["cul_level"], ref["cul_level"][idx]) and np.array_equal(got["status"], ref["status"][idx]), (name, max_grid)
            assert rq.crc(got["dqcoeff"][:n0]) == ref["dqcoeff_crc"] and np.array_equal(got["dqcoeff"], got["dqcoeff"][:n0][idx]), (name, max_grid)
        ran += 1
    assert ran == len(rq.VARIANTS)


@pytest.mark.parametrize("tx_size", range(cr.N_TX_SIZES))
def test_rate_fixture_cases_do_not_change_a_byte_under_a_cap_of_one_and_two_workgroups(hip_ctx, golden, rate_cases, dev_tables, tx_size):
    """the three cases of the size at every (mds_fast_coeff_est_level, mds_subres_step), against the reference's own results and the restatement"""
    ran = 0
    for c in rate_cases:
        if c["tx_size"] != tx_size:
            continue
        T = rq.shared()["tables"][c["table"]]
        n = cg.odd_count(tx_size, len(c["jobs"]))
        assert lt.repeats_for_three_trips(tx_size, n) == 1
        _, want = cr.run_case(T, c)
        for v, variant in enumerate(cr.RATE_VARIANTS):
            ref = golden["bits"][v, c["first_job"]:c["first_job"] + n]
            fixture = np.array([cr.frame_bits(T, tx_size, c["plane"], int(r), int(e), int(j["txb_skip_ctx"]), 1, variant[1])
                                for r, e, j in zip(ref, c["eob"], c["jobs"])], np.uint64)
            for max_grid in lt.GRIDS:
                if v == 0:
                    assert trips(tx_size, n, max_grid, f"rate plane {c['plane']} reduced {c['reduced']}") >= (3 if max_grid == 1 else 2)
                got = capped(hip_ctx, max_grid, lambda: cg.run(hip_ctx, dev_tables[c["table"]], c, n, variant))["bits"]
                assert np.array_equal(got, fixture) and np.array_equal(got, want[v][:n]), (c["plane"], c["reduced"], variant, max_grid)
                ran += 1
    assert ran == 3 * len(cr.RATE_VARIANTS) * len(lt.GRIDS)


# ---- b, c. orders in which every wave meets heavy and light jobs in turn ---------------------------------------------------------------------
@pytest.mark.parametrize("tx_size,name,fallback", lt.RDOQ_ORDER_CASES)
def test_rdoq_heavy_and_light_jobs_in_turn_on_every_wave(hip_ctx, dev_tables, tx_size, name, fallback):
    """heavy -> light and light -> heavy under both caps (tests/test_lvmap_trips.py proves the orders are what they claim): a long optimised job
    followed on the same lanes by an empty, a one-coefficient, a gated, an undefined or an over-long one, and the reverse.  Without the fallback
    arrays a gated job on a later trip must be left untouched."""
    k = lt.rdoq_case(tx_size, name)
    for max_grid, light_first in lt.ORDERS:
        c, inp, kinds, light, order, slots = lt.rdoq_ordered(k, max_grid, light_first)
        n = len(order)
        assert trips(tx_size, n, max_grid, f"rdoq {name} {'light' if light_first else 'heavy'} first") >= 3
        want = rq.run_case(rq.shared()["tables"][c["table"]], c, inp, fallback)
        got = capped(hip_ctx, max_grid, lambda: rg.run(hip_ctx, dev_tables[c["table"]], c, inp, n, fallback=fallback))
        rg.compare(got, want, n, (name, fallback, max_grid, light_first))
        gated = np.array([kinds[i] == "gated" for i in order])
        assert np.any(gated[slots:]) == ("gated" in light)  # on a trip behind the first
        if not fallback:
            assert np.array_equal(got["qcoeff"][gated], inp["qcoeff"][gated]) and np.array_equal(got["dqcoeff"][gated], inp["dqcoeff"][gated])
            assert np.array_equal(got["eob"][gated], inp["eob"][gated]) and np.all(got["status"][gated] == rq.ST_GATED)


@pytest.mark.parametrize("lvl", [1, 2])
@pytest.mark.parametrize("tx_size", lt.RATE_ORDER_SIZES)
def test_rate_heavy_and_light_jobs_in_turn_on_every_wave(hip_ctx, rate_cases, dev_tables, tx_size, lvl):
    """a job of a full block with clamped levels followed on the same lanes by one that writes no level at all (a short-cut at level 2, eob 0,
    a context or a transform type outside its table), and the reverse"""
    c0 = next(c for c in rate_cases if c["tx_size"] == tx_size and c["plane"] == 0 and c["reduced"] == 0)
    for max_grid, light_first in lt.ORDERS:
        c, _, _, order, _ = lt.rate_ordered(c0, lvl, max_grid, light_first)
        n = len(order)
        assert trips(tx_size, n, max_grid, f"rate level {lvl} {'light' if light_first else 'heavy'} first") >= 3
        want = cr.run_case(rq.shared()["tables"][c["table"]], c, lvl, variants=[(1, 0)])[1][0]
        got = capped(hip_ctx, max_grid, lambda: cg.run(hip_ctx, dev_tables[c["table"]], c, n, (1, 0), lvl))["bits"]
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (max_grid, light_first, [(int(i), int(order[i]), int(got[i]), int(want[i])) for i in bad[:6]])


# ---- d. the default cap --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tx_size,n_packs,last", lt.PRODUCTION)
def test_rdoq_under_the_default_cap(hip_ctx, dev_tables, tx_size, n_packs, last):
    """the plain case of the size (eob_th85 for the TX_8X8 batch of 8193 packs) repeated to batches of production size; 8192 packs are the
    last single trip"""
    k = lt.rdoq_case(tx_size, "eob_th85" if (tx_size, n_packs) == (1, lt.CAP_PACKS + 1) else "plain")
    c0 = rq.shared()["cases"][k]
    inp0, want0, _ = rq.restated(k)
    n = lt.production_jobs(tx_size, n_packs, last)
    trips(tx_size, n, 0, "rdoq, default cap", single=n_packs == lt.CAP_PACKS)
    idx = lt.tiled(len(c0["jobs"]), n, tx_size)
    c, inp, want = lt.take(c0, idx, lt.RDOQ_JOB_KEYS), lt.take(inp0, idx), lt.take(want0, idx)
    assert np.any(want["qcoeff"] != inp["qcoeff"])  # RDOQ acts
    got = rg.run(hip_ctx, dev_tables[c["table"]], c, inp, n, spare=lt.SPARE)
    compare_rdoq(got, want, n, (tx_size, n_packs))


@pytest.mark.parametrize("tx_size,n_packs,last", lt.PRODUCTION)
def test_rate_under_the_default_cap(hip_ctx, rate_cases, dev_tables, tx_size, n_packs, last):
    c0 = next(c for c in rate_cases if c["tx_size"] == tx_size and c["plane"] == 0 and c["reduced"] == 0)
    n = lt.production_jobs(tx_size, n_packs, last)
    trips(tx_size, n, 0, "rate, default cap", single=n_packs == lt.CAP_PACKS)
    idx = lt.tiled(len(c0["jobs"]), n, tx_size)
    c = lt.take(c0, idx, lt.RATE_JOB_KEYS)
    want = cr.run_case(rq.shared()["tables"][c0["table"]], c0, variants=[(1, 0)])[1][0][idx]
    got = cg.run(hip_ctx, dev_tables[c["table"]], c, n, spare=lt.SPARE)["bits"]
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), int(idx[i]), int(got[i]), int(want[i])) for i in bad[:6]]


def test_rate_group_winners_under_the_default_cap(hip_ctx, rate_cases, dev_tables):
    """TX_8X8, 2 * 8192 + 1 packs, RD costs and groups of 1 .. 7 jobs in turn: the winners are picked from costs that three trips wrote, two groups
    have jobs on both sides of a trip's first job, and every fifth group holds one job repeated, whose equal costs go to the first"""
    tx_size = 1
    c0 = next(c for c in rate_cases if c["tx_size"] == tx_size and c["plane"] == 0 and c["reduced"] == 0)
    n = lt.production_jobs(tx_size, 2 * lt.CAP_PACKS + 1, 1)
    assert trips(tx_size, n, 0, "rate with groups, default cap") == 3
    gs = lt.ragged_groups(n)
    idx = lt.tiled(len(c0["jobs"]), n, tx_size).copy()
    same = [g for g in range(0, len(gs) - 1, 5) if gs[g + 1] - gs[g] > 1]
    for g in same:
        idx[gs[g]:gs[g + 1]] = idx[gs[g]]
    for edge in (lt.CAP_PACKS, 2 * lt.CAP_PACKS):
        g = int(np.searchsorted(gs, edge, side="right")) - 1
        assert gs[g] < edge < gs[g + 1]
    c = lt.take(c0, idx, lt.RATE_JOB_KEYS)
    rng = np.random.default_rng(77)
    dist0 = rng.integers(0, 1 << 40, len(c0["jobs"]), dtype=np.uint64)
    lam = 51234
    bits0 = cr.run_case(rq.shared()["tables"][c0["table"]], c0, variants=[(1, 0)])[1][0]
    cost0 = np.array([cr.rdcost(lam, int(b), int(d)) for b, d in zip(bits0, dist0)], np.uint64)
    want_job, want_cost = cr.group_winners(cost0[idx], gs)
    got = cg.run(hip_ctx, dev_tables[c["table"]], c, n, spare=lt.SPARE, lam=lam, dist=dist0[idx], group_start=gs)
    assert np.array_equal(got["bits"], bits0[idx]) and np.array_equal(got["rd_cost"], cost0[idx])
    assert np.array_equal(got["best_job"], want_job) and np.array_equal(got["best_cost"], want_cost)
    assert len(same) > len(gs) // 7 and np.array_equal(got["best_job"][same], gs[same])  # equal costs: the first job
    assert np.any(want_job != gs[:-1]) and not np.any(want_job == cr.NO_JOB)


# ---- e. the device chain at several trips ---------------------------------------------------------------------------------------------------
def test_chain_rd_batch_rdoq_rate_batch_inverse_at_48_trips(hip_ctx, dev_tables):
    """the TX_4X4 chain of test_rdoq_gpu.py (RD batch -> RDOQ -> rate with groups -> inverse, one synchronisation) under a cap of two workgroups"""
    n = capped(hip_ctx, 2, lambda: rg.chain(hip_ctx, dev_tables, 0))
    assert trips(0, n, 2, "chain") == 48
