"""CPU: what tests/test_lvmap_trips_gpu.py relies on (tests/lvmap_trip_cases.py) -- the launch plan of the rate and RDOQ batches against
svt_hip_lvmap_plan, the adversarial orders (every pair of consecutive trips on every wave slot is heavy / light in turn, every kind is met), the
restatements' independence of the job order, and the tiling of the large batches."""
import ctypes as C

import numpy as np
import pytest

import coeff_rate_cases as cr
import lvmap_trip_cases as lt
import rdoq_cases as rq
from svt_av1_psyex_amd import api


@pytest.fixture(scope="module")
def rate_cases():
    return [c for c in cr.cases_from_arrays(np.load(cr.GOLDEN)) if c["plane"] == 0 and c["reduced"] == 0]


@pytest.mark.parametrize("tx_size", range(cr.N_TX_SIZES))
def test_plan_equals_svt_hip_lvmap_plan(tx_size):
    w, h = cr.packed_dims(tx_size)
    jpw = {16: 4, 32: 2}.get(w * h, 1)
    for max_grid in (0, 1, 2, 2048):
        cap = (max_grid or 2048) * 4 * jpw  # the jobs of one trip under the cap
        for n_jobs in (1, jpw, jpw + 1, cap - 1, cap, cap + 1, 2 * cap + 1):
            got = api.lvmap_plan(tx_size, n_jobs, max_grid)
            assert got == lt.plan(tx_size, n_jobs, max_grid), (n_jobs, max_grid)
            grid, n_packs, per_pack = got
            assert per_pack == jpw and (n_packs - 1) * jpw < n_jobs <= n_packs * jpw and 1 <= grid <= (max_grid or 2048)
            assert grid * 4 >= n_packs or grid == (max_grid or 2048)
            assert lt.trips_of(got) == (1 if n_jobs <= cap else 2 if n_jobs <= 2 * cap else 3)
    assert api.lvmap_plan(tx_size, 0) == lt.plan(tx_size, 0) == (0, 0, jpw)
    assert api.lvmap_plan(tx_size, 0xFFFFFFFF, 0)[:2] == (2048, -(-0xFFFFFFFF // jpw))


def test_plan_rejects_what_it_cannot_answer():
    with pytest.raises(api.SvtHipError):
        api.lvmap_plan(cr.N_TX_SIZES, 1)
    out = C.c_uint32()
    assert api.lib().svt_hip_lvmap_plan(0, 1, 0, None, C.byref(out), C.byref(out)) == 2
    assert api.lib().svt_hip_context_set_lvmap_max_grid(None, 1) == 2


def test_the_production_launches_are_what_they_claim():
    """trips under the default cap: none beyond the first at 8192 packs, two at 8193, three at 2 * 8192 + 1; a few waves only at 8192 + 9"""
    assert lt.CAP_PACKS == 8192
    for tx_size, n_packs, last in lt.PRODUCTION:
        n = lt.production_jobs(tx_size, n_packs, last)
        p = api.lvmap_plan(tx_size, n)
        assert p == lt.plan(tx_size, n) and p[:2] == (2048, n_packs) and n == (n_packs - 1) * p[2] + 1
        assert lt.trips_of(p) == -(-n_packs // 8192)
    assert sorted(lt.trips_of(lt.plan(ts, lt.production_jobs(ts, n, last))) for ts, n, last in lt.PRODUCTION if ts == 1) == [1, 2, 3]
    assert all(n - 8192 == 9 for ts, n, _ in lt.PRODUCTION if ts in (2, 4))  # nine waves of 8192 take a second pack


def check_orders(build, size_of, run):
    """every order of lt.ORDERS of a case: the pairs, the coverage, the plan, the restatement on the ordered case against the ordered results"""
    for max_grid, light_first in lt.ORDERS:
        c, kinds, light, order, slots, want_all = build(max_grid, light_first)
        p = lt.plan(c["tx_size"], len(order), max_grid)
        assert p[0] == max_grid and lt.slots_of(p) == slots and lt.trips_of(p) >= 3
        assert p[2] == 1 or len(order) % p[2]  # the last pack is short
        assert lt.order_faults(kinds, order, light, slots) == [], (max_grid, light_first)
        first = kinds[order[0]]
        assert (first in light) == light_first and (first == "heavy") != light_first
        got = run(c)
        for name in got:
            assert np.array_equal(got[name], want_all[name][order]), (name, max_grid, light_first)
        assert size_of(c) == len(order)


@pytest.mark.parametrize("tx_size,name,fallback", lt.RDOQ_ORDER_CASES)
def test_rdoq_orders_alternate_heavy_and_light_on_every_wave_slot(tx_size, name, fallback):
    k = lt.rdoq_case(tx_size, name)
    c_all, inp_all, kinds, n0 = lt.rdoq_extended(k)
    T = rq.shared()["tables"][c_all["table"]]
    want_all = rq.run_case(T, c_all, inp_all, fallback)
    light = lt.rdoq_light_kinds(c_all)
    assert ("gated" in light) == (name == "eob_th85" and tx_size != 4) and set(light) | {"gated"} == set(lt.RDOQ_LIGHT)
    heavy = [i for i, kind in enumerate(kinds) if kind == "heavy"]
    top = np.percentile(inp_all["eob"][:n0], 75) if name != "eob_th85" else 0  # behind the gate: the top quartile of what it lets through
    for i in heavy:  # what "heavy" means, on the results
        q_in, q_out = inp_all["qcoeff"][i], want_all["qcoeff"][i]
        assert want_all["status"][i] == rq.ST_OPTIMISED and inp_all["eob"][i] >= top
        assert np.any((q_out != 0) & (np.abs(q_out) == np.abs(q_in) - 1)) and np.any((q_in != 0) & (q_out == 0))
    ordered = {}

    def build(max_grid, light_first):
        c, inp, kinds_, light_, order, slots = lt.rdoq_ordered(k, max_grid, light_first)
        ordered[id(c)] = inp
        return c, kinds_, light_, order, slots, want_all
    check_orders(build, lambda c: len(c["jobs"]), lambda c: rq.run_case(T, c, ordered[id(c)], fallback))


@pytest.mark.parametrize("lvl", [1, 2])
@pytest.mark.parametrize("tx_size", lt.RATE_ORDER_SIZES)
def test_rate_orders_alternate_heavy_and_light_on_every_wave_slot(rate_cases, tx_size, lvl):
    c0 = next(c for c in rate_cases if c["tx_size"] == tx_size)
    T = rq.shared()["tables"][c0["table"]]
    c_all, n0 = lt.rate_extended(c0)
    assert len(c_all["jobs"]) == n0 + 2
    kinds = lt.rate_kinds(c_all, lvl)
    n = c_all["qcoeff"].shape[1]
    for i, kind in enumerate(kinds):
        if kind == "heavy":
            assert c_all["eob"][i] >= n - 1 and np.max(np.abs(c_all["qcoeff"][i])) >= 127
    want_all = {"bits": cr.run_case(T, c_all, lvl, variants=[(1, 0)])[1][0]}
    light = lt.rate_light_kinds(c_all, lvl)
    assert ("shortcut" in light) == (lvl == 2 and tx_size not in (0, 5)) and ("eob0" in light) != ("shortcut" in light)
    # the kinds are the kernel's branches: a short-cut job costs 6000 + 1000 * eob, the two spoiled kinds are undefined, a heavy job is neither
    for i, kind in enumerate(kinds):
        bits = int(want_all["bits"][i])
        assert (bits == cr.UNDEFINED) == (kind in ("skip_ctx", "tx_type")) or kind == "other", (i, kind)
        assert kind != "shortcut" or bits == 6000 + 1000 * int(c_all["eob"][i])

    def build(max_grid, light_first):
        c, kinds_, light_, order, slots = lt.rate_ordered(c0, lvl, max_grid, light_first)
        return c, kinds_, light_, order, slots, want_all
    check_orders(build, lambda c: len(c["jobs"]), lambda c: {"bits": cr.run_case(T, c, lvl, variants=[(1, 0)])[1][0]})


def test_order_faults_sees_a_broken_order():
    kinds = ["heavy", "eob0", "eob1", "other"]
    light = ("eob0", "eob1")
    order = lt.adversarial_order(kinds, light, 2)
    assert lt.order_faults(kinds, order, light, 2) == []
    assert [kinds[i] for i in order[:4]] == ["heavy", "heavy", "eob0", "eob1"]
    assert lt.order_faults(kinds, order, light, 3)  # other wave slots: the pairs no longer alternate
    swapped = order.copy()
    swapped[2] = 0
    assert any("heavy then heavy" in f for f in lt.order_faults(kinds, swapped, light, 2))
    assert any("eob1 never follows" in f for f in lt.order_faults(kinds, np.where(order == 2, 1, order), ("eob0", "eob1"), 2))
    with pytest.raises(AssertionError):
        lt.adversarial_order(["heavy", "eob0"], light, 2)  # a light kind without a job fails, it is not passed over


def test_tiled_batches_shift_the_case_against_the_wave_slots(rate_cases):
    """the large batches and the repeated fixture cases: the period of the jobs is no divisor of the wave slots, so on every slot the job of a
    trip is not the job of the trip before"""
    cases = rq.shared()["cases"]
    seen_drop = False
    for tx_size, n_packs, last in lt.PRODUCTION:
        n = lt.production_jobs(tx_size, n_packs, last)
        for n_case in (len(cases[lt.rdoq_case(tx_size, "plain")]["jobs"]), len(next(c for c in rate_cases if c["tx_size"] == tx_size)["jobs"])):
            idx = lt.tiled(n_case, n, tx_size)
            s = lt.slots_of(lt.plan(tx_size, n))
            period = int(idx.max()) + 1
            assert len(idx) == n and period in (n_case, n_case - 1) and s % period and np.array_equal(idx[period:], idx[:-period])
            assert n <= s or np.all(idx[s:] != idx[:-s])
    idx = lt.tiled(16, 100, 0, 1)  # sixteen wave slots, sixteen jobs: the last job goes
    assert int(idx.max()) == 14 and np.all(idx[16:] != idx[:-16])
    for ts in range(cr.N_TX_SIZES):  # the fixture cases under a cap of one workgroup: three trips, repeated where they are short
        for n_case in [len(c["jobs"]) for c in cases if c["tx_size"] == ts] + [len(c["jobs"]) for c in rate_cases if c["tx_size"] == ts]:
            reps = lt.repeats_for_three_trips(ts, n_case)
            seen_drop |= reps > 1
            assert reps <= 2 and lt.trips_of(lt.plan(ts, reps * n_case, 1)) >= 3 and lt.trips_of(lt.plan(ts, reps * n_case, 2)) >= 2
            assert reps == 1 or np.array_equal(lt.tiled(n_case, reps * n_case, ts, 1), np.arange(reps * n_case) % n_case)
    assert seen_drop  # the 25 jobs of a 16-coefficient case are seven packs: two trips


def test_ragged_groups_straddle_the_trips_of_the_production_cap():
    n = lt.production_jobs(1, 2 * lt.CAP_PACKS + 1, 1)
    gs = lt.ragged_groups(n)
    assert gs[0] == 0 and gs[-1] == n and set(np.diff(gs)[:-1].tolist()) == {1, 2, 3, 4, 5, 6, 7}
    for edge in (lt.CAP_PACKS, 2 * lt.CAP_PACKS):  # a group with jobs on both sides of the first job of trip 2, of trip 3
        g = int(np.searchsorted(gs, edge, side="right")) - 1
        assert gs[g] < edge < gs[g + 1]
