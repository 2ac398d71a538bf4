"""GPU: svt_hip_coeff_rate_batch on the MI355X, every comparison exact -- against the reference's own results (golden/coeff_rate.npz) and the
restatement (tests/coeff_rate_cases.py) on every case and (level, step) variant, the short-cuts, the RD cost and the group winners, the jobs
the reference leaves undefined, and the device-side chain RD batch -> rate batch."""
import numpy as np
import pytest

import coeff_rate_cases as cr
from svt_av1_psyex_amd import abi, rate, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def cases(golden):
    return cr.cases_from_arrays(golden)


@pytest.fixture(scope="module")
def tables(golden):
    return [cr.Tables.from_golden(golden, k) for k in range(len(cr.QINDEXES))]


@pytest.fixture(scope="module")
def dev_tables(hip_ctx, tables):
    return [rate.upload_tables(T) for T in tables]


@pytest.fixture(scope="module")
def restated(tables, cases):
    """the restatement's (raw, bits) of every fixture case for every variant, computed once"""
    return [cr.run_case(tables[c["table"]], c) for c in cases]


def jobs_per_wave(tx_size):
    w, h = cr.packed_dims(tx_size)
    return max(1, 64 // (w * h))


def odd_count(tx_size, n):
    """the largest job count <= n that is no multiple of the jobs per wave (a wave's last group then has no job)"""
    jpw = jobs_per_wave(tx_size)
    return n - 1 if jpw > 1 and n % jpw == 0 else n


def run(ctx, dev_table, c, n, variant=(1, 0), lvl=1, spare=None, **kw):
    """the batch on the first n jobs of a case, outputs pre-filled with 0xA5 and `spare` spare slots (default n) behind each: checks the guards,
    returns the rest"""
    spare = n if spare is None else spare
    out = rate.run_rate_hip(ctx, dev_table, c["tx_size"], c["plane"], c["jobs"][:n], c["qcoeff"][:n], c["eob"][:n], reduced_tx_set=c["reduced"],
                            coeff_rate_est_lvl=lvl, mds_fast_coeff_est_level=variant[0], mds_subres_step=variant[1], spare_jobs=spare, fill=FILL, **kw)
    res = {}
    for name, a in out.items():
        m = len(a) - spare
        assert np.all(a[m:].view(np.uint8) == FILL), f"{name}: spare slots written"
        res[name] = a[:m]
    return res


@pytest.mark.parametrize("tx_size", range(cr.N_TX_SIZES))
def test_every_size_equals_the_fixture_and_the_restatement(hip_ctx, golden, cases, tables, dev_tables, restated, tx_size):
    """every class the size admits, inter / intra, both reduced sets, luma and chroma, the eob and magnitude grids, dense and sparse blocks,
    every (mds_fast_coeff_est_level, mds_subres_step)"""
    ran = 0
    for c, (_, want) in zip(cases, restated):
        if c["tx_size"] != tx_size:
            continue
        n = odd_count(tx_size, len(c["jobs"]))
        assert jobs_per_wave(tx_size) == 1 or n % jobs_per_wave(tx_size)
        T = tables[c["table"]]
        for v, variant in enumerate(cr.RATE_VARIANTS):
            got = run(hip_ctx, dev_tables[c["table"]], c, n, variant)["bits"]
            ref = golden["bits"][v, c["first_job"]:c["first_job"] + n]
            fixture = np.array([cr.frame_bits(T, tx_size, c["plane"], int(r), int(e), int(j["txb_skip_ctx"]), 1, variant[1])
                                for r, e, j in zip(ref, c["eob"], c["jobs"])], np.uint64)
            bad = np.nonzero(got != fixture)[0]
            assert not len(bad), (c["plane"], c["reduced"], variant, [(int(i), int(c["eob"][i]), int(got[i]), int(fixture[i])) for i in bad[:5]])
            assert np.array_equal(got, want[v][:n]), (c["plane"], c["reduced"], variant)
            ran += 1
    assert ran == 3 * len(cr.RATE_VARIANTS)


@pytest.mark.parametrize("tx_size", [0, 1, 2, 3, 4])  # th = 0, 1, 4, 16, 64
def test_short_cuts_by_coeff_rate_est_lvl(hip_ctx, cases, tables, dev_tables, restated, tx_size):
    assert cr.shortcut_threshold(tx_size) == (0, 1, 4, 16, 64)[tx_size]
    for c, (raw, _) in zip(cases, restated):
        if c["tx_size"] != tx_size or c["reduced"]:
            continue
        n = odd_count(tx_size, len(c["jobs"]))
        T = tables[c["table"]]
        for lvl in (0, 1, 2, 3):
            for v, variant in ((0, (1, 0)), (8, (4, 2))):
                assert cr.RATE_VARIANTS[v] == variant
                want = np.array([cr.frame_bits(T, tx_size, c["plane"], r, int(e), int(j["txb_skip_ctx"]), lvl, variant[1])
                                 for r, e, j in zip(raw[v][:n], c["eob"], c["jobs"])], np.uint64)
                got = run(hip_ctx, dev_tables[c["table"]], c, n, variant, lvl)["bits"]
                assert np.array_equal(got, want), (c["plane"], lvl, variant)
                if c["plane"] == 0 and lvl == 0:
                    assert set(want.tolist()) <= {6000 + 1000 * e for e in range(64)} | {3000 + 100 * e for e in range(1025)}
                    assert 3000 + 100 * c["qcoeff"].shape[1] in want and (6000 in want) == (tx_size > 0)  # both sides of th


@pytest.mark.parametrize("tx_size", [1, 9, 18])
def test_level_2_with_step_1_equals_level_1_with_step_1(hip_ctx, cases, dev_tables, tx_size):
    c = next(c for c in cases if c["tx_size"] == tx_size and c["plane"] == 0 and c["reduced"] == 0)
    n = len(c["jobs"])
    a, b = run(hip_ctx, dev_tables[c["table"]], c, n, (2, 1))["bits"], run(hip_ctx, dev_tables[c["table"]], c, n, (1, 1))["bits"]
    full = run(hip_ctx, dev_tables[c["table"]], c, n, (1, 0))["bits"]
    assert np.array_equal(a, b)  # MAX(1, 2 - 1) == MAX(1, 1 - 1): the same loop before the shift ...
    assert np.array_equal(a[c["eob"] > 0], full[c["eob"] > 0] << np.uint64(1))  # ... which is the whole loop, shifted by the step


@pytest.mark.parametrize("tx_size", [0, 5, 2, 4])
def test_undefined_jobs_report_the_sentinels_and_leave_their_neighbours(hip_ctx, tables, dev_tables, tx_size):
    c, bad = cr.undefined_case(tx_size)
    assert len(bad) >= 7
    assert any(c["jobs"][i]["intra_dir"] == 13 and not c["jobs"][i]["is_inter"] for i in bad)  # an intra luma job with intra_dir out of range
    n = odd_count(tx_size, len(c["jobs"]))
    assert max(bad) < n
    _, want = cr.run_case(tables[0], c, variants=[(1, 0)])
    got = run(hip_ctx, dev_tables[0], c, n)["bits"]
    assert np.array_equal(got, want[0][:n])
    assert np.all(got[bad] == cr.UNDEFINED) and np.count_nonzero(got == cr.UNDEFINED) == len(bad)


@pytest.mark.parametrize("tx_size", [0, 6, 2, 10])
def test_intra_dir_is_read_for_intra_luma_jobs_only(hip_ctx, golden, cases, tables, dev_tables, restated, tx_size):
    """a host that copies cand->pred_mode into intra_dir for every candidate passes 13 .. 24 on inter jobs, and anything on chroma: the reference
    reads intra_dir in the intra branch of av1_transform_type_rate_estimation alone (luma), so the results are the fixture's"""
    ran = 0
    for c, (_, want) in zip(cases, restated):
        if c["tx_size"] != tx_size or c["reduced"]:
            continue
        m = cr.with_inter_pred_modes(c)
        changed = m["jobs"]["intra_dir"] != c["jobs"]["intra_dir"]
        assert np.all(m["jobs"]["intra_dir"][changed] >= 13) and np.count_nonzero(changed) > len(changed) // 3
        assert c["plane"] or not np.any(changed & (c["jobs"]["is_inter"] == 0))
        n = len(c["jobs"])
        got = run(hip_ctx, dev_tables[c["table"]], m, n)["bits"]
        ref = golden["bits"][0, c["first_job"]:c["first_job"] + n]
        fixture = np.array([cr.frame_bits(tables[c["table"]], tx_size, c["plane"], int(r), int(e), int(j["txb_skip_ctx"]), 1, 0)
                            for r, e, j in zip(ref, c["eob"], c["jobs"])], np.uint64)
        assert np.array_equal(got, fixture) and np.array_equal(got, want[0]), c["plane"]
        assert not np.any(got == cr.UNDEFINED)
        ran += 1
    assert ran == 2  # luma and chroma


@pytest.mark.parametrize("tx_size", [0, 5, 2])  # four, two and one job per wave
def test_rd_cost_and_group_winners(hip_ctx, tables, dev_tables, tx_size):
    c, bad = cr.undefined_case(tx_size)
    n0 = len(c["jobs"])
    tie = int(np.argmax(c["eob"] >= 2)) + 2
    assert tie not in bad
    extra = [tie, tie, tie, bad[0], bad[0]]  # a group of equal costs, a group whose jobs are all undefined
    extra += [tie] * (1 if (n0 + len(extra)) % max(jobs_per_wave(tx_size), 2) == 0 else 0)
    for k in ("jobs", "qcoeff", "eob"):
        c[k] = np.concatenate([c[k], c[k][extra]])
    n = len(c["jobs"])
    assert n % max(jobs_per_wave(tx_size), 2)
    sizes, starts = (3, 1, 5, 2, 7, 4, 1, 6), [0]  # no multiple of a wave's four (two) jobs: the groups straddle the waves' packing
    while starts[-1] < n0:
        starts.append(min(n0, starts[-1] + sizes[(len(starts) - 1) % len(sizes)]))
    starts += [n0 + 3, n0 + 5] + ([n] if n > n0 + 5 else [])
    group_start = np.array(starts, np.uint32)
    rng = np.random.default_rng(40 + tx_size)
    dist = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    dist[rng.integers(0, n0, 8)] = (1 << 40) - 1
    dist[n0:n0 + 3] = dist[tie]
    _, bits = cr.run_case(tables[1], c, variants=[(1, 0)])
    for lam in (1, 7, 51234, 1 << 31):
        want = np.array([cr.rdcost(lam, int(b), int(d)) for b, d in zip(bits[0], dist)], np.uint64)
        want_job, want_cost = cr.group_winners(want, group_start)
        got = run(hip_ctx, dev_tables[1], c, n, lam=lam, dist=dist, group_start=group_start)
        assert np.array_equal(got["bits"], bits[0])
        assert np.array_equal(got["rd_cost"], want), lam
        assert np.array_equal(got["best_job"], want_job) and np.array_equal(got["best_cost"], want_cost), lam
        g_tie, g_undef = len(starts) - (3 if n > n0 + 5 else 2) - 1, len(starts) - (3 if n > n0 + 5 else 2)
        assert got["best_job"][g_tie] == n0 and got["rd_cost"][n0] == got["rd_cost"][n0 + 1]  # equal costs: the first one wins
        assert got["best_job"][g_undef] == cr.NO_JOB and got["best_cost"][g_undef] == cr.UNDEFINED
        mixed = [g for g in range(len(starts) - 1) if any(starts[g] <= b < starts[g + 1] for b in bad) and starts[g + 1] - starts[g] > 1 and g < g_tie]
        assert mixed and all(got["best_job"][g] != cr.NO_JOB and got["best_job"][g] not in bad for g in mixed)  # an undefined job inside a group
        assert any(starts[g + 1] - starts[g] == 1 and got["best_job"][g] == starts[g] for g in range(g_tie))  # a group of one job


@pytest.mark.parametrize("tx_size", [0, 2, 17, 4])  # TX_4X4, TX_16X16, TX_16X64, TX_64X64
def test_chain_rd_batch_then_rate_batch_on_device(hip_ctx, tables, dev_tables, tx_size):
    """tx_type_search's cost on the device: svt_hip_rd_batch writes qcoeff, eob and the distortion, svt_hip_coeff_rate_batch reads them on the
    same stream (no host copy, one synchronisation at the end); equal to the restatement fed with the oracle's RD outputs."""
    import pyoracle
    import torch
    rng = np.random.default_rng(1300 + tx_size)
    W, H = 192, 128
    src = rng.integers(0, 1024, (H, W)).astype(np.uint16)
    pred = np.clip(src.astype(np.int32) + rng.integers(-90, 91, src.shape), 0, 1023).astype(np.uint16)
    jobs = rd.grid_jobs(W, H, W, tx_size)
    n = len(jobs)
    types = [t for t in range(16) if cr.EXT_TX_USED[cr.ext_tx_set_type(tx_size, 1, 0)][t]]
    jobs["tx_type"] = [types[i % len(types)] for i in range(n)]
    rows = np.stack([rd.quant_row_from_step(160, 220)])
    f = dict(bit_depth=10, quant_kind=0, tx_size=tx_size, src_stride=W, pred_stride=W)
    rjobs = np.zeros(n, abi.RATE_JOB_DTYPE)
    rjobs["tx_type"], rjobs["txb_skip_ctx"], rjobs["dc_sign_ctx"], rjobs["is_inter"] = jobs["tx_type"], np.arange(n) % 13, np.arange(n) % 3, 1
    rjobs["intra_dir"] = 13 + np.arange(n) % 12  # cand->pred_mode of an inter candidate (NEARESTMV ..): not read, not refused
    if len(types) > 1:  # a block's candidates: one group per run of all the admitted types
        assert tx_size in (0, 2) and n % len(types) == 0
        group_start = np.arange(0, n + 1, len(types), dtype=np.uint32)
    else:  # DCT_DCT alone: ragged groups of blocks
        starts = [0]
        while starts[-1] < n:
            starts.append(min(n, starts[-1] + (2, 3, 1)[(len(starts) - 1) % 3]))
        group_start = np.array(starts, np.uint32)
    assert np.max(np.diff(group_start)) > 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t_rjobs, t_gs = dev(rjobs), dev(group_start)
    lam = 41000
    rd_run = rd.enqueue_hip(hip_ctx, f, src, pred, jobs, rows, outputs=("qcoeff",))
    outs = rd_run.outs
    res = rate.run_rate_device(hip_ctx, dev_tables[0], tx_size, 0, t_rjobs, n, outs["qcoeff"], outs["eob"], lam=lam, dist=outs["dist_coeff"], dist_stride=2,
                               group_start=t_gs, n_groups=len(group_start) - 1)
    hip_ctx.sync()
    got = rate.download(res)
    want_rd = pyoracle.rd_batch(f, src, pred, jobs, rows, want_recon=False)
    assert np.array_equal(outs["eob"].cpu().numpy().view(np.uint16), want_rd["eob"].reshape(-1))
    assert np.count_nonzero(want_rd["eob"] > 1) > n // 2
    c = {"tx_size": tx_size, "plane": 0, "reduced": 0, "jobs": rjobs, "qcoeff": want_rd["qcoeff"], "eob": want_rd["eob"].reshape(-1)}
    _, bits = cr.run_case(tables[0], c, variants=[(1, 0)])
    assert np.array_equal(got["bits"], bits[0])
    want = np.array([cr.rdcost(lam, int(b), int(d)) for b, d in zip(bits[0], want_rd["dist_coeff"][:, 0])], np.uint64)
    assert np.array_equal(got["rd_cost"], want)
    want_job, want_cost = cr.group_winners(want, group_start)
    assert np.array_equal(got["best_job"], want_job) and np.array_equal(got["best_cost"], want_cost)
    assert not np.any(want_job == cr.NO_JOB)
    if len(types) > 1:
        assert np.any(want_job != group_start[:-1])  # the winner is not always a group's first job
