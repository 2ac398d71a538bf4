"""CPU: the restatement of the coefficient rate estimation (tests/coeff_rate_cases.py) against the reference's own results
(golden/coeff_rate.npz), what the case lists reach, and the C-ABI of svt_hip_coeff_rate_batch (validation needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import coeff_rate_cases as cr
from batch_entry_cases import good_coeff_rate_desc
from svt_av1_psyex_amd import abi, api

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def cases(golden):
    return cr.cases_from_arrays(golden)


@pytest.fixture(scope="module")
def restated(golden, cases):
    """[(raw, bits) of every case for every variant], and what the restatement read on the way"""
    tables = [cr.Tables.from_golden(golden, k) for k in range(len(cr.QINDEXES))]
    stats = [cr.new_stats() for _ in range(cr.N_TX_SIZES)]
    return [cr.run_case(tables[c["table"]], c, stats=stats[c["tx_size"]]) for c in cases], stats


def test_restatement_equals_the_reference_on_every_case(golden, cases, restated):
    assert [tuple(int(v) for v in golden["qindex"])] == [cr.QINDEXES]
    bits = golden["bits"]
    assert bits.shape == (len(cr.RATE_VARIANTS), len(golden["eob"]))
    checked = 0
    for c, (raw, _) in zip(cases, restated[0]):
        for v in range(len(cr.RATE_VARIANTS)):
            for i, r in enumerate(raw[v]):
                if c["eob"][i]:
                    assert r == int(bits[v, c["first_job"] + i]), (c["tx_size"], c["plane"], c["reduced"], i, cr.RATE_VARIANTS[v])
                    checked += 1
    assert checked > 30000


def test_intra_dir_is_read_for_intra_luma_jobs_only(golden, cases):
    """inter and chroma jobs with an intra_dir of 13 and above (an inter candidate's pred_mode) keep the reference's result; an intra luma
    job with 13 is undefined"""
    tables = [cr.Tables.from_golden(golden, k) for k in range(len(cr.QINDEXES))]
    for c in cases:
        if c["tx_size"] not in (0, 2, 10) or c["reduced"]:
            continue
        m = cr.with_inter_pred_modes(c)
        assert np.count_nonzero(m["jobs"]["intra_dir"] >= 13) > len(m["jobs"]) // 3
        raw, _ = cr.run_case(tables[c["table"]], m, variants=[(1, 0)])
        for i, r in enumerate(raw[0]):
            if c["eob"][i]:
                assert r == int(golden["bits"][0, c["first_job"] + i]), (c["tx_size"], c["plane"], i)
    c, bad = cr.undefined_case(2)
    intra13 = [i for i in bad if c["jobs"][i]["intra_dir"] == 13 and not c["jobs"][i]["is_inter"]]
    assert intra13 and len(bad) >= 7
    raw, bits = cr.run_case(tables[0], c, variants=[(1, 0)])
    assert all(raw[0][i] is None and bits[0][i] == cr.UNDEFINED for i in bad)
    assert np.count_nonzero(bits[0] == cr.UNDEFINED) == len(bad)


def test_the_two_tables_differ(golden):
    for name in cr.TABLE_SHAPES:
        assert golden[f"{name}_0"].shape == cr.TABLE_SHAPES[name]
    assert not np.array_equal(golden["coeff_fac_bits_0"], golden["coeff_fac_bits_1"])
    assert len(cr.Tables.from_golden(golden, 0).to_bytes()) == C.sizeof(abi.RateTables)


def test_fixture_holds_the_generated_cases(golden):
    want = cr.cases_to_arrays(cr.build_cases())
    for k, v in want.items():
        assert golden[k].dtype == v.dtype and np.array_equal(golden[k], v), k


def test_case_lists_reach_what_they_claim(cases, restated):
    assert {(c["tx_size"], c["plane"], c["reduced"]) for c in cases} == set(cr.CASE_KEYS)
    assert {c["table"] for c in cases} == {0, 1}
    seen_skip = {0: set(), 1: set()}
    seen_dc, seen_dir = set(), set()
    mags = {"last": set(), "dc": set(), "mid": set()}
    beyond = 0
    for c in cases:
        ts, n = c["tx_size"], c["qcoeff"].shape[1]
        assert 0 < len(c["jobs"]) < 3000
        assert set(cr.eob_grid(n)) == set(c["eob"].tolist())
        for is_inter in (0, 1):
            jobs = c["jobs"][c["jobs"]["is_inter"] == is_inter]
            used = cr.EXT_TX_USED[cr.ext_tx_set_type(ts, is_inter, c["reduced"])]
            types = set(jobs["tx_type"].tolist())
            assert types and all(used[t] for t in types)  # only types inside the size's set
            assert {cr.tx_class(t) for t in types} == {cr.tx_class(t) for t in range(16) if used[t]}  # one of every class the set admits
            if max(cr.TX_W[ts], cr.TX_H[ts]) == 64:
                assert types == {0}
        for j, q, e in zip(c["jobs"], c["qcoeff"], c["eob"]):
            e = int(e)
            seen_skip[1 if e else 0].add(int(j["txb_skip_ctx"]))
            seen_dc.add(int(j["dc_sign_ctx"]))
            seen_dir.add(int(j["intra_dir"]))
            if e:
                scan = cr.scan_order(ts, int(j["tx_type"]))
                mags["last"].add(abs(int(q[scan[e - 1]])))
                if e >= 2:
                    mags["dc"].add(int(q[0]))
                if e >= 3:
                    mags["mid"].add(abs(int(q[scan[e // 2]])))
                beyond += bool(np.any(q[scan[e:]]))
    assert seen_skip[0] == seen_skip[1] == set(range(13)) and seen_dc == set(range(3)) and seen_dir == set(range(13))
    assert mags["last"] >= set(cr.MAGNITUDES) and mags["mid"] >= set(cr.MAGNITUDES)
    assert mags["dc"] >= set(cr.MAGNITUDES) | {-m for m in cr.MAGNITUDES} | {0}  # both signs of the DC
    assert beyond > 100  # blocks with coefficients behind eob: the levels array takes the whole block
    stats = restated[1]
    base, base_eob, lps = set(), set(), set()
    nonzero = golomb = 0
    for ts, s in enumerate(stats):
        assert s["short_loop"], ts  # a case with c_start < eob - 2 for every size
        base |= s["base"]
        base_eob |= s["base_eob"]
        lps |= s["lps"]
        nonzero += s["nonzero"]
        golomb += s["golomb"]
    # base_cost has SIG_COEF_CONTEXTS = 42 rows, but the reference can index only 41 of them: the largest context of
    # get_nz_map_ctx_from_stats is AOMMIN((stats + 1) >> 1, 4) + nz_map_ctx_offset_1d's top value 36 = 40 (the 2-D contexts end at 21 + 4 = 25,
    # the 1-D ones take 26 .. 40), so row 41 is dead in the reference itself.  Every row it can read is read:
    assert base == set(range(41)) and base_eob == set(range(4)) and lps == set(range(21))
    assert golomb >= 0.05 * nonzero, (golomb, nonzero)


def test_dense_blocks_saturate_the_context_sums(cases):
    """in a dense block every neighbour is >= 3: get_nz_mag reaches its top (context offset + 4) and get_br_ctx's sum its cap of 6"""
    c = next(c for c in cases if c["tx_size"] == 2 and c["plane"] == 0 and c["reduced"] == 0)
    dense = [k for k in range(len(c["eob"])) if c["eob"][k] == 256 and np.count_nonzero(np.abs(c["qcoeff"][k]) >= 3) > 250]
    assert dense
    for k in dense:
        cls = cr.tx_class(int(c["jobs"][k]["tx_type"]))
        ctx, br, _ = cr.block_contexts(c["qcoeff"][k], 2, cls)
        assert ctx.reshape(16, 16)[5, 5] == (25 if cls == 0 else 40) and br.max() == 20


def test_short_cuts_and_frame():
    z = np.load(cr.GOLDEN)
    T = cr.Tables.from_golden(z, 0)
    assert [cr.shortcut_threshold(ts) for ts in (0, 1, 2, 3, 4, 11, 17)] == [0, 1, 4, 16, 64, 32, 16]
    skip1 = int(T.coeff_costs(4, 0)["txb_skip_cost"][5][1])
    for lvl, eob, want in ((0, 63, 6000 + 63000), (0, 64, 3000 + 6400), (2, 63, 6000 + 63000), (2, 64, 777 << 2), (1, 3, 777 << 2), (1, 0, skip1), (2, 0, 6000)):
        assert cr.frame_bits(T, 4, 0, 777, eob, 5, lvl, 2) == want, (lvl, eob)
    assert cr.frame_bits(T, 0, 0, 777, 0, 5, 0, 0) == 3000  # TX_4X4: th = 0, no short-cut below it
    assert cr.frame_bits(T, 4, 1, 777, 3, 5, 0, 2) == 777  # chroma: no short-cut, no shift
    assert cr.frame_bits(T, 4, 0, None, 70, 5, 1, 0) == cr.UNDEFINED
    assert cr.rdcost(1, 511, 0) == 1 and cr.rdcost(1, 255, 3) == 384 and cr.rdcost(1 << 31, 1000, 1 << 40) == ((1000 << 31) + 256 >> 9) + (1 << 47)
    assert cr.rdcost(5, cr.UNDEFINED, 7) == cr.UNDEFINED
    jobs, best = cr.group_winners(np.array([5, 3, 3, cr.UNDEFINED, cr.UNDEFINED, 9], np.uint64), [0, 3, 5, 6, 6])
    assert jobs.tolist() == [1, cr.NO_JOB, 5, cr.NO_JOB] and best.tolist() == [3, cr.UNDEFINED, 9, cr.UNDEFINED]


def test_the_module_and_its_entries_are_exported():
    from svt_av1_psyex_amd import rate
    assert callable(rate.upload_tables) and callable(rate.run_rate_hip) and callable(rate.run_rate_device)
    L = api.lib()
    for name in ("svt_hip_coeff_rate_batch", "svt_hip_coeff_rate_desc_size", "svt_hip_rate_tables_size"):
        assert hasattr(L, name), name


def test_struct_sizes_match_ctypes():
    L = api.lib()
    L.svt_hip_coeff_rate_desc_size.restype = C.c_size_t
    L.svt_hip_rate_tables_size.restype = C.c_size_t
    assert L.svt_hip_coeff_rate_desc_size() == C.sizeof(abi.CoeffRateDesc)
    assert L.svt_hip_rate_tables_size() == C.sizeof(abi.RateTables) == 4 * sum(int(np.prod(s)) for _, s in abi.RATE_TABLE_SHAPES)
    assert C.sizeof(abi.RateJob) == 8 == np.dtype(abi.RATE_JOB_DTYPE).itemsize == np.dtype(cr.RATE_JOB_DTYPE).itemsize
    assert C.sizeof(abi.LvMapCoeffCost) == 4 * cr.COEFF_COST_INTS
    for name, (first, shape) in cr.COEFF_MEMBERS.items():
        assert getattr(abi.LvMapCoeffCost, name).offset == 4 * first and getattr(abi.LvMapCoeffCost, name).size == 4 * int(np.prod(shape)), name


# (null arguments: tests/test_batch_entries.py)
BAD = ["tx_size_19", "tx_size_255", "plane_type_2", "subres_3", "fast_0", "no_jobs", "no_tables", "no_qcoeff", "no_eob", "no_bits",
       "unaligned_qcoeff", "rd_cost_without_dist", "groups_without_rd_cost", "group_count_without_rd_cost", "groups_without_group_start", "groups_without_best_job",
       "groups_without_best_cost"]


@pytest.mark.parametrize("bad", BAD)
def test_bad_descriptor_is_rejected_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_coeff_rate_desc(n_groups=0)
    p = C.c_void_p(0x1000)
    if bad.startswith("tx_size"):
        d.tx_size = int(bad.split("_")[-1])
    elif bad == "plane_type_2":
        d.plane_type = 2
    elif bad == "subres_3":
        d.mds_subres_step = 3
    elif bad == "fast_0":
        d.mds_fast_coeff_est_level = 0
    elif bad.startswith("no_"):
        setattr(d, bad[3:], None)
    elif bad == "unaligned_qcoeff":
        d.qcoeff = 0x1004
    elif bad == "rd_cost_without_dist":
        d.rd_cost, d.lambda_ = p, 100
    else:
        d.group_start, d.best_job, d.best_cost, d.n_groups = p, p, p, 2
        if bad == "groups_without_rd_cost":
            pass
        elif bad == "group_count_without_rd_cost":
            d.group_start = d.best_job = d.best_cost = None
        else:
            d.rd_cost, d.dist = p, p
            setattr(d, bad[len("groups_without_"):], None)
    assert L.svt_hip_coeff_rate_batch(ctx, C.byref(d)) == BAD_PARAM
    assert b"svt_hip_coeff_rate_batch" in L.svt_hip_last_error(None)
