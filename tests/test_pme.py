"""The mode-decision full-pel refinement search: svt_pme_sad_loop_kernel = SAD + MV-rate cost over a (sparse) search area
(Codec/product_coding_loop.c:1905-1950).  CPU: the oracle against the reference's own svt_pme_sad_loop_kernel_c (oracle/_ref), grid after
test/SadTest.cc:1580-1640.  GPU: svt_hip_pme_sad_batch and the pointer-level svt_pme_sad_loop_kernel_hip against the oracle.
The edge sets (pme_cases.edge_sets: widths that are no multiple of 8, empty searches, item counts around the wave size, ties between lanes,
between one lane's iterations and with the incoming best, source and reference planes of different widths) are pinned on the reference's
own results in golden/pme_edges.npz, on the CPU (oracle) and on the device (batch and pointer-level entry)."""
import ctypes as C

import numpy as np
import pytest

import pme_cases as pc
from pme_cases import MV_CENTRE, cost_tables, random_jobs, run_hip, run_oracle, run_ref
from svt_av1_psyex_amd import abi, api

W, H = 448, 320


def planes(rng, kind):
    if kind == "extremes":
        return np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    b = np.clip(np.roll(a, (3, -5), (0, 1)).astype(np.int32) + rng.integers(-12, 13, (H, W)), 0, 255).astype(np.uint8)
    return a, b


@pytest.mark.parametrize("cost_type", [0, 1, 2, 3, 4, 5])
def test_oracle_matches_reference(oracle, ref, cost_type):
    rng = np.random.default_rng(100 + cost_type)
    tables = cost_tables(rng)
    for kind in ("noise", "extremes"):
        src, rp = planes(rng, kind)
        for wild in (False, True):
            jobs = random_jobs(rng, W, H, 60, wild=wild)
            epb = 20542 if wild else int(rng.integers(1, 60000))
            a = run_ref(ref, src, rp, jobs, cost_type, epb, tables)
            b = run_oracle(oracle, src, rp, jobs, cost_type, epb, tables)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (kind, wild)


def test_struct_layouts(oracle):
    oracle.orc_sizeof_pme.restype = C.c_size_t
    assert oracle.orc_sizeof_pme(0) == abi.PME_JOB_DTYPE.itemsize
    assert oracle.orc_sizeof_pme(1) == C.sizeof(abi.PmeBatchDesc)
    assert oracle.orc_sizeof_pme(2) == C.sizeof(abi.MvCostParam)


def test_mv_cost_param_layout_is_the_references(oracle, ref):
    """SvtHipMvCostParam == MV_COST_PARAMS field by field: offsets, size, and the ONE-byte mv_cost_type (UENUM1BYTE); ctypes mirror too"""
    a, b = (C.c_size_t * 9)(), (C.c_size_t * 9)()
    ref.ref_mv_cost_param_layout(a)
    oracle.orc_mv_cost_param_layout(b)
    assert list(a) == list(b)
    assert a[3] >> 16 == 1
    m = abi.MvCostParam
    assert [C.sizeof(m), m.ref_mv.offset, m.full_ref_mv.offset, m.mv_cost_type.offset | (m.mv_cost_type.size << 16), m.mvjcost.offset, m.mvcost.offset,
            m.error_per_bit.offset, m.early_exit_th.offset, m.sad_per_bit.offset] == list(a)


@pytest.mark.parametrize("cost_type", [0, 1, 3, 4, 5])
def test_garbage_padding_after_mv_cost_type(oracle, ref, cost_type):
    """md_full_pel_search builds MV_COST_PARAMS on its stack field by field (product_coding_loop.c:2030-2049): the three padding bytes behind
    the one-byte mv_cost_type are garbage.  The oracle must read the type exactly as the reference does."""
    rng = np.random.default_rng(300 + cost_type)
    tables = cost_tables(rng)
    src, rp = planes(rng, "noise")
    jobs = random_jobs(rng, W, H, 40)
    a = run_ref(ref, src, rp, jobs, cost_type, 20542, tables)
    b = run_ref(ref, src, rp, jobs, cost_type, 20542, tables, garbage=0xFF)
    c = run_ref(oracle, src, rp, jobs, cost_type, 20542, tables, garbage=0x5A, fn="orc_pme_sad_loop_kernel")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


@pytest.mark.gpu
@pytest.mark.parametrize("cost_type", [0, 1, 2, 3, 4, 5])
def test_hip_batch_matches_oracle(hip_ctx, oracle, cost_type):
    rng = np.random.default_rng(200 + cost_type)
    tables = cost_tables(rng)
    for kind in ("noise", "extremes"):
        src, rp = planes(rng, kind)
        for wild in (False, True):
            jobs = random_jobs(rng, W, H, 400, wild=wild)
            epb = int(rng.integers(1, 60000))
            a = run_oracle(oracle, src, rp, jobs, cost_type, epb, tables)
            b = run_hip(hip_ctx, src, rp, jobs, cost_type, epb, tables)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (kind, wild)


@pytest.mark.gpu
def test_leaf_pme_sad_loop_kernel(hip_ctx, oracle):
    """svt_pme_sad_loop_kernel_hip with the reference's prototype and its MV_COST_PARAMS struct"""
    L = api.lib()
    assert L.svt_hip_leaf_bind(hip_ctx._h) == 0
    try:
        rng = np.random.default_rng(7)
        jc, tr, tc = cost_tables(rng)
        src, rp = planes(rng, "noise")
        jobs = random_jobs(rng, W, H, 24)
        want = run_oracle(oracle, src, rp, jobs, 0, 20542, (jc, tr, tc))
        for i, j in enumerate(jobs):
            rmv = abi.Mv(int(j["ref_mv"][0]), int(j["ref_mv"][1]))
            p = abi.MvCostParam()
            C.memset(C.byref(p), 0xA5, C.sizeof(p))  # the caller's stack garbage, padding bytes included
            p.ref_mv, p.mv_cost_type, p.mvjcost, p.error_per_bit = C.pointer(rmv), 0, jc.ctypes.data, 20542
            p.mvcost[0], p.mvcost[1] = tr.ctypes.data + 4 * MV_CENTRE, tc.ctypes.data + 4 * MV_CENTRE
            bc, bx, by = C.c_uint32(int(j["best_cost"])), C.c_int16(int(j["best_mvx"])), C.c_int16(int(j["best_mvy"]))
            L.svt_pme_sad_loop_kernel_hip(C.byref(p), C.c_void_p(src.ctypes.data + int(j["src_offset"])), C.c_uint32(W), C.c_void_p(rp.ctypes.data + int(j["ref_offset"])),
                                          C.c_uint32(W), C.c_uint32(int(j["height"])), C.c_uint32(int(j["width"])), C.byref(bc), C.byref(bx), C.byref(by),
                                          C.c_int16(int(j["start_x"])), C.c_int16(int(j["start_y"])), C.c_int16(int(j["sa_w"])), C.c_int16(int(j["sa_h"])),
                                          C.c_int16(int(j["step"])), C.c_int16(int(j["mvx"])), C.c_int16(int(j["mvy"])))
            assert (bc.value, bx.value, by.value) == (int(want[0][i]), int(want[1][i][0]), int(want[1][i][1])), i
    finally:
        L.svt_hip_leaf_bind(None)


# ---- the edge sets ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_sets():
    return pc.edge_sets()


@pytest.fixture(scope="module")
def edge_golden():
    return np.load(pc.GOLDEN_EDGES)


def _same(got, golden, name, cost_type):
    bad = np.nonzero((got[0] != golden[name + "_cost"][cost_type]) | (got[1] != golden[name + "_mv"][cost_type]).any(axis=1))[0]
    assert not len(bad), (name, cost_type, bad[:8].tolist(), got[0][bad[:8]].tolist(), golden[name + "_cost"][cost_type][bad[:8]].tolist())


def test_edge_inputs_are_the_fixtures(edge_sets, edge_golden):
    import zlib
    for name, (src, rp, jobs, tables) in edge_sets.items():
        assert zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in (src, rp, jobs) + tuple(tables))) == int(edge_golden[name + "_crc"]), name
        assert src.shape[1] != rp.shape[1]


@pytest.mark.parametrize("cost_type", [0, 1, 2, 3, 4, 5])
def test_oracle_matches_reference_and_fixture_on_the_edge_sets(oracle, ref, edge_sets, edge_golden, cost_type):
    for name, (src, rp, jobs, tables) in edge_sets.items():
        _same(run_ref(ref, src, rp, jobs, cost_type, pc.EDGE_EPB, tables), edge_golden, name, cost_type)
        _same(run_oracle(oracle, src, rp, jobs, cost_type, pc.EDGE_EPB, tables), edge_golden, name, cost_type)


def test_edge_sets_cover_what_they_are_for(edge_sets, edge_golden):
    """From a plain walk of the reference's visiting order, under a cost without an MV rate (cost = SAD; cost types 5 and 2)."""
    jobs = np.concatenate([s[2] for s in edge_sets.values()])
    grid = edge_sets["grid"][2]
    for step in pc.EDGE_STEPS:
        g = grid[grid["step"] == step]
        assert {1, 7, 8, 9, 15, 16, 17, 7 + 7 + step, 8 + 7 + step, 7 + 2 * (7 + step), 8 + 2 * (7 + step)} <= set(g["sa_w"].tolist())
        for sa_w in set(g["sa_w"].tolist()):
            assert {1, step, step + 1, 2 * step + 1} <= set(g[g["sa_w"] == sa_w]["sa_h"].tolist())
    census = [c for (src, rp, jb, _) in edge_sets.values() for c in pc.tie_census(src, rp, jb)]
    quads = sorted({(n + 3) // 4 for n, _, _ in census})
    assert {0, 2, 62, 64, 66, 126, 128, 130, 258, 1000} <= set(quads), quads  # a quad count is even: 2 x (1, 31, 32, 33, 63, 64, 65, 129, 500) groups
    assert sum(len(q) >= 2 for _, q, _ in census) >= 30                      # minima held by different lanes
    assert sum(len(q) >= 2 and q[-1] - q[0] >= 64 for _, q, _ in census) >= 10  # ... by different passes of the 64 lanes
    assert sum(any((b - a) % 64 == 0 for a in q for b in q if b > a) for _, q, _ in census) >= 10  # ... by one lane in two passes
    assert sum(tie for _, _, tie in census) >= 10                              # the incoming best equals the minimum: it must stay
    narrow = jobs["sa_w"] < 8
    assert narrow.sum() >= 30 and all(n == 0 for (n, _, _), nar in zip(census, narrow) if nar) and all(n > 0 for (n, _, _), nar in zip(census, narrow) if not nar)
    for ct in (2, 5):  # where nothing is visited, and where the incoming best ties, what came in goes out
        cost = np.concatenate([edge_golden[k + "_cost"][ct] for k in edge_sets])
        mv = np.concatenate([edge_golden[k + "_mv"][ct] for k in edge_sets])
        keep = np.array([n == 0 or tie for n, _, tie in census])
        assert np.array_equal(cost[keep], jobs["best_cost"][keep]) and np.array_equal(mv[keep], np.stack([jobs["best_mvx"], jobs["best_mvy"]], axis=1)[keep])
    src, rp, jb, _ = edge_sets["grid"]
    cols, rows = pc.read_extent(jb[0])
    assert int(jb[0]["ref_offset"]) + (rows - 1) * rp.shape[1] + cols == rp.size  # this window ends at the reference plane's last sample


@pytest.mark.gpu
@pytest.mark.parametrize("cost_type", [0, 1, 2, 3, 4, 5])
def test_hip_batch_matches_oracle_and_fixture_on_the_edge_sets(hip_ctx, oracle, edge_sets, edge_golden, cost_type):
    for name, (src, rp, jobs, tables) in edge_sets.items():
        got = run_hip(hip_ctx, src, rp, jobs, cost_type, pc.EDGE_EPB, tables, fill=0xA5, spare_jobs=9)
        _same(got, edge_golden, name, cost_type)
        _same(run_oracle(oracle, src, rp, jobs, cost_type, pc.EDGE_EPB, tables), edge_golden, name, cost_type)


@pytest.mark.gpu
def test_hip_batch_of_one_job_and_of_none(hip_ctx, edge_sets, edge_golden):
    """the first grid job alone: its window ends at the reference plane's last sample, and the device plane is REF_SLACK bytes longer"""
    src, rp, jobs, tables = edge_sets["grid"]
    for i in (0, len(jobs) - 1):
        cost, mv = run_hip(hip_ctx, src, rp, jobs[i:i + 1], 0, pc.EDGE_EPB, tables, fill=0xA5, spare_jobs=5)
        assert cost[0] == edge_golden["grid_cost"][0][i] and np.array_equal(mv[0], edge_golden["grid_mv"][0][i])
    cost, mv = run_hip(hip_ctx, src, rp, jobs[:0], 0, pc.EDGE_EPB, tables, fill=0xA5, spare_jobs=5)  # asserts the five slots untouched
    assert len(cost) == 0 and len(mv) == 0


@pytest.mark.gpu
def test_leaf_pme_sad_loop_kernel_on_the_edge_sets(hip_ctx, edge_sets, edge_golden):
    """the pointer-level entry with different strides, on host arrays that end with the last sample the reference reads: empty searches
    (the incoming best comes back), widths that are no multiple of 8, ties"""
    L = api.lib()
    assert L.svt_hip_leaf_bind(hip_ctx._h) == 0
    try:
        L.svt_hip_leaf_status(None, None, None, C.c_size_t(0))
        n_empty = n_odd = 0
        for name, pick, cost_type in (("grid", slice(0, None, 8), 0), ("grid", slice(3, None, 16), 4), ("ties", slice(0, None, 12), 5), ("flat", slice(0, None, 12), 1), ("extremes", slice(0, 2), 3)):
            src, rp, jobs, (jc, tr, tc) = edge_sets[name]
            fs, fr = src.reshape(-1), rp.reshape(-1)
            for i in range(len(jobs))[pick]:
                j = jobs[i]
                cols, rows = pc.read_extent(j)
                n_empty, n_odd = n_empty + (rows == 0), n_odd + (rows > 0 and j["sa_w"] % 8 != 0)
                s = fs[int(j["src_offset"]):int(j["src_offset"]) + (int(j["height"]) - 1) * src.shape[1] + int(j["width"])].copy()
                r = fr[int(j["ref_offset"]):int(j["ref_offset"]) + max(rows - 1, 0) * rp.shape[1] + max(cols, 1)].copy()
                rmv = abi.Mv(int(j["ref_mv"][0]), int(j["ref_mv"][1]))
                p = abi.MvCostParam()
                C.memset(C.byref(p), 0xA5, C.sizeof(p))
                p.ref_mv, p.mv_cost_type, p.mvjcost, p.error_per_bit = C.pointer(rmv), cost_type, jc.ctypes.data, pc.EDGE_EPB
                p.mvcost[0], p.mvcost[1] = tr.ctypes.data + 4 * MV_CENTRE, tc.ctypes.data + 4 * MV_CENTRE
                bc, bx, by = C.c_uint32(int(j["best_cost"])), C.c_int16(int(j["best_mvx"])), C.c_int16(int(j["best_mvy"]))
                L.svt_pme_sad_loop_kernel_hip(C.byref(p), C.c_void_p(s.ctypes.data), C.c_uint32(src.shape[1]), C.c_void_p(r.ctypes.data), C.c_uint32(rp.shape[1]),
                                              C.c_uint32(int(j["height"])), C.c_uint32(int(j["width"])), C.byref(bc), C.byref(bx), C.byref(by),
                                              C.c_int16(int(j["start_x"])), C.c_int16(int(j["start_y"])), C.c_int16(int(j["sa_w"])), C.c_int16(int(j["sa_h"])),
                                              C.c_int16(int(j["step"])), C.c_int16(int(j["mvx"])), C.c_int16(int(j["mvy"])))
                want = edge_golden[name + "_cost"][cost_type][i], edge_golden[name + "_mv"][cost_type][i]
                assert (bc.value, bx.value, by.value) == (int(want[0]), int(want[1][0]), int(want[1][1])), (name, i)
        assert n_empty >= 4 and n_odd >= 8
        assert L.svt_hip_leaf_status(None, None, None, C.c_size_t(0)) == 0  # nothing fell back
    finally:
        L.svt_hip_leaf_bind(None)
