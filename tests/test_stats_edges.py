"""CPU: the inputs of the block-statistics edge tests (tests/stats_edge_cases.py) cover what they are meant to cover, and on them
oracle/stats_oracle.c agrees with the committed fixture (tests/golden/block_stats_edges.npz: the reference's `_c` outputs, from
oracle/gen_golden.py block_stats_edges) and, in the build container, with the reference itself."""
import ctypes as C

import numpy as np
import pyoracle
import pytest

import stats_edge_cases as ec
from svt_av1_psyex_amd import abi, stats


@pytest.mark.parametrize("av1_only", [True, False])
def test_packed_list_covers_every_mixed_wave(oracle, av1_only):
    src, ref, jobs, kinds = ec.standard_packed(av1_only)
    assert len(jobs) >= ec.PACKED_N_MIN and len(jobs) % 4 != 0
    satd = pyoracle.block_stats(oracle, src, ref, jobs, 8)["satd"]
    c = ec.assert_packed_coverage(jobs, kinds, satd)
    print(len(jobs), "jobs:", c)
    odd = np.isin(jobs["width"], [12, 3, 1])
    assert odd.any() != av1_only
    sub = (jobs["subpel_x"] != 0) | (jobs["subpel_y"] != 0)
    assert {(int(j["subpel_x"]) != 0, int(j["subpel_y"]) != 0) for j in jobs[sub]} == {(True, False), (False, True), (True, True)}
    # every job stays inside its plane (a sub-pel view reads one more source row and column)
    x0, y0 = jobs["src_offset"] % ec.W, jobs["src_offset"] // ec.W
    x1, y1 = jobs["ref_offset"] % ec.REF_STRIDE, jobs["ref_offset"] // ec.REF_STRIDE
    assert (x0 + jobs["width"] + sub <= ec.W).all() and (y0 + jobs["height"] + sub <= ec.H).all()
    assert (x1 + jobs["width"] <= ec.REF_STRIDE).all() and (y1 + jobs["height"] <= ec.H).all()


def test_packed_list_grows_by_whole_groups():
    _, _, jobs, kinds = ec.standard_packed(True)
    _, _, more, more_kinds = ec.standard_packed(True, ec.PACKED_N_MIN + 1024)
    n = 4 * len(kinds)
    assert len(more_kinds) == len(kinds) + 256 and np.array_equal(more[:n], jobs[:n]) and np.array_equal(more_kinds[:len(kinds)], kinds)


def test_walsh_planes_put_the_block_into_one_coefficient(oracle):
    """every (u, v, sign) at 8, 16 and 32: the SATD constants, by the oracle's hadamard_path"""
    oracle.orc_hadamard_path.restype = C.c_uint32
    P = C.c_void_p
    for n in (8, 16, 32):
        for u in range(8):
            for v in range(8):
                for sign in (1, -1):
                    a, b = ec.walsh_planes(n, u, v, sign)
                    assert set(np.unique(a.astype(int) - b)) <= {sign * 255, -sign * 255} and int(a[0, 0]) - int(b[0, 0]) == sign * 255
                    assert oracle.orc_hadamard_path(a.ctypes.data_as(P), C.c_uint32(n), b.ctypes.data_as(P), C.c_uint32(n), C.c_uint32(n)) == ec.WALSH_SATD[n], (n, u, v, sign)
    a, b = ec.walsh_mixed16([(1, 2, 1), (7, 7, -1), (0, 0, -1), (5, 3, 1)])
    assert oracle.orc_hadamard_path(a.ctypes.data_as(P), C.c_uint32(16), b.ctypes.data_as(P), C.c_uint32(16), C.c_uint32(16)) == ec.WALSH_MIXED16_SATD


def test_walsh_atlas_holds_the_walsh_planes():
    src, ref = ec.walsh_atlas()
    for s, sign in enumerate((1, -1)):
        for u, v in ((0, 0), (3, 5), (7, 7)):
            a, b = ec.walsh_planes(32, u, v, sign)
            y, x = 256 * s + 32 * u, 32 * v
            assert np.array_equal(src[y:y + 32, x:x + 32], a) and np.array_equal(ref[y:y + 32, ec.WALSH_REF_X0 + x:ec.WALSH_REF_X0 + x + 32], b)
    jobs, satd = ec.walsh_jobs()
    assert len(jobs) == 2 * 64 * 21 + 15 * 7 and (satd > 0).all()
    assert (ec.walsh_region_satd(2)[[0, 1, 5, 21, 85]] == [130560, 32640, 32640, 16320, 130560]).all()


@pytest.mark.parametrize("name", ["walsh", "max8", "max10", "split10", "packed"])
def test_oracle_matches_edge_fixture(oracle, name):
    bd, src, ref, jobs, val, ok = ec.load_fixture(name)
    got = ec.oracle_outputs(oracle, src, ref, jobs, bd)
    assert not ec.disagreements(val, ok, got)
    assert sum(int(m.sum()) for m in ok.values()) >= 5 * len(jobs)  # the fixture says something about every job
    if name == "walsh":
        assert np.array_equal(val["satd"], ec.walsh_jobs()[1]) and ok["satd"].all()
    if name == "max10":
        big = jobs["width"].astype(int) * jobs["height"] == 128 * 128
        assert (val["sse"][big] > 1 << 32).all() and (val["sse"][big] != val["var_sse"][big]).all()
        assert (val["var_sse"] == (val["sse"] & 0xFFFFFFFF)).all()
    if name == "split10":  # the sum of the 128x128 block is 0: its variance is the wrapped var_sse
        assert (int(val["sse"][0]), int(val["var_sse"][0]), int(val["variance"][0])) == (17146331136, 4261429248, 4261429248)
        assert int(val["variance10"][0]) == int(val["var_sse10"][0]) == 1071645696


def test_oracle_matches_reference_on_edge_sets(ref, oracle):
    """SAD, SSE, variance, the highbd_10 variance, hadamard_path and svt_psy_distortion{,_hbd} of the reference itself on every fixture set
    (the packed list in full, with the shapes that are no AV1 block sizes), on single Walsh planes and on the psy patterns"""
    sets = dict(ec.fixture_sets())
    for av1_only in (True, False):
        src, refp, jobs, _ = ec.standard_packed(av1_only)
        sets[f"packed_full_{av1_only}"] = (8, src, refp, jobs)
    for bd in (8, 10):
        for pat in ec.PSY_PATTERNS:
            sets[f"psy_{pat}{bd}"] = (bd,) + ec.psy_planes(bd, pat) + (ec.psy_jobs(),)
    one = lambda n: np.array([(0, 0, n, n, 0, 0)], dtype=abi.BLOCK_JOB_DTYPE)
    for n, u, v, sign in ((8, 1, 6, 1), (16, 7, 7, -1), (32, 4, 2, 1)):
        sets[f"walsh_{n}_{u}_{v}_{sign}"] = (8,) + ec.walsh_planes(n, u, v, sign) + (one(n),)
    sets["walsh_mixed16"] = (8,) + ec.walsh_mixed16([(1, 2, 1), (7, 7, -1), (0, 0, -1), (5, 3, 1)]) + (one(16),)
    for name, (bd, src, refp, jobs) in sets.items():
        val, ok = ec.reference_outputs(ref, src, refp, jobs, bd)
        assert not ec.disagreements(val, ok, ec.oracle_outputs(oracle, src, refp, jobs, bd)), name


def test_region_expansion_takes_two_strides():
    r = np.array([(5 * 320 + 7, 9 * 352 + 11, 64, 64, 0, 0)], dtype=abi.BLOCK_JOB_DTYPE)[0]
    e = stats.expand_pyramid(r, 320, 352)
    assert len(e) == abi.PYRAMID_BLOCKS and tuple(e[0]) == tuple(r)
    assert (int(e[84]["src_offset"]), int(e[84]["ref_offset"])) == ((5 + 56) * 320 + 7 + 56, (9 + 56) * 352 + 11 + 56)
