"""GPU: svt_hip_ssim_batch and the SSIM leaves off the grids they were written on (tests/ssim_cases.py: edge_case) -- source and reference
planes of different widths with the block at unrelated places of the two, the smallest sizes that separate the kernel's paths, a psy
strength that fills the high half of the distortion, output slots pre-filled and guarded, explicit pyramid_out_base, single outputs, and the
jobs the host check refuses met by the kernel itself.  Every comparison is exact, against the reference's own results
(golden/ssim_edges.npz) and the restatement."""
import ctypes as C

import numpy as np
import pytest

import ssim_cases as sc
from svt_av1_psyex_amd import abi, api, stats

pytestmark = pytest.mark.gpu

FILL = 0xA5
BAD = {"ssim": np.float64(-1.0), "ssim_dist": np.uint64(0xFFFFFFFFFFFFFFFF)}


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN_EDGES)


def same(got, want_ssim, want_dist, what):
    assert np.array_equal(sc.bits(got["ssim"]), sc.bits(want_ssim)), what
    bad = np.nonzero(got["ssim_dist"] != want_dist)[0]
    assert not len(bad), (what, bad[:5].tolist(), got["ssim_dist"][bad[:5]].tolist(), np.asarray(want_dist)[bad[:5]].tolist())


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


@pytest.mark.parametrize("bd", [8, 10])
def test_batch_equals_the_fixture_and_the_restatement(hip_ctx, golden, oracle, bd):
    e = sc.edge_expected(oracle, bd)
    n = len(e["jobs"])
    for k, psy in enumerate(sc.EDGE_PSY_RDS):
        got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["jobs"], bd, psy_rd=psy, fill=FILL, spare_jobs=9)
        same(got, e["ssim"][:n], golden[f"dist{bd}"][k][:n], (bd, psy, "fixture"))
        same(got, e["ssim"][:n], e["dist"][psy][:n], (bd, psy, "restatement"))
    flat = (e["src"].reshape(-1), e["src"].shape[1]), (e["ref"].reshape(-1), e["ref"].shape[1])  # the same planes as (array, stride) views
    same(stats.run_ssim_hip(hip_ctx, flat[0], flat[1], e["jobs"], bd, psy_rd=1.0, fill=FILL, spare_jobs=1), e["ssim"][:n], e["dist"][1.0][:n], (bd, "views"))


@pytest.mark.parametrize("bd", [8, 10])
def test_pyramids_on_unequal_strides_equal_their_plain_jobs(hip_ctx, golden, oracle, bd):
    e = sc.edge_expected(oracle, bd)
    n = len(e["jobs"])
    none = e["jobs"][:0]
    for psy in (0.0, 1.0, sc.PSY_LARGE):
        k = sc.EDGE_PSY_RDS.index(psy)
        pyr = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], none, bd, psy_rd=psy, pyramids=e["regions"], fill=FILL, spare_jobs=9)
        plain = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["every"][n:], bd, psy_rd=psy, fill=FILL, spare_jobs=9)
        same(pyr, plain["ssim"], plain["ssim_dist"], (bd, psy, "plain jobs"))
        same(pyr, e["ssim"][n:], golden[f"dist{bd}"][k][n:], (bd, psy, "fixture"))
        same(pyr, e["ssim"][n:], e["dist"][psy][n:], (bd, psy, "restatement"))


@pytest.mark.parametrize("bd", [8, 10])
def test_slots_between_the_plain_jobs_and_pyramid_out_base_keep_the_fill(hip_ctx, oracle, bd):
    e = sc.edge_expected(oracle, bd)
    n, m = len(e["jobs"]), 6
    got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["jobs"][:m], bd, psy_rd=1.0, pyramids=e["regions"], out_base=m + 7, fill=FILL, spare_jobs=9)
    assert len(got["ssim"]) == m + 7 + 85 * len(e["regions"])
    for name in got:
        assert untouched(got[name][m:m + 7]), name
    same({k: v[:m] for k, v in got.items()}, e["ssim"][:m], e["dist"][1.0][:m], (bd, "plain"))
    same({k: v[m + 7:] for k, v in got.items()}, e["ssim"][n:], e["dist"][1.0][n:], (bd, "regions"))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("outputs,psy", [(("ssim",), 0.0), (("ssim_dist",), 0.4), (("ssim_dist",), sc.PSY_LARGE), (("ssim",), 1.0)])
def test_one_output_alone(hip_ctx, oracle, bd, outputs, psy):
    """ssim alone with psy_rd > 0: the psy term has no output to go to and its loop is skipped"""
    e = sc.edge_expected(oracle, bd)
    n = len(e["jobs"])
    got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["jobs"], bd, psy_rd=psy, pyramids=e["regions"], outputs=outputs, fill=FILL, spare_jobs=9)
    if outputs == ("ssim",):
        assert np.array_equal(sc.bits(got["ssim"]), sc.bits(e["ssim"])) and untouched(got["ssim_dist"])
    else:
        assert np.array_equal(got["ssim_dist"], e["dist"][psy]) and untouched(got["ssim"])


@pytest.mark.parametrize("bd", [8, 10])
def test_jobs_the_host_check_refuses_are_marked_by_the_kernel(hip_ctx, oracle, bd):
    """svt_hip_ssim_batch without svt_hip_ssim_check_jobs in front: an undefined job gives ssim = -1 and ssim_dist = 2^64 - 1 (a region: all
    85 of its slots), its neighbours are exact.  The undefined jobs keep in-plane offsets."""
    e = sc.edge_expected(oracle, bd)
    good = e["jobs"]
    n = len(good)
    shapes = [(0, 8, 0, 0), (8, 0, 0, 0), (2, 8, 0, 0), (8, 2, 0, 0), (6, 8, 0, 0), (8, 6, 0, 0), (132, 8, 0, 0), (8, 132, 0, 0), (132, 132, 0, 0), (0, 0, 0, 0),
              (8, 8, 1, 0), (8, 8, 0, 3), (64, 64, 7, 7), (4, 4, 0, 1), (255, 255, 0, 0)]
    jobs, is_bad, k = [], [], 0
    for i, (w, h, fx, fy) in enumerate(shapes):
        for _ in range(1 + i % 3):  # one to three good jobs between two bad ones
            jobs.append(tuple(good[k % n]))
            is_bad.append(False)
            k += 5
        jobs.append((int(good[i]["src_offset"]), int(good[i]["ref_offset"]), w, h, fx, fy))
        is_bad.append(True)
    jobs, is_bad = np.array(jobs, dtype=abi.BLOCK_JOB_DTYPE), np.array(is_bad)
    with pytest.raises(api.SvtHipError):
        stats.check_ssim_jobs(jobs)
    regions = np.concatenate([e["regions"][:1], e["regions"][1:2], e["regions"][1:2], e["regions"][2:3], e["regions"][:1]])
    regions[1]["width"] = regions[1]["height"] = 32
    regions[3]["subpel_x"] = 2
    bad_region = np.array([False, True, False, True, False])
    for r in regions[bad_region]:
        with pytest.raises(api.SvtHipError):
            stats.check_ssim_jobs(np.array([r]), pyramids=True)
    src_of = np.array([0, 1, 1, 2, 0])  # which of the case's regions each slot group restates
    for psy in (0.0, 1.0):
        got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], jobs, bd, psy_rd=psy, pyramids=regions, check=False, fill=FILL, spare_jobs=9)
        want = {"ssim": np.zeros(len(got["ssim"]), np.float64), "ssim_dist": np.zeros(len(got["ssim"]), np.uint64)}
        idx = np.zeros(len(jobs), np.int64)
        idx[~is_bad] = (5 * np.arange((~is_bad).sum())) % n  # the good jobs, in the order they were taken
        for name, full in (("ssim", e["ssim"]), ("ssim_dist", e["dist"][psy])):
            want[name][:len(jobs)] = np.where(is_bad, BAD[name], full[idx])
            for g in range(len(regions)):
                lo = len(jobs) + 85 * g
                want[name][lo:lo + 85] = BAD[name] if bad_region[g] else full[n + 85 * src_of[g]:n + 85 * src_of[g] + 85]
        same(got, want["ssim"], want["ssim_dist"], (bd, psy))
        assert (got["ssim"] == -1.0).sum() == is_bad.sum() + 85 * bad_region.sum()


@pytest.mark.parametrize("bd", [8, 10])
def test_one_job_one_region_and_an_empty_batch(hip_ctx, oracle, bd):
    e = sc.edge_expected(oracle, bd)
    n = len(e["jobs"])
    for i in (0, 13, n - 1):
        got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["jobs"][i:i + 1], bd, psy_rd=sc.PSY_LARGE, fill=FILL, spare_jobs=5)
        same(got, e["ssim"][i:i + 1], e["dist"][sc.PSY_LARGE][i:i + 1], (bd, i))
    for g in range(len(e["regions"])):
        got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["jobs"][:0], bd, psy_rd=0.4, pyramids=e["regions"][g:g + 1], fill=FILL, spare_jobs=5)
        same(got, e["ssim"][n + 85 * g:n + 85 * g + 85], e["dist"][0.4][n + 85 * g:n + 85 * g + 85], (bd, "region", g))
    got = stats.run_ssim_hip(hip_ctx, e["src"], e["ref"], e["jobs"][:0], bd, psy_rd=1.0, pyramids=e["regions"][:0], fill=FILL, spare_jobs=5)
    assert len(got["ssim"]) == 0 and len(got["ssim_dist"]) == 0  # returned 0; the runner found the five filled slots as they were


def test_pointer_level_entries_with_unequal_strides(hip_ctx, golden, oracle):
    """every entry with two different strides and offsets, on host arrays that end with the last sample the reference reads: for 12x8 with
    the psy term that is the eighth row of a 16-column window, for 4x8 the block itself"""
    L = api.lib()
    entries = ["svt_ssim_8x8_hip", "svt_ssim_4x4_hip", "svt_ssim_8x8_hbd_hip", "svt_ssim_4x4_hbd_hip"]
    for name in entries:
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    f = L.svt_spatial_full_distortion_ssim_kernel_hip
    f.restype = C.c_uint64
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_bool, C.c_double]
    assert L.svt_hip_leaf_bind(hip_ctx._h) == 0
    try:
        L.svt_hip_leaf_status(None, None, None, C.c_size_t(0))
        for bd in (8, 10):
            e = sc.edge_expected(oracle, bd)
            src, ref, jobs = e["src"], e["ref"], e["jobs"]
            sp, rp = src.shape[1], ref.shape[1]
            fs, fr = src.reshape(-1), ref.reshape(-1)
            got = []
            for kind, (n, so, ro) in zip(golden[f"tile_kind{bd}"], sc.edge_tiles(jobs)):
                s, r = fs[so:so + (n - 1) * sp + n].copy(), fr[ro:ro + (n - 1) * rp + n].copy()
                got.append(getattr(L, entries[int(kind)])(s.ctypes.data, sp, r.ctypes.data, rp))
            assert np.array_equal(sc.bits(got), golden[f"tile_bits{bd}"]), bd
            small = [i for i, j in enumerate(jobs) if (int(j["width"]), int(j["height"])) in ((12, 8), (4, 8))]
            sample = [(i, (i // 4) % 5) for i in range(0, len(jobs), 4)] + [(i, 1 + 3 * (t & 1)) for t, i in enumerate(small[::4])]
            assert {(int(jobs[i]["width"]), int(jobs[i]["height"])) for i, k in sample if k} >= {(12, 8), (4, 8), (128, 124), (64, 64)}
            for i, k in sample:
                j, psy = jobs[i], sc.EDGE_PSY_RDS[k]
                w, h = int(j["width"]), int(j["height"])
                cw, ch = sc.read_extent(w, h) if psy > 0.0 else (w, h)
                so, ro = int(j["src_offset"]), int(j["ref_offset"])
                s, r = fs[:so + (ch - 1) * sp + cw].copy(), fr[:ro + (ch - 1) * rp + cw].copy()
                d = f(s.ctypes.data, so, sp, r.ctypes.data, ro, rp, w, h, bd == 10, psy)
                assert d == int(golden[f"dist{bd}"][k][i]), (bd, psy, w, h)
        assert L.svt_hip_leaf_status(None, None, None, C.c_size_t(0)) == 0  # nothing fell back
    finally:
        L.svt_hip_leaf_bind(None)
