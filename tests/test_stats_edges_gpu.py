"""GPU: svt_hip_block_stats_batch on the launch paths and at the value ranges its older tests do not reach (tests/stats_edge_cases.py): four
hadamard_path jobs per wave with mixed block kinds, flat waves beside regions, regions with two strides, Walsh residuals, 32-bit wraps,
null outputs.  Every call pre-fills its outputs with 0xA5 and has five spare slots; every comparison is exact.  Which path a batch takes
is asked of svt_hip_block_stats_jobs_per_wave, never restated."""
import numpy as np
import pyoracle
import pytest

import stats_edge_cases as ec
from svt_av1_psyex_amd import abi, stats

pytestmark = pytest.mark.gpu
GUARD = dict(fill=0xA5, spare_jobs=5)
NO_JOBS = np.zeros(0, abi.BLOCK_JOB_DTYPE)


def same(got, want, what, keys=None):
    for k in keys or want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == GUARD["fill"]).all())


def expanded(jobs, reg, src, ref):
    return np.concatenate([jobs] + [stats.expand_pyramid(r, src.shape[1], ref.shape[1]) for r in reg])


@pytest.fixture(scope="module")
def packed(hip_ctx, oracle):
    """per av1_only: the packed list grown by whole groups until the launch packs four jobs per wave, the oracle's outputs and the batch's"""
    res = {}
    for av1_only in (True, False):
        n_min = ec.PACKED_N_MIN
        while True:
            src, ref, jobs, kinds = ec.standard_packed(av1_only, n_min)
            if stats.jobs_per_wave(hip_ctx, len(jobs)) == 4 or n_min >= 1 << 17:
                break
            n_min += 1024
        want = pyoracle.block_stats(oracle, src, ref, jobs, 8, satd=True)
        ec.assert_packed_coverage(jobs, kinds, want["satd"])
        jpw = stats.jobs_per_wave(hip_ctx, len(jobs))
        got = stats.run_hip(hip_ctx, src, ref, jobs, 8, satd=True, **GUARD)
        print(f"packed list (av1_only={av1_only}): {len(jobs)} jobs, {jpw} per wave")
        res[av1_only] = dict(src=src, ref=ref, jobs=jobs, kinds=kinds, want=want, got=got, jpw=jpw, n_min=n_min)
    return res


@pytest.mark.parametrize("av1_only", [True, False])
def test_packed_waves_match_oracle(packed, av1_only):
    """four jobs per wave, the flat kernel: A (one shared tile), B (three 8x8 and another job), C (a sub-pel 8x8 among them), D groups and
    a last wave of one to three jobs, every output"""
    p = packed[av1_only]
    assert p["jpw"] == 4
    same(p["got"], p["want"], "packed list")
    if av1_only:  # its first jobs against the reference's own outputs
        _, _, _, fj, val, ok = ec.load_fixture("packed")
        assert np.array_equal(fj, p["jobs"][:len(fj)])
        assert not ec.disagreements(val, ok, {k: v[:len(fj)] for k, v in p["got"].items()})


def test_packed_waves_with_psy_in_the_same_launch(hip_ctx, oracle, packed):
    p = packed[True]
    want = pyoracle.block_stats(oracle, p["src"], p["ref"], p["jobs"], 8, satd=True, psy_rd=0.75)
    got = stats.run_hip(hip_ctx, p["src"], p["ref"], p["jobs"], 8, satd=True, psy_rd=0.75, **GUARD)
    print(f"packed list with psy: {len(p['jobs'])} jobs, {p['jpw']} per wave")
    same(got, want, "packed list, hadamard_path and psy")
    assert len(np.unique(got["psy_energy"])) > 500


def test_one_job_per_wave_agrees_with_four(hip_ctx, packed):
    """the same list cut to 4,000 jobs takes the other path: its outputs are the packed run's, job for job"""
    for av1_only in (True, False):
        p = packed[av1_only]
        assert stats.jobs_per_wave(hip_ctx, 4000) == 1 and p["jpw"] == 4
        got = stats.run_hip(hip_ctx, p["src"], p["ref"], p["jobs"][:4000], 8, satd=True, **GUARD)
        same(got, {k: v[:4000] for k, v in p["got"].items()}, "4,000 jobs, one per wave")
    print("cut list: 4000 jobs, 1 per wave")


@pytest.mark.parametrize("waves_mod_4", [1, 2])
def test_packed_flat_waves_beside_regions(hip_ctx, oracle, packed, waves_mod_4):
    """block_stats4_kernel: 9 regions, then packed flat waves that fill the last workgroup with one or two waves, the last of them partly"""
    src, ref, jobs, _ = ec.standard_packed(True, packed[True]["n_min"] + 64)
    n = max(k for k in range(len(jobs) - 20, len(jobs) + 1) if ((k + 3) // 4) % 4 == waves_mod_4 and k % 4)
    jobs = jobs[:n]
    assert stats.jobs_per_wave(hip_ctx, n) == 4
    reg = ec.regions(np.random.default_rng(90 + waves_mod_4), ec.W, ec.REF_STRIDE, ec.H, 9)
    want = pyoracle.block_stats(oracle, src, ref, expanded(jobs, reg, src, ref), 8, satd=True)
    got = stats.run_hip(hip_ctx, src, ref, jobs, 8, satd=True, pyramids=reg, **GUARD)
    print(f"regions + packed list: 9 regions, {n} jobs, 4 per wave, {(n + 3) // 4} flat waves")
    same(got, want, f"9 regions and {n} flat jobs")


def test_regions_with_unequal_strides(hip_ctx, oracle):
    """source stride 320, reference stride 352: the one-wave form (10-bit, psy and facade) and the four-wave form (8-bit, hadamard_path)"""
    rng = np.random.default_rng(91)
    h = 160
    src10 = rng.integers(0, 1024, (h, 320)).astype(np.uint16)
    ref10 = rng.integers(0, 1024, (h, 352)).astype(np.uint16)
    ref10[:, :320] = np.clip(src10.astype(np.int32) + rng.integers(-90, 91, src10.shape), 0, 1023)
    reg = ec.regions(rng, 320, 352, h, 13)
    reg[0] = (17 * 320 + 3, 17 * 352 + 3, 64, 64, 0, 0)  # one region of small residuals
    plain = np.array([ec.random_job(rng, 320, 352, h, w, hh) for w, hh in ec.AV1_SHAPES[:7]], dtype=abi.BLOCK_JOB_DTYPE)
    ex = expanded(plain, reg, src10, ref10)
    assert np.array_equal(ex[len(plain):len(plain) + 85], stats.expand_pyramid(reg[0], 320, 352))
    facade = dict(pred_mode=rng.integers(0, 25, len(ex)).astype(np.uint8), compound_type=rng.integers(0, 4, len(ex)).astype(np.uint8), temporal_layer_index=2, spy_rd=1)
    want = pyoracle.block_stats(oracle, src10, ref10, ex, 10, satd=False, psy_rd=1.35, facade=facade)
    got = stats.run_hip(hip_ctx, src10, ref10, plain, 10, satd=False, psy_rd=1.35, facade=facade, pyramids=reg, **GUARD)
    flat = stats.run_hip(hip_ctx, src10, ref10, ex, 10, satd=False, psy_rd=1.35, facade=facade, **GUARD)
    same(got, want, "one-wave regions vs oracle")
    same(got, flat, "one-wave regions vs plain jobs")
    src8, ref8 = (src10 >> 2).astype(np.uint8), (ref10 >> 2).astype(np.uint8)
    plain = plain[(plain["width"] == plain["height"])]
    ex = expanded(plain, reg, src8, ref8)
    want = pyoracle.block_stats(oracle, src8, ref8, ex, 8, satd=True)
    got = stats.run_hip(hip_ctx, src8, ref8, plain, 8, satd=True, pyramids=reg, **GUARD)
    flat = stats.run_hip(hip_ctx, src8, ref8, ex, 8, satd=True, **GUARD)
    print(f"unequal strides: 13 regions + {len(plain)} jobs; the plain-job form of the 8-bit run: {len(ex)} jobs, {stats.jobs_per_wave(hip_ctx, len(ex))} per wave")
    same(got, want, "four-wave regions vs oracle")
    same(got, flat, "four-wave regions vs plain jobs")


def test_walsh_planes_as_flat_jobs(hip_ctx):
    """+-255 residuals that are one Hadamard coefficient: |X H16| reaches 2040, a coefficient 16,320.  One job per wave"""
    _, src, ref, jobs, val, ok = ec.load_fixture("walsh")
    assert stats.jobs_per_wave(hip_ctx, len(jobs)) == 1
    got = stats.run_hip(hip_ctx, src, ref, jobs, 8, satd=True, psy_rd=1.0, **GUARD)
    print(f"Walsh planes, flat: {len(jobs)} jobs, 1 per wave")
    np.testing.assert_array_equal(got["satd"], ec.walsh_jobs()[1])
    assert not ec.disagreements(val, ok, got)
    area = jobs["width"].astype(np.uint64) * jobs["height"]
    assert np.array_equal(got["sad"], area * 255) and np.array_equal(got["sse"], area * 255 * 255)


def test_walsh_planes_as_shared_tiles(hip_ctx):
    """the atlas's 8x8 blocks as A groups: four Walsh planes of different (u, v, sign) side by side in one matrix-core tile"""
    n_min = ec.PACKED_N_MIN
    while stats.jobs_per_wave(hip_ctx, n_min) != 4 and n_min < 1 << 17:
        n_min += 1024
    src, ref = ec.walsh_atlas()
    jobs, satd = ec.walsh_quads(np.random.default_rng(92), n_min)
    assert stats.jobs_per_wave(hip_ctx, len(jobs)) == 4 and len(jobs) % 4 == 0
    q = satd.reshape(-1, 4)
    assert ((q[:, 1] != q[:, 2]).sum() > 100) and ((q[:, 0] != q[:, 3]).sum() > 100)  # quads whose results are not all alike
    got = stats.run_hip(hip_ctx, src, ref, jobs, 8, satd=True, **GUARD)
    print(f"Walsh planes, shared tiles: {len(jobs)} jobs, 4 per wave")
    np.testing.assert_array_equal(got["satd"], satd)
    full = (satd != 0) * np.uint32(64 * 255)
    assert np.array_equal(got["sad"], full) and np.array_equal(got["sse"], full.astype(np.uint64) * 255) and np.array_equal(got["var_sse"], full * 255)


def test_walsh_planes_as_regions(hip_ctx, oracle):
    src, ref = ec.walsh_atlas()
    reg = ec.walsh_regions()
    got = stats.run_hip(hip_ctx, src, ref, NO_JOBS, 8, satd=True, pyramids=reg, **GUARD)
    print(f"Walsh planes, regions: {len(reg)} regions")
    np.testing.assert_array_equal(got["satd"], ec.walsh_region_satd(len(reg)))
    same(got, pyoracle.block_stats(oracle, src, ref, expanded(NO_JOBS, reg, src, ref), 8, satd=True), "Walsh regions")


@pytest.mark.parametrize("name", list(ec.RANGE_SETS))
def test_range_limit_blocks(hip_ctx, oracle, name):
    """all-max against zero at every variance size and the +1023 / -1023 block: the 32-bit wrap of var_sse and variance, the split reduction
    of the sum of squares; as flat jobs against the reference's outputs, and at 64x64 as regions"""
    bd, src, ref, jobs, val, ok = ec.load_fixture(name)
    got = stats.run_hip(hip_ctx, src, ref, jobs, bd, satd=(bd == 8), psy_rd=1.0, **GUARD)
    print(f"range limits {name}, flat: {len(jobs)} jobs, {stats.jobs_per_wave(hip_ctx, len(jobs), satd=(bd == 8))} per wave")
    assert not ec.disagreements(val, ok, got)
    assert all(ok[k].all() for k in ok if k != "satd")
    if bd == 10:
        over = got["sse"] > 1 << 32
        assert over.any() and (got["sse"][over] != got["var_sse"][over]).all()
    reg = ec.range_regions(ec.RANGE_SETS[name][1])
    ex = expanded(NO_JOBS, reg, src, ref)
    want = pyoracle.block_stats(oracle, src, ref, ex, bd, satd=(bd == 8), psy_rd=1.0)
    one = stats.run_hip(hip_ctx, src, ref, NO_JOBS, bd, satd=False, psy_rd=1.0, pyramids=reg, **GUARD)
    same(one, want, "one-wave regions", keys=one)
    if bd == 8:
        same(stats.run_hip(hip_ctx, src, ref, NO_JOBS, bd, satd=True, psy_rd=1.0, pyramids=reg, **GUARD), want, "four-wave regions")
    if name != "split10":  # the first region is the 64x64 job of the flat list
        j = abi.VARIANCE_SIZES.index((64, 64))
        for k in val:
            if ok[k][j] and k in one:
                assert one[k][0] == val[k][j], k


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("pat", ec.PSY_PATTERNS)
def test_psy_patterns(hip_ctx, oracle, bd, pat):
    """all-max, checkerboard, min-max and near-black planes through the psy energy: four jobs of four sizes per wave, and regions"""
    src, ref = ec.psy_planes(bd, pat)
    jobs = ec.psy_jobs()
    assert stats.jobs_per_wave(hip_ctx, len(jobs), satd=False) == 4 and len(jobs) % 4 == 2
    want = pyoracle.block_stats(oracle, src, ref, jobs, bd, satd=False, psy_rd=1.35)
    same(stats.run_hip(hip_ctx, src, ref, jobs, bd, satd=False, psy_rd=1.35, **GUARD), want, "flat")
    reg = ec.regions(np.random.default_rng(93), ec.W, ec.REF_STRIDE, ec.H, 6)
    want = pyoracle.block_stats(oracle, src, ref, expanded(NO_JOBS, reg, src, ref), bd, satd=(bd == 8), psy_rd=1.35)
    one = stats.run_hip(hip_ctx, src, ref, NO_JOBS, bd, satd=False, psy_rd=1.35, pyramids=reg, **GUARD)
    same(one, want, "one-wave regions", keys=one)
    if bd == 8:
        same(stats.run_hip(hip_ctx, src, ref, NO_JOBS, bd, satd=True, psy_rd=1.35, pyramids=reg, **GUARD), want, "four-wave regions")
    if pat in ("minmax", "low"):  # random content: the energies differ from block to block (all-max and, at 10 bits, the checkerboard give 0)
        assert len(np.unique(want["psy_energy"])) > 50


def test_optional_outputs_alone(hip_ctx, packed):
    """one output pointer set, the others null: the named array is the full run's, no other array is touched"""
    p = packed[True]
    for name in ("sse", "satd"):
        got = stats.run_hip(hip_ctx, p["src"], p["ref"], p["jobs"], 8, outputs=(name,), **GUARD)
        assert stats.jobs_per_wave(hip_ctx, len(p["jobs"]), satd=(name == "satd")) == 4
        np.testing.assert_array_equal(got[name], p["got"][name], err_msg=name)
        np.testing.assert_array_equal(got[name], p["want"][name], err_msg=f"{name} vs oracle")
        assert sorted(got) == sorted(p["got"]) and all(untouched(got[k]) for k in got if k != name), name
    print(f"optional outputs: {len(p['jobs'])} jobs, 4 per wave")
