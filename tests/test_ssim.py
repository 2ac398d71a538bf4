"""CPU: the SSIM distortion of the SSIM tunes -- the restatement (tests/ssim_cases.py) against the reference's own results (golden/ssim.npz),
the C-ABI of svt_hip_ssim_batch (validation needs no GPU), the rtcd names of the SSIM leaves, and their fail-closed behaviour."""
import ctypes as C

import numpy as np
import pytest

import ssim_cases as sc
from batch_entry_cases import good_ssim_desc
from svt_av1_psyex_amd import abi, api, stats

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN)


@pytest.mark.parametrize("bd", [8, 10])
def test_restated_leaves_equal_the_reference_bit_for_bit(golden, bd):
    src, ref = golden[f"src{bd}"], golden[f"ref{bd}"]
    stride = src.shape[1]
    kinds = golden[f"tile_kind{bd}"]
    assert set(kinds.tolist()) == ({0, 1} if bd == 8 else {2, 3})
    got = []
    for kind, so, ro in zip(kinds, golden[f"tile_src{bd}"], golden[f"tile_ref{bd}"]):
        n = 8 if kind in (0, 2) else 4
        (sy, sx), (ry, rx) = divmod(int(so), stride), divmod(int(ro), stride)
        got.append(sc.tile_score(src[sy:sy + n, sx:sx + n], ref[ry:ry + n, rx:rx + n], bd))
    want = golden[f"tile_bits{bd}"]
    assert np.array_equal(sc.bits(got), want)
    vals = want.view(np.float64)
    assert (vals < 0).any() and (vals == 1.0).any()  # the inverted content scores below zero; src == ref scores exactly one


@pytest.mark.parametrize("bd", [8, 10])
def test_restated_distortion_equals_the_reference(golden, oracle, bd):
    src, ref, jobs = golden[f"src{bd}"], golden[f"ref{bd}"], golden[f"jobs{bd}"]
    sizes = {(int(j["width"]), int(j["height"])) for j in jobs}
    assert sizes >= set(sc.AV1_BLOCKS) | set(sc.TX_SIZES) | set(sc.CROPPED)
    for k, psy in enumerate(golden["psy_rds"]):
        got = sc.run_jobs(oracle, src, ref, jobs, bd, float(psy))
        assert np.array_equal(got["ssim_dist"], golden[f"dist{bd}"][k]), f"psy_rd {psy}"
    assert (golden[f"dist{bd}"][0] == 0).any()  # src == ref: ssim exactly 1


@pytest.fixture(scope="module")
def golden_edges():
    return np.load(sc.GOLDEN_EDGES)


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_equals_the_reference_on_the_edge_cases(golden_edges, oracle, bd):
    """source and reference planes of different widths, the blocks at unrelated places of the two (golden/ssim_edges.npz)"""
    import zlib
    e = sc.edge_expected(oracle, bd)
    assert zlib.crc32(b"".join(np.ascontiguousarray(e[k]).tobytes() for k in ("src", "ref", "jobs", "regions"))) == int(golden_edges[f"crc{bd}"])
    assert tuple(golden_edges["psy_rds"]) == sc.EDGE_PSY_RDS
    for k, psy in enumerate(sc.EDGE_PSY_RDS):
        bad = np.nonzero(e["dist"][psy] != golden_edges[f"dist{bd}"][k])[0]
        assert not len(bad), (psy, bad[:5].tolist())
    src, ref = e["src"], e["ref"]
    got = []
    for (n, so, ro) in sc.edge_tiles(e["jobs"]):
        (sy, sx), (ry, rx) = divmod(so, src.shape[1]), divmod(ro, ref.shape[1])
        got.append(sc.tile_score(src[sy:sy + n, sx:sx + n], ref[ry:ry + n, rx:rx + n], bd))
    assert np.array_equal(sc.bits(got), golden_edges[f"tile_bits{bd}"])
    assert set(golden_edges[f"tile_kind{bd}"].tolist()) == ({0, 1} if bd == 8 else {2, 3})


@pytest.mark.parametrize("bd", [8, 10])
def test_edge_cases_cover_what_they_are_for(golden_edges, oracle, bd):
    e = sc.edge_expected(oracle, bd)
    src, ref, jobs = e["src"], e["ref"], e["jobs"]
    sp, rp = src.shape[1], ref.shape[1]
    assert sp != rp and src.shape[0] <= 256 and max(sp, rp) <= 256
    assert {(int(j["width"]), int(j["height"])) for j in jobs} == set(sc.EDGE_SIZES) | {(128, 124)}
    for kind in sc.EDGE_KINDS:
        assert {(int(j["width"]), int(j["height"])) for j, k in zip(jobs, e["kinds"]) if k == kind} >= set(sc.EDGE_SIZES)
    for j in e["every"]:  # different rows and columns of the two planes, and every read inside the common length whichever stride is taken
        (sy, sx), (ry, rx) = divmod(int(j["src_offset"]), sp), divmod(int(j["ref_offset"]), rp)
        cw, ch = sc.read_extent(int(j["width"]), int(j["height"]))
        assert sx + cw <= sp and rx + cw <= rp and max(sy, ry) + ch <= src.shape[0]
        assert max(int(j["src_offset"]), int(j["ref_offset"])) + (ch - 1) * max(sp, rp) + cw <= max(src.size, ref.size)
    rows = [(divmod(int(j["src_offset"]), sp), divmod(int(j["ref_offset"]), rp)) for j in jobs]
    assert sum(a[0] != b[0] and a[1] != b[1] for a, b in rows) >= len(jobs) * 3 // 4
    n = len(jobs)
    assert (e["ssim"][:n] == 1.0).sum() >= 4 and (e["ssim"][:n] == 0.0).sum() >= 4  # src == ref scores exactly 1; the inverted content clamps to 0
    assert (golden_edges[f"dist{bd}"][0] == 0).any()
    assert (golden_edges[f"tile_bits{bd}"].view(np.float64) < 0).any() and (golden_edges[f"tile_bits{bd}"].view(np.float64) == 1.0).any()
    # the large strength: energy * psy_rd below 2^53 (exact in a double) everywhere and at or above 2^32 on at least a quarter of the jobs
    prod = [int(x) * sc.PSY_LARGE for x in e["energy"]]
    assert max(prod) < 2.0 ** 53 and sum(p >= 2.0 ** 32 for p in prod) * 4 >= len(prod) and sum(p >= 2.0 ** 32 for p in prod[:n]) * 4 >= n
    assert all(int(x) * max(sc.PSY_RDS) < 2.0 ** 32 for x in e["energy"])  # what the other strengths leave untested


def test_descriptor_size_matches_ctypes():
    L = api.lib()
    L.svt_hip_ssim_desc_size.restype = C.c_size_t
    assert L.svt_hip_ssim_desc_size() == C.sizeof(abi.SsimBatchDesc)


# (null arguments: tests/test_batch_entries.py)
@pytest.mark.parametrize("bad", ["bit_depth_9", "bit_depth_12", "no_src", "no_ref", "no_jobs", "no_pyramids", "no_outputs",
                                 "zero_stride", "nan_psy"])
def test_bad_descriptor_is_rejected_without_a_gpu(bad):
    L = api.lib()
    ctx = C.create_string_buffer(64)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    d = good_ssim_desc(n_pyramids=0)
    if bad.startswith("bit_depth"):
        d.bit_depth = int(bad.split("_")[-1])
    elif bad == "no_src":
        d.src = None
    elif bad == "no_ref":
        d.ref = None
    elif bad == "no_jobs":
        d.jobs = None
    elif bad == "no_pyramids":
        d.n_pyramids = 1
    elif bad == "no_outputs":
        d.ssim = d.ssim_dist = None
    elif bad == "zero_stride":
        d.src_stride = 0
    elif bad == "nan_psy":
        d.psy_rd = float("nan")
    assert L.svt_hip_ssim_batch(ctx, C.byref(d)) == BAD_PARAM
    assert b"svt_hip_ssim_batch" in L.svt_hip_last_error(None)


def _jobs(*rows):
    return np.array(list(rows), dtype=abi.BLOCK_JOB_DTYPE)


@pytest.mark.parametrize("job", [(0, 0, 6, 8, 0, 0), (0, 0, 8, 2, 0, 0), (0, 0, 0, 8, 0, 0), (0, 0, 132, 8, 0, 0), (0, 0, 8, 136, 0, 0), (0, 0, 8, 8, 1, 0),
                                 (0, 0, 8, 8, 0, 3)])
def test_job_sizes_and_subpel_are_checked_on_the_host(job):
    stats.check_ssim_jobs(_jobs((0, 0, 12, 8, 0, 0), (0, 0, 4, 128, 0, 0), (0, 0, 128, 128, 0, 0)))
    with pytest.raises(api.SvtHipError):
        stats.check_ssim_jobs(_jobs((0, 0, 8, 8, 0, 0), job))


def test_pyramid_regions_must_be_64x64():
    stats.check_ssim_jobs(_jobs((0, 0, 64, 64, 0, 0)), pyramids=True)
    for bad in [(0, 0, 32, 32, 0, 0), (0, 0, 64, 128, 0, 0), (0, 0, 64, 64, 2, 0)]:
        with pytest.raises(api.SvtHipError):
            stats.check_ssim_jobs(_jobs(bad), pyramids=True)


SSIM_NAMES = ["svt_ssim_8x8", "svt_ssim_4x4", "svt_ssim_8x8_hbd", "svt_ssim_4x4_hbd"]


def test_rtcd_lookup_resolves_the_ssim_slots():
    L = api.lib()
    L.svt_hip_rtcd_lookup.restype = C.c_void_p
    for name in SSIM_NAMES:
        assert L.svt_hip_rtcd_lookup(name.encode()) == C.cast(getattr(L, name + "_hip"), C.c_void_p).value, name
    assert L.svt_hip_rtcd_lookup(b"svt_spatial_full_distortion_ssim_kernel") == C.cast(L.svt_spatial_full_distortion_ssim_kernel_hip, C.c_void_p).value


class Slot(C.Structure):
    _fields_ = [("name", C.c_char_p), ("slot", C.POINTER(C.c_void_p))]


TILE8 = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32)
SSIM_DIST = C.CFUNCTYPE(C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_bool, C.c_double)


def test_ssim_leaves_fail_closed_without_a_device():
    """No context bound: each entry installed over a stand-in hands its call, arguments intact, to the stand-in and counts the fallback."""
    L = api.lib()
    L.svt_hip_leaf_bind(None)
    L.svt_hip_leaf_status(None, None, None, C.c_size_t(0))
    calls = []

    def stand_in(k):
        def f(s, sp, r, rp):
            calls.append((k, sp, rp))
            return 0.25 + k
        return f

    def dist(inp, io, ist, rec, ro, rst, w, h, hbd, psy):
        calls.append(("dist", io, ist, ro, rst, w, h, hbd, psy))
        return 123456789

    keep = [TILE8(stand_in(k)) for k in range(4)] + [SSIM_DIST(dist)]
    names = [n.encode() for n in SSIM_NAMES] + [b"svt_spatial_full_distortion_ssim_kernel"]
    prev = [C.cast(k, C.c_void_p).value for k in keep]
    vals = [C.c_void_p(p) for p in prev]
    slots = (Slot * len(names))(*[Slot(n, C.pointer(v)) for n, v in zip(names, vals)])
    skipped = C.c_uint32(9)
    try:
        assert L.svt_hip_rtcd_store(slots, len(names), C.byref(skipped)) == 0 and skipped.value == 0
        for v, n in zip(vals, names):
            assert v.value == C.cast(getattr(L, n.decode() + "_hip"), C.c_void_p).value
        a = np.arange(1024, dtype=np.uint16)
        for k in range(4):
            assert TILE8(vals[k].value)(a.ctypes.data, 16 + k, a.ctypes.data, 32 + k) == 0.25 + k
        assert SSIM_DIST(vals[4].value)(a.ctypes.data, 3, 40, a.ctypes.data, 5, 48, 12, 8, True, 0.4) == 123456789
        assert calls[:4] == [(k, 16 + k, 32 + k) for k in range(4)]
        assert calls[4][:8] == ("dist", 3, 40, 5, 48, 12, 8, True) and calls[4][8] == 0.4
        fb, un = C.c_ulonglong(0), C.c_ulonglong(0)
        msg = C.create_string_buffer(512)
        assert L.svt_hip_leaf_status(C.byref(fb), C.byref(un), msg, C.c_size_t(512)) == 5
        assert (fb.value, un.value) == (5, 0) and b"svt_spatial_full_distortion_ssim_kernel_hip" in msg.value
    finally:
        L.svt_hip_uninstall_rtcd(slots, len(names))
    assert [v.value for v in vals] == prev
