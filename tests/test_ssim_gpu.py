"""GPU: svt_hip_ssim_batch and the SSIM leaves on the MI355X, every comparison exact (doubles as uint64 bit patterns) -- against the
reference's own results (golden/ssim.npz), against the restatement (tests/ssim_cases.py) on a seeded grid, pyramid form against plain jobs,
and the device-side chain RD batch -> SSIM batch."""
import ctypes as C

import numpy as np
import pytest

import ssim_cases as sc
from svt_av1_psyex_amd import abi, api, rd, stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN)


@pytest.mark.parametrize("bd", [8, 10])
def test_batch_equals_the_reference_fixture(hip_ctx, golden, oracle, bd):
    src, ref, jobs = golden[f"src{bd}"], golden[f"ref{bd}"], golden[f"jobs{bd}"]
    for k, psy in enumerate(golden["psy_rds"]):
        got = stats.run_ssim_hip(hip_ctx, src, ref, jobs, bd, psy_rd=float(psy))
        assert np.array_equal(got["ssim_dist"], golden[f"dist{bd}"][k]), f"psy_rd {psy}"
        if k == 0:
            assert np.array_equal(sc.bits(got["ssim"]), sc.bits(sc.run_jobs(oracle, src, ref, jobs, bd)["ssim"]))


@pytest.mark.parametrize("bd", [8, 10])
def test_batch_equals_the_restatement_on_a_seeded_grid(hip_ctx, oracle, bd):
    rng = np.random.default_rng(700 + bd)
    src, ref = sc.make_planes(rng, bd)
    jobs = sc.region_jobs(rng, sc.SIZES, sc.ALL_PAIRS, per_size=2)
    want0 = sc.run_jobs(oracle, src, ref, jobs, bd)
    for psy in (0.0, 0.4, 1.0):
        got = stats.run_ssim_hip(hip_ctx, src, ref, jobs, bd, psy_rd=psy)
        want = want0 if psy == 0.0 else sc.run_jobs(oracle, src, ref, jobs, bd, psy)
        assert np.array_equal(sc.bits(got["ssim"]), sc.bits(want["ssim"])), psy
        bad = np.nonzero(got["ssim_dist"] != want["ssim_dist"])[0]
        assert not len(bad), [(int(jobs[i]["width"]), int(jobs[i]["height"]), int(got["ssim_dist"][i]), int(want["ssim_dist"][i])) for i in bad[:5]]


@pytest.mark.parametrize("bd", [8, 10])
def test_pyramid_equals_85_plain_jobs(hip_ctx, oracle, bd):
    rng = np.random.default_rng(900 + bd)
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    src = rng.integers(0, mx + 1, (192, 320)).astype(dt)
    ref = np.clip(src.astype(np.int32) + rng.integers(-mx // 8, mx // 8 + 1, src.shape), 0, mx).astype(dt)
    ref[64:128, 64:128] = src[64:128, 64:128]  # one region identical (every score 1), one inverted (the clamp)
    ref[0:64, 192:256] = mx - src[0:64, 192:256]
    regions = np.array([(y * 320 + x, y * 320 + x, 64, 64, 0, 0) for y in (0, 64, 128) for x in (0, 64, 128, 192, 256)], dtype=abi.BLOCK_JOB_DTYPE)
    plain = np.concatenate([stats.expand_pyramid(r, 320, 320) for r in regions])
    for psy in (0.0, 1.0):
        pyr = stats.run_ssim_hip(hip_ctx, src, ref, np.zeros(0, abi.BLOCK_JOB_DTYPE), bd, psy_rd=psy, pyramids=regions)
        flat = stats.run_ssim_hip(hip_ctx, src, ref, plain, bd, psy_rd=psy)
        assert np.array_equal(sc.bits(pyr["ssim"]), sc.bits(flat["ssim"])), psy
        assert np.array_equal(pyr["ssim_dist"], flat["ssim_dist"]), psy
        want = sc.run_jobs(oracle, src, ref, plain, bd, psy)
        assert np.array_equal(sc.bits(pyr["ssim"]), sc.bits(want["ssim"])) and np.array_equal(pyr["ssim_dist"], want["ssim_dist"]), psy
    # plain jobs and regions in one batch: the regions' slots follow the plain ones
    both = stats.run_ssim_hip(hip_ctx, src, ref, plain[:7], bd, psy_rd=1.0, pyramids=regions[:2])
    assert np.array_equal(both["ssim_dist"][:7], flat["ssim_dist"][:7]) and np.array_equal(both["ssim_dist"][7:], flat["ssim_dist"][:170])


def test_pointer_level_entries_equal_the_reference_fixture(hip_ctx, golden):
    L = api.lib()
    for name in ("svt_ssim_8x8_hip", "svt_ssim_4x4_hip", "svt_ssim_8x8_hbd_hip", "svt_ssim_4x4_hbd_hip"):
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    f = L.svt_spatial_full_distortion_ssim_kernel_hip
    f.restype = C.c_uint64
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_bool, C.c_double]
    entries = ["svt_ssim_8x8_hip", "svt_ssim_4x4_hip", "svt_ssim_8x8_hbd_hip", "svt_ssim_4x4_hbd_hip"]
    assert L.svt_hip_leaf_bind(hip_ctx._h) == 0
    try:
        L.svt_hip_leaf_status(None, None, None, C.c_size_t(0))
        for bd in (8, 10):
            src, ref = golden[f"src{bd}"], golden[f"ref{bd}"]
            stride, bpp = src.shape[1], src.itemsize
            got = [getattr(L, entries[int(k)])(src.ctypes.data + int(so) * bpp, stride, ref.ctypes.data + int(ro) * bpp, stride)
                   for k, so, ro in zip(golden[f"tile_kind{bd}"], golden[f"tile_src{bd}"], golden[f"tile_ref{bd}"])]
            assert np.array_equal(sc.bits(got), golden[f"tile_bits{bd}"]), bd
            jobs = golden[f"jobs{bd}"]
            for k, psy in enumerate(golden["psy_rds"]):
                for i in range(k, len(jobs), 5):  # a fifth of the jobs per strength: every call is a round trip
                    j = jobs[i]
                    d = f(src.ctypes.data, int(j["src_offset"]), stride, ref.ctypes.data, int(j["ref_offset"]), stride, int(j["width"]), int(j["height"]),
                          bd == 10, float(psy))
                    assert d == int(golden[f"dist{bd}"][k][i]), (bd, float(psy), int(j["width"]), int(j["height"]))
        assert L.svt_hip_leaf_status(None, None, None, C.c_size_t(0)) == 0  # nothing fell back
    finally:
        L.svt_hip_leaf_bind(None)


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_rd_batch_then_ssim_batch_on_device(hip_ctx, oracle, bd):
    """tx_type_search's distortion on the device: svt_hip_rd_batch writes the reconstruction, svt_hip_ssim_batch reads it on the same stream
    (no host copy in between); equal to the restatement on the reconstruction read back."""
    import torch
    rng = np.random.default_rng(1100 + bd)
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    W, H = 192, 128
    src = rng.integers(0, mx + 1, (H, W)).astype(dt)
    pred = np.clip(src.astype(np.int32) + rng.integers(-mx // 10, mx // 10 + 1, src.shape), 0, mx).astype(dt)
    ts = 2  # TX_16X16
    jobs = rd.grid_jobs(W, H, W, ts)
    rows = np.stack([rd.quant_row_from_step(60 if bd == 8 else 240, 75 if bd == 8 else 300)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    t_src, t_pred, t_jobs, t_q = dev(src), dev(pred), dev(jobs), dev(rows)
    t_rec = t_pred.clone()
    n = len(jobs)
    outs = {name: torch.zeros(n * k * np.dtype(d).itemsize, dtype=torch.uint8, device="cuda") for name, d, k in abi.RD_OUT_FIELDS}
    d = abi.RdBatchDesc(bit_depth=bd, quant_kind=0, tx_size=ts, n_jobs=n, src_stride=W, pred_stride=W, src=t_src.data_ptr(), pred=t_pred.data_ptr(),
                        recon=t_rec.data_ptr(), jobs=t_jobs.data_ptr(), quant_rows=t_q.data_ptr(), n_quant_rows=1)
    for name, t in outs.items():
        setattr(d, name, t.data_ptr())
    sjobs = np.zeros(n, abi.BLOCK_JOB_DTYPE)
    sjobs["src_offset"], sjobs["ref_offset"], sjobs["width"], sjobs["height"] = jobs["src_offset"], jobs["pred_offset"], abi.TX_W[ts], abi.TX_H[ts]
    t_sjobs = dev(sjobs)
    t_ssim, t_dist = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    s = abi.SsimBatchDesc(bit_depth=bd, n_jobs=n, src_stride=W, ref_stride=W, src=t_src.data_ptr(), ref=t_rec.data_ptr(), jobs=t_sjobs.data_ptr(), psy_rd=1.0,
                          ssim=t_ssim.data_ptr(), ssim_dist=t_dist.data_ptr())
    torch.cuda.synchronize()
    L = api.lib()
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(d)), "svt_hip_rd_batch")
    hip_ctx.check(L.svt_hip_ssim_batch(hip_ctx._h, C.byref(s)), "svt_hip_ssim_batch")
    hip_ctx.sync()
    recon = t_rec.cpu().numpy().view(dt).reshape(H, W)
    assert not np.array_equal(recon, pred)  # the RD batch did write the reconstruction
    want = sc.run_jobs(oracle, src, recon, sjobs, bd, 1.0)
    assert np.array_equal(sc.bits(t_ssim.cpu().numpy()), sc.bits(want["ssim"]))
    assert np.array_equal(t_dist.cpu().numpy().view(np.uint64), want["ssim_dist"])
