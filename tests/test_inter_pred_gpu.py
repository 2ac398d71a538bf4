"""GPU: svt_hip_inter_pred_batch on the MI355X, every comparison exact -- against the reference's own results (golden/inter_pred.npz) and the
restatement (tests/inter_pred_cases.py) for the six case groups, with guards around every block, status slot and reference plane; the jobs
the entry defines itself (status 0xFF), job counts that leave lanes, groups and waves empty, rejected descriptors, source coordinates outside
the padded plane, the full-pel case against svt_hip_fullpel_pred, and the chain sub-pel search -> prediction -> RD batch on one stream."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
import md_search_cases as mc
from svt_av1_psyex_amd import abi, api, pred, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5
SPARE = 5


@pytest.fixture(scope="module")
def golden():
    return np.load(ip.GOLDEN)


def run(ctx, b, jobs=None):
    """the batch (or `jobs` of it) on a destination and a status array pre-filled with 0xA5: checks that the spare status slots and the
    reference planes are as they were; returns (destination plane, status)"""
    jobs = b["jobs"] if jobs is None else jobs
    planes = ip.batch_planes(b)
    out = pred.run_inter_pred_hip(ctx, b["bit_depth"], b["ss"], b["ss"], planes, jobs, b["dst_shape"], b["dst_stride"], mv_array=b["mv_array"], spare_jobs=SPARE,
                                  fill=FILL)
    n = len(jobs)
    assert len(out["status"]) == n + SPARE and np.all(out["status"][n:] == FILL), "spare status slots written"
    for got, (p, _, _) in zip(out["planes"], planes):
        assert np.array_equal(got, p), "a reference plane changed"
    return out["dst"], out["status"][:n]


def blocks_of(b, img, jobs=None):
    out = []
    for j in (b["jobs"] if jobs is None else jobs):
        y, x = divmod(int(j["dst_offset"]), b["dst_stride"])
        out.append(img[y:y + int(j["height"]), x:x + int(j["width"])].astype(np.uint16))
    return out


def check(ctx, golden, name):
    """device == restatement on every sample of the destination (so every sample outside the jobs' blocks is still 0xA5) == the fixture"""
    b = ip.batch(name)
    want, _ = ip.restated(name)
    img, status = run(ctx, b)
    assert np.all(status == ip.ST_OK), name
    bad = [i for i, (g, w) in enumerate(zip(blocks_of(b, img), want)) if not np.array_equal(g, w)]
    assert not bad, (name, bad[:8])
    assert np.array_equal(img, ip.expected_image(b, want, FILL)), f"{name}: a sample outside the jobs' blocks was written"
    assert np.array_equal(ip.batch_crcs(name, blocks_of(b, img)), golden[f"crc_{name}"]), name


@pytest.mark.parametrize("size", ip.BLOCK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_group1_every_size_variant_mode_and_depth(hip_ctx, golden, size):
    """{copy, x, y, 2d} x {single, average, distance-weighted} x 8- / 10-bit, random MVs and dual filters; on the sub-sampled plane too (odd phases)"""
    w, h = size
    for bd in (8, 10):
        check(hip_ctx, golden, f"sizes_{w}x{h}_{bd}_ss0")
        if w <= 64 and h <= 64:
            check(hip_ctx, golden, f"sizes_{w}x{h}_{bd}_ss1")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", ip.SWEEP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_group2_all_256_phases_and_16_filter_pairs(hip_ctx, golden, size, bd):
    check(hip_ctx, golden, f"sweep_{size[0]}x{size[1]}_{bd}")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", ["compound", "clamp_ss0", "clamp_ss1", "extremes", "geometry_stride204", "geometry_stride203"])
def test_groups_3_to_6(hip_ctx, golden, group, bd):
    """compound (offset pairs, one and two planes, every pairing of variants), the clamp (luma and sub-sampled), the extreme planes with the
    sharp filter, destination strides and offsets"""
    kind, _, rest = group.partition("_")
    check(hip_ctx, golden, f"{kind}_{bd}" + (f"_{rest}" if rest else ""))


def test_sample_blocks_equal_the_fixture(hip_ctx, golden):
    for bd in (8, 10):
        b = ip.batch(f"sizes_16x16_{bd}_ss0")
        got = blocks_of(b, run(hip_ctx, b)[0])
        for key, name, i in ip.sample_jobs():
            if name == b["name"]:
                assert np.array_equal(got[i], golden[key]), key


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_report_0xff_write_nothing_else_and_leave_their_neighbours(hip_ctx, bd):
    b, bad = ip.undefined_batch(bd)
    planes = ip.batch_planes(b)
    n_dst = b["dst_shape"][0] * b["dst_stride"]
    defined = [ip.job_defined(j, len(planes), b["mv_array"], n_dst, b["dst_stride"]) for j in b["jobs"]]
    assert [i for i, ok in enumerate(defined) if not ok] == bad and len(bad) == 24
    img, status = run(hip_ctx, b)
    assert np.array_equal(status, np.where(defined, ip.ST_OK, ip.ST_UNDEFINED))
    zero = np.zeros((1, 1), np.uint16)
    want = [ip.restate_job(planes, bd, b["ss"], j, b["mv_array"])[0] if ok else zero for j, ok in zip(b["jobs"], defined)]
    # the whole plane: the ordinary jobs exact, the undefined jobs' blocks and everything else still 0xA5
    assert np.array_equal(img, ip.expected_image(b, want, FILL, defined))
    assert b["jobs"][-1]["flags"] == 3 and defined[-1]  # both MVs from mv_array


@pytest.mark.parametrize("n,name", [(1, "sweep_4x4_8"), (3, "sweep_4x4_10"), (5, "sweep_4x4_8"), (63, "sweep_4x4_10"), (65, "sweep_4x4_8"),
                                    (1, "sizes_128x128_10_ss0"), (3, "sizes_128x128_8_ss0")])
def test_job_counts_that_leave_lanes_and_waves_empty(hip_ctx, n, name):
    b = ip.batch(name)
    jobs = b["jobs"][7:7 + n]
    want, _ = ip.restated(name)
    img, status = run(hip_ctx, b, jobs)
    assert np.all(status == ip.ST_OK)
    sub = dict(b, jobs=jobs)
    assert np.array_equal(img, ip.expected_image(sub, want[7:7 + n], FILL))
    assert np.any(img != (FILL * 0x0101 if b["bit_depth"] > 8 else FILL))


def test_no_jobs_enqueue_nothing(hip_ctx):
    b = ip.batch("sizes_8x8_8_ss0")
    img, status = run(hip_ctx, b, b["jobs"][:0])
    assert np.all(img == FILL) and len(status) == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_source_coordinates_outside_the_padded_plane_are_clamped(hip_ctx, bd):
    """defined where the reference is not: edges that let the MV through, MVs that take the block and its filter reach past every side of the
    plane (and of a plane without padding)"""
    rng = np.random.default_rng(40 + bd)
    jobs = []
    for w, h in ((4, 4), (8, 8), (16, 16), (32, 16), (64, 64)):
        for mv in ((-1500, -3000), (-1500, 3000), (1500, 3000), (1500, -3000), (-1281, 5), (7, -2555), (1411, -9), (3, 2899), (-1290, 2893)):
            for refs in ((0, ip.NO_REF), (1, 0)):
                j = ip.make_job(0, w, h, ip.random_org(rng, 0, w, h), [mv, (mv[1] // 2, mv[0])], (int(rng.integers(0, 4)), int(rng.integers(0, 4))), refs,
                                int(rng.integers(0, 2)), ip.DIST_PAIRS[int(rng.integers(0, 8))])
                j["mb_to_left_edge"], j["mb_to_top_edge"] = -(1 << 20), -(1 << 20)
                j["mb_to_right_edge"], j["mb_to_bottom_edge"] = 1 << 20, 1 << 20
                jobs.append(j)
    b = ip.finish(f"outside_{bd}", bd, 0, ip.NOISE2, jobs)
    planes = ip.batch_planes(b)
    res = [ip.restate_job(planes, bd, 0, j) for j in b["jobs"]]
    assert sum(not e["inside"] for _, e in res) > len(jobs) // 2
    img, status = run(hip_ctx, b)
    assert np.all(status == ip.ST_OK)
    assert np.array_equal(img, ip.expected_image(b, [r[0] for r in res], FILL))


@pytest.mark.parametrize("bad", ["bit_depth_12", "ss_x_2", "n_refs_9", "zero_stride", "null_plane", "no_status", "no_jobs", "zero_dst_stride"])
def test_rejected_descriptor_returns_non_zero_and_leaves_the_buffers_as_filled(hip_ctx, bad):
    import torch
    fill = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    bufs = {"plane": fill(2 * 512 * 448), "dst": fill(2 * 256 * 64), "jobs": fill(56 * 6), "status": fill(6), "mv_array": fill(4 * 6)}
    d = abi.InterPredDesc(bit_depth=10, ss_x=0, ss_y=0, n_refs=2, n_jobs=6, dst=bufs["dst"].data_ptr(), dst_stride=256, dst_samples=256 * 64,
                          jobs=bufs["jobs"].data_ptr(), status=bufs["status"].data_ptr(), mv_array=bufs["mv_array"].data_ptr(), n_mvs=6)
    for i in range(2):
        d.refs[i] = pred.plane_ref(bufs["plane"], 512, 160, 160, 512, 448)
    ip.spoil_desc(d, bad)
    torch.cuda.synchronize()
    assert api.lib().svt_hip_inter_pred_batch(hip_ctx._h, C.byref(d)) == 2
    assert b"svt_hip_inter_pred_check_desc" in api.lib().svt_hip_last_error(None)
    hip_ctx.sync()
    for name, t in bufs.items():
        assert bool(torch.all(t == FILL)), name


@pytest.mark.parametrize("bd", [8, 10])
def test_full_pel_mvs_equal_svt_hip_fullpel_pred(hip_ctx, bd):
    """the 16x16 PUs of a 128x128 picture: the new entry on an unpadded plane (its coordinate clamp is the copy kernel's edge replication)
    against svt_hip_fullpel_pred on the same plane and vectors"""
    import torch
    w = h = 128
    rng = np.random.default_rng(90 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    ref = rng.integers(0, 1 << bd, (h, w)).astype(dt)
    nb = 4
    mvx, mvy = rng.integers(-70, 71, (nb, 8, 85)), rng.integers(-70, 71, (nb, 8, 85))
    mvx[::3] = rng.integers(-1900, 1900, mvx[::3].shape)  # far outside the picture: pure edge replication
    mv = ((mvy.astype(np.int64) & 0xFFFF) << 16 | (mvx.astype(np.int64) & 0xFFFF)).astype(np.uint32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t_ref, t_mv = dev(ref), dev(mv)
    t_old = torch.zeros(h * w * ref.itemsize, dtype=torch.uint8, device="cuda")
    lst, ri = 1, 2
    jobs = []
    for y0 in range(0, h, 16):
        for x0 in range(0, w, 16):
            b64 = (x0 >> 6) + (y0 >> 6) * 2
            qx, qy = (x0 >> 4) & 3, (y0 >> 4) & 3
            z = (qx & 1) | ((qy & 1) << 1) | ((qx >> 1) << 2) | ((qy >> 1) << 3)
            j = ip.make_job(0, 16, 16, (x0, y0), [(int(mvy[b64, lst * 4 + ri, 5 + z]) * 8, int(mvx[b64, lst * 4 + ri, 5 + z]) * 8)], (2, 1))
            j["mb_to_left_edge"], j["mb_to_top_edge"], j["mb_to_right_edge"], j["mb_to_bottom_edge"] = -(1 << 20), -(1 << 20), 1 << 20, 1 << 20
            j["dst_offset"] = y0 * w + x0
            jobs.append(j)
    torch.cuda.synchronize()
    assert api.lib().svt_hip_fullpel_pred(hip_ctx._h, C.c_void_p(t_ref.data_ptr()), w, w, h, bd, C.c_void_p(t_mv.data_ptr()), lst, ri, 0, 0,
                                          C.c_void_p(t_old.data_ptr()), w) == 0
    new = pred.run_inter_pred_hip(hip_ctx, bd, 0, 0, [(ref, 0, 0)], np.array(jobs, ip.JOB_DTYPE), (h, w), fill=FILL)
    old = t_old.cpu().numpy().view(dt).reshape(h, w)
    assert np.all(new["status"] == ip.ST_OK)
    assert np.array_equal(new["dst"], old)
    assert np.any(old != ref)


@pytest.mark.parametrize("size,tx_size,si", [(8, 1, 1), (16, 2, 6), (64, 4, 1)])
def test_chain_subpel_search_prediction_rd_batch_on_device(hip_ctx, oracle, size, tx_size, si):
    """svt_hip_md_subpel_batch writes best_mv, svt_hip_inter_pred_batch takes every job's MV from it (the mv_array flag) and writes the prediction
    plane, svt_hip_rd_batch reads that plane: the same device buffers, the context stream, one synchronisation at the end.  Against
    oracle/pyoracle.py's sub-pel search and RD batch with the restatement in between."""
    import pyoracle
    import torch
    L = api.lib()
    W, H, PAD = mc.W, mc.H, mc.PAD
    rng = np.random.default_rng(700 + size)
    src, refp = mc.planes(31 + size)
    tables = mc.cost_tables(rng)
    setting = mc.SUBPEL_SETTINGS[si]
    org = [(x, y) for y in range(32, H - 32 - size + 1, size) for x in range(32, W - 32 - size + 1, size)][:96]
    n = len(org)
    sjobs = np.zeros(n, abi.SUBPEL_JOB_DTYPE)
    pjobs = np.zeros(n, ip.JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        j = sjobs[i]
        j["src_offset"], j["ref_offset"] = y * W + x, (y + PAD) * (W + 2 * PAD) + x + PAD
        j["width"], j["height"], j["log2_pels"] = size, size, int(np.log2(size * size))
        smv = rng.integers(-4, 5, 2) * 8
        j["start_mv"], j["ref_mv"] = smv, smv + rng.integers(-30, 31, 2)
        j["col_min"], j["col_max"], j["row_min"], j["row_max"] = smv[1] - 2000, smv[1] + 2000, smv[0] - 2000, smv[0] + 2000
        j["early_exit_th"] = 1020 - (size >> 2)
        j["best_mvp"] = smv
        p = ip.make_job(0, size, size, (x, y), [(0, 0)], (i & 3, (i >> 2) & 3))
        p["mb_to_right_edge"], p["mb_to_bottom_edge"] = (W - size - x) * 8, (H - size - y) * 8
        p["flags"], p["mv_index"][0], p["dst_offset"] = ip.MV0_FROM_ARRAY, i, y * W + x
        pjobs[i] = p
    rjobs = np.zeros(n, abi.JOB_DTYPE)
    rjobs["src_offset"] = rjobs["pred_offset"] = [y * W + x for x, y in org]
    rjobs["tx_type"] = np.arange(n) % 2 if size <= 16 else 0  # a 64-point transform is DCT_DCT alone
    rows = np.stack([rd.quant_row_from_step(40, 52)])
    f = dict(bit_depth=8, quant_kind=0, tx_size=tx_size, src_stride=W, pred_stride=W)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    jc, tr, tc = tables
    t = {k: dev(v) for k, v in dict(src=src, ref=refp, jc=jc, tr=tr, tc=tc, sjobs=sjobs, pjobs=pjobs, rjobs=rjobs, rows=rows).items()}
    t_mv = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    s_out = {k: torch.zeros(n, dtype=torch.int32, device="cuda") for k in ("besterr", "distortion", "sse", "center_err")}
    t_pred = torch.full((H * W,), FILL, dtype=torch.uint8, device="cuda")
    t_status = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    r_out = {name: torch.zeros(n * k * dt.itemsize, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    hp, stop, iters, pvt, atm, rdt, sdr, bias, ctype, method, taps, mvp_th, hp_mv_th = mc.full_setting(setting)
    ds = abi.SubpelBatchDesc(n_jobs=n, src_stride=W, ref_stride=W + 2 * PAD, src=t["src"].data_ptr(), ref=t["ref"].data_ptr(), jobs=t["sjobs"].data_ptr(),
                             allow_hp=hp, forced_stop=stop, iters_per_step=iters, pred_variance_th=pvt, abs_th_mult=atm, round_dev_th=rdt,
                             skip_diag_refinement=sdr, bias_fp=bias, qp=36, search_method=method, subpel_search_type=taps, mvp_th=mvp_th, hp_mv_th=hp_mv_th,
                             mv_cost_type=ctype, error_per_bit=41, mvjcost=t["jc"].data_ptr(), best_mv=t_mv.data_ptr(),
                             **{k: v.data_ptr() for k, v in s_out.items()})
    ds.mvcost[0], ds.mvcost[1] = t["tr"].data_ptr() + 4 * mc.MV_CENTRE, t["tc"].data_ptr() + 4 * mc.MV_CENTRE
    dr = abi.RdBatchDesc(n_jobs=n, src=t["src"].data_ptr(), pred=t_pred.data_ptr(), recon=None, jobs=t["rjobs"].data_ptr(), quant_rows=t["rows"].data_ptr(),
                         n_quant_rows=1, **f)
    for name, tt in r_out.items():
        setattr(dr, name, tt.data_ptr())
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream
    hip_ctx.check(L.svt_hip_md_subpel_batch(hip_ctx._h, C.byref(ds)), "svt_hip_md_subpel_batch")
    pred.run_inter_pred_device(hip_ctx, 8, 0, 0, [pred.plane_ref(t["ref"], W + 2 * PAD, PAD, PAD, W + 2 * PAD, H + 2 * PAD)], t_pred, W, t["pjobs"], n, t_status,
                               mv_array=t_mv, n_mvs=n)
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")
    hip_ctx.sync()  # the one synchronisation

    want_s = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, src, refp, sjobs, setting, 41, 36, tables)
    got_mv = t_mv.cpu().numpy().reshape(n, 2)
    assert np.array_equal(got_mv, want_s["best_mv"])
    assert np.count_nonzero(got_mv & 7) > n // 4  # fractional vectors: the chain is sensitive to the interpolation
    planes = [(refp, PAD, PAD)]
    want_blocks = [ip.restate_job(planes, 8, 0, j, want_s["best_mv"])[0] for j in pjobs]
    b = {"bit_depth": 8, "dst_shape": (H, W), "dst_stride": W, "jobs": pjobs}
    want_pred = ip.expected_image(b, want_blocks, FILL)
    got_pred = t_pred.cpu().numpy().reshape(H, W)
    assert np.all(t_status.cpu().numpy() == ip.ST_OK)
    assert np.array_equal(got_pred, want_pred)
    want_r = pyoracle.rd_batch(f, src, want_pred, rjobs, rows, want_coeffs=False, want_recon=False)
    for name, (dt, k) in shapes.items():
        assert np.array_equal(r_out[name].cpu().numpy().view(dt).reshape(n, k), want_r[name]), name
