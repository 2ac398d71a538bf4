"""GPU: svt_hip_intra_pred_batch on the MI355X, every comparison exact -- against the reference's own results (golden/intra_pred.npz) and the
restatement (tests/intra_pred_cases.py) for the five case groups, with the whole destination plane, the spare status slots and the neighbour
plane guarded; the jobs the entry defines itself (status 0xFF), job counts that leave lanes, waves and workgroups empty, a sentinel band around
the neighbour plane, rejected descriptors, DC_PRED against the TPL dispenser's, and the chain intra prediction -> RD batch -> rate batch on one
stream."""
import ctypes as C

import numpy as np
import pytest

import coeff_rate_cases as cr
import intra_pred_cases as ic
import tpl_dispenser_cases as tc
from svt_av1_psyex_amd import abi, api, intra, rate, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5
SPARE = 5


@pytest.fixture(scope="module")
def golden():
    return np.load(ic.GOLDEN)


def run(ctx, b, jobs=None, nbr=None, nbr_size=None):
    """the batch (or `jobs` of it) on a destination and a status array pre-filled with 0xA5: checks that the spare status slots and the
    neighbour plane are as they were; returns (destination plane, status)"""
    jobs = b["jobs"] if jobs is None else jobs
    nbr = ic.plane(b["plane"], b["bit_depth"]) if nbr is None else nbr
    out = intra.run_intra_pred_hip(ctx, b["bit_depth"], b["disable_edge_filter"], nbr, jobs, b["dst_shape"], b["dst_stride"], spare_jobs=SPARE, fill=FILL,
                                   nbr_size=nbr_size)
    n = len(jobs)
    assert len(out["status"]) == n + SPARE and np.all(out["status"][n:] == FILL), "spare status slots written"
    assert np.array_equal(out["nbr"], nbr), "the neighbour plane changed"
    return out["dst"], out["status"][:n]


def check(ctx, golden, name):
    """device == restatement on every sample of the destination (so every sample outside the jobs' blocks is still 0xA5) == the fixture"""
    b = ic.batch(name)
    want, _ = ic.restated(name)
    img, status = run(ctx, b)
    assert np.all(status == ic.ST_OK), name
    got = [ic.block_of(b, img, j) for j in b["jobs"]]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
    assert not bad, (name, bad[:8], [(int(b["jobs"][i]["mode"]), int(b["jobs"][i]["angle_delta"])) for i in bad[:8]])
    assert np.array_equal(img, ic.expected_image(b, want, FILL)), f"{name}: a sample outside the jobs' blocks was written"
    assert np.array_equal(ic.batch_crcs(got), golden[f"crc_{name}"]), name


@pytest.mark.parametrize("bd", [8, 10])
def test_group1_every_size_non_directional_mode_and_availability(hip_ctx, golden, bd):
    check(hip_ctx, golden, f"nondir_{bd}")


@pytest.mark.parametrize("tx", range(ic.N_TX), ids=lambda tx: f"{ic.TX_W[tx]}x{ic.TX_H[tx]}")
def test_group2_all_56_angles_both_filt_types_edge_filter_on_and_off(hip_ctx, golden, tx):
    for bd in (8, 10):
        for ef in (1, 0):
            check(hip_ctx, golden, f"dir_tx{tx}_{bd}_ef{ef}")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", ["fi", "extreme_zero", "extreme_max", "extreme_checker", "extreme_ramp", "geometry_stride204", "geometry_stride203"])
def test_groups_3_to_5(hip_ctx, golden, group, bd):
    """filter-intra (five modes, every size up to 32x32, four availabilities), the extreme planes, the geometry (plane corners, odd nbr_x,
    destination pitches and offsets)"""
    kind, _, rest = group.partition("_")
    check(hip_ctx, golden, f"fi_{bd}" if kind == "fi" else (f"extreme_{rest}_{bd}" if kind == "extreme" else f"geometry_{bd}_{rest}"))


def test_sample_blocks_equal_the_fixture(hip_ctx, golden):
    imgs = {}
    for key, name, i in ic.sample_jobs():
        b = ic.batch(name)
        if name not in imgs:
            imgs[name] = run(hip_ctx, b)[0]
        assert np.array_equal(ic.block_of(b, imgs[name], b["jobs"][i]), golden[key]), key


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_report_0xff_write_nothing_else_and_leave_their_neighbours(hip_ctx, bd):
    b, bad = ic.undefined_batch(bd)
    nbr = ic.plane(b["plane"], bd)
    n_dst = b["dst_shape"][0] * b["dst_stride"]
    defined = [ic.job_defined(j, ic.NBR_W, ic.NBR_H, n_dst, b["dst_stride"]) for j in b["jobs"]]
    assert [i for i, ok in enumerate(defined) if not ok] == bad and len(bad) == 22
    img, status = run(hip_ctx, b)
    assert np.array_equal(status, np.where(defined, ic.ST_OK, ic.ST_UNDEFINED))
    zero = np.zeros((1, 1), np.uint16)
    want = [ic.restate_job(nbr, bd, 0, j)[0] if ok else zero for j, ok in zip(b["jobs"], defined)]
    # the whole plane: the ordinary jobs exact, the undefined jobs' blocks and everything else still 0xA5
    assert np.array_equal(img, ic.expected_image(b, want, FILL, defined))


@pytest.mark.parametrize("n,name", [(1, "dir_tx0_8_ef1"), (3, "dir_tx0_10_ef1"), (5, "dir_tx0_8_ef0"), (63, "dir_tx0_10_ef1"), (65, "dir_tx0_8_ef1"),
                                    (1, "dir_tx4_10_ef1"), (3, "dir_tx4_8_ef1")])
def test_job_counts_that_leave_lanes_waves_and_workgroups_empty(hip_ctx, n, name):
    b = ic.batch(name)
    jobs = b["jobs"][7:7 + n]
    want, _ = ic.restated(name)
    img, status = run(hip_ctx, b, jobs)
    assert np.all(status == ic.ST_OK)
    assert np.array_equal(img, ic.expected_image(dict(b, jobs=jobs), want[7:7 + n], FILL))
    assert np.any(img != (FILL * 0x0101 if b["bit_depth"] > 8 else FILL))


def test_no_jobs_enqueue_nothing(hip_ctx):
    b = ic.batch("fi_8")
    img, status = run(hip_ctx, b, b["jobs"][:0])
    assert np.all(img == FILL) and len(status) == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_the_band_around_the_neighbour_plane_is_never_read(hip_ctx, bd):
    """the picture sits in a band of sentinel samples; the blocks on its first row / column have the count of that side 0, the blocks at its
    right / bottom end no top-right / bottom-left.  The same jobs on the same picture without the band give the restatement's blocks, which do
    not know the sentinel: equal results mean it was never read.  The plane the kernel is told of is the band's: the test is about what the
    counts make it read, not about the bounds check."""
    g = ic.batch(f"geometry_{bd}_stride204")
    pic = ic.plane("noise", bd)
    band = 8
    big = np.full((ic.NBR_H + 2 * band, ic.NBR_W + 2 * band), 0x3C3 if bd > 8 else 0xC3, pic.dtype)
    big[band:-band, band:-band] = pic
    jobs = g["jobs"].copy()
    jobs["nbr_x"] += band
    jobs["nbr_y"] += band
    edge = [i for i, j in enumerate(g["jobs"]) if int(j["nbr_x"]) == 0 or int(j["nbr_y"]) == 0]
    assert len(edge) > 100
    img, status = run(hip_ctx, g, jobs, nbr=big)
    assert np.all(status == ic.ST_OK)
    assert np.array_equal(img, ic.expected_image(g, ic.restated(g["name"])[0], FILL))


@pytest.mark.parametrize("bad", ["bit_depth_12", "zero_stride", "stride_below_width", "no_nbr", "no_status", "no_jobs", "zero_dst_stride", "dst_inside_nbr"])
def test_rejected_descriptor_returns_non_zero_and_leaves_the_buffers_as_filled(hip_ctx, bad):
    import torch
    fill = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    bufs = {"nbr": fill(2 * 256 * 144), "dst": fill(2 * 256 * 64), "jobs": fill(24 * 6), "status": fill(6)}
    d = abi.IntraPredDesc(bit_depth=10, n_jobs=6, nbr=bufs["nbr"].data_ptr(), nbr_stride=256, nbr_width=208, nbr_height=144, dst=bufs["dst"].data_ptr(),
                          dst_stride=256, dst_samples=256 * 64, jobs=bufs["jobs"].data_ptr(), status=bufs["status"].data_ptr())
    ic.spoil_desc(d, bad)
    torch.cuda.synchronize()
    assert api.lib().svt_hip_intra_pred_batch(hip_ctx._h, C.byref(d)) == 2
    assert b"svt_hip_intra_pred_check_desc" in api.lib().svt_hip_last_error(None)
    hip_ctx.sync()
    for name, t in bufs.items():
        assert bool(torch.all(t == FILL)), name


def test_dc_pred_16x16_equals_the_tpl_dispensers_dc(hip_ctx):
    """DC_PRED on 16x16 blocks with both edges available against tests/tpl_dispenser_cases.py's dc_pred (the TPL kernels' DC) on the same
    padded 8-bit plane"""
    W, H, pad, S = 96, 64, tc.PAD, 16
    rng = np.random.default_rng(1600)
    padded = rng.integers(0, 256, (H + 2 * pad, W + 2 * pad)).astype(np.uint8)
    org = [(x, y) for y in range(S, H - S + 1, S) for x in range(S, W - S + 1, S)]
    jobs = [ic.make_job(2, ic.DC_PRED, (x + pad, y + pad), (S, 0, S, 0)) for x, y in org]
    b = ic.finish("dc_tpl", 8, "noise", 0, jobs)
    img, status = run(hip_ctx, b, nbr=padded)
    assert np.all(status == ic.ST_OK)
    for j, (x, y) in zip(b["jobs"], org):
        blk = ic.block_of(b, img, j)
        assert np.all(blk == tc.dc_pred(padded, x, y, S, W, H, pad)), (x, y)


FIMODE_TO_INTRADIR = [ic.DC_PRED, ic.V_PRED, ic.H_PRED, ic.D157_PRED, ic.DC_PRED]  # fimode_to_intradir


@pytest.mark.parametrize("size,tx_size", [(8, 1), (16, 2), (64, 4)])
def test_chain_intra_prediction_rd_batch_rate_batch_on_device(hip_ctx, oracle, size, tx_size):
    """svt_hip_intra_pred_batch writes the prediction plane from the source plane's neighbours (open loop), svt_hip_rd_batch reads that plane,
    svt_hip_coeff_rate_batch prices the coefficients with is_inter = 0 and the job's intra_dir: the same device buffers, the context stream, one
    synchronisation at the end.  Against the restatement followed by oracle/pyoracle.py's RD batch and the rate restatement."""
    import pyoracle
    import torch
    L = api.lib()
    golden_rate = np.load(cr.GOLDEN)
    tables = cr.Tables.from_golden(golden_rate, 0)
    W, H = 192, 128
    rng = np.random.default_rng(1700 + size)
    yy, xx = np.mgrid[0:H, 0:W]
    src = np.clip(120 + 60 * np.sin(xx / 9.0) + 50 * np.cos(yy / 7.0) + rng.integers(-12, 13, (H, W)), 0, 255).astype(np.uint8)
    org = [(x, y) for y in range(size, H - size + 1, size) for x in range(size, W - 2 * size + 1, size)][:60]
    n = len(org)
    kinds = [(ic.D113_PRED, 2, ic.NO_FI), (ic.SMOOTH_PRED, 0, ic.NO_FI), (ic.DC_PRED, 0, 3 if size <= 32 else ic.NO_FI)]
    pjobs = np.zeros(n, ic.JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        mode, delta, fim = kinds[i % 3]
        pjobs[i] = ic.make_job(tx_size, mode, (x, y), (size, 0 if fim != ic.NO_FI else size, size, 0), delta, fim, i & 1)
        pjobs[i]["dst_offset"] = y * W + x
    assert {int(f) != ic.NO_FI for f in pjobs["filter_intra_mode"]} == ({True, False} if size <= 32 else {False})
    rjobs = np.zeros(n, abi.JOB_DTYPE)
    rjobs["src_offset"] = rjobs["pred_offset"] = [y * W + x for x, y in org]
    types = [t for t in range(16) if cr.EXT_TX_USED[cr.ext_tx_set_type(tx_size, 0, 0)][t]]
    rjobs["tx_type"] = [types[i % len(types)] for i in range(n)]
    cjobs = np.zeros(n, abi.RATE_JOB_DTYPE)
    cjobs["tx_type"], cjobs["txb_skip_ctx"], cjobs["dc_sign_ctx"], cjobs["is_inter"] = rjobs["tx_type"], np.arange(n) % 13, np.arange(n) % 3, 0
    cjobs["intra_dir"] = [int(j["mode"]) if int(j["filter_intra_mode"]) == ic.NO_FI else FIMODE_TO_INTRADIR[int(j["filter_intra_mode"])] for j in pjobs]
    rows = np.stack([rd.quant_row_from_step(40, 52)])
    f = dict(bit_depth=8, quant_kind=0, tx_size=tx_size, src_stride=W, pred_stride=W)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = {k: dev(v) for k, v in dict(src=src, pjobs=pjobs, rjobs=rjobs, cjobs=cjobs, rows=rows).items()}
    dev_tables = rate.upload_tables(tables)
    t_pred = torch.full((H * W,), FILL, dtype=torch.uint8, device="cuda")
    t_status = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    npk = min(size, 32) ** 2
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    shapes["qcoeff"] = (np.dtype(np.int32), npk)
    r_out = {name: torch.zeros(n * k * dt.itemsize, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    dr = abi.RdBatchDesc(n_jobs=n, src=t["src"].data_ptr(), pred=t_pred.data_ptr(), recon=None, jobs=t["rjobs"].data_ptr(), quant_rows=t["rows"].data_ptr(),
                         n_quant_rows=1, **f)
    for name, tt in r_out.items():
        setattr(dr, name, tt.data_ptr())
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream
    intra.run_intra_pred_device(hip_ctx, 8, 0, t["src"], W, W, H, t_pred, W, t["pjobs"], n, t_status)
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")
    lam = 41000
    res = rate.run_rate_device(hip_ctx, dev_tables, tx_size, 0, t["cjobs"], n, r_out["qcoeff"], r_out["eob"], lam=lam, dist=r_out["dist_coeff"], dist_stride=2)
    hip_ctx.sync()  # the one synchronisation

    want_blocks = [ic.restate_job(src, 8, 0, j)[0] for j in pjobs]
    b = {"bit_depth": 8, "dst_shape": (H, W), "dst_stride": W, "jobs": pjobs}
    want_pred = ic.expected_image(b, want_blocks, FILL)
    assert np.all(t_status.cpu().numpy() == ic.ST_OK)
    assert np.array_equal(t_pred.cpu().numpy().reshape(H, W), want_pred)
    want_r = pyoracle.rd_batch(f, src, want_pred, rjobs, rows, want_recon=False)
    for name, (dt, k) in shapes.items():
        assert np.array_equal(r_out[name].cpu().numpy().view(dt).reshape(n, k), want_r[name].reshape(n, k)), name
    assert np.count_nonzero(want_r["eob"] > 1) > n // 2
    c = {"tx_size": tx_size, "plane": 0, "reduced": 0, "jobs": cjobs, "qcoeff": want_r["qcoeff"], "eob": want_r["eob"].reshape(-1)}
    _, bits = cr.run_case(tables, c, variants=[(1, 0)])
    got = rate.download(res)
    assert np.array_equal(got["bits"], bits[0])
    want_cost = np.array([cr.rdcost(lam, int(bb), int(dd)) for bb, dd in zip(bits[0], want_r["dist_coeff"][:, 0])], np.uint64)
    assert np.array_equal(got["rd_cost"], want_cost)
