"""GPU: the chroma-from-luma candidate through the whole device chain on one stream, no host copy in between:
svt_hip_intra_pred_batch (DC chroma) -> svt_hip_cfl_pred_batch (33 slots x 2 planes) -> svt_hip_rd_batch (pred_offset per slot) ->
svt_hip_coeff_rate_batch (plane_type 1) -> svt_hip_cfl_pick_alpha_batch, against the same chain on the CPU: the restatements of
tests/intra_pred_cases.py, tests/cfl_cases.py and tests/coeff_rate_cases.py and the RD oracle (oracle/pyoracle.py)."""
import ctypes as C

import numpy as np
import pytest

import cfl_cases as cc
import coeff_rate_cases as cr
import intra_pred_cases as ic
from svt_av1_psyex_amd import abi, api, cfl, intra, rate, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5
COLS, ROWS = 6, 4  # of chroma blocks: two dozen
TX_OF = {(8, 8): 1, (4, 16): 13}  # TX_8X8, TX_4X16


def build(w, h, bd):
    """the picture (a luma reconstruction, two chroma sources in one buffer), the jobs of the four batches with jobs, the shared values"""
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    rng = np.random.default_rng(8800 + w + 10 * h + bd)
    pad = 16  # chroma samples around the blocks: the DC prediction reads the row above and the column on the left
    cw, ch = COLS * w + 2 * pad, ROWS * h + 2 * pad
    yy, xx = np.mgrid[0:2 * ch, 0:2 * cw]
    luma = np.clip(mx * (0.5 + 0.3 * np.sin(xx / 11.0) * np.cos(yy / 7.0)) + rng.integers(-mx // 40, mx // 40 + 1, xx.shape), 0, mx).astype(dt)
    y2, x2 = np.mgrid[0:ch, 0:cw]
    src = np.stack([np.clip(mx * (0.5 + s * 0.25 * np.sin((2 * x2) / 11.0) * np.cos((2 * y2) / 7.0)) + rng.integers(-mx // 30, mx // 30 + 1, x2.shape), 0, mx)
                    for s in (1.0, -0.8)]).astype(dt)  # [2][ch][cw]: Cb follows the luma, Cr runs against it
    org = [(pad + bx * w, pad + by * h) for by in range(ROWS) for bx in range(COLS)]
    n = len(org)
    tx = TX_OF[(w, h)]
    plane_samples = ch * cw
    ijobs = np.zeros(n, ic.JOB_DTYPE)  # one DC_PRED job per block; the same jobs serve both planes
    for i, (x, y) in enumerate(org):
        ijobs[i] = ic.make_job(tx, ic.DC_PRED, (x, y), (w, 0, h, 0))
        ijobs[i]["dst_offset"] = y * cw + x
    cjobs = np.zeros(n, cc.JOB_DTYPE)
    slot = w * h
    for i, (x, y) in enumerate(org):
        cjobs[i]["luma_x"], cjobs[i]["luma_y"] = 2 * x, 2 * y
        cjobs[i]["dc_offset"] = y * cw + x
        cjobs[i]["dst_offset"] = i * cc.SLOTS * slot
    pred_plane = n * cc.SLOTS * slot  # samples of one plane's slots; the two planes lie back to back in one buffer
    types = [t for t in range(16) if cr.EXT_TX_USED[cr.ext_tx_set_type(tx, 0, 0)][t]]
    rjobs = np.zeros(n * 2 * cc.SLOTS, abi.JOB_DTYPE)  # in the alpha search's order: block, plane, slot
    rate_jobs = np.zeros(len(rjobs), abi.RATE_JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        for p in range(2):
            for k in range(cc.SLOTS):
                at = (i * 2 + p) * cc.SLOTS + k
                rjobs[at]["src_offset"] = p * plane_samples + y * cw + x
                rjobs[at]["pred_offset"] = p * pred_plane + int(cjobs[i]["dst_offset"][p]) + k * slot
                rjobs[at]["tx_type"] = types[i % len(types)]
                rate_jobs[at]["tx_type"], rate_jobs[at]["txb_skip_ctx"], rate_jobs[at]["dc_sign_ctx"] = rjobs[at]["tx_type"], 7 + (i + p) % 6, (i + 2 * p) % 3
                rate_jobs[at]["intra_dir"] = 13  # UV_CFL_PRED
    rows = np.stack([rd.quant_row_from_step(44 << (bd - 8), 58 << (bd - 8))])
    return dict(bd=bd, w=w, h=h, tx=tx, cw=cw, ch=ch, luma=luma, src=src, org=org, n=n, ijobs=ijobs, cjobs=cjobs, rjobs=rjobs, rate_jobs=rate_jobs, rows=rows,
                slot=slot, pred_plane=pred_plane, lam=52000 if bd == 8 else 830000, itr_th=1 + (w == 4),
                mode_bits=rng.integers(900, 5000, n).astype(np.int32), fac=rng.integers(300, 4000, (8, 2, 16)).astype(np.int32))


def cpu_chain(s, tables, oracle):
    import pyoracle
    bd, w, h, n = s["bd"], s["w"], s["h"], s["n"]
    dt = s["src"].dtype
    dc = [np.full((s["ch"], s["cw"]), cc.fill_sample(bd, FILL), dt) for _ in range(2)]
    for p in range(2):
        for j, (x, y) in zip(s["ijobs"], s["org"]):
            dc[p][y:y + h, x:x + w] = ic.restate_job(s["src"][p], bd, 0, j)[0]
    b = {"bit_depth": bd, "width": w, "height": h, "alphas": cc.ALPHAS_FULL, "luma": s["luma"], "luma_size": (s["luma"].shape[1], s["luma"].shape[0]), "dc": dc,
         "jobs": s["cjobs"], "dst_samples": s["pred_plane"], "dst_stride": w, "slot_stride": s["slot"]}
    preds, _, _ = cc.restate_batch(b)
    pred = np.concatenate(cc.expected_dst(b, preds, FILL))
    f = dict(bit_depth=bd, quant_kind=0, tx_size=s["tx"], src_stride=s["cw"], pred_stride=w)
    want_r = pyoracle.rd_batch(f, np.ascontiguousarray(s["src"].reshape(-1)), pred, s["rjobs"], s["rows"], want_recon=False)
    c = {"tx_size": s["tx"], "plane": 1, "reduced": 0, "jobs": s["rate_jobs"], "qcoeff": want_r["qcoeff"], "eob": want_r["eob"].reshape(-1)}
    _, bits = cr.run_case(tables, c, variants=[(1, 0)])
    bits, dist = bits[0].reshape(n, 2, cc.SLOTS), want_r["dist_coeff"][:, 0].reshape(n, 2, cc.SLOTS)
    picks = [cc.pick_alpha(bb, dd, s["fac"], int(m), s["lam"], s["itr_th"]) for bb, dd, m in zip(bits, dist, s["mode_bits"])]
    return dc, pred, f, want_r, bits.reshape(-1), picks


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(8, 8), (4, 16)], ids=["8x8", "4x16"])
def test_chain_dc_cfl_rd_rate_pick_on_device(hip_ctx, oracle, size, bd):
    import torch
    L = api.lib()
    w, h = size
    s = build(w, h, bd)
    tables = cr.Tables.from_golden(np.load(cr.GOLDEN), 0)
    n, sb = s["n"], 2 if bd > 8 else 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = {k: dev(s[k]) for k in ("luma", "src", "ijobs", "cjobs", "rjobs", "rate_jobs", "rows", "mode_bits", "fac")}
    dev_tables = rate.upload_tables(tables)
    plane_bytes = s["ch"] * s["cw"] * sb
    t_src = [t["src"][p * plane_bytes:(p + 1) * plane_bytes] for p in range(2)]
    t_dc = [torch.full((plane_bytes,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    t_pred = torch.full((2 * s["pred_plane"] * sb,), FILL, dtype=torch.uint8, device="cuda")
    t_dst = [t_pred[p * s["pred_plane"] * sb:(p + 1) * s["pred_plane"] * sb] for p in range(2)]
    t_istatus = [torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    t_cstatus = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    nj, npk = len(s["rjobs"]), w * h
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    shapes["qcoeff"] = (np.dtype(np.int32), npk)
    r_out = {name: torch.zeros(nj * k * dt.itemsize, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    f = dict(bit_depth=bd, quant_kind=0, tx_size=s["tx"], src_stride=s["cw"], pred_stride=w)
    dr = abi.RdBatchDesc(n_jobs=nj, src=t["src"].data_ptr(), pred=t_pred.data_ptr(), recon=None, jobs=t["rjobs"].data_ptr(), quant_rows=t["rows"].data_ptr(),
                         n_quant_rows=1, **f)
    for name, tt in r_out.items():
        setattr(dr, name, tt.data_ptr())
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream

    for p in range(2):  # 1: DC chroma from the source's neighbours (open loop)
        intra.run_intra_pred_device(hip_ctx, bd, 0, t_src[p], s["cw"], s["cw"], s["ch"], t_dc[p], s["cw"], t["ijobs"], n, t_istatus[p])
    # 2: 33 slots x 2 planes
    cfl.run_cfl_pred_device(hip_ctx, bd, w, h, cc.ALPHAS_FULL, t["luma"], s["luma"].shape[1], s["luma"].shape[1], s["luma"].shape[0], t_dc, s["cw"], t_dst, w,
                            s["slot"], t["cjobs"], n, t_cstatus)
    # 3: transform, quantizer, distortion of every slot
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")
    # 4: the rate, chroma
    res = rate.run_rate_device(hip_ctx, dev_tables, s["tx"], 1, t["rate_jobs"], nj, r_out["qcoeff"], r_out["eob"])
    # 5: the alpha search over bits and the first column of dist_coeff in place
    picked = cfl.run_pick_device(hip_ctx, n, res["bits"], r_out["dist_coeff"], t["mode_bits"], t["fac"], s["lam"], s["itr_th"], 16, dist_stride=2)
    hip_ctx.sync()  # the one synchronisation

    want_dc, want_pred, f2, want_r, want_bits, picks = cpu_chain(s, tables, oracle)
    assert f2 == f
    dt = s["src"].dtype
    for p in range(2):
        assert np.all(t_istatus[p].cpu().numpy() == ic.ST_OK)
        assert np.array_equal(t_dc[p].cpu().numpy().view(dt).reshape(s["ch"], s["cw"]), want_dc[p]), f"DC plane {p}"
    assert np.all(t_cstatus.cpu().numpy() == cc.ST_OK)
    assert np.array_equal(t_pred.cpu().numpy().view(dt), want_pred), "the CfL slots"
    for name, (d_t, k) in shapes.items():
        assert np.array_equal(r_out[name].cpu().numpy().view(d_t).reshape(nj, k), want_r[name].reshape(nj, k)), name
    assert np.array_equal(rate.download(res)["bits"], want_bits)
    got = cfl.download_pick(picked)
    assert [int(v) for v in got["best_rd"]] == [r["best_rd"] for r in picks]
    assert [int(v) for v in got["cfl_alpha_idx"]] == [r["idx"] for r in picks]
    assert [int(v) for v in got["cfl_alpha_signs"]] == [r["signs"] for r in picks]
    assert np.all(got["status"] == 0)
    # the chain has something to decide: coefficients survive, and the blocks do not all choose one pair
    assert np.count_nonzero(want_r["eob"] > 1) > nj // 4
    assert len({(r["idx"], r["signs"]) for r in picks}) >= 4 and all(r["found"] for r in picks)
