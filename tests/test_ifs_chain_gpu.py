"""GPU: an inter candidate with a switchable filter through the device chain on one stream, no host look in between: svt_hip_md_subpel_batch ->
svt_hip_ifs_batch (MV from the search's array; the winner's luma goes to the prediction plane) -> svt_hip_ifs_scatter_filters (the chosen filters into
the chroma job records) -> svt_hip_inter_pred_batch on the sub-sampled plane (MV from the same array, filters from the scatter) -> svt_hip_rd_batch on
the luma prediction, on a handful of 16x16 blocks, against the same chain on the host: the sub-pel oracle, the restatements of tests/ifs_cases.py and
tests/inter_pred_cases.py and the RD oracle."""
import ctypes as C

import numpy as np
import pytest

import ifs_cases as ic
import inter_pred_cases as ip
import md_search_cases as mc
import warp_cases as wc
from svt_av1_psyex_amd import abi, api, ifs, pred, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5
PW, PH, PAD, B = 96, 64, 24, 16
PARAMS = dict(ic.PARAMS, psy_rd=0.9, lambda_=2000, spy_rd=1)


def build():
    rng = np.random.default_rng(2027)
    src, luma = wc.moving_planes(rng, PW, PH, pad=PAD)
    y2, x2 = np.mgrid[0:PH // 2 + 2 * PAD, 0:PW // 2 + 2 * PAD]
    cb = np.clip(128 + 60 * np.sin(x2 / 3.1 + y2 / 5.0) + rng.normal(0, 5, x2.shape), 0, 255).astype(np.uint8)
    org = [(16 * bx, 16 * by) for by in (0, 1, 3) for bx in (0, 2, 5)][:7]
    n = len(org)
    tables = mc.cost_tables(rng)
    stride = luma[0].shape[1]
    sjobs = np.zeros(n, abi.SUBPEL_JOB_DTYPE)
    ijobs = np.zeros(n, ic.JOB_DTYPE)
    cjobs = np.zeros(n, ip.JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        start = (int(rng.integers(-1, 2)) * 8 + 8, int(rng.integers(-1, 2)) * 8 - 16)
        j = sjobs[i]
        j["src_offset"], j["ref_offset"] = y * PW + x, (y + PAD) * stride + x + PAD
        j["width"], j["height"], j["log2_pels"], j["start_mv"], j["ref_mv"] = B, B, 8, start, (start[0] + int(rng.integers(-12, 13)), start[1] + int(rng.integers(-12, 13)))
        j["col_min"], j["col_max"], j["row_min"], j["row_max"] = start[1] - 40, start[1] + 40, start[0] - 40, start[0] + 40
        j["early_exit_th"], j["best_mvp"] = 1020 - (B >> 2), start
        for ss, jobs in ((0, ijobs["pred"]), (1, cjobs)):
            w = B >> ss
            p = ip.make_job(ss, w, w, (x >> ss, y >> ss), [(0, 0)], (3, 3))  # the filters: BILINEAR until something better is known
            p["mb_to_right_edge"], p["mb_to_bottom_edge"] = (PW - B - x) * 8, (PH - B - y) * 8
            p["flags"], p["mv_index"][0], p["dst_offset"] = ip.MV0_FROM_ARRAY, i, i * w * w
            jobs[i] = p
        ijobs[i]["src_offset"] = y * PW + x
        nbr = (None if i == 2 else (i % 3, (i + 1) % 3), (2 - i % 3, i % 2))
        ijobs[i]["pred_ctx"] = [ic.pred_context(False, d, nbr[0], nbr[1]) for d in (0, 1)]
    patches = np.zeros(n, abi.IFS_PATCH_DTYPE)
    patches["result_index"] = patches["record_index"] = np.arange(n)
    tjobs = np.zeros(n, abi.JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        tjobs[i]["src_offset"], tjobs[i]["pred_offset"], tjobs[i]["tx_type"] = y * PW + x, i * B * B, (0, 1, 2, 3, 9)[i % 5]
    rows = np.stack([rd.quant_row_from_step(40, 52)])
    return dict(src=src, luma=luma[0], cb=cb, n=n, tables=tables, sjobs=sjobs, ijobs=ijobs, cjobs=cjobs, patches=patches, tjobs=tjobs, rows=rows,
                fac=ic.fac_table("random"))


def host_chain(s, oracle):
    import pyoracle
    n = s["n"]
    a = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, s["src"], s["luma"], s["sjobs"], mc.SUBPEL_SETTINGS[0], 41, 36, s["tables"])
    res = [ic.restate_job([(s["luma"], PAD, PAD)], s["src"], 8, j, PARAMS, s["fac"], a["best_mv"]) for j in s["ijobs"]]
    luma = np.stack([r["pred"].astype(np.uint8) for r in res])
    cjobs = s["cjobs"].copy()
    cjobs["filter_x"], cjobs["filter_y"] = [r["filter_x"] for r in res], [r["filter_y"] for r in res]
    chroma = np.stack([ip.restate_job([(s["cb"], PAD, PAD)], 8, 1, j, a["best_mv"])[0].astype(np.uint8) for j in cjobs])
    f = dict(bit_depth=8, quant_kind=0, tx_size=2, src_stride=PW, pred_stride=B)
    want_r = pyoracle.rd_batch(f, np.ascontiguousarray(s["src"].reshape(-1)), np.ascontiguousarray(luma.reshape(-1)), s["tjobs"], s["rows"], want_recon=False)
    return a, res, luma, cjobs, chroma, f, want_r


def test_chain_subpel_ifs_scatter_chroma_rd_on_device(hip_ctx, oracle):
    import torch
    L = api.lib()
    s = build()
    n = s["n"]
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()
    t = {k: dev(s[k]) for k in ("src", "sjobs", "ijobs", "cjobs", "patches", "tjobs", "rows", "luma", "cb", "fac")}
    t_cost = [dev(x) for x in s["tables"]]
    filled = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    sp = {k: filled(n * 4) for k in ("best_mv", "besterr", "distortion", "sse", "center_err")}
    t_res, t_rd, t_sse = filled(n * np.dtype(abi.IFS_RESULT_DTYPE).itemsize), filled(n * 72), filled(n * 72)
    t_pred = {0: filled(n * B * B), 1: filled(n * B * B // 4)}
    t_st = {k: filled(n) for k in ("ifs", "scatter", "chroma")}
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    r_out = {name: torch.zeros(n * k * dt.itemsize, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    f = dict(bit_depth=8, quant_kind=0, tx_size=2, src_stride=PW, pred_stride=B)
    dr = abi.RdBatchDesc(n_jobs=n, src=t["src"].data_ptr(), pred=t_pred[0].data_ptr(), recon=None, jobs=t["tjobs"].data_ptr(), quant_rows=t["rows"].data_ptr(),
                         n_quant_rows=1, **f)
    for name, tt in r_out.items():
        setattr(dr, name, tt.data_ptr())
    hp, stop, iters, pvt, atm, rdt, sdr, bias, ctype, method, taps, mvp_th, hp_mv_th = mc.full_setting(mc.SUBPEL_SETTINGS[0])
    stride = s["luma"].shape[1]
    ds = abi.SubpelBatchDesc(n_jobs=n, src_stride=PW, ref_stride=stride, src=t["src"].data_ptr(), ref=t["luma"].data_ptr(), jobs=t["sjobs"].data_ptr(), allow_hp=hp,
                             forced_stop=stop, iters_per_step=iters, pred_variance_th=pvt, abs_th_mult=atm, round_dev_th=rdt, skip_diag_refinement=sdr, bias_fp=bias,
                             qp=36, search_method=method, subpel_search_type=taps, mvp_th=mvp_th, hp_mv_th=hp_mv_th, mv_cost_type=ctype, error_per_bit=41,
                             mvjcost=t_cost[0].data_ptr(), **{k: v.data_ptr() for k, v in sp.items()})
    ds.mvcost[0], ds.mvcost[1] = t_cost[1].data_ptr() + 4 * mc.MV_CENTRE, t_cost[2].data_ptr() + 4 * mc.MV_CENTRE
    luma_ref = pred.plane_ref(t["luma"], stride, PAD, PAD, stride, s["luma"].shape[0])
    cb_ref = pred.plane_ref(t["cb"], s["cb"].shape[1], PAD, PAD, s["cb"].shape[1], s["cb"].shape[0])
    mv = dict(mv_array=sp["best_mv"].view(torch.int16), n_mvs=n)
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream

    hip_ctx.check(L.svt_hip_md_subpel_batch(hip_ctx._h, C.byref(ds)), "svt_hip_md_subpel_batch")  # 1: the sub-pel search
    ifs.run_ifs_device(hip_ctx, 8, [luma_ref], t["src"], PW, t["ijobs"], n, t["fac"], t_res, t_st["ifs"], PARAMS, dst=t_pred[0], dst_stride=B, rd=t_rd, sse=t_sse,
                       **mv)  # 2: the filter search, from the search's MVs; the winner's luma
    ifs.run_scatter_device(hip_ctx, t["patches"], n, t_res, t_st["ifs"], n, t["cjobs"], n, np.dtype(ip.JOB_DTYPE).itemsize, abi.InterPredJob.filter_x.offset,
                           t_st["scatter"])  # 3: the filters into the chroma records
    pred.run_inter_pred_device(hip_ctx, 8, 1, 1, [cb_ref], t_pred[1], B // 2, t["cjobs"], n, t_st["chroma"], **mv)  # 4: Cb with the chosen filters
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")  # 5: transform, quantizer and distortion on the luma prediction
    hip_ctx.sync()  # the one synchronisation

    a, res, luma, cjobs, chroma, f2, want_r = host_chain(s, oracle)
    assert f2 == f
    assert np.array_equal(sp["best_mv"].cpu().numpy().view(np.int16).reshape(n, 2), a["best_mv"]), "sub-pel search"
    assert all(np.all(v.cpu().numpy() == 0) for v in t_st.values())
    rec, rd_all, sse_all, _ = ic.expected_outputs("main_8", res, FILL, with_dst=False)
    assert t_res.cpu().numpy().tobytes() == rec.tobytes(), "the search's results"
    assert np.array_equal(t_rd.cpu().numpy().view(np.uint64).reshape(n, 9), rd_all) and np.array_equal(t_sse.cpu().numpy().view(np.uint64).reshape(n, 9), sse_all)
    assert t["cjobs"].cpu().numpy().tobytes() == cjobs.tobytes(), "the chroma records after the scatter"
    assert np.array_equal(t_pred[0].cpu().numpy().reshape(luma.shape), luma), "luma prediction"
    assert np.array_equal(t_pred[1].cpu().numpy().reshape(chroma.shape), chroma), "chroma prediction"
    for name, (d_t, k) in shapes.items():
        assert np.array_equal(r_out[name].cpu().numpy().view(d_t).reshape(n, k), want_r[name].reshape(n, k)), name
    # the chain had something to do: sub-pel MVs, more than one winner, none of them the records' first filters
    assert np.any(a["best_mv"] & 7) and len({r["winner"] for r in res}) > 1 and np.all(cjobs["filter_x"] < 3)
