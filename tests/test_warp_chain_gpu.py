"""GPU: a WARPED_CAUSAL candidate through the whole device chain on one stream, no host copy in between: svt_hip_md_subpel_batch ->
svt_hip_wm_refine_batch (start MV from the search's array) -> svt_hip_warp_model_batch (MV from the refinement's array) -> svt_hip_warp_pred_batch
(model from the fit's array; Y, and Cb on the sub-sampled plane, of 16x16 blocks) -> svt_hip_rd_batch on that prediction plane, against the same
chain on the CPU: the sub-pel oracle, the restatements of tests/warp_cases.py and the RD oracle.  One block has no usable samples: its final fit
is invalid, its prediction jobs report 0xFE, and its slot of the prediction plane is still as it was."""
import ctypes as C

import numpy as np
import pytest

import md_search_cases as mc
import warp_cases as wc
from svt_av1_psyex_amd import abi, api, rd, warp

pytestmark = pytest.mark.gpu

FILL = wc.FILL
PW, PH, PAD, B = 96, 64, 24, 16
SETTINGS = dict(iterations=8, refine_diag=0, mv_prec_shift=1, shut_approx=0, lower_band_th=0, upper_band_th=65535, approx_inter_rate=0, error_per_bit=41)
LOST = 3  # the block without a model


def build():
    rng = np.random.default_rng(2026)
    src, luma = wc.moving_planes(rng, PW, PH, pad=PAD)
    y2, x2 = np.mgrid[0:PH // 2 + 2 * PAD, 0:PW // 2 + 2 * PAD]
    cb = (np.clip(128 + 60 * np.sin(x2 / 3.1 + y2 / 5.0) + rng.normal(0, 5, x2.shape), 0, 255).astype(np.uint8), PAD, PAD, PW // 2, PH // 2)
    org = [(16 * bx, 16 * by) for by in (0, 1, 3) for bx in (0, 2, 5)][:6]
    n = len(org)
    tables = mc.cost_tables(rng)
    stride = luma[0].shape[1]
    sjobs = np.zeros(n, abi.SUBPEL_JOB_DTYPE)
    rjobs = np.zeros(n, wc.REFINE_JOB_DTYPE)
    mjobs = np.zeros(n, wc.MODEL_JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        start = (int(rng.integers(-1, 2)) * 8 + 8, int(rng.integers(-1, 2)) * 8 - 16)
        pred_mv = (start[0] + int(rng.integers(-12, 13)), start[1] + int(rng.integers(-12, 13)))
        j = sjobs[i]
        j["src_offset"], j["ref_offset"] = y * PW + x, (y + PAD) * stride + x + PAD
        j["width"], j["height"], j["log2_pels"], j["start_mv"], j["ref_mv"] = B, B, 8, start, pred_mv
        j["col_min"], j["col_max"], j["row_min"], j["row_max"] = start[1] - 40, start[1] + 40, start[0] - 40, start[0] + 40
        j["early_exit_th"], j["best_mvp"] = 1020 - (B >> 2), start
        r = wc.refine_job(rng, x, y, B, B, PW, 6, "lost" if i == LOST else "mild", start, pred_mv)
        r["flags"], r["mv_index"], r["start_mv"] = wc.WM_START_FROM_ARRAY, i, (0, 0)
        rjobs[i] = r
        m = mjobs[i]
        m["pts"], m["pts_inref"], m["blk_org_x"], m["blk_org_y"], m["bwidth"], m["bheight"], m["n_samples"] = r["pts"], r["pts_inref"], x, y, B, B, 6
        m["flags"], m["mv_index"] = wc.MV_FROM_ARRAY, i
    pjobs = {}
    for ss, w in ((0, B), (1, B // 2)):
        pjobs[ss] = wc.pack_jobs([wc.pred_job(i * w * w, x >> ss, y >> ss, w, w, [0], [], flags=wc.MODEL0_FROM_ARRAY, model_index=(i, 0))
                                  for i, (x, y) in enumerate(org)], wc.PRED_JOB_DTYPE)
    tjobs = np.zeros(n, abi.JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        tjobs[i]["src_offset"], tjobs[i]["pred_offset"], tjobs[i]["tx_type"] = y * PW + x, i * B * B, (0, 1, 2, 3, 9)[i % 5]
    rows = np.stack([rd.quant_row_from_step(40, 52)])
    return dict(src=src, luma=luma, cb=cb, org=org, n=n, tables=tables, sjobs=sjobs, rjobs=rjobs, mjobs=mjobs, pjobs=pjobs, tjobs=tjobs, rows=rows)


def cpu_chain(s, oracle):
    import pyoracle
    n = s["n"]
    a = mc.run_subpel_cpu(oracle.orc_md_subpel_batch, s["src"], s["luma"][0], s["sjobs"], mc.SUBPEL_SETTINGS[0], SETTINGS["error_per_bit"], 36, s["tables"])
    rb = dict(settings=SETTINGS, planes=[s["luma"]], src=s["src"], jobs=s["rjobs"], mv_array=a["best_mv"], cost_tables=s["tables"])
    refined = wc.restate_refine(rb)
    mb = dict(jobs=s["mjobs"], mv_array=refined["best_mv"], shut_approx=0, lower_band_th=0, upper_band_th=65535)
    models, mstatus = wc.restate_models(mb)
    preds = {}
    for ss, planes, w in ((0, [s["luma"]], B), (1, [s["cb"]], B // 2)):
        pb = dict(bit_depth=8, ss_x=ss, ss_y=ss, planes=planes, jobs=s["pjobs"][ss], dst_shape=(n * w, w), dst_stride=w, models=models)
        preds[ss] = wc.restate_pred(pb)[:2]
    f = dict(bit_depth=8, quant_kind=0, tx_size=2, src_stride=PW, pred_stride=B)
    want_r = pyoracle.rd_batch(f, np.ascontiguousarray(s["src"].reshape(-1)), np.ascontiguousarray(preds[0][0].reshape(-1)), s["tjobs"], s["rows"], want_recon=False)
    return a, refined, models, mstatus, preds, f, want_r


def test_chain_subpel_refine_fit_warp_rd_on_device(hip_ctx, oracle):
    import torch
    L = api.lib()
    s = build()
    n = s["n"]
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()
    t = {k: dev(s[k]) for k in ("src", "sjobs", "rjobs", "mjobs", "tjobs", "rows")}
    t_luma, t_cb = dev(s["luma"][0]), dev(s["cb"][0])
    t_pj = {ss: dev(s["pjobs"][ss]) for ss in (0, 1)}
    t_cost = [dev(x) for x in s["tables"]]
    filled = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    sp = {k: filled(n * b) for k, b in (("best_mv", 4), ("besterr", 4), ("distortion", 4), ("sse", 4), ("center_err", 4))}
    ref_out = {k: filled(n * (2 if k == "best_mv" else 1) * np.dtype(d).itemsize) for k, d in warp.REFINE_OUT_DTYPES.items()}
    t_models, t_mstatus = filled(n * np.dtype(abi.WARP_MODEL_DTYPE).itemsize), filled(n)
    t_pred = {0: filled(n * B * B), 1: filled(n * B * B // 4)}
    t_pstatus = {0: filled(n), 1: filled(n)}
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    shapes["qcoeff"] = (np.dtype(np.int32), B * B)
    r_out = {name: torch.zeros(n * k * dt.itemsize, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    f = dict(bit_depth=8, quant_kind=0, tx_size=2, src_stride=PW, pred_stride=B)
    dr = abi.RdBatchDesc(n_jobs=n, src=t["src"].data_ptr(), pred=t_pred[0].data_ptr(), recon=None, jobs=t["tjobs"].data_ptr(), quant_rows=t["rows"].data_ptr(),
                         n_quant_rows=1, **f)
    for name, tt in r_out.items():
        setattr(dr, name, tt.data_ptr())
    hp, stop, iters, pvt, atm, rdt, sdr, bias, ctype, method, taps, mvp_th, hp_mv_th = mc.full_setting(mc.SUBPEL_SETTINGS[0])
    stride = s["luma"][0].shape[1]
    ds = abi.SubpelBatchDesc(n_jobs=n, src_stride=PW, ref_stride=stride, src=t["src"].data_ptr(), ref=t_luma.data_ptr(), jobs=t["sjobs"].data_ptr(), allow_hp=hp,
                             forced_stop=stop, iters_per_step=iters, pred_variance_th=pvt, abs_th_mult=atm, round_dev_th=rdt, skip_diag_refinement=sdr, bias_fp=bias,
                             qp=36, search_method=method, subpel_search_type=taps, mvp_th=mvp_th, hp_mv_th=hp_mv_th, mv_cost_type=ctype,
                             error_per_bit=SETTINGS["error_per_bit"], mvjcost=t_cost[0].data_ptr(), **{k: v.data_ptr() for k, v in sp.items()})
    ds.mvcost[0], ds.mvcost[1] = t_cost[1].data_ptr() + 4 * mc.MV_CENTRE, t_cost[2].data_ptr() + 4 * mc.MV_CENTRE
    luma_ref = warp.plane_ref(t_luma, stride, PAD, PAD, PW, PH, s["luma"][0].shape[0])
    cb_ref = warp.plane_ref(t_cb, s["cb"][0].shape[1], PAD, PAD, PW // 2, PH // 2, s["cb"][0].shape[0])
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream

    hip_ctx.check(L.svt_hip_md_subpel_batch(hip_ctx._h, C.byref(ds)), "svt_hip_md_subpel_batch")  # 1: the sub-pel search
    warp.run_wm_refine_device(hip_ctx, SETTINGS, [luma_ref], t["src"], PW, t["rjobs"], n, mv_array=sp["best_mv"], n_mvs=n, cost_tables=t_cost,
                              outs=ref_out)  # 2: the refinement, from the search's MVs
    warp.run_warp_model_device(hip_ctx, t["mjobs"], n, t_models, t_mstatus, 0, 0, 65535, mv_array=ref_out["best_mv"], n_mvs=n)  # 3: the fit, from the refined MVs
    warp.run_warp_pred_device(hip_ctx, 8, 0, 0, [luma_ref], t_pred[0], B, t_pj[0], n, t_pstatus[0], models=t_models, n_models=n)  # 4: Y
    warp.run_warp_pred_device(hip_ctx, 8, 1, 1, [cb_ref], t_pred[1], B // 2, t_pj[1], n, t_pstatus[1], models=t_models, n_models=n)  # and Cb
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")  # 5: transform, quantizer and distortion on the Y prediction
    hip_ctx.sync()  # the one synchronisation

    a, refined, models, mstatus, preds, f2, want_r = cpu_chain(s, oracle)
    assert f2 == f
    assert np.array_equal(sp["best_mv"].cpu().numpy().view(np.int16).reshape(n, 2), a["best_mv"]), "sub-pel search"
    for k, d in warp.REFINE_OUT_DTYPES.items():
        got = ref_out[k].cpu().numpy().view(d)
        assert np.array_equal(got.reshape(refined[k].shape), refined[k].view(d) if k == "n_checked" else refined[k]), f"refinement: {k}"
    assert np.all(t_mstatus.cpu().numpy() == wc.ST_OK) and np.all(mstatus == wc.ST_OK)
    assert t_models.cpu().numpy().tobytes() == models.tobytes(), "the fits"
    valid = models["valid"] == 1
    assert list(np.flatnonzero(~valid)) == [LOST] and int(refined["best_cost"][LOST]) == wc.INT_MAX
    for ss in (0, 1):
        want_dst, want_status = preds[ss]
        assert [int(v) for v in want_status] == [wc.ST_NO_MODEL if i == LOST else wc.ST_OK for i in range(n)]
        assert np.array_equal(t_pstatus[ss].cpu().numpy(), want_status), f"prediction status, ss {ss}"
        assert np.array_equal(t_pred[ss].cpu().numpy().reshape(want_dst.shape), want_dst), f"prediction plane, ss {ss}"
    slot = t_pred[0].cpu().numpy().reshape(n, B * B)[LOST]
    assert np.all(slot == FILL)  # nothing was predicted for the block without a model: its RD slot is not consumed
    for name, (d_t, k) in shapes.items():
        got, want = r_out[name].cpu().numpy().view(d_t).reshape(n, k), want_r[name].reshape(n, k)
        assert np.array_equal(got[valid], want[valid]), name
    # the chain had something to do: the refinement moved an MV, and coefficients survive
    assert np.any(refined["best_mv"][valid] != a["best_mv"][valid]) and np.count_nonzero(want_r["eob"].reshape(-1)[valid] > 1) >= 3
