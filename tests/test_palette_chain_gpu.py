"""GPU: palette candidates through the device chain on one stream, no host look in between: svt_hip_palette_search_batch ->
svt_hip_palette_pred_batch for every one of the 14 slots of every block, enqueued blindly (a slot past n_cands gets 0xFF and leaves its part of the
prediction plane as it was) -> svt_hip_rd_batch on the prediction plane, on a handful of 16x16 blocks, against the same chain on the host: the
restatement of tests/palette_cases.py and the RD oracle."""
import ctypes as C

import numpy as np
import pytest

import palette_cases as pc
from svt_av1_psyex_amd import abi, api, palette, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5
PW, PH, B = 96, 32, 16
PARAMS = dict(pc.PARAMS, dominant_color_step=2)


def build():
    rng = np.random.default_rng(2028)
    src = rng.integers(0, 256, (PH, PW)).astype(np.uint8)
    org = [(16 * bx, 16 * by) for by in (0, 1) for bx in (0, 1, 3, 5)][:7]
    n = len(org)
    jobs = np.zeros(n, pc.JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        kind, k = (("k", 5), ("near", 9), ("k", 2), ("k", 30), ("stripes", 4), ("noise", 0), ("k", 12))[i]
        src[y:y + B, x:x + B] = pc.make_block(rng, pc.spec(B, B, kind, k=k), 8)
        cache = pc.palette_cache(pc.near_palette(rng, src[y:y + B, x:x + B], 3, 255), pc.near_palette(rng, src[y:y + B, x:x + B], 4, 255) if i % 2 else None)
        j = jobs[i]
        j["src_offset"], j["width"], j["height"], j["rows"], j["cols"], j["bsize_ctx"], j["mode_ctx"] = y * PW + x, B, B, B, B, 2, 1 + i % 2
        j["n_cache"], j["color_cache"][:len(cache)] = len(cache), cache
    pjobs = np.array([(i, q, (i * pc.MAX_CANDS + q) * B * B, 0) for i in range(n) for q in range(pc.MAX_CANDS)], pc.PRED_JOB_DTYPE)
    tjobs = np.zeros(len(pjobs), abi.JOB_DTYPE)
    for s, p in enumerate(pjobs):
        x, y = org[int(p["search_index"])]
        tjobs[s]["src_offset"], tjobs[s]["pred_offset"], tjobs[s]["tx_type"] = y * PW + x, p["dst_offset"], (0, 1, 2, 3, 9)[s % 5]
    return dict(src=src, n=n, jobs=jobs, pjobs=pjobs, tjobs=tjobs, rows=np.stack([rd.quant_row_from_step(40, 52)]), tables=pc.cost_tables(77))


def test_chain_search_pred_rd_on_device(hip_ctx, oracle):
    import pyoracle
    import torch
    L = api.lib()
    s = build()
    n, m = s["n"], len(s["pjobs"])
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()
    t = {k: dev(s[k]) for k in ("src", "jobs", "pjobs", "tjobs", "rows")}
    t_tab = [dev(s["tables"][k]) for k in ("ycolor", "ysize", "ymode")]
    filled = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    t_res, t_st, t_pst, t_pred = filled(n * np.dtype(pc.RESULT_DTYPE).itemsize), filled(n), filled(m), filled(m * B * B)
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    r_out = {name: torch.zeros(m * k * dt.itemsize, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    f = dict(bit_depth=8, quant_kind=0, tx_size=2, src_stride=PW, pred_stride=B)
    dr = abi.RdBatchDesc(n_jobs=m, src=t["src"].data_ptr(), pred=t_pred.data_ptr(), recon=None, jobs=t["tjobs"].data_ptr(), quant_rows=t["rows"].data_ptr(),
                         n_quant_rows=1, **f)
    for name, tt in r_out.items():
        setattr(dr, name, tt.data_ptr())
    torch.cuda.synchronize()  # the uploads and fills ran on torch's stream

    palette.run_search_device(hip_ctx, 8, t["src"], PW, t["jobs"], n, t_tab, t_res, t_st, PARAMS)  # 1: the candidates and their rates
    palette.run_pred_device(hip_ctx, 8, t["src"], PW, t_pred, B, t["jobs"], t_res, t_st, n, t["pjobs"], m, t_pst)  # 2: every slot's prediction
    hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")  # 3: transform, quantizer and distortion on every slot
    hip_ctx.sync()  # the one synchronisation

    res = [pc.restate_job(s["src"], 8, j, PARAMS, s["tables"]) for j in s["jobs"]]
    luma = np.full((m, B, B), FILL, np.uint8)
    status = np.full(m, pc.ST_UNDEFINED, np.uint8)
    for i, r in enumerate(res):
        for q, c in enumerate(r["cands"]):
            luma[i * pc.MAX_CANDS + q], status[i * pc.MAX_CANDS + q] = c["pred"].astype(np.uint8), pc.ST_OK
    want_r = pyoracle.rd_batch(f, np.ascontiguousarray(s["src"].reshape(-1)), np.ascontiguousarray(luma.reshape(-1)), s["tjobs"], s["rows"], want_recon=False)
    assert np.all(t_st.cpu().numpy() == pc.ST_OK) and np.array_equal(t_pst.cpu().numpy(), status)
    assert t_res.cpu().numpy().tobytes() == pc.result_records(res, FILL).tobytes(), "the search's results"
    assert np.array_equal(t_pred.cpu().numpy().reshape(luma.shape), luma), "the prediction plane"
    for name, (d_t, k) in shapes.items():
        assert np.array_equal(r_out[name].cpu().numpy().view(d_t).reshape(m, k), want_r[name].reshape(m, k)), name
    # the chain had something to do: blocks with and without candidates, more than one palette size
    assert {0} < {r["n_cands"] for r in res} and len({c["size"] for r in res for c in r["cands"]}) > 2
