"""GPU: the masked predictions in their chains, on one stream without a host read in between:
  two single-reference svt_hip_inter_pred_batch launches -> svt_hip_mask_search_batch (pick_interinter_wedge / pick_interinter_seg) ->
  svt_hip_masked_pred_batch taking each job's wedge / mask type from the search's result array -> svt_hip_rd_batch on the prediction;
  svt_hip_intra_pred_batch (the four inter-intra modes) + svt_hip_inter_pred_batch -> svt_hip_mask_search_batch (inter_intra_search) ->
  svt_hip_interintra_blend_batch taking mode, use_wedge and wedge_index from the result array.
Each chain equals the same steps with the host carrying the parameters, and the restatements of tests/mask_cases.py step by step."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
import intra_pred_cases as ic
import mask_cases as mc
from svt_av1_psyex_amd import abi, api, intra, mask, pred, rd

pytestmark = pytest.mark.gpu

FILL = 0xA5
W, H = ip.PIC_W, ip.PIC_H


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def blocks(size, n):
    return [(x, y) for y in range(0, H - size + 1, size) for x in range(0, W - size + 1, size)][:n]


def single_jobs(org, size, mvs, ref):
    jobs = np.zeros(len(org), ip.JOB_DTYPE)
    for i, ((x, y), mv) in enumerate(zip(org, mvs)):
        j = ip.make_job(0, size, size, (x, y), [mv], (0, 0), (ref, ip.NO_REF))  # the fixed filter of the compound and inter-intra searches
        j["dst_offset"] = y * W + x
        jobs[i] = j
    return jobs


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_predictions_search_masked_prediction_rd_batch_on_device(hip_ctx, bd):
    import torch
    L = api.lib()
    size, n, isz = 16, 48, 2 if bd > 8 else 1
    dt = np.uint16 if bd > 8 else np.uint8
    rng = np.random.default_rng(800 + bd)
    pad = ip.plane_dims(0)[2]
    planes = [(ip.plane("noise", bd, 0, k), pad, pad) for k in range(2)]
    # a source the two predictions explain in parts, so that the searches have something to find
    src = np.clip(planes[0][0][pad:pad + H, pad:pad + W].astype(np.int64) + rng.integers(-30, 31, (H, W)), 0, (1 << bd) - 1).astype(dt)
    org = blocks(size, n)
    mvs = [[mc.random_mv(rng, 0, 0, int(rng.integers(0, 4)), 3) for _ in org] for _ in range(2)]
    sjobs = [single_jobs(org, size, mvs[k], k) for k in range(2)]
    search = np.zeros(n, mc.SEARCH_JOB_DTYPE)
    search["src_offset"] = search["pred0_offset"] = search["pred1_offset"] = [y * W + x for x, y in org]
    search["width"], search["height"], search["kind"] = size, size, np.arange(n) & 1
    mjobs = np.zeros(n, mc.PRED_JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        j = mc.make_pred_job(0, 0, size, size, (x, y), [mvs[0][i], mvs[1][i]], (i & 3, (i >> 2) & 3), comp_type=int(search["kind"][i]), wedge=(0xEE, 0xEE),
                             mask_type=0xEE, mask_offset=i * size * size)
        j["pred"]["dst_offset"], j["pred"]["flags"], j["result_index"] = y * W + x, mc.PARAMS_FROM_ARRAY, i
        mjobs[i] = j
    rjobs = np.zeros(n, abi.JOB_DTYPE)
    rjobs["src_offset"] = rjobs["pred_offset"] = search["src_offset"]
    rows = np.stack([rd.quant_row_from_step(40, 52) if bd == 8 else rd.quant_row_from_step(160, 208)])
    f = dict(bit_depth=bd, quant_kind=0, tx_size=2, src_stride=W, pred_stride=W)
    shapes = {name: (np.dtype(t), k) for name, t, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    t_ref = [dev(p) for p, _, _ in planes]
    refs = [pred.plane_ref(t, p.shape[1], pad, pad, p.shape[1], p.shape[0]) for t, (p, _, _) in zip(t_ref, planes)]
    t_src, t_rows, t_rjobs, t_search = dev(src), dev(rows), dev(rjobs), dev(search)
    t_sjobs = [dev(j) for j in sjobs]

    def run(host_carries):
        t = {k: filled(H * W * isz) for k in ("p0", "p1", "pred")}
        t_st = {k: filled(n) for k in ("s0", "s1", "search", "pred")}
        t_res, t_mask = filled(n * 24), filled(n * size * size)
        r_out = {name: torch.zeros(n * k * d.itemsize, dtype=torch.uint8, device="cuda") for name, (d, k) in shapes.items()}
        dr = abi.RdBatchDesc(n_jobs=n, src=t_src.data_ptr(), pred=t["pred"].data_ptr(), recon=None, jobs=t_rjobs.data_ptr(), quant_rows=t_rows.data_ptr(),
                             n_quant_rows=1, **f)
        for name, tt in r_out.items():
            setattr(dr, name, tt.data_ptr())
        torch.cuda.synchronize()  # the uploads and fills ran on torch's stream
        for k in range(2):
            pred.run_inter_pred_device(hip_ctx, bd, 0, 0, refs, t[f"p{k}"], W, t_sjobs[k], n, t_st[f"s{k}"])
        mask.run_mask_search_device(hip_ctx, bd, 0, t_src, W, t["p0"], W, t["p1"], W, None, 0, t_search, n, t_res, t_st["search"])
        jobs = mjobs
        if host_carries:
            hip_ctx.sync()
            res = t_res.cpu().numpy().view(mc.RESULT_DTYPE)
            jobs = mjobs.copy()
            jobs["pred"]["flags"] = 0
            jobs["wedge_index"], jobs["wedge_sign"], jobs["mask_type"] = res["wedge_index"], res["wedge_sign"], res["mask_type"]
        t_jobs = dev(jobs)
        torch.cuda.synchronize()
        mask.run_masked_pred_device(hip_ctx, bd, 0, 0, 0, refs, t["pred"], W, t_jobs, n, t_st["pred"], results=None if host_carries else t_res,
                                    n_results=0 if host_carries else n, mask_buf=t_mask)
        hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")
        hip_ctx.sync()  # the one synchronisation of the device chain
        out = {k: v.cpu().numpy().view(dt).reshape(H, W) for k, v in t.items()}
        out.update({f"st_{k}": v.cpu().numpy() for k, v in t_st.items()})
        out["results"], out["mask"] = t_res.cpu().numpy().view(mc.RESULT_DTYPE), t_mask.cpu().numpy()
        out.update({name: r_out[name].cpu().numpy() for name in r_out})
        return out

    a, b = run(False), run(True)
    for k in a:
        assert np.array_equal(a[k], b[k]) if a[k].dtype.names is None else a[k].tobytes() == b[k].tobytes(), k
    assert all(np.all(a[f"st_{k}"] == 0) for k in ("s0", "s1", "search", "pred"))
    # step by step against the restatements
    for k in range(2):
        want = np.full((H, W), FILL * 0x0101 if bd > 8 else FILL, dt)
        for j in sjobs[k]:
            y, x = divmod(int(j["dst_offset"]), W)
            want[y:y + size, x:x + size] = ip.restate_job(planes, bd, 0, j)[0]
        assert np.array_equal(a[f"p{k}"], want), f"prediction {k}"
    sp = {"src": src, "pred0": a["p0"], "pred1": a["p1"]}
    want_res = np.array([mc.restate_search_job(sp, bd, 0, j)[0] for j in search], mc.RESULT_DTYPE)
    assert a["results"].tobytes() == want_res.tobytes()
    assert len(set(want_res["wedge_index"][0::2])) > 3 and set(want_res["mask_type"][1::2]) == {0, 1}  # the parameters differ from job to job
    batch = {"bit_depth": bd, "ss_x": 0, "ss_y": 0, "plane": 0, "planes": mc.NOISE2, "jobs": mjobs, "mv_array": None, "results": want_res, "dst_shape": (H, W),
             "dst_stride": W, "mask_bytes": n * size * size}
    want_blocks, defined, want_mask, _ = mc.run_pred_restated(batch)
    assert all(defined)
    want_pred = mc.pred_expected_image(batch, want_blocks, FILL)
    assert np.array_equal(a["pred"], want_pred)
    assert np.array_equal(a["mask"], want_mask)
    import pyoracle
    want_r = pyoracle.rd_batch(f, src, want_pred, rjobs, rows, want_coeffs=False, want_recon=False)
    for name, (d, k) in shapes.items():
        assert np.array_equal(a[name].view(d).reshape(n, k), want_r[name]), name


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_intra_and_inter_predictions_search_interintra_blend_on_device(hip_ctx, bd):
    import torch
    size, n, isz, tx = 16, 40, 2 if bd > 8 else 1, 2  # TX_16X16
    dt = np.uint16 if bd > 8 else np.uint8
    rng = np.random.default_rng(900 + bd)
    pad = ip.plane_dims(0)[2]
    planes = [(ip.plane("noise", bd, 0, 0), pad, pad)]
    nbr = ic.plane("noise", bd)
    org = blocks(size, n)
    mvs = [mc.random_mv(rng, 0, 0, int(rng.integers(0, 4)), 3) for _ in org]
    sjobs = single_jobs(org, size, mvs, 0)
    modes = [ic.DC_PRED, ic.V_PRED, ic.H_PRED, ic.SMOOTH_PRED]  # II_DC_PRED, II_V_PRED, II_H_PRED, II_SMOOTH_PRED
    ijobs = np.zeros(4 * n, ic.JOB_DTYPE)
    search = np.zeros(n, mc.SEARCH_JOB_DTYPE)
    bjobs = np.zeros(n, mc.BLEND_JOB_DTYPE)
    for i, (x, y) in enumerate(org):
        pos = ic.random_pos(rng)
        for m in range(4):
            j = ic.make_job(tx, modes[m], pos, (size, size, size, size))
            j["dst_offset"] = (m * H + y) * W + x  # the four modes' planes one below the other
            ijobs[4 * i + m] = j
            search[i]["intra_offset"][m] = j["dst_offset"]
        search[i]["src_offset"] = search[i]["pred1_offset"] = y * W + x
        search[i]["width"], search[i]["height"], search[i]["kind"], search[i]["ii_wedge_mode"] = size, size, mc.KIND_INTERINTRA, i % 3
        b = bjobs[i]
        b["intra_offset"] = search[i]["intra_offset"]
        b["inter_offset"] = b["dst_offset"] = y * W + x
        b["width"], b["height"], b["luma_width"], b["luma_height"], b["flags"], b["result_index"] = size, size, size, size, mc.PARAMS_FROM_ARRAY, i
        b["interintra_mode"], b["use_wedge"], b["wedge_index"] = 0xEE, 0xEE, 0xEE
    # the source: per block a blend of its own, so that the winners differ
    want_intra = np.full((4 * H, W), FILL * 0x0101 if bd > 8 else FILL, dt)
    for j in ijobs:
        y, x = divmod(int(j["dst_offset"]), W)
        want_intra[y:y + size, x:x + size] = ic.restate_job(nbr, bd, 0, j)[0]
    want_inter = np.full((H, W), FILL * 0x0101 if bd > 8 else FILL, dt)
    for j in sjobs:
        y, x = divmod(int(j["dst_offset"]), W)
        want_inter[y:y + size, x:x + size] = ip.restate_job(planes, bd, 0, j)[0]
    src = np.zeros((H, W), dt)
    for i, (x, y) in enumerate(org):
        inter = want_inter[y:y + size, x:x + size].astype(np.int64)
        ii = want_intra[(i % 4) * H + y:(i % 4) * H + y + size, x:x + size].astype(np.int64)
        m = mc.wedge_mask(size, size, i % 16, 0) if i % 5 == 0 else mc.smooth_mask(size, size, i % 4)
        src[y:y + size, x:x + size] = np.clip(mc.blend_a64(m, ii, inter) + rng.integers(-2, 3, (size, size)), 0, (1 << bd) - 1)
    t_ref, t_nbr, t_src = dev(planes[0][0]), dev(nbr), dev(src)
    refs = [pred.plane_ref(t_ref, planes[0][0].shape[1], pad, pad, planes[0][0].shape[1], planes[0][0].shape[0])]
    t_sjobs, t_ijobs, t_search = dev(sjobs), dev(ijobs), dev(search)
    def run(host_carries):
        t_intra, t_inter, t_out = filled(4 * H * W * isz), filled(H * W * isz), filled(H * W * isz)
        t_st = {k: filled(c) for k, c in (("intra", 4 * n), ("inter", n), ("search", n), ("blend", n))}
        t_res = filled(n * 24)
        torch.cuda.synchronize()
        intra.run_intra_pred_device(hip_ctx, bd, 0, t_nbr, nbr.shape[1], nbr.shape[1], nbr.shape[0], t_intra, W, t_ijobs, 4 * n, t_st["intra"])
        pred.run_inter_pred_device(hip_ctx, bd, 0, 0, refs, t_inter, W, t_sjobs, n, t_st["inter"])
        mask.run_mask_search_device(hip_ctx, bd, 0, t_src, W, None, 0, t_inter, W, t_intra, W, t_search, n, t_res, t_st["search"])
        jobs = bjobs
        if host_carries:
            hip_ctx.sync()
            res = t_res.cpu().numpy().view(mc.RESULT_DTYPE)
            jobs = bjobs.copy()
            jobs["flags"] = 0
            jobs["interintra_mode"], jobs["use_wedge"], jobs["wedge_index"] = res["interintra_mode"], res["use_wedge_interintra"], res["wedge_index"].astype(np.uint8)
        t_jobs = dev(jobs)
        torch.cuda.synchronize()
        mask.run_interintra_blend_device(hip_ctx, bd, t_intra, W, t_inter, W, t_out, W, t_jobs, n, t_st["blend"], results=None if host_carries else t_res,
                                         n_results=0 if host_carries else n)
        hip_ctx.sync()  # the one synchronisation of the device chain
        out = {"intra": t_intra.cpu().numpy().view(dt).reshape(4 * H, W), "inter": t_inter.cpu().numpy().view(dt).reshape(H, W),
               "out": t_out.cpu().numpy().view(dt).reshape(H, W), "results": t_res.cpu().numpy().view(mc.RESULT_DTYPE)}
        out.update({f"st_{k}": v.cpu().numpy() for k, v in t_st.items()})
        return out

    a, b = run(False), run(True)
    for k in a:
        assert np.array_equal(a[k], b[k]) if a[k].dtype.names is None else a[k].tobytes() == b[k].tobytes(), k
    assert all(np.all(a[k] == 0) for k in a if k.startswith("st_"))
    assert np.array_equal(a["intra"], want_intra) and np.array_equal(a["inter"], want_inter)
    sp = {"src": src, "pred1": want_inter, "intra": want_intra}
    want_res = np.array([mc.restate_search_job(sp, bd, 0, j)[0] for j in search], mc.RESULT_DTYPE)
    assert a["results"].tobytes() == want_res.tobytes()
    assert set(want_res["interintra_mode"]) == {0, 1, 2, 3} and set(want_res["use_wedge_interintra"]) == {0, 1}
    geo = {"intra_shape": want_intra.shape, "inter_shape": (H, W), "dst_shape": (H, W)}
    assert all(mc.blend_job_defined(geo, j, want_res) for j in bjobs)
    want = [mc.restate_blend_job(geo, want_intra, want_inter, j, want_res) for j in bjobs]
    base = np.full((H, W), FILL * 0x0101 if bd > 8 else FILL, dt)
    assert np.array_equal(a["out"], mc.blend_expected_image({"jobs": bjobs}, want, base))
