"""GPU: the OBMC entries in their chain, on one stream without a host read in between:
  svt_hip_inter_pred_batch (the block's prediction at its start MV, three planes, MV0_FROM_ARRAY) -> svt_hip_obmc_neighbour_batch (three planes, the
  neighbours' MVs from the same device array) -> svt_hip_obmc_target_batch -> svt_hip_obmc_search_batch on wsrc / mask -> svt_hip_inter_pred_batch again
  with MV0_FROM_ARRAY on the search's best_mv -> svt_hip_obmc_blend_batch (three planes, in place) -> svt_hip_rd_batch on the blended luma plane.
The chain equals the same steps with the host reading best_mv back and carrying every MV in the job and block records, and the restatements of
tests/inter_pred_cases.py, tests/obmc_cases.py and tests/obmc_search_cases.py step by step."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
import obmc_cases as oc
import obmc_search_cases as sc
from svt_av1_psyex_amd import abi, api, obmc, pred, rd

pytestmark = pytest.mark.gpu

FILL = oc.FILL
W, H = ip.PIC_W, ip.PIC_H


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_prediction_neighbours_target_search_prediction_blend_rd_batch_on_device(hip_ctx, bd):
    import torch
    L = api.lib()
    size, n, isz = 16, 40, 2 if bd > 8 else 1
    dt = np.uint16 if bd > 8 else np.uint8
    rng = np.random.default_rng(1500 + bd)
    org = [(x, y) for y in range(16, H - size + 1, size) for x in range(16, W - size + 1, size)][:n]
    # MV array: [0, n) the blocks' own, then two above and one left neighbour per block
    mvs = rng.integers(-40, 41, (4 * n, 2)).astype(np.int16)
    blocks, pjobs = [], {p: np.zeros(n, ip.JOB_DTYPE) for p in range(3)}
    for i, (x, y) in enumerate(org):
        above = [oc.nb(0, 2, (0, 0), i & 1, (i & 3, (i >> 2) & 3), mv_index=n + 3 * i), oc.nb(2, 2, (0, 0), 1 - (i & 1), (1, 2), mv_index=n + 3 * i + 1)][:1 + (i % 3 > 0)]
        left = [oc.nb(0, 4, (0, 0), (i >> 1) & 1, (3, i & 3), mv_index=n + 3 * i + 2)] if i % 5 else []
        blocks.append(oc.make_block(size, size, (x, y), above, left))
        for p in range(3):
            ss = oc.SS[p]
            j = ip.make_job(ss, size >> ss, size >> ss, (x >> ss, y >> ss), [(0, 0)], (i & 3, (i >> 2) & 3), (i & 1, ip.NO_REF))
            j["flags"], j["mv_index"][0], j["dst_offset"] = ip.MV0_FROM_ARRAY, i, (y >> ss) * (W >> ss) + (x >> ss)
            pjobs[p][i] = j
    b = oc.finish(f"chain_{bd}", bd, blocks, mv_array=mvs)
    # the source: what reference 0 / 1 predicts a sample or so away from the block's start MV, so that the search has something to find
    src8 = oc.src_plane("noise").copy()
    luma = oc.ref_planes(b, 0)
    for i, (x, y) in enumerate(org):
        pl, ox, oy = luma[i & 1]
        src8[y:y + size, x:x + size] = sc.upsampled(pl >> (bd - 8), oy + y, ox + x, size, size, int(mvs[i][0]) + 5 - i % 11, int(mvs[i][1]) - 6 + i % 13)
    ref8 = [np.ascontiguousarray((pl >> (bd - 8)).astype(np.uint8)) for pl, _, _ in luma]  # the search works on 8-bit planes
    sparams = sc.params(0, 1, 1, 8, 1)
    sjobs = [np.zeros(0, sc.JOB_DTYPE), np.zeros(0, sc.JOB_DTYPE)]  # per reference plane: one search launch each
    order = [[i for i in range(n) if i & 1 == r] for r in range(2)]
    src = (src8.astype(np.uint16) << 2 | 1).astype(dt) if bd > 8 else src8  # the RD batch's source at the prediction's depth
    off, n_out = oc.target_offsets(b)
    rjobs = np.zeros(n, abi.JOB_DTYPE)
    rjobs["src_offset"] = rjobs["pred_offset"] = [y * W + x for x, y in org]
    rows = np.stack([rd.quant_row_from_step(40, 52) if bd == 8 else rd.quant_row_from_step(160, 208)])
    f = dict(bit_depth=bd, quant_kind=0, tx_size=2, src_stride=W, pred_stride=W)
    shapes = {name: (np.dtype(t), k) for name, t, k in abi.RD_OUT_FIELDS if name != "cul_level"}
    planes = {p: oc.ref_planes(b, p) for p in range(3)}
    t_ref = {p: [dev(pl) for pl, _, _ in planes[p]] for p in range(3)}
    refs = {p: [pred.plane_ref(t, pl.shape[1], ox, oy, pl.shape[1], pl.shape[0]) for t, (pl, ox, oy) in zip(t_ref[p], planes[p])] for p in range(3)}
    t_src, t_src8, t_rows, t_rjobs, t_mv = dev(src), dev(src8), dev(rows), dev(rjobs), dev(mvs)
    dims = {p: (H >> oc.SS[p], W >> oc.SS[p]) for p in range(3)}
    bjobs = {p: oc.all_jobs(b, pjobs[p]["dst_offset"]) for p in range(3)}
    t_bjobs, t_tjobs = {p: dev(bjobs[p]) for p in range(3)}, dev(oc.all_jobs(b, off))
    for r in range(2):
        j = np.zeros(len(order[r]), sc.JOB_DTYPE)
        for k, i in enumerate(order[r]):
            x, y = org[i]
            j[k]["target_offset"], j[k]["ref_offset"], j[k]["width"], j[k]["height"] = off[i], (luma[r][2] + y) * ref8[r].shape[1] + luma[r][1] + x, size, size
            j[k]["start_mv"] = j[k]["ref_mv"] = mvs[i]
            j[k]["col_min"], j[k]["col_max"], j[k]["row_min"], j[k]["row_max"] = sc.mv_limits((x, y), size, size)
        sjobs[r] = j
    t_ref8, t_sjobs = [dev(a) for a in ref8], [dev(j) for j in sjobs]
    pjobs2 = {p: pjobs[p].copy() for p in range(3)}  # the second prediction: MV = best_mv of the block's search job
    for p in range(3):
        for r in range(2):
            pjobs2[p]["mv_index"][order[r], 0] = np.arange(len(order[r])) + r * len(order[0])

    def run(host_carries):
        blk, pj = b["blocks"], pjobs
        if host_carries:  # the MVs in the records, no array
            blk = b["blocks"].copy()
            for side in ("above", "left"):
                for k in range(oc.MAX_NB):
                    used = blk[side][:, k]["flags"] == oc.MV_FROM_ARRAY
                    blk[side]["mv"][used, k] = mvs[blk[side]["mv_index"][used, k]]
                    blk[side]["flags"][:, k] = 0
            pj = {p: pjobs[p].copy() for p in range(3)}
            for p in range(3):
                pj[p]["mv"][:, 0], pj[p]["flags"] = mvs[:n], 0
        t_blk, t_pj = dev(blk), {p: dev(pj[p]) for p in range(3)}
        mv = dict(mv_array=None, n_mvs=0) if host_carries else dict(mv_array=t_mv, n_mvs=len(mvs))
        t_pred = {p: filled(dims[p][0] * dims[p][1] * isz) for p in range(3)}
        t_above, t_left = filled(b["strip_samples"] * isz), filled(b["strip_samples"] * isz)
        t_wsrc, t_mask = filled(n_out * 4), filled(n_out * 4)
        t_st = {k: filled(n) for k in [f"{e}{p}" for e in ("pred", "again", "nb", "blend") for p in range(3)] + ["target"]}
        t_st.update(search0=filled(len(order[0])), search1=filled(len(order[1])))
        t_best, t_sres = filled(n * 4), filled(n * 24)
        r_out = {name: torch.zeros(n * k * d.itemsize, dtype=torch.uint8, device="cuda") for name, (d, k) in shapes.items()}
        dr = abi.RdBatchDesc(n_jobs=n, src=t_src.data_ptr(), pred=t_pred[0].data_ptr(), recon=None, jobs=t_rjobs.data_ptr(), quant_rows=t_rows.data_ptr(),
                             n_quant_rows=1, **f)
        for name, tt in r_out.items():
            setattr(dr, name, tt.data_ptr())
        t_pj2 = {p: dev(pjobs2[p]) for p in range(3)}
        torch.cuda.synchronize()  # the uploads and fills ran on torch's stream
        for p in range(3):
            ss = oc.SS[p]
            pred.run_inter_pred_device(hip_ctx, bd, ss, ss, refs[p], t_pred[p], dims[p][1], t_pj[p], n, t_st[f"pred{p}"], **mv)
            obmc.run_neighbour_device(hip_ctx, bd, ss, ss, p, refs[p], t_blk, n, t_bjobs[p], n, t_above, t_left, t_st[f"nb{p}"], **mv)
        obmc.run_target_device(hip_ctx, bd, t_blk, n, t_tjobs, n, t_above, t_left, t_src8, W, t_wsrc, t_mask, t_st["target"])
        for r in range(2):  # best_mv of reference 0's jobs first, then reference 1's
            at = r * len(order[0])
            obmc.run_search_device(hip_ctx, sparams, t_ref8[r], ref8[r].shape[1], t_wsrc, t_mask, t_sjobs[r], len(order[r]), t_best[4 * at:], t_sres[24 * at:],
                                   t_st[f"search{r}"])
        mv2 = dict(mv_array=t_best.view(torch.int16), n_mvs=n)
        if host_carries:
            hip_ctx.sync()
            best = t_best.cpu().numpy().view(np.int16).reshape(n, 2)
            pj2 = {p: pjobs2[p].copy() for p in range(3)}
            for p in range(3):
                pj2[p]["mv"][:, 0], pj2[p]["flags"] = best[pjobs2[p]["mv_index"][:, 0]], 0
            mv2 = dict(mv_array=None, n_mvs=0)
            t_pj2 = {p: dev(pj2[p]) for p in range(3)}
            torch.cuda.synchronize()
        for p in range(3):
            ss = oc.SS[p]
            pred.run_inter_pred_device(hip_ctx, bd, ss, ss, refs[p], t_pred[p], dims[p][1], t_pj2[p], n, t_st[f"again{p}"], **mv2)
        for p in range(3):
            ss = oc.SS[p]
            obmc.run_blend_device(hip_ctx, bd, ss, ss, p, t_blk, n, t_bjobs[p], n, t_above, t_left, t_pred[p], dims[p][1], t_st[f"blend{p}"])
        hip_ctx.check(L.svt_hip_rd_batch(hip_ctx._h, C.byref(dr)), "svt_hip_rd_batch")
        hip_ctx.sync()  # the one synchronisation of the device chain
        out = {f"pred{p}": t_pred[p].cpu().numpy().view(dt).reshape(dims[p]) for p in range(3)}
        out.update(above=t_above.cpu().numpy().view(dt), left=t_left.cpu().numpy().view(dt), wsrc=t_wsrc.cpu().numpy().view(np.int32),
                   mask=t_mask.cpu().numpy().view(np.int32), best=t_best.cpu().numpy().view(np.int16).reshape(n, 2), sres=t_sres.cpu().numpy())
        out.update({f"st_{k}": v.cpu().numpy() for k, v in t_st.items()})
        out.update({name: r_out[name].cpu().numpy() for name in r_out})
        return out

    a, c = run(False), run(True)
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    assert all(np.all(a[k] == 0) for k in a if k.startswith("st_"))
    # step by step against the restatements
    above, left, events = oc.restate_neighbours(b)
    assert all(e["inside"] for evs in events.values() for _, e in evs)
    assert np.array_equal(a["above"], above) and np.array_equal(a["left"], left)
    wsrc, mask = oc.restate_target(b, above, left, oc.all_jobs(b, off), n_out, src=src8)
    assert np.array_equal(a["wsrc"], wsrc) and np.array_equal(a["mask"], mask)
    want_best, want_res = [], []
    for r in range(2):
        got = [sc.restate_job(sparams, ref8[r], wsrc, mask, j, None) for j in sjobs[r]]
        want_best += [g[0] for g in got]
        want_res += [g[1] for g in got]
    want_best = np.array(want_best, np.int16)
    assert np.array_equal(a["best"], want_best) and a["sres"].tobytes() == np.array(want_res, sc.RESULT_DTYPE).tobytes()
    moved = sum(tuple(want_best[pjobs2[0]["mv_index"][i, 0]]) != tuple(mvs[i]) for i in range(n))
    assert moved > n // 2  # the refined MVs differ from the start MVs: the second prediction shows whether it read them
    want = {}
    for p in range(3):
        own = np.full(dims[p], FILL * 0x0101 if bd > 8 else FILL, dt)
        for j in pjobs2[p]:
            y, x = divmod(int(j["dst_offset"]), dims[p][1])
            own[y:y + int(j["height"]), x:x + int(j["width"])] = ip.restate_job(planes[p], bd, oc.SS[p], j, want_best)[0]
        want[p] = oc.restate_blend(b, p, above, left, own, bjobs[p])
        assert np.array_equal(a[f"pred{p}"], want[p]), p
        assert not np.array_equal(want[p], own)  # the blend changed the plane
    import pyoracle
    want_r = pyoracle.rd_batch(f, src, want[0], rjobs, rows, want_coeffs=False, want_recon=False)
    for name, (d, k) in shapes.items():
        assert np.array_equal(a[name].view(d).reshape(n, k), want_r[name]), name
