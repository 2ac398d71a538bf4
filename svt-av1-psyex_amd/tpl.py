"""Host-side helpers for the TPL dispenser (svt_hip_tpl_dispense, include/svt_hip_tpl.h): descriptor construction from a case
(tests/tpl_dispenser_cases.py layout: padded numpy planes, ME arrays, controls) and torch-backed runners.  torch is plumbing here;
the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api


def _lib():
    L = api.lib()
    L.svt_hip_tpl_desc_size.restype = C.c_size_t
    return L


def desc_size():
    return _lib().svt_hip_tpl_desc_size()


def plane(ptr, buf, pad, width, height):
    return abi.PlaneDesc(buffer_y=ptr, stride_y=buf.shape[1], org_x=pad, org_y=pad, width=width, height=height)


def make_desc(case, pad, cur, recon, refs, me, tpl_stats, tpl_src_stats):
    """SvtHipTplDesc of a case (level 4 / 5 controls: SAD search, DC_PRED, FULL_PEL = 3, no rate); cur / recon / refs[(l, r)] = (src_ptr, recon_ptr) / me = (total, mv, cand) / outputs: pointers."""
    c = case
    d = abi.TplDesc(aligned_width=c["aligned_width"], aligned_height=c["aligned_height"], n_pu=c["n_pu"], max_cand=c["max_cand"],
                    max_refs=c["max_refs"], max_l0=c["max_l0"], enable_me_16x16=c["enable_me_16x16"], dispenser_search_level=c["level"],
                    subsample_tx=c["sub"], pf_shape=c["pf"], synth_blk_size=c["synth"], disable_intra_pred=c["disable_intra_pred"], is_ref=c["is_ref"],
                    slice_is_i=c["slice_is_i"], tpl_slice_is_i=c["tpl_slice_is_i"], src_pass=c["src_pass"], store_src_stats=c["store_src_stats"],
                    use_sad_in_src_search=1, intra_mode_end=0, subpel_depth=3, compute_rate=0, in_loop_ois=1,
                    n_tpl_stats=len(c["tpl_stats"]), n_tpl_src_stats=len(c["tpl_src_stats"]))
    d.cur = plane(cur, c["cur"], pad, c["width"], c["height"])
    d.recon = plane(recon, c["recon"], pad, c["recon_width"], c["recon_height"])
    for (lst, ref), r in c["refs"].items():
        e = d.refs[lst][ref]
        e.src = plane(refs[(lst, ref)][0], r["src"], pad, c["width"], c["height"])
        e.recon = plane(refs[(lst, ref)][1], r["recon"], pad, c["width"], c["height"])
        e.picture_number, e.max_width, e.max_height, e.usable = r["poc"], r["max_width"], r["max_height"], r["usable"]
    if me is not None:
        d.me.total_me_candidate_index, d.me.me_mv_array, d.me.me_candidate_array = me
    for i, f in enumerate(abi.QUANT_ROW_DTYPE):
        getattr(d.quant, f[0])[:] = c["quant"][f[0]]
    d.tpl_stats, d.tpl_src_stats = tpl_stats, tpl_src_stats
    return d


def check_desc(d):
    """svt_hip_tpl_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_tpl_check_desc", d)


def upload_case(case):
    """Device copies of a case's inputs and outputs (torch uint8 tensors), keyed like the case."""
    dev = api.to_device
    t = dict(cur=dev(case["cur"]), recon=dev(case["recon"]), tpl_stats=dev(case["tpl_stats"]), tpl_src_stats=dev(case["tpl_src_stats"]),
             refs={k: (dev(r["src"]), dev(r["recon"])) for k, r in case["refs"].items()})
    me = case["me"]
    t["me"] = (dev(me["total"]), dev(me["mv"]), dev(me["cand"])) if not case["slice_is_i"] else None
    return t


def dispense_dev(ctx, case, t, pad, me_ptrs=None, recon_ptr=None, ref_ptrs=None):
    """Enqueues svt_hip_tpl_dispense on the device tensors `t` (upload_case layout); me_ptrs / recon_ptr / ref_ptrs override the ME
    result pointers, the recon plane and the (src, recon) planes of references with device buffers the caller already holds."""
    me = me_ptrs if me_ptrs is not None else (tuple(x.data_ptr() for x in t["me"]) if t["me"] is not None else None)
    refs = {k: (v[0].data_ptr(), v[1].data_ptr()) for k, v in t["refs"].items()}
    if ref_ptrs:
        refs.update(ref_ptrs)
    d = make_desc(case, pad, t["cur"].data_ptr(), recon_ptr if recon_ptr is not None else t["recon"].data_ptr(), refs, me,
                  t["tpl_stats"].data_ptr(), t["tpl_src_stats"].data_ptr())
    ctx.check(_lib().svt_hip_tpl_dispense(ctx._h, C.byref(d)), "svt_hip_tpl_dispense")
    return d


def download(case, t):
    return (t["tpl_stats"].cpu().numpy().view(abi.TPL_STATS_DTYPE).copy(), t["tpl_src_stats"].cpu().numpy().view(abi.TPL_SRC_STATS_DTYPE).copy(),
            t["recon"].cpu().numpy().reshape(case["recon"].shape).copy())


def run_tpl_hip(ctx, case, pad):
    """Uploads the case, dispenses it, returns (tpl_stats grid, tpl_src_stats, padded recon plane) as numpy arrays."""
    import torch
    t = upload_case(case)
    torch.cuda.synchronize()
    dispense_dev(ctx, case, t, pad)
    ctx.sync()
    return download(case, t)


# ---- the TPL group: svt_hip_tpl_group (dispense / synthesize / r0beta over a window) ----
OUT_FILL = 0x5C  # bytes the r0beta outputs are pre-filled with: what is not written keeps them


def _group_lib():
    L = api.lib()
    L.svt_hip_tpl_group_desc_size.restype = C.c_size_t
    L.svt_hip_tpl_group_frame_size.restype = C.c_size_t
    return L


def group_desc_size():
    return _group_lib().svt_hip_tpl_group_desc_size()


def group_frame_size():
    return _group_lib().svt_hip_tpl_group_frame_size()


def make_group_desc(win, stages, grids, outputs=None, dispense=None):
    """SvtHipTplGroupDesc of a window (tests/tpl_group_cases.py layout).  grids: per frame (pointer, cells); outputs: per frame None or
    (r0, tpl_is_valid, beta, n_beta, scaling, n_scaling) pointers / counts; dispense: per frame None or an abi.TplDesc.  The frame array
    and the dispenser descriptors are kept alive by the returned descriptor."""
    fr = win["frames"]
    frames = (abi.TplGroupFrame * len(fr))()
    for i, f in enumerate(fr):
        e = frames[i]
        e.picture_number, e.tpl_valid_pic, e.base_rdmult = f["poc"], f["valid"], f["base_rdmult"]
        e.tpl_stats, e.n_tpl_stats = grids[i]
        if outputs and outputs[i] is not None:
            e.r0, e.tpl_is_valid, e.beta, e.n_beta, e.scaling, e.n_scaling = outputs[i]
        if dispense and dispense[i] is not None:
            e.dispense = C.pointer(dispense[i])
    d = abi.TplGroupDesc(width=win["width"], height=win["height"], aligned_width=win["aligned_width"], aligned_height=win["aligned_height"],
                         synth_blk_size=win["synth"], sb_size=win["sb_size"], compute_rate=0, superres_denom=8, stages=stages,
                         n_frames=len(fr), frames=frames)
    d._keep = (frames, dispense)
    return d


def group_check_desc(d):
    """svt_hip_tpl_group_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_tpl_group_check_desc", d)


def upload_window(win, n_beta, n_scaling, tail=4):
    """Device copies of a window: per frame its grid (or, for a dispensed window, its dispenser case's tensors, upload_case), r0 holding
    the frame's r0 value, tpl_is_valid / beta / scaling pre-filled with OUT_FILL and `tail` entries past what stage 3 writes."""
    import torch
    t = dict(frames=[])
    for f in win["frames"]:
        e = {}
        if "case" in f:
            e["case"] = upload_case(f["case"])
            e["grid"] = e["case"]["tpl_stats"]
        else:
            e["grid"] = torch.from_numpy(np.ascontiguousarray(f["grid"]).view(np.uint8).copy()).cuda()
        e["r0"] = torch.tensor([f["r0"]], dtype=torch.float64).cuda()
        e["valid"] = torch.full((1,), OUT_FILL, dtype=torch.uint8).cuda()
        e["beta"] = torch.full(((n_beta + tail) * 8,), OUT_FILL, dtype=torch.uint8).cuda()
        e["scaling"] = torch.full(((n_scaling + tail) * 8,), OUT_FILL, dtype=torch.uint8).cuda()
        t["frames"].append(e)
    return t


def enqueue_group(ctx, win, t, stages, n_beta, n_scaling, outputs=True, over=None):
    """svt_hip_tpl_group on the tensors of upload_window; a dispensed window's pictures take the previous picture's TPL recon as their
    list-0 recon-path reference.  over(desc) may change the descriptor first.  Returns the call's status."""
    grids, outs, disp = [], [], []
    for i, (f, e) in enumerate(zip(win["frames"], t["frames"])):
        grids.append((e["grid"].data_ptr(), e["grid"].numel() // abi.TPL_STATS_DTYPE.itemsize))
        outs.append((e["r0"].data_ptr(), e["valid"].data_ptr(), e["beta"].data_ptr(), n_beta, e["scaling"].data_ptr(), n_scaling)
                    if outputs and f["outputs"] else None)
        if "case" in f:
            tc = e["case"]
            refs = {k: (v[0].data_ptr(), v[1].data_ptr()) for k, v in tc["refs"].items()}
            if i:
                refs[(0, 0)] = (tc["refs"][(0, 0)][0].data_ptr(), t["frames"][i - 1]["case"]["recon"].data_ptr())
            me = tuple(x.data_ptr() for x in tc["me"]) if tc["me"] is not None else None
            disp.append(make_desc(f["case"], 40, tc["cur"].data_ptr(), tc["recon"].data_ptr(), refs, me, tc["tpl_stats"].data_ptr(),
                                  tc["tpl_src_stats"].data_ptr()))
        else:
            disp.append(None)
    d = make_group_desc(win, stages, grids, outs, disp)
    if over:
        over(d)
    return _group_lib().svt_hip_tpl_group(ctx._h, C.byref(d))


def download_window(t):
    """Per frame: (grid, r0, tpl_is_valid, beta bytes as uint64, scaling bytes as uint64, padded recon plane or None)."""
    out = []
    for e in t["frames"]:
        rec = e["case"]["recon"].cpu().numpy().copy() if "case" in e else None
        out.append((e["grid"].cpu().numpy().view(abi.TPL_STATS_DTYPE).copy(), float(e["r0"].cpu()[0]), int(e["valid"].cpu()[0]),
                    e["beta"].cpu().numpy().view(np.uint64).copy(), e["scaling"].cpu().numpy().view(np.uint64).copy(), rec))
    return out


def run_group_hip(ctx, win, stages, n_beta, n_scaling, outputs=True):
    """Uploads a window, runs the stages, returns download_window's per-frame results."""
    import torch
    t = upload_window(win, n_beta, n_scaling)
    torch.cuda.synchronize()
    ctx.check(enqueue_group(ctx, win, t, stages, n_beta, n_scaling, outputs), "svt_hip_tpl_group")
    ctx.sync()
    return download_window(t)
