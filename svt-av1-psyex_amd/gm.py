"""Host-side helpers of the global-motion entries (svt_hip_gm_refine_batch, svt_hip_gm_correspondence_batch): runners on device buffers (the
correspondences read the result arrays an asynchronous ME launch wrote; the refined models are the array svt_hip_warp_pred_batch takes) and on host
arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api
from .warp import plane_ref

REFINE_OUT_DTYPES = {"models": abi.WARP_MODEL_DTYPE, "best_error": "<i8", "pic_sad": "<u4", "status": "u1"}
ME_ARRAYS = ("total_me_candidate_index", "me_candidate_array", "me_mv_array", "rc_me_distortion", "stationary_block_present_sb", "rc_me_allow_gm")


def work_bytes(n_jobs):
    """svt_hip_gm_refine_work_bytes: the scratch a refine batch of n_jobs jobs needs"""
    f = api.lib().svt_hip_gm_refine_work_bytes
    f.restype, f.argtypes = C.c_size_t, [C.c_uint32]
    return int(f(n_jobs))


def refine_desc(src, refs, n_refinements, chess_refn, rfn_early_exit, jobs, n_jobs, work, outs, round_error=None):
    """SvtHipGmRefineDesc from an abi.WarpRef for the source, a list of them for the references, and addresses (ints); outs: addresses by the names
    of REFINE_OUT_DTYPES"""
    if len(refs) > abi.WARP_MAX_REFS:
        raise ValueError(f"{len(refs)} reference planes: at most {abi.WARP_MAX_REFS}")
    d = abi.GmRefineDesc(n_jobs=n_jobs, n_refs=len(refs), n_refinements=n_refinements, chess_refn=chess_refn, rfn_early_exit=rfn_early_exit, src=src,
                         jobs=jobs, work=work, round_error=round_error, **outs)
    for i, r in enumerate(refs):
        d.refs[i] = r
    return d


def check_refine_desc(d):
    """svt_hip_gm_refine_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_gm_refine_check_desc", d)


def check_corr_desc(d):
    """svt_hip_gm_corr_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_gm_corr_check_desc", d)


def run_gm_refine_device(ctx, src, refs, n_refinements, chess_refn, rfn_early_exit, jobs, n_jobs, with_round_error=True, spare=0, fill=0):
    """Enqueues svt_hip_gm_refine_batch on the context stream and returns (the outputs as device byte tensors by name -- "round_error" among them
    when asked for --, the scratch tensor, which must live until the batch is done), without waiting.  src: an abi.WarpRef, refs: a list of them;
    jobs: a device tensor of abi.GM_REFINE_JOB_DTYPE records.  Every output has `spare` slots past n_jobs and starts as the byte `fill`."""
    import torch
    sizes = {k: np.dtype(dt).itemsize for k, dt in REFINE_OUT_DTYPES.items()}
    if with_round_error:
        sizes["round_error"] = 8 * abi.GM_ROUND_ERRORS
    outs = {k: api.filled(max(1, n_jobs + spare) * sz, fill) for k, sz in sizes.items()}
    work = torch.empty((work_bytes(n_jobs),), dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()  # the fills ran on torch's stream
    d = refine_desc(src, refs, n_refinements, chess_refn, rfn_early_exit, jobs.data_ptr(), n_jobs, work.data_ptr(),
                    {k: outs[k].data_ptr() for k in REFINE_OUT_DTYPES}, outs["round_error"].data_ptr() if with_round_error else None)
    ctx.check(api.lib().svt_hip_gm_refine_batch(ctx._h, C.byref(d)), "svt_hip_gm_refine_batch")
    return outs, work


def run_gm_refine_hip(ctx, src, planes, n_refinements, chess_refn, rfn_early_exit, jobs, with_round_error=True, spare=0, fill=0):
    """svt_hip_gm_refine_batch on host arrays.  src and every entry of planes: (padded plane [rows][stride] uint8, org_x, org_y, picture width, picture
    height); jobs: abi.GM_REFINE_JOB_DTYPE.  Returns the outputs by name, each [n + spare] (round_error [n + spare][61]), and "planes" / "src" read
    back."""
    n = len(jobs)
    t_planes = [api.to_device(p[0], np.uint8) for p in [src] + list(planes)]
    refs = [plane_ref(t, p[0].shape[1], p[1], p[2], p[3], p[4], p[0].shape[0]) for t, p in zip(t_planes, [src] + list(planes))]
    t_jobs = api.records_to_device(jobs, abi.GM_REFINE_JOB_DTYPE)
    outs, work = run_gm_refine_device(ctx, refs[0], refs[1:], n_refinements, chess_refn, rfn_early_exit, t_jobs, n, with_round_error, spare, fill)
    ctx.sync()
    del work
    out = {k: api.to_host(outs[k], np.dtype(dt)) for k, dt in REFINE_OUT_DTYPES.items()}
    if with_round_error:
        out["round_error"] = api.to_host(outs["round_error"], "<i8", (-1, abi.GM_ROUND_ERRORS))
    out["src"] = api.to_host(t_planes[0], shape=src[0].shape)
    out["planes"] = [api.to_host(t, shape=p[0].shape) for t, p in zip(t_planes[1:], planes)]
    return out


def corr_desc(pic, method, shift, pairs, cap, me, corr, count, sums):
    """SvtHipGmCorrDesc.  pic: an abi.MePictureDesc (aligned size, enable_me_8x8 / _16x16, max_cand, max_refs, max_l0) or a mapping with those
    names; pairs: (list, ref) tuples; me: an abi.MeResults of device pointers; corr / count / sums: addresses"""
    get = (lambda k: pic[k]) if isinstance(pic, dict) else (lambda k: getattr(pic, k))
    if len(pairs) > abi.GM_MAX_PAIRS:
        raise ValueError(f"{len(pairs)} pairs: at most {abi.GM_MAX_PAIRS}")
    d = abi.GmCorrDesc(aligned_width=get("aligned_width"), aligned_height=get("aligned_height"), enable_me_8x8=get("enable_me_8x8"),
                       enable_me_16x16=get("enable_me_16x16"), max_cand=get("max_cand"), max_refs=get("max_refs"), max_l0=get("max_l0"),
                       n_pu=abi.n_pu(get("enable_me_16x16"), get("enable_me_8x8")), method=method, shift=shift, n_pairs=len(pairs), cap=cap, me=me, corr=corr,
                       count=count, sums=sums)
    for i, (li, ri) in enumerate(pairs):
        d.pairs[i].list, d.pairs[i].ref = li, ri
    return d


def run_gm_correspondence_device(ctx, pic, method, shift, pairs, me, cap=None, spare=0, fill=0):
    """Enqueues svt_hip_gm_correspondence_batch on the context stream and returns {"corr": int32 [pairs + spare][cap][4], "count": uint32 [pairs +
    spare], "sums": uint32 [3 + spare]} as device tensors that start as the byte `fill`, without waiting.  me: an abi.MeResults of device pointers such
    as an asynchronous ME launch filled."""
    import torch
    get = (lambda k: pic[k]) if isinstance(pic, dict) else (lambda k: getattr(pic, k))
    if cap is None:
        cap = (1 << (2 * method)) * ((get("aligned_width") + 63) // 64) * ((get("aligned_height") + 63) // 64)
    word = np.frombuffer(bytes([fill]) * 4, "<i4")[0].item()
    outs = {"corr": torch.full((max(1, len(pairs) + spare), cap, 4), word, dtype=torch.int32, device="cuda"),
            "count": torch.full((max(1, len(pairs) + spare),), word, dtype=torch.int32, device="cuda"),
            "sums": torch.full((3 + spare,), word, dtype=torch.int32, device="cuda")}
    torch.cuda.current_stream().synchronize()
    d = corr_desc(pic, method, shift, pairs, cap, me, outs["corr"].data_ptr(), outs["count"].data_ptr(), outs["sums"].data_ptr())
    ctx.check(api.lib().svt_hip_gm_correspondence_batch(ctx._h, C.byref(d)), "svt_hip_gm_correspondence_batch")
    return outs


def run_gm_correspondence_hip(ctx, pic, method, shift, pairs, arrays, cap=None, spare=0, fill=0):
    """svt_hip_gm_correspondence_batch on host arrays.  arrays: the six ME result arrays of ME_ARRAYS by name (numpy, [n_b64][...]).  Returns
    {"corr", "count" (uint32), "sums" (uint32)} as numpy arrays."""
    me, keep = abi.MeResults(), []
    for name in ME_ARRAYS:
        keep.append(api.to_device(arrays[name]))
        setattr(me, name, keep[-1].data_ptr())
    outs = run_gm_correspondence_device(ctx, pic, method, shift, pairs, me, cap, spare, fill)
    ctx.sync()
    return {"corr": outs["corr"].cpu().numpy(), "count": outs["count"].cpu().numpy().view(np.uint32), "sums": outs["sums"].cpu().numpy().view(np.uint32)}
