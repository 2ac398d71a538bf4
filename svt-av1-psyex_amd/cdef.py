"""Host-side helpers of the CDEF entries (svt_hip_cdef_search_batch, svt_hip_cdef_pick_batch, svt_hip_cdef_apply_batch): the ctypes mirrors of
include/svt_hip_cdef.h, runners on device buffers -- the three can be chained on the context stream with no host read in between -- and on host
arrays.  torch is plumbing here; the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import api

MAX_STRENGTHS = 64
MAX_PAIRS = 8
DEFAULT_MSE_UV = 1040400 * 64


class CdefPlane(C.Structure):
    _fields_ = [("plane", C.c_void_p), ("stride", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("reserved", C.c_uint32)]


class CdefSearchDesc(C.Structure):
    _fields_ = [("n_fb", C.c_uint32), ("bit_depth", C.c_uint8), ("base_q_idx", C.c_uint8), ("subsampling_factor", C.c_uint8), ("n_strengths", C.c_uint8),
                ("recon", CdefPlane * 3), ("src", CdefPlane * 3), ("strength_y", C.c_int8 * MAX_STRENGTHS), ("strength_uv", C.c_int8 * MAX_STRENGTHS),
                ("masks", C.c_void_p), ("mse", C.c_void_p), ("dir", C.c_void_p), ("var", C.c_void_p), ("block_dist", C.c_void_p)]


class CdefPick(C.Structure):
    _fields_ = [("cdef_bits", C.c_int32), ("nb_strengths", C.c_int32), ("y_strength", C.c_int32 * MAX_PAIRS), ("uv_strength", C.c_int32 * MAX_PAIRS),
                ("best_cost", C.c_uint64), ("zero_cost", C.c_uint64), ("cdef_dist_dev", C.c_int32), ("reserved", C.c_int32)]


class CdefPickDesc(C.Structure):
    _fields_ = [("n_fb", C.c_uint32), ("n_strengths", C.c_uint32), ("is_hbd", C.c_uint32), ("zero_fs_cost_bias", C.c_uint32), ("full_lambda", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("reserved", C.c_uint32), ("filter_map_y", C.c_uint8 * MAX_STRENGTHS), ("filter_map_uv", C.c_uint8 * MAX_STRENGTHS), ("masks", C.c_void_p),
                ("mse", C.c_void_p), ("work", C.c_void_p), ("result", C.c_void_p), ("fb_strength", C.c_void_p)]


class CdefApplyDesc(C.Structure):
    _fields_ = [("n_fb", C.c_uint32), ("bit_depth", C.c_uint8), ("cdef_damping", C.c_uint8), ("n_planes", C.c_uint8), ("reserved", C.c_uint8),
                ("in", CdefPlane * 3), ("out", CdefPlane * 3), ("masks", C.c_void_p), ("fb_strength", C.c_void_p), ("y_strength", C.c_void_p),
                ("uv_strength", C.c_void_p)]


MIRRORS = (CdefPlane, CdefSearchDesc, CdefPick, CdefPickDesc, CdefApplyDesc)
PICK_DTYPE = np.dtype([("cdef_bits", "<i4"), ("nb_strengths", "<i4"), ("y_strength", "<i4", (MAX_PAIRS,)), ("uv_strength", "<i4", (MAX_PAIRS,)),
                       ("best_cost", "<u8"), ("zero_cost", "<u8"), ("cdef_dist_dev", "<i4"), ("reserved", "<i4")])


def n_fb_of(width, height):
    """The 64x64 filter blocks of a width x height luma picture"""
    return ((width + 63) // 64) * ((height + 63) // 64)


def plane(address, stride, width, height):
    return CdefPlane(plane=address, stride=stride, width=width, height=height)


def planes_of(tensors, width, height, strides=None):
    """Three CdefPlane of a 4:2:0 picture whose planes are the byte tensors `tensors`, tightly packed unless strides (in samples) says otherwise"""
    dims = [(width, height), (width // 2, height // 2), (width // 2, height // 2)]
    return [plane(t.data_ptr(), s if strides is None else strides[i], s, h) for i, (t, (s, h)) in enumerate(zip(tensors, dims))]


def work_bytes():
    """svt_hip_cdef_pick_work_bytes: the scratch of a pick"""
    f = api.lib().svt_hip_cdef_pick_work_bytes
    f.restype = C.c_size_t
    return int(f())


def search_desc(recon, src, bit_depth, base_q_idx, subsampling_factor, strengths_y, strengths_uv, n_fb, masks, mse, dir_, var, block_dist=None):
    """SvtHipCdefSearchDesc.  recon / src: three CdefPlane each; strengths: the two passes' lists concatenated; the rest: addresses"""
    if len(strengths_y) != len(strengths_uv) or len(strengths_y) > MAX_STRENGTHS:
        raise ValueError(f"{len(strengths_y)} luma and {len(strengths_uv)} chroma strengths: as many of each, at most {MAX_STRENGTHS}")
    d = CdefSearchDesc(n_fb=n_fb, bit_depth=bit_depth, base_q_idx=base_q_idx, subsampling_factor=subsampling_factor, n_strengths=len(strengths_y), masks=masks,
                       mse=mse, dir=dir_, var=var, block_dist=block_dist)
    for i in range(3):
        d.recon[i], d.src[i] = recon[i], src[i]
    for i, (y, uv) in enumerate(zip(strengths_y, strengths_uv)):
        d.strength_y[i], d.strength_uv[i] = int(y), int(uv)
    return d


def pick_desc(width, height, n_strengths, is_hbd, zero_fs_cost_bias, full_lambda, filter_map_y, filter_map_uv, masks, mse, work, result, fb_strength, n_fb=None):
    """SvtHipCdefPickDesc of a width x height luma picture; filter_map_*: the strength value of an index, n_strengths of them"""
    d = CdefPickDesc(n_fb=n_fb_of(width, height) if n_fb is None else n_fb, width=width, height=height, n_strengths=n_strengths, is_hbd=is_hbd, zero_fs_cost_bias=zero_fs_cost_bias, full_lambda=full_lambda, masks=masks, mse=mse,
                     work=work, result=result, fb_strength=fb_strength)
    for i, (y, uv) in enumerate(zip(filter_map_y, filter_map_uv)):
        d.filter_map_y[i], d.filter_map_uv[i] = int(y), int(uv)
    return d


def apply_desc(planes_in, planes_out, bit_depth, cdef_damping, n_planes, n_fb, masks, fb_strength, y_strength, uv_strength):
    """SvtHipCdefApplyDesc; planes_*: n_planes CdefPlane each; the rest: addresses"""
    d = CdefApplyDesc(n_fb=n_fb, bit_depth=bit_depth, cdef_damping=cdef_damping, n_planes=n_planes, masks=masks, fb_strength=fb_strength, y_strength=y_strength,
                      uv_strength=uv_strength)
    for i in range(n_planes):
        getattr(d, "in")[i], d.out[i] = planes_in[i], planes_out[i]
    return d


def check_search_desc(d):
    """svt_hip_cdef_search_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_cdef_search_check_desc", d)


def check_pick_desc(d):
    """svt_hip_cdef_pick_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_cdef_pick_check_desc", d)


def check_apply_desc(d):
    """svt_hip_cdef_apply_check_desc: raises api.SvtHipError when the descriptor is refused."""
    api.check_desc("svt_hip_cdef_apply_check_desc", d)


def _sync_torch():
    import torch
    torch.cuda.current_stream().synchronize()  # fills and uploads ran on torch's stream


def run_cdef_search_device(ctx, recon, src, width, height, bit_depth, base_q_idx, subsampling_factor, strengths_y, strengths_uv, masks, with_block_dist=True,
                           spare=0, fill=0):
    """Enqueues svt_hip_cdef_search_batch and returns its outputs as device byte tensors by name ("mse", "dir", "var" and, when asked for,
    "block_dist"), without waiting.  recon / src: three device byte tensors each, tightly packed planes; masks: a device byte tensor of n_fb uint64.
    Every output has `spare` filter blocks more than the picture and starts as the byte `fill`; mse is [2][n_fb][64] with 2 * spare blocks behind it."""
    n_fb, n = n_fb_of(width, height), len(strengths_y)
    outs = {"mse": api.filled(2 * (n_fb + spare) * 64 * 8, fill), "dir": api.filled((n_fb + spare) * 64, fill), "var": api.filled((n_fb + spare) * 64 * 4, fill)}
    if with_block_dist:
        outs["block_dist"] = api.filled((n_fb + spare) * n * 64 * 8, fill)
    _sync_torch()
    d = search_desc(planes_of(recon, width, height), planes_of(src, width, height), bit_depth, base_q_idx, subsampling_factor, strengths_y, strengths_uv, n_fb,
                    masks.data_ptr(), outs["mse"].data_ptr(), outs["dir"].data_ptr(), outs["var"].data_ptr(), api.ptr(outs.get("block_dist")))
    ctx.check(api.lib().svt_hip_cdef_search_batch(ctx._h, C.byref(d)), "svt_hip_cdef_search_batch")
    return outs


def run_cdef_pick_device(ctx, width, height, n_strengths, is_hbd, zero_fs_cost_bias, full_lambda, filter_map_y, filter_map_uv, masks, mse, spare=0, fill=0):
    """Enqueues svt_hip_cdef_pick_batch for a width x height luma picture on mse ([2][n_fb][64] uint64, biased in place) and masks where they lie; returns ({"result": one SvtHipCdefPick
    and `spare` bytes, "fb_strength": n_fb + spare int8} as device byte tensors that start as `fill`, the scratch tensor, which must live until the
    batch is done), without waiting."""
    import torch
    n_fb = n_fb_of(width, height)
    outs = {"result": api.filled(C.sizeof(CdefPick) + spare, fill), "fb_strength": api.filled(n_fb + spare, fill)}
    work = torch.empty((work_bytes(),), dtype=torch.uint8, device="cuda")
    _sync_torch()
    d = pick_desc(width, height, n_strengths, is_hbd, zero_fs_cost_bias, full_lambda, filter_map_y, filter_map_uv, masks.data_ptr(), mse.data_ptr(), work.data_ptr(),
                  outs["result"].data_ptr(), outs["fb_strength"].data_ptr())
    ctx.check(api.lib().svt_hip_cdef_pick_batch(ctx._h, C.byref(d)), "svt_hip_cdef_pick_batch")
    return outs, work


def run_cdef_apply_device(ctx, planes_in, width, height, bit_depth, cdef_damping, n_planes, masks, fb_strength, result, spare=0, fill=0):
    """Enqueues svt_hip_cdef_apply_batch with the strengths of `result` (a device byte tensor that holds an SvtHipCdefPick, such as the pick's) and
    returns the n_planes output planes as device byte tensors, `spare` bytes longer than the plane and `fill` to start with, without waiting."""
    n_fb, bps = n_fb_of(width, height), 2 if bit_depth > 8 else 1
    dims = [(width, height), (width // 2, height // 2), (width // 2, height // 2)][:n_planes]
    outs = [api.filled(w * h * bps + spare, fill) for w, h in dims]
    _sync_torch()
    d = apply_desc(planes_of(planes_in[:n_planes], width, height), planes_of(outs, width, height), bit_depth, cdef_damping, n_planes, n_fb, masks.data_ptr(),
                   fb_strength.data_ptr(), result.data_ptr() + CdefPick.y_strength.offset, result.data_ptr() + CdefPick.uv_strength.offset)
    ctx.check(api.lib().svt_hip_cdef_apply_batch(ctx._h, C.byref(d)), "svt_hip_cdef_apply_batch")
    return outs


def _upload_planes(planes, bit_depth):
    return [api.to_device(p, api.sample_dtype(bit_depth)) for p in planes]


def run_cdef_search_hip(ctx, recon, src, bit_depth, base_q_idx, subsampling_factor, strengths_y, strengths_uv, masks, with_block_dist=True, spare=0, fill=0):
    """svt_hip_cdef_search_batch on host arrays.  recon / src: three planes [height][width] each; masks: n_fb uint64.  Returns "mse" [2][n_fb][64]
    uint64 and "mse_spare" (what lies behind it), "dir" [n_fb + spare][64] uint8, "var" [n_fb + spare][64] int32, "block_dist" [n_fb + spare][n][64] uint64, and "recon" / "src" read back."""
    h, w = recon[0].shape
    t_recon, t_src = _upload_planes(recon, bit_depth), _upload_planes(src, bit_depth)
    t_masks = api.records_to_device(np.asarray(masks, "<u8"), "<u8")
    outs = run_cdef_search_device(ctx, t_recon, t_src, w, h, bit_depth, base_q_idx, subsampling_factor, strengths_y, strengths_uv, t_masks, with_block_dist, spare, fill)
    ctx.sync()
    dt = api.sample_dtype(bit_depth)
    n_fb = n_fb_of(w, h)
    flat = api.to_host(outs["mse"], "<u8")
    out = {"mse": flat[:2 * n_fb * 64].reshape(2, n_fb, 64), "mse_spare": flat[2 * n_fb * 64:], "dir": api.to_host(outs["dir"], np.uint8, (-1, 64)), "var": api.to_host(outs["var"], "<i4", (-1, 64))}
    if with_block_dist:
        out["block_dist"] = api.to_host(outs["block_dist"], "<u8", (-1, len(strengths_y), 64))
    out["recon"] = [api.to_host(t, dt, p.shape) for t, p in zip(t_recon, recon)]
    out["src"] = [api.to_host(t, dt, p.shape) for t, p in zip(t_src, src)]
    return out


def run_cdef_pick_hip(ctx, width, height, mse, masks, n_strengths, is_hbd, zero_fs_cost_bias, full_lambda, filter_map_y, filter_map_uv, spare=0, fill=0):
    """svt_hip_cdef_pick_batch on host arrays.  mse: [2][n_fb][64] uint64.  Returns "result" (a PICK_DTYPE record), "fb_strength" [n_fb + spare] int8,
    "mse" as the bias left it, and "tail": the `spare` bytes behind the result."""
    n_fb = len(masks)
    t_mse, t_masks = api.to_device(np.asarray(mse, "<u8")), api.records_to_device(np.asarray(masks, "<u8"), "<u8")
    outs, work = run_cdef_pick_device(ctx, width, height, n_strengths, is_hbd, zero_fs_cost_bias, full_lambda, filter_map_y, filter_map_uv, t_masks, t_mse, spare, fill)
    ctx.sync()
    del work
    raw = api.to_host(outs["result"])
    return {"result": raw[:PICK_DTYPE.itemsize].view(PICK_DTYPE)[0], "tail": raw[PICK_DTYPE.itemsize:], "fb_strength": api.to_host(outs["fb_strength"], np.int8),
            "mse": api.to_host(t_mse, "<u8", (2, n_fb, 64))}


def run_cdef_apply_hip(ctx, planes_in, bit_depth, cdef_damping, n_planes, masks, fb_strength, y_strength, uv_strength, spare=0, fill=0):
    """svt_hip_cdef_apply_batch on host arrays.  planes_in: three planes [height][width]; y_strength / uv_strength: up to 8 strength values.  Returns
    "planes" (n_planes arrays, each flat and `spare` bytes longer than its plane) and "in" read back."""
    h, w = planes_in[0].shape
    dt = api.sample_dtype(bit_depth)
    t_in = _upload_planes(planes_in, bit_depth)
    rec = np.zeros(1, PICK_DTYPE)
    rec["y_strength"][0, :len(y_strength)], rec["uv_strength"][0, :len(uv_strength)] = y_strength, uv_strength
    t_rec, t_masks = api.to_device(rec), api.records_to_device(np.asarray(masks, "<u8"), "<u8")
    t_fbs = api.records_to_device(np.asarray(fb_strength, np.int8), np.int8)
    outs = run_cdef_apply_device(ctx, t_in, w, h, bit_depth, cdef_damping, n_planes, t_masks, t_fbs, t_rec, spare, fill)
    ctx.sync()
    return {"planes": [api.to_host(t) for t in outs], "in": [api.to_host(t, dt, p.shape) for t, p in zip(t_in, planes_in)]}
