"""GPU: the host runtime under the entries (csrc/context.cpp): the grow-on-demand buffers of a lane and of the context when a small call
follows a large one, the leaf binding of a context that is destroyed, the transfer stream.  Every test makes its own context: the buffers
start empty and nothing another test left in the session's context takes part."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from me_cases import MeCase, compare, fill_unsearched
from svt_av1_psyex_amd import abi, api, synth, tpl

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    c = api.Context()
    yield c
    c.close()


def dense_bytes(ctx):
    """the size svt_hip_me_dense_slots reports; without a buffer to copy into the entry does not wait for the launch"""
    L = api.lib()
    L.svt_hip_me_dense_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    n = C.c_size_t()
    ctx.check(L.svt_hip_me_dense_slots(ctx._h, None, 0, C.byref(n)), "svt_hip_me_dense_slots")
    return n.value


def test_me_launch_buffers_grow_under_enqueued_launches(ctx):
    """Staged launches with a pre-pass use the lane's slot buffer and its stage buffer.  2 blocks, 15 blocks (both buffers are freed and
    replaced), 2 blocks again, the last two enqueued back to back: every result equals the oracle's."""
    import torch
    ctx.set_me_dense(True)
    ctx.set_me_staged(2)
    small, large = MeCase(128, 64, enc_mode=6), MeCase(320, 192, enc_mode=6, seed=7)
    want = {id(c): c.run_cpu("oracle") for c in (small, large)}
    runs = []
    for c in (small, large, small):
        cur, refs = ctx.upload(c.cur), {k: ctx.upload(v) for k, v in c.refs.items()}
        n = abi.n_pu(c.desc.enable_me_16x16, c.desc.enable_me_8x8)
        nb = ((c.width + 63) // 64) * ((c.height + 63) // 64)
        res, keep = abi.MeResults(), {}
        for name, dt, cnt in abi.RESULT_FIELDS:
            t = torch.zeros(nb * cnt(n, c.desc.max_refs, c.desc.max_cand) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
            keep[name] = (t, dt)
            setattr(res, name, t.data_ptr())
        runs.append((c, cur, refs, res, keep, nb))
    torch.cuda.synchronize()
    ctx.sync()
    sizes = []
    for c, cur, refs, res, _, _ in runs:  # no synchronise in between: the launcher waits where it has to free a block
        ctx.me_picture_async(c.cfg, c.desc, cur, refs, res)
        sizes.append(dense_bytes(ctx))
    ctx.sync()
    # one 16-byte slot per block, searched reference (two here) and kind (SVT_HIP_ME_DENSE_KINDS = 6)
    assert sizes == [nb * 2 * 6 * 16 for *_, nb in runs] and sizes[1] > sizes[0] == sizes[2], sizes
    for i, (c, cur, refs, _, keep, _) in enumerate(runs):
        w = want[id(c)]
        got = fill_unsearched(c.desc, {name: t.cpu().numpy().view(dt).reshape(w[name].shape) for name, (t, dt) in keep.items()})
        assert not compare(w, got), i
        cur.free()
        for r in refs.values():
            r.free()


def test_tpl_scratch_grows_and_is_reused(ctx):
    """The dispenser's per-block state: 16, 128 and 16 blocks of 16x16"""
    from tpl_dispenser_cases import PAD, assert_same, make_case, restate
    for seed, (w, h) in zip((31, 32, 33), ((64, 64), (256, 128), (64, 64))):
        c = make_case(seed, w, h, level=0, sub=0, synth=16)
        assert_same(c, tpl.run_tpl_hip(ctx, c, PAD), restate(c), f"{w}x{h}")


def test_lane_scratch_grows_and_is_reused(ctx):
    """svt_hip_dg_detector_hme_level0 takes its result block (metrics, a SAD and a vector per 64x64 block) from the borrowed lane's scratch:
    1 block, 4096 blocks, 1 block.  Resolution class 0 keeps the search at 16x16 positions, so the oracle is quick at 4096x4096 too."""
    rng = np.random.default_rng(5)
    for w, h in ((64, 64), (4096, 4096), (64, 64)):
        src = synth.HostPyramid(rng.integers(0, 256, (h, w), dtype=np.uint8), 1)
        ref = synth.HostPyramid(rng.integers(0, 256, (h, w), dtype=np.uint8), 0)
        want = pyoracle.dg_detector("oracle", src, ref, w, h, 0)
        s, r = ctx.upload(src), ctx.upload(ref)
        try:
            got = ctx.dg_detector_hme_level0(s, r, w, h, 0)
        finally:
            s.free()
            r.free()
        assert got["b64_sad"].shape == ((w // 64) * (h // 64),)
        for k in want:
            assert np.array_equal(want[k], got[k]), (w, h, k)


def test_destroying_the_bound_context_unbinds_it():
    """A `_hip` entry called after its context is gone goes to the previous kernel: it does not touch the freed context."""
    L = api.lib()
    VAR = C.CFUNCTYPE(C.c_uint, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint))

    class Slot(C.Structure):
        _fields_ = [("name", C.c_char_p), ("slot", C.POINTER(C.c_void_p))]

    calls = []

    def stand_in(src, ss, ref, rs, sse):
        calls.append((ss, rs))
        sse[0] = 777
        return 55

    keep = VAR(stand_in)
    val = C.c_void_p(C.cast(keep, C.c_void_p).value)
    slots = (Slot * 1)(Slot(b"svt_aom_variance16x16", C.pointer(val)))
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 256, (16, 16), dtype=np.uint8), rng.integers(0, 256, (16, 16), dtype=np.uint8)
    d = a.astype(np.int64) - b
    want_sse = int((d * d).sum())
    want_var = want_sse - int(d.sum()) ** 2 // 256  # aom variance: sse - sum^2 / (w h)
    sse = C.c_uint(0)
    ctx = api.Context()
    try:
        assert L.svt_hip_rtcd_store(slots, 1, None) == 0
        assert L.svt_hip_leaf_bind(ctx._h) == 0
        L.svt_hip_leaf_status(None, None, None, C.c_size_t(0))
        assert VAR(val.value)(a.ctypes.data, 16, b.ctypes.data, 16, C.byref(sse)) == want_var and sse.value == want_sse
        assert calls == [] and L.svt_hip_leaf_status(None, None, None, C.c_size_t(0)) == 0  # the device computed it
        ctx.close()
        assert VAR(val.value)(a.ctypes.data, 16, b.ctypes.data, 16, C.byref(sse)) == 55 and sse.value == 777
        fb, un = C.c_ulonglong(0), C.c_ulonglong(0)
        msg = C.create_string_buffer(512)
        L.svt_hip_leaf_status(C.byref(fb), C.byref(un), msg, C.c_size_t(512))
        assert calls == [(16, 16)] and (fb.value, un.value) == (1, 0) and b"no context bound" in msg.value
    finally:
        ctx.close()
        L.svt_hip_leaf_bind(None)
        L.svt_hip_uninstall_rtcd(slots, 1)


def test_transfer_stream_is_made_once_and_carries_a_refill(ctx):
    L = api.lib()
    L.svt_hip_context_transfer_stream.restype = C.c_void_p
    L.svt_hip_context_transfer_stream.argtypes = [C.c_void_p]
    io = L.svt_hip_context_transfer_stream(ctx._h)
    assert io and io != ctx.stream and L.svt_hip_context_transfer_stream(ctx._h) == io
    rng = np.random.default_rng(3)
    first = synth.HostPyramid(rng.integers(0, 256, (64, 64), dtype=np.uint8))
    other = synth.HostPyramid(rng.integers(0, 256, (64, 64), dtype=np.uint8))
    pic = ctx.upload(first)
    try:
        full = other.desc(2)
        ctx.check(L.svt_hip_pa_picture_update_ahead(ctx._h, pic._h, C.byref(full), 0), "svt_hip_pa_picture_update_ahead")
        assert L.svt_hip_context_transfer_stream(ctx._h) == io
        for level in (2, 1, 0):  # the download waits for the refill through the picture's event
            buf, _, pad, w, _ = other.planes[level]
            assert np.array_equal(pic.download(level), buf[:, :w + 2 * pad]), level
    finally:
        pic.free()
