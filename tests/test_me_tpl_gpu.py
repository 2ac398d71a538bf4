"""GPU: the ME -> TPL chain on one stream.  svt_hip_me_picture_async / svt_hip_me_pictures_async write their results into device buffers
and svt_hip_tpl_dispense / svt_hip_tpl_group read them from there, enqueued back to back: no synchronisation and no host copy between the
two, one sync at the end.  Everything is compared bit for bit with the oracle's ME, with the dispenser's / group's restatement fed with
the oracle's ME arrays (tests/me_tpl_cases.py) and with the reference fixture tests/golden/tpl_me_chain.npz.  Both forms of the ME pipeline."""
import ctypes as C

import numpy as np
import pytest

import me_tpl_cases as mt
import tpl_group_cases as gc
from me_cases import compare, fill_unsearched
from svt_av1_psyex_amd import abi, api, tpl
from tpl_dispenser_cases import assert_same
from test_tpl_group_gpu import assert_group, from_fixture

pytestmark = pytest.mark.gpu
ME_FILL = 0xA5


@pytest.fixture(scope="module", autouse=True, params=[0, 2], ids=["one-kernel", "staged"])
def me_form(request, hip_ctx):
    """Every chain runs with the ME's per-block pipeline as one kernel and as the chain of small kernels (the default picks by launch
    size); the context is session-scoped, so the default comes back afterwards."""
    hip_ctx.set_me_staged(request.param)
    yield request.param
    hip_ctx.set_me_staged(1)


@pytest.fixture(scope="module")
def fixture():
    return mt.load_fixture()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def me_buffers(desc):
    """Device buffers for every ME result of a picture, pre-filled with ME_FILL: (abi.MeResults of device pointers, tensors, n_b64)."""
    import torch
    n = abi.n_pu(desc.enable_me_16x16, desc.enable_me_8x8)
    nb = ((desc.aligned_width + 63) // 64) * ((desc.aligned_height + 63) // 64)
    res, bufs = abi.MeResults(), {}
    for name, dt, cnt in abi.RESULT_FIELDS:
        bufs[name] = torch.full((nb * cnt(n, desc.max_refs, desc.max_cand) * np.dtype(dt).itemsize,), ME_FILL, dtype=torch.uint8, device="cuda")
        setattr(res, name, bufs[name].data_ptr())
    return res, bufs, nb


def me_download(desc, bufs, nb):
    return fill_unsearched(desc, {name: bufs[name].cpu().numpy().view(dt).reshape(nb, -1).copy() for name, dt, _ in abi.RESULT_FIELDS})


def me_ptrs(res):
    return res.total_me_candidate_index, res.me_mv_array, res.me_candidate_array  # tpl.make_desc's order: total, mv, cand


def picture(ctx, pyramid):
    """(plane tensor, SvtHipPaPicture made from it on the device) of a HostPyramid's padded full-resolution plane."""
    buf, stride, pad, w, h = pyramid.planes[2]
    t = dev(buf)
    return t, ctx.upload_dev(t.data_ptr(), stride, w, h, pad, pyramid.picture_number)


def own_plane(pic, W, H):
    g = pic.geometry(2)
    assert (g.width, g.height) == (W, H) and g.org_x >= abi.TPL_PAD and g.org_y >= abi.TPL_PAD
    return g


@pytest.mark.parametrize("name", list(mt.SINGLE))
def test_me_then_dispense_on_one_stream(hip_ctx, fixture, name):
    import torch
    mc, own = mt.me_case(name), mt.SINGLE[name][1].get("own_planes", False)
    case, want = mt.oracle_single(name)
    cur_t, cur = picture(hip_ctx, mc.cur)
    refs = {k: picture(hip_ctx, v) for k, v in mc.refs.items()}
    try:
        res, bufs, nb = me_buffers(mc.desc)
        out = dict(recon=dev(case["recon"]), tpl_stats=dev(case["tpl_stats"]), tpl_src_stats=dev(case["tpl_src_stats"]))
        ref_recon = {k: dev(r["recon"]) for k, r in case["refs"].items()}
        d = tpl.make_desc(case, mt.PAD, cur_t.data_ptr(), out["recon"].data_ptr(), {k: (refs[k][0].data_ptr(), ref_recon[k].data_ptr()) for k in refs},
                          me_ptrs(res), out["tpl_stats"].data_ptr(), out["tpl_src_stats"].data_ptr())
        if own:  # ME and TPL read one copy: the picture's own full-resolution plane
            d.cur = own_plane(cur, mc.width, mc.height)
            for (li, ri), (_, pic) in refs.items():
                d.refs[li][ri].src = own_plane(pic, mc.width, mc.height)
        torch.cuda.synchronize()  # the uploads ran on torch's stream
        hip_ctx.me_picture_async(mc.cfg, mc.desc, cur, {k: v[1] for k, v in refs.items()}, res)
        hip_ctx.check(api.lib().svt_hip_tpl_dispense(hip_ctx._h, C.byref(d)), "svt_hip_tpl_dispense")
        hip_ctx.sync()
        got_me = me_download(mc.desc, bufs, nb)
        got = tpl.download(case, out)
    finally:
        cur.free()
        for _, pic in refs.values():
            pic.free()
    assert not compare(mt.oracle_me(name), got_me), name
    assert_same(case, got, want, name)
    if name in fixture:
        mt.assert_equals_fixture(fixture[name], got, name + " (fixture)")


class Window:
    """A chain window on the device: the pictures, the ME result buffers of pictures 1 .. 3 and the group's buffers (the layout of
    tpl.upload_window, so tpl.download_window reads them)."""

    def __init__(self, ctx, name):
        import torch
        self.ctx, self.name = ctx, name
        self.win = win = mt.oracle_window(name)[0]
        mcs = mt.window_me_cases(name)
        W, H = win["width"], win["height"]
        self.nb, self.ns = gc.n_beta(win), gc.n_scaling(win)
        pyramids = [mcs[0].refs[(0, 0)]] + [mc.cur for mc in mcs]
        assert [p.picture_number for p in pyramids] == list(range(mt.N_WINDOW))
        self.pics = [picture(ctx, p) for p in pyramids]
        self.me = [me_buffers(mc.desc) for mc in mcs]
        self.jobs = [(mc.cfg, mc.desc, self.pics[i + 1][1], {(0, 0): self.pics[i][1]}, self.me[i][0]) for i, mc in enumerate(mcs)]
        self.t = dict(frames=[])
        disp = []
        for i, f in enumerate(win["frames"]):
            c = f["case"]
            e = dict(case=dict(recon=dev(c["recon"]), tpl_stats=dev(c["tpl_stats"]), tpl_src_stats=dev(c["tpl_src_stats"])),
                     r0=torch.tensor([f["r0"]], dtype=torch.float64).cuda(), valid=torch.full((1,), tpl.OUT_FILL, dtype=torch.uint8).cuda(),
                     beta=torch.full(((self.nb + 4) * 8,), tpl.OUT_FILL, dtype=torch.uint8).cuda(),
                     scaling=torch.full(((self.ns + 4) * 8,), tpl.OUT_FILL, dtype=torch.uint8).cuda())
            e["grid"] = e["case"]["tpl_stats"]
            self.t["frames"].append(e)
            refs = {(0, 0): (self.pics[i - 1][0].data_ptr(), self.t["frames"][i - 1]["case"]["recon"].data_ptr())} if i else {}
            d = tpl.make_desc(c, mt.PAD, self.pics[i][0].data_ptr(), e["case"]["recon"].data_ptr(), refs, me_ptrs(self.me[i - 1][0]) if i else None,
                              e["grid"].data_ptr(), e["case"]["tpl_src_stats"].data_ptr())
            if mt.WINDOWS[name].get("own_planes"):
                d.cur = own_plane(self.pics[i][1], W, H)
                if i:
                    d.refs[0][0].src = own_plane(self.pics[i - 1][1], W, H)
            disp.append(d)
        grids = [(e["grid"].data_ptr(), e["grid"].numel() // abi.TPL_STATS_DTYPE.itemsize) for e in self.t["frames"]]
        outs = [(e["r0"].data_ptr(), e["valid"].data_ptr(), e["beta"].data_ptr(), self.nb, e["scaling"].data_ptr(), self.ns) for e in self.t["frames"]]
        self.desc = tpl.make_group_desc(win, gc.STAGES_ALL, grids, outs, disp)
        self.outputs = [b for _, bufs, _ in self.me for b in bufs.values()]
        for e in self.t["frames"]:
            self.outputs += [e["case"]["recon"], e["grid"], e["case"]["tpl_src_stats"], e["r0"], e["valid"], e["beta"], e["scaling"]]
        self.initial = [b.clone() for b in self.outputs]
        torch.cuda.synchronize()

    def refill(self):
        import torch
        for b, a in zip(self.outputs, self.initial):
            b.copy_(a)
        torch.cuda.synchronize()

    def run(self):
        """The ME of pictures 1 .. 3 as one launch, then the three stages of the group as one call, then the only sync."""
        self.ctx.me_pictures_async(self.jobs)
        self.ctx.check(api.lib().svt_hip_tpl_group(self.ctx._h, C.byref(self.desc)), "svt_hip_tpl_group")
        self.ctx.sync()
        mcs = mt.window_me_cases(self.name)
        return [me_download(mc.desc, bufs, nb) for mc, (_, bufs, nb) in zip(mcs, self.me)], tpl.download_window(self.t)

    def free(self):
        for _, pic in self.pics:
            pic.free()


@pytest.mark.parametrize("name", list(mt.WINDOWS))
def test_me_launch_then_group_on_one_stream(hip_ctx, fixture, name):
    win, _, recons, grids, outs = mt.oracle_window(name)
    w = Window(hip_ctx, name)
    try:
        me1, got1 = w.run()
        w.refill()
        me2, got2 = w.run()
    finally:
        w.free()
    for i, (want, a) in enumerate(zip(mt.oracle_window_me(name), me1)):
        assert not compare(want, a), f"{name}: ME of picture {i + 1}"
    assert_group(win, got1, grids, outs, name)
    for i, want in enumerate(recons):
        np.testing.assert_array_equal(got1[i][5].reshape(want.shape), want, err_msg=f"{name}: frame {i}: recon")
    if name == mt.FIXTURE_WINDOW:
        rec = fixture["window_" + name]
        assert_group(win, got1, *from_fixture(win, rec, None), name + " (fixture)")
        np.testing.assert_array_equal(np.stack([mt.plane_sha(g[5].reshape(recons[0].shape)) for g in got1]), rec["recon_sha"], err_msg="recon planes (fixture)")
    # the same buffers again, outputs refilled: identical results
    for i, (a, b) in enumerate(zip(me1, me2)):
        assert not compare(a, b), f"{name}: second run: ME of picture {i + 1}"
    for i, (a, b) in enumerate(zip(got1, got2)):
        assert a[0].tobytes() == b[0].tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes() and a[2] == b[2], f"{name}: second run: frame {i}"
        assert (a[3] == b[3]).all() and (a[4] == b[4]).all() and (a[5] == b[5]).all(), f"{name}: second run: frame {i}"
