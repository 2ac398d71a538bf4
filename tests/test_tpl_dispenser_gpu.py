"""GPU: svt_hip_tpl_dispense against the restatement of tests/tpl_dispenser_cases.py -- the TplStats grid, the TplSrcStats and the
whole padded recon plane, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from svt_av1_psyex_amd import api, tpl
from tpl_dispenser_cases import PAD, assert_same, make_case, restate, seeded_grid, src_pass0_case

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name,kw", seeded_grid())
def test_dispense_vs_restatement(hip_ctx, name, kw):
    c = make_case(**kw)
    assert_same(c, tpl.run_tpl_hip(hip_ctx, c, PAD), restate(c), name)


def test_dispense_with_stored_source_stats(hip_ctx):
    c = src_pass0_case(61, W=200, H=136)
    assert_same(c, tpl.run_tpl_hip(hip_ctx, c, PAD), restate(c), "src_pass 0")


def test_dispense_1080p_level4_synth32(hip_ctx):
    c = make_case(70, 1920, 1080, level=0, sub=0, synth=32, pf=2)
    assert_same(c, tpl.run_tpl_hip(hip_ctx, c, PAD), restate(c), "1080p")


def test_group_of_four_on_the_device(hip_ctx):
    """Four pictures, each one's TPL recon the next one's recon-path reference (list 0, ref 0), kept on the device throughout."""
    import torch
    kw = dict(W=200, H=136, level=0, sub=0, synth=16, n_refs=(1, 0))
    cases = [make_case(80 + i, **kw) for i in range(4)]
    cases[0]["slice_is_i"] = cases[0]["tpl_slice_is_i"] = 1
    cases[-1]["is_ref"] = 0
    cases[-1]["disable_intra_pred"] = 1
    prev_rec_host, prev_rec_dev = None, None
    for i, c in enumerate(cases):
        if prev_rec_host is not None:
            c["refs"][(0, 0)]["recon"] = prev_rec_host
        t = tpl.upload_case(c)
        torch.cuda.synchronize()
        tpl.dispense_dev(hip_ctx, c, t, PAD, ref_ptrs={(0, 0): (t["refs"][(0, 0)][0].data_ptr(), prev_rec_dev.data_ptr())} if prev_rec_dev is not None else None)
        want = restate(c)
        hip_ctx.sync()
        assert_same(c, tpl.download(c, t), want, f"picture {i}")
        prev_rec_host, prev_rec_dev = want[2], t["recon"]


def test_refused_descriptor_leaves_outputs_untouched(hip_ctx):
    import torch
    c = make_case(90, 128, 96)
    t = tpl.upload_case(c)
    for k in ("recon", "tpl_stats", "tpl_src_stats"):
        t[k].fill_(0x5C)
    torch.cuda.synchronize()
    for field, value in (("compute_rate", 1), ("dispenser_search_level", 2), ("synth_blk_size", 8), ("use_sad_in_src_search", 0)):
        d = tpl.make_desc(c, PAD, t["cur"].data_ptr(), t["recon"].data_ptr(), {k: (v[0].data_ptr(), v[1].data_ptr()) for k, v in t["refs"].items()},
                          tuple(x.data_ptr() for x in t["me"]), t["tpl_stats"].data_ptr(), t["tpl_src_stats"].data_ptr())
        setattr(d, field, value)
        assert api.lib().svt_hip_tpl_dispense(hip_ctx._h, C.byref(d)) == 2  # SVT_HIP_ERR_BAD_PARAM
    hip_ctx.sync()
    for k in ("recon", "tpl_stats", "tpl_src_stats"):
        assert (t[k].cpu().numpy() == 0x5C).all(), k


def test_dispense_vs_reference_fixture(hip_ctx):
    """The device against the reference's own dispenser (tests/golden/tpl_dispenser.npz, tools/gen_tpl_golden.py), bit for bit."""
    from test_tpl_dispenser import fixture
    n = 0
    for name, c, want in fixture():
        assert_same(c, tpl.run_tpl_hip(hip_ctx, c, PAD), want, name)
        n += 1
    assert n == 15
