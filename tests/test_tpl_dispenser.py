"""CPU: the TPL dispenser's C-ABI (descriptor size, host-side validation) and the restatement's own consistency
(tests/tpl_dispenser_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from svt_av1_psyex_amd import abi, api, tpl
from tpl_dispenser_cases import PAD, dc_pred, make_case, restate, seeded_grid, src_pass0_case

FIELDS_S = ("srcrf_dist", "recrf_dist", "srcrf_rate", "recrf_rate", "mc_dep_rate", "mc_dep_dist", "mv_row", "mv_col", "ref_frame_poc")
FIELDS_SRC = ("srcrf_dist", "srcrf_rate", "ref_frame_poc", "mv_row", "mv_col", "best_mode", "best_rf_idx", "best_intra_mode")


def fake_desc(case, **over):
    """A descriptor of the case with host addresses as stand-ins: svt_hip_tpl_check_desc reads no sample."""
    keep = [case["cur"], case["recon"], case["tpl_stats"], case["tpl_src_stats"]]
    refs = {k: (r["src"].ctypes.data, r["recon"].ctypes.data) for k, r in case["refs"].items()}
    me = tuple(case["me"][k].ctypes.data for k in ("total", "mv", "cand"))
    d = tpl.make_desc(case, PAD, keep[0].ctypes.data, keep[1].ctypes.data, refs, me, keep[2].ctypes.data, keep[3].ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_desc_size_matches_ctypes():
    assert tpl.desc_size() == C.sizeof(abi.TplDesc)
    assert abi.TPL_STATS_DTYPE.itemsize == 64 and abi.TPL_SRC_STATS_DTYPE.itemsize == 40


@pytest.mark.parametrize("name,kw", seeded_grid())
def test_check_desc_accepts_the_cases(name, kw):
    tpl.check_desc(fake_desc(make_case(**kw)))


@pytest.mark.parametrize("field,value", [("use_sad_in_src_search", 0), ("intra_mode_end", 12), ("intra_mode_end", 1), ("subpel_depth", 2),
                                         ("subpel_depth", 1), ("subpel_depth", 0), ("compute_rate", 1), ("dispenser_search_level", 2), ("synth_blk_size", 8),
                                         ("synth_blk_size", 64), ("in_loop_ois", 0), ("n_tpl_stats", 3)])
def test_check_desc_refuses(field, value):
    with pytest.raises(api.SvtHipError):
        tpl.check_desc(fake_desc(make_case(1, 128, 96), **{field: value}))


def test_check_desc_refuses_small_recon_padding():
    c = make_case(1, 128, 96)
    d = fake_desc(c)
    d.recon.org_x = 31
    with pytest.raises(api.SvtHipError):
        tpl.check_desc(d)
    d = fake_desc(c)
    d.recon.org_y = 16
    with pytest.raises(api.SvtHipError):
        tpl.check_desc(d)
    d = fake_desc(c)
    d.refs[0][0].recon.org_x = 8
    with pytest.raises(api.SvtHipError):
        tpl.check_desc(d)


def test_dc_neighbours_cut_at_the_picture():
    """The open-loop fills give DC the above row cut at the width (127 past it) and the left column cut at the height (129 past it):
    the form the device kernels use."""
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 256, (96 + 2 * PAD, 136 + 2 * PAD)).astype(np.uint8)
    W, H = 130, 90
    for S in (16, 32):
        for y in range(0, H - S // 2 + 1, S):
            for x in range(0, W - S // 2 + 1, S):
                a = [int(plane[PAD + y - 1, PAD + x + i]) if x + i < W else 127 for i in range(S)]
                l = [int(plane[PAD + y + i, PAD + x - 1]) if y + i < H else 129 for i in range(S)]
                want = ((sum(a) + sum(l) + S) // (2 * S) if x and y else (sum(l) + S // 2) // S if x else (sum(a) + S // 2) // S if y else 128)
                assert dc_pred(plane, x, y, S, W, H) == want, (S, x, y)


@pytest.mark.parametrize("kw", [dict(W=200, H=136), dict(W=232, H=178, level=1, sub=2, synth=16), dict(W=210, H=150, synth=32, disable_intra_pred=1)])
def test_stored_source_stats_give_the_same_picture(kw):
    """src_pass 0 with the stats of the same picture's source pass reproduces that dispense."""
    c = make_case(60, **kw)
    g1, _, r1 = restate(c)
    g2, _, r2 = restate(src_pass0_case(60, **kw))
    np.testing.assert_array_equal(r1, r2)
    for k in FIELDS_S:
        np.testing.assert_array_equal(g1[k], g2[k], err_msg=k)


def fixture():
    from tpl_dispenser_cases import GOLDEN, fixture_cases, input_checksum
    z = np.load(GOLDEN)
    recons = []
    for i, (name, kw, c) in enumerate(fixture_cases(lambda _: recons[-1])):
        assert str(z[f"name_{i}"]) == name
        np.testing.assert_array_equal(input_checksum(c), z[f"checksum_{i}"], err_msg=f"{name}: the case's inputs changed")
        recons.append(z[f"recon_{i}"])
        yield name, c, (z[f"tpl_stats_{i}"], z[f"tpl_src_stats_{i}"], z[f"recon_{i}"])


def test_restatement_equals_the_reference_fixture():
    """tools/gen_tpl_golden.py: the reference's own tpl_mc_flow_dispenser_sb_generic + svt_aom_generate_padding on every case."""
    n = 0
    for name, c, (grid, src, rec) in fixture():
        g, s, r = restate(c)
        np.testing.assert_array_equal(r, rec, err_msg=f"{name}: recon")
        for k in FIELDS_S:
            np.testing.assert_array_equal(g[k], grid[k], err_msg=f"{name}: tpl_stats.{k}")
        for k in FIELDS_SRC:
            np.testing.assert_array_equal(s[k], src[k], err_msg=f"{name}: tpl_src_stats.{k}")
        n += 1
    assert n == 15
