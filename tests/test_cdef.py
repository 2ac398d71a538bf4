"""CPU: the restatements of the three CDEF stages (tests/cdef_cases.py) against the reference's own results (golden/cdef.npz: cdef_seg_search,
finish_cdef_search and svt_av1_cdef_frame themselves, driven by tools/gen_cdef_golden.py), the conditions of the case list recomputed from the
restatements, the struct lay-outs of cdef.py against the library's, the three descriptor validations and the empty batches (they need no GPU)."""
import ctypes as C

import numpy as np
import pytest

import cdef_cases as cc
from abi_mirror import check_layout
from svt_av1_psyex_amd import api, cdef

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(cc.GOLDEN)


# ---- the restatements against the fixture ----
def test_restatements_equal_the_reference_on_every_output(golden):
    """per search case the search's mse, dir and var, the pick behind it (bits, strengths, cdef_dist_dev, per-block indices, the biased mse) and the
    filtered planes; per pick case and per apply case the same of that stage alone"""
    mine = cc.fixture_arrays()
    assert set(golden.files) == set(mine)
    for key, a in mine.items():
        assert a.dtype == golden[key].dtype and np.array_equal(a, golden[key]), key


def test_a_changed_sample_changes_the_restatement():
    """the comparison can fail: one reconstruction sample off by one changes the block's distortion"""
    c = cc.search_case("noise_8x8_8")
    want = cc.restated_search("noise_8x8_8")[0]["block_dist"]
    recon = [p.copy() for p in c["recon"]]
    recon[0][3, 4] ^= 1
    got = cc.restate_search(recon, c["src"], c["bd"], c["base_q_idx"], c["sf"], c["sy"], c["suv"], c["masks"])["block_dist"]
    assert not np.array_equal(got, want)


def test_the_luma_distortion_is_the_reference_formula_on_known_sums():
    """flat source 100, flat filtered 101, 64 samples: both variances 0, so 64 * .5 * 400 / sqrt(20000) = 90.5..., + .5 and floored"""
    s, y = np.full((1, 8, 8), 100), np.full((1, 8, 8), 101)
    assert cc.luma_dist(s, y, 0).tolist() == [91]
    assert cc.luma_dist(s << 2, y << 2, 2).tolist() == [int(np.floor(.5 + 1024 * .5 * 6400 / np.sqrt(5120000.)))]


# ---- coverage ----
def test_coverage_conditions_hold():
    """every direction, var 0 and the cap of 12, both tap sets, t == 0 with a primary strength, every damping and chroma's 2, both clamps, a
    CDEF_VERY_LARGE tap on every side in either position, a secondary-only strength off direction 0, a chroma strength of -1, every subsampling factor;
    every cdef_bits, every branch of both bias rules, ties; every copy-through rule; the sizes, depths, pictures and masks of the list"""
    assert cc.coverage_missing() == []
    assert cc.coverage_missing(["noise_8x8_8"], [], []) != []  # the check can fail


# ---- lay-outs ----
def test_struct_layouts_match_the_library():
    check_layout("svt_hip_cdef_layout", cdef.MIRRORS, multiple_of_8=True)
    assert cdef.PICK_DTYPE.itemsize == C.sizeof(cdef.CdefPick)
    for name, *_ in cdef.CdefPick._fields_:
        assert cdef.PICK_DTYPE.fields[name][1] == getattr(cdef.CdefPick, name).offset, name
    assert cdef.DEFAULT_MSE_UV == cc.DEFAULT_MSE_UV and cdef.work_bytes() % 8 == 0 and cdef.work_bytes() >= 64 * 64 * 8 + 65536 * 8
    assert cdef.n_fb_of(136, 72) == cc.n_fb_of(136, 72) == 6


# ---- the descriptor checks ----
def planes(w=136, h=72, base=0x10000, stride_extra=8):
    return [cdef.plane(base + 0x100000 * i, (w >> (i > 0)) + stride_extra, w >> (i > 0), h >> (i > 0)) for i in range(3)]


def good_search(n_fb=6, bit_depth=10):
    return cdef.search_desc(planes(), planes(base=0x1000000), bit_depth, 130, 2, [0, 5, 63], [0, -1, 63], n_fb, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000)


def good_pick(n_fb=None):
    return cdef.pick_desc(136, 72, 3, 1, 60, 500, [0, 5, 63], [0, 5, 63], 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, n_fb=n_fb)


def good_apply(n_fb=6, n_planes=3):
    return cdef.apply_desc(planes(), planes(base=0x1000000), 8, 4, n_planes, n_fb, 0x2000, 0x3000, 0x4000, 0x5000)


def spoil(d, bad):
    """no_<pointer>; <array>_<index>_<field>_<value> for a plane; <array>_<index>_<value> for a list; <field>_<value>"""
    if bad.startswith("no_"):
        setattr(d, bad[3:], None)
        return d
    parts = bad.split("_")
    head = parts[0]
    if head in ("recon", "src", "in", "out"):
        p = getattr(d, head)[int(parts[1])]
        setattr(p, parts[2], None if parts[2] == "plane" else int(parts[3]))
    elif head == "strength":
        getattr(d, f"strength_{parts[1]}")[int(parts[2])] = int(parts[3])
    else:
        name, _, v = bad.rpartition("_")
        setattr(d, name, int(v))
    return d


def refused(entry, batch, d, bad):
    L = api.lib()
    ctx = C.create_string_buffer(8192)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    if bad == "null_desc":
        assert getattr(L, entry)(None) == BAD_PARAM and getattr(L, batch)(ctx, None) == BAD_PARAM
    else:
        spoil(d, bad)
        assert getattr(L, entry)(C.byref(d)) == BAD_PARAM
        with pytest.raises(api.SvtHipError, match=entry):
            api.check_desc(entry, d)
        assert getattr(L, batch)(ctx, C.byref(d)) == BAD_PARAM
    assert entry.rsplit("_", 2)[0].encode() in L.svt_hip_last_error(None)


def test_check_descs_accept_good_descriptors():
    for bd in (8, 10):
        cdef.check_search_desc(good_search(bit_depth=bd))
    d = good_search(n_fb=0)
    d.block_dist = None
    cdef.check_search_desc(d)
    cdef.check_pick_desc(good_pick())
    cdef.check_pick_desc(good_pick(n_fb=0))
    d = good_pick()
    d.zero_fs_cost_bias = 0
    cdef.check_pick_desc(d)
    for n_planes in (1, 3):
        cdef.check_apply_desc(good_apply(n_planes=n_planes))
    d = good_apply(n_planes=1)
    d.out[1].plane = None  # planes past n_planes are not looked at
    cdef.check_apply_desc(d)


SEARCH_BAD = ["null_desc", "no_masks", "no_mse", "no_dir", "no_var", "bit_depth_12", "bit_depth_9", "subsampling_factor_3", "subsampling_factor_0", "n_strengths_0",
              "n_strengths_65", "strength_y_1_64", "strength_y_2_-1", "strength_uv_0_-2", "strength_uv_2_64", "recon_0_plane", "src_2_plane", "recon_1_stride_67",
              "recon_0_width_132", "recon_0_height_68", "recon_1_width_66", "src_2_height_40", "src_0_width_128", "recon_0_width_0", "n_fb_5", "n_fb_7"]
PICK_BAD = ["null_desc", "no_masks", "no_mse", "no_work", "no_result", "no_fb_strength", "work_16388", "n_strengths_0", "n_strengths_65", "is_hbd_2",
            "zero_fs_cost_bias_9", "zero_fs_cost_bias_65", "width_0", "width_132", "height_16392", "n_fb_5"]
APPLY_BAD = ["null_desc", "no_masks", "no_fb_strength", "no_y_strength", "no_uv_strength", "bit_depth_12", "cdef_damping_2", "cdef_damping_7", "n_planes_2", "n_planes_0",
             "in_0_plane", "out_2_plane", "out_1_stride_67", "in_0_width_132", "out_0_height_64", "in_2_width_70", "n_fb_5"]


@pytest.mark.parametrize("bad", SEARCH_BAD)
def test_search_check_desc_refuses_with_an_error_text(bad):
    refused("svt_hip_cdef_search_check_desc", "svt_hip_cdef_search_batch", good_search(), bad)


@pytest.mark.parametrize("bad", PICK_BAD)
def test_pick_check_desc_refuses_with_an_error_text(bad):
    refused("svt_hip_cdef_pick_check_desc", "svt_hip_cdef_pick_batch", good_pick(), bad)


@pytest.mark.parametrize("bad", APPLY_BAD)
def test_apply_check_desc_refuses_with_an_error_text(bad):
    refused("svt_hip_cdef_apply_check_desc", "svt_hip_cdef_apply_batch", good_apply(), bad)


def test_apply_check_desc_refuses_aliasing():
    L = api.lib()
    for alias in ("in_place", "overlap", "two_outputs"):
        d = good_apply()
        if alias == "in_place":
            d.out[0].plane = getattr(d, "in")[0].plane
        elif alias == "overlap":
            d.out[1].plane = getattr(d, "in")[1].plane + 76 * 35  # the last row of the input's picture
        else:
            d.out[2].plane = d.out[1].plane + 16
        assert L.svt_hip_cdef_apply_check_desc(C.byref(d)) == BAD_PARAM, alias
        assert b"overlaps" in L.svt_hip_last_error(None)
    d = good_apply()
    d.out[1].plane = getattr(d, "in")[1].plane + 76 * 35 + 68  # just behind it
    assert L.svt_hip_cdef_apply_check_desc(C.byref(d)) == 0


def test_empty_batches_return_0_and_touch_nothing():
    L = api.lib()
    ctx = C.create_string_buffer(8192)
    for batch, d in (("svt_hip_cdef_search_batch", good_search(n_fb=0)), ("svt_hip_cdef_pick_batch", good_pick(n_fb=0)), ("svt_hip_cdef_apply_batch", good_apply(n_fb=0))):
        assert getattr(L, batch)(ctx, C.byref(d)) == 0, batch
        assert getattr(L, batch)(None, C.byref(d)) == BAD_PARAM, batch
