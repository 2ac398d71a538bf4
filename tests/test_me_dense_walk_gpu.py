"""GPU: the two walks of the ME dense pre-pass (csrc/me_dense.inl) -- the static one for full-height blocks over segments of 16, 24, 32 ... search rows,
the generic one for the rest -- and the planner's segments (48 rows and a shorter last one).

Every case sizes its searches itself (cfg_edit), so that which unit takes which walk follows from the geometry below and not from a preset:
the sixteenth-resolution plane has H / 4 rows and 16 rows of padding a search may enter; block row r sits at plane row 16 r.
  * a level-0 region of h rows (two regions, stacked): the upper one covers search rows 16 r - h .., the lower one 16 r ..; a region that
    leaves the padded plane is clipped, which gives heights that are no multiple of 8 and heights below 16.
  * a pre-HME strip of h rows is centred on the block: 16 r - h / 2 ...
Every case is compared with the oracle in all SvtHipMeResults fields, in the one-kernel and in the forced staged form, the pre-pass's "not
found" counter must be 0 (all blocks are 64 wide: every search is covered, as before the static walk existed), and the path counters must show
the walks the case was built for."""
import numpy as np
import pytest

from me_cases import MeCase, compare
from svt_av1_psyex_amd import synth

pytestmark = pytest.mark.gpu


def sizes(l0=None, strip0=None, strip1=None, skip_line=0):
    """cfg_edit: level-0 regions of l0 = (width, height) each, pre-HME strips of (width, height); None switches the search off"""
    def edit(cfg):
        cfg.hme_search_method = 0
        cfg.enable_me_sr_adjustment = 0  # no division of the level-0 area: every searched reference gets the sizes below
        cfg.enable_hme_flag = cfg.enable_hme_level0_flag = 1
        if l0:
            for sa in (cfg.hme_l0_sa.sa_min, cfg.hme_l0_sa.sa_max):
                sa.width, sa.height = l0[0] * cfg.num_hme_sa_w, l0[1] * cfg.num_hme_sa_h
        cfg.prehme_enable = 1 if (strip0 or strip1) else 0
        cfg.prehme_skip_search_line = skip_line
        for i, strip in enumerate((strip0, strip1)):
            w, h = strip or (8, 3)
            for sa in (cfg.prehme_sa_cfg[i].sa_min, cfg.prehme_sa_cfg[i].sa_max):
                sa.width, sa.height = w, h
    return edit


def shifted_case(width, height, shifts, edit, seed):
    """noise; reference (list, 0) is the current picture moved down by 4 * shifts[list] rows: on the sixteenth plane the match of an interior
    block is exact (SAD 0) at the vertical displacement shifts[list]"""
    case = MeCase(width, height, enc_mode=6, cur=1, refs={(0, 0): 0, (1, 0): 2}, seed=seed, kind="noise", cfg_edit=edit)
    frame = np.random.default_rng(seed).integers(0, 256, (height, width), dtype=np.uint8)
    case.cur = synth.HostPyramid(frame, 1)
    case.refs = {(li, 0): synth.HostPyramid(np.roll(frame, 4 * s, axis=0), 2 * li) for li, s in enumerate(shifts)}
    return case


# name -> (case builder, paths at least one unit must take, segment lengths (rows) at least one unit of the static walk must have, unit plan).
# Plan 0 is the library's choice, for pictures this small the fine plan (segments of 16 rows); plan 1 is the one of a launch that fills the chip:
# areas up to 64 rows in one piece, taller ones in segments of 48 (svt_hip_context_set_me_dense_plan).
CASES = {
    # 52 plane rows: block rows 1 and 2 hold both 16-row regions unclipped; the last block row is 16 samples high (2 source rows)
    "l0_16": (lambda: MeCase(256, 208, enc_mode=6, seed=41, cfg_edit=sizes(l0=(32, 16))), ("fast", "partial_row"), (16,), 0),
    # 48 plane rows, three full block rows: the lower 32-row region is whole in rows 0 and 1, the upper one in rows 1 and 2; clipped to 16 rows elsewhere
    "l0_32": (lambda: MeCase(320, 192, enc_mode=6, seed=42, kind="noise", cfg_edit=sizes(l0=(24, 32))), ("fast",), (16, 32), 1),
    # 68 plane rows: the lower 48-row region is whole in rows 0 and 1, the upper one in rows 2 and 3; the rest clips to 16 .. 47 rows, odd ones among them
    "l0_48": (lambda: MeCase(384, 272, enc_mode=6, seed=43, cfg_edit=sizes(l0=(16, 48))), ("fast", "odd", "partial_row"), (48,), 1),
    # 24- and 40-row regions: the static walk's second form (n = 8 mod 16), whole in block rows 1 .. 3 (lower) and 2, 3 (upper) of 5
    "l0_24": (lambda: MeCase(256, 320, enc_mode=6, seed=48, cfg_edit=sizes(l0=(32, 24))), ("fast",), (24,), 1),
    "l0_40": (lambda: MeCase(256, 384, enc_mode=6, seed=49, kind="noise", cfg_edit=sizes(l0=(16, 40))), ("fast",), (40,), 1),
    # 8-row regions: fewer than 16 search rows never take the static walk
    "l0_8": (lambda: MeCase(256, 208, enc_mode=6, seed=44, cfg_edit=sizes(l0=(32, 8))), ("short", "partial_row"), (), 0),
    # a 112-row strip: segments 48 + 48 + 16 where it is whole (block rows 3 and 4 of 8), 48 + a clipped remainder (a multiple of 8 here) elsewhere; a 44-wide strip
    # of 48 rows: its sixth octet holds 4 positions.  The exact matches lie at displacement -9 / -8: search row 47 / 48 of the whole strip,
    # the last row of its first segment and the first row of its second
    "strips": (lambda: shifted_case(128, 512, (-9, -8), sizes(l0=(16, 16), strip0=(16, 112), strip1=(44, 48)), 45), ("fast", "octet"), (16, 48), 1),
    "skip_line": (lambda: MeCase(256, 208, enc_mode=6, seed=46, cfg_edit=sizes(l0=(32, 16), strip0=(16, 112), strip1=(44, 48), skip_line=1)), ("fast", "skip_line"), (16,), 1),
    # constant planes: every position of every search ties at SAD 0, within a segment and between segments; the first in raster order wins
    "flat": (lambda: MeCase(128, 512, enc_mode=6, seed=47, kind="flat", cfg_edit=sizes(l0=(16, 16), strip0=(16, 112), strip1=(44, 48))), ("fast", "octet"), (16, 48), 1),
}

_cache = {}


def built(name):
    """the case and the oracle's results, computed once and shared by the tests"""
    if name not in _cache:
        case = CASES[name][0]()
        _cache[name] = (case, case.run_cpu("oracle"))
    return _cache[name]


def counted_run(hip_ctx, name, form, fast=True):
    """results, (taken, not found), path counters and the slot buffer of one launch of case `name`"""
    case = built(name)[0]
    hip_ctx.set_me_counting(True)
    hip_ctx.set_me_dense_plan(CASES[name][3])
    hip_ctx.set_me_staged(form)
    hip_ctx.set_me_dense_fast(fast)
    try:
        hip_ctx.me_dense_counters()
        hip_ctx.me_dense_path_counters()
        got = case.run_hip(hip_ctx)
        return got, hip_ctx.me_dense_counters(), hip_ctx.me_dense_path_counters(), hip_ctx.me_dense_slots()
    finally:
        hip_ctx.set_me_dense_fast(True)
        hip_ctx.set_me_dense_plan(0)
        hip_ctx.set_me_staged(1)
        hip_ctx.set_me_counting(False)


@pytest.mark.parametrize("form", [0, 2], ids=["one-kernel", "staged"])
@pytest.mark.parametrize("name", list(CASES))
def test_walks_match_the_oracle_and_are_taken(hip_ctx, name, form):
    case, want = built(name)
    got, (taken, own), paths, _ = counted_run(hip_ctx, name, form)
    print(name, form, "taken / not found", taken, own, "paths", paths)
    assert not compare(want, got)
    assert own == 0 and (taken > 0 or name == "flat"), (taken, own)  # (on constant planes the per-block kernel asks for no search result)
    for path in CASES[name][1]:
        assert paths[path][0] > 0 and paths[path][1] > 0, (path, paths)
    for rows in CASES[name][2]:
        assert paths["fast_rows"][rows] > 0, (rows, paths)
    assert paths["off"] == (0, 0)
    assert sum(paths["fast_rows"].values()) == paths["fast"][0]


@pytest.mark.parametrize("name", list(CASES))
def test_static_and_generic_walks_agree(hip_ctx, name):
    """the same launch with the static walk switched off: every unit goes the generic way, slots and results are the same bytes"""
    case, want = built(name)
    on, _, paths_on, slots_on = counted_run(hip_ctx, name, 2, fast=True)
    off, _, paths_off, slots_off = counted_run(hip_ctx, name, 2, fast=False)
    assert paths_off["fast"] == (0, 0) and paths_off["off"][0] > 0, paths_off
    assert sum(v[0] for k, v in paths_off.items() if k != "fast_rows") == sum(v[0] for k, v in paths_on.items() if k != "fast_rows")  # the same units
    assert sum(v[1] for k, v in paths_off.items() if k != "fast_rows") == sum(v[1] for k, v in paths_on.items() if k != "fast_rows")  # the same pairs
    assert slots_on.size and slots_on.tobytes() == slots_off.tobytes()
    assert not compare(on, off)
    assert not compare(want, off)


def slot_fields(slots):
    filled = slots[slots["key"] != np.uint64(0xFFFFFFFFFFFFFFFF)]
    return filled, filled["key"] >> np.uint64(32), (filled["key"] >> np.uint64(16)) & np.uint64(0xFFFF), filled["key"] & np.uint64(0xFFFF), filled["size"] >> 16


def test_segments_of_a_tall_strip(hip_ctx):
    """where the 112-row strip is whole its winner (SAD 0) sits in search row 47 for list 0 -- the last row of the first segment -- and in row 48
    for list 1, the first row of the second segment"""
    _, _, paths, slots = counted_run(hip_ctx, "strips", 2)
    filled, sad, y, x, sa_h = slot_fields(slots)
    whole = (sa_h == 112) & (sad == 0)
    assert np.count_nonzero(whole & (y == 47)) > 0 and np.count_nonzero(whole & (y == 48)) > 0, (y[sa_h == 112], sad[sa_h == 112])


def test_ties_between_segments_go_to_the_first_position(hip_ctx):
    _, _, _, slots = counted_run(hip_ctx, "flat", 2)
    filled, sad, y, x, sa_h = slot_fields(slots)
    assert filled.size and np.count_nonzero(sa_h == 112) > 0
    assert not filled["key"].any()  # SAD 0 at search index (0, 0) in every slot, the three-segment strips included
