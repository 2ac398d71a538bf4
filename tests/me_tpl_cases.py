"""The ME -> TPL chain: cases whose dispenser input is the output of motion estimation on the same pictures.  Test infrastructure.

A chain case is an me_cases.MeCase (the pictures of the "mixed" sequence, the preset's SvtHipMeConfig, the SvtHipMePictureDesc) plus the
dispenser's controls.  case_dict() turns it, with the three ME result arrays of whichever implementation ran the ME, into the case dict
that tpl_dispenser_cases.restate and tpl.make_desc take: `cur` and every reference's `src` ARE the MeCase's padded full-resolution planes
(padding 68, case["pad"]), the ME arrays keep the layout svt_hip_me_picture* writes (n_pu, max_cand, max_refs, max_l0 from the ME
descriptor), `poc` is the reference's picture number, and a reference's recon-path plane is its source plane plus seeded noise of +-3
(single pictures) or the previous picture's TPL recon (windows).

A chain window is four consecutive pictures in decode order: picture 0 an I picture (no ME), picture i searching picture i - 1 as list 0 /
reference 0, the last picture tpl_valid_pic 0 (tpl_group_cases.dispensed_window's shape)."""
import functools
import hashlib
import os

import numpy as np

from me_cases import MeCase
from svt_av1_psyex_amd import abi, rd
import tpl_dispenser_cases as tc
import tpl_group_cases as gc

PAD = 68  # the padding of ME's full-resolution planes (synth.HostPyramid)
ME_KEYS = (("total", "total_me_candidate_index"), ("cand", "me_candidate_array"), ("mv", "me_mv_array"))
TWO = {(0, 0): 0, (1, 0): 3}
FIELDS_S = ("srcrf_dist", "recrf_dist", "srcrf_rate", "recrf_rate", "mc_dep_rate", "mc_dep_dist", "mv_row", "mv_col", "ref_frame_poc")
FIELDS_SRC = ("srcrf_dist", "srcrf_rate", "ref_frame_poc", "mv_row", "mv_col", "best_mode", "best_rf_idx", "best_intra_mode")

# name -> (MeCase arguments, dispenser controls).  own_planes: the GPU test hands the dispenser the SvtHipPaPicture's own full plane.
SINGLE = {
    "352x288_m6_L4_s16": (dict(width=352, height=288, enc_mode=6, refs=TWO), dict(level=0, sub=0, synth=16, own_planes=True)),
    "360x200_m3_L4_s32": (dict(width=360, height=200, enc_mode=3, refs={(0, 0): 1, (0, 1): 0, (1, 0): 3, (1, 1): 4}, n_frames=5),
                          dict(level=0, sub=0, synth=32)),
    "232x184_m10_L5_s32": (dict(width=232, height=184, enc_mode=10, refs={(0, 0): 1}), dict(level=1, sub=2, synth=32)),
    "352x288_m8_L5_s16": (dict(width=352, height=288, enc_mode=8, refs=TWO), dict(level=1, sub=2, synth=16, own_planes=True)),
    "200x136_m12_L4_s16": (dict(width=200, height=136, enc_mode=12, refs=TWO), dict(level=0, sub=0, synth=16)),
    "640x360_m4_L4_s16": (dict(width=640, height=360, enc_mode=4, refs={(0, 0): 1, (1, 0): 3}), dict(level=0, sub=0, synth=16)),
    # intra off: the recon of a non-reference picture keeps the prediction (is_ref 0), a reference picture's takes the inverse (is_ref 1)
    "360x200_m3_L4_s32_intra_off_nonref": (dict(width=360, height=200, enc_mode=3, refs={(0, 0): 1, (0, 1): 0, (1, 0): 3, (1, 1): 4}, n_frames=5),
                                           dict(level=0, sub=0, synth=32, disable_intra_pred=1, is_ref=0)),
    "232x184_m10_L5_s32_intra_off_ref": (dict(width=232, height=184, enc_mode=10, refs={(0, 0): 1}),
                                         dict(level=1, sub=2, synth=32, disable_intra_pred=1, is_ref=1)),
}
WINDOWS = {
    "352x288_m6_s16": dict(width=352, height=288, enc_mode=6, synth=16, own_planes=True),
    "360x200_m3_s32": dict(width=360, height=200, enc_mode=3, synth=32),   # ceil(360 / 16) = 23 is odd: the stride alias of DESIGN 4.13
    "200x136_m12_s16": dict(width=200, height=136, enc_mode=12, synth=16),  # the fixture's window
}
N_WINDOW = 4


@functools.lru_cache(maxsize=None)
def me_case(name):
    return MeCase(kind="mixed", **SINGLE[name][0])


@functools.lru_cache(maxsize=None)
def window_me_cases(name):
    """The MeCases of pictures 1 .. 3 of a window (picture 0 is an I picture)."""
    w = WINDOWS[name]
    return [MeCase(w["width"], w["height"], enc_mode=w["enc_mode"], cur=i, refs={(0, 0): i - 1}, kind="mixed", n_frames=N_WINDOW)
            for i in range(1, N_WINDOW)]


def me_arrays(results):
    """The three arrays the dispenser reads, flattened, from an ME result dict (pyoracle.me_picture, Context.me_picture, a download)."""
    return {k: np.ascontiguousarray(results[name]).reshape(-1) for k, name in ME_KEYS}


def padded_noise(rng, plane, W, H, amp=3):
    out = plane.copy()
    inner = plane[PAD:PAD + H, PAD:PAD + W].astype(np.int32) + rng.integers(-amp, amp + 1, (H, W))
    out[PAD:PAD + H, PAD:PAD + W] = np.clip(inner, 0, 255)
    tc.generate_padding(out, W, H, PAD, PAD)
    return out


def case_dict(mc, me, level=0, sub=0, pf=2, synth=16, disable_intra_pred=0, is_ref=1, slice_is_i=0, seed=7, qstep=(40, 52)):
    """mc: the MeCase (for an I picture: its `cur` alone is used); me: me_arrays() of its ME, None for an I picture."""
    W, H = mc.width, mc.height
    rng = np.random.default_rng(seed)
    cur = mc.cur.planes[2][0]
    refs = {}
    if not slice_is_i:
        for k in sorted(mc.refs):
            src = mc.refs[k].planes[2][0]
            refs[k] = dict(src=src, recon=padded_noise(rng, src, W, H), poc=mc.refs[k].picture_number, max_width=W, max_height=H, usable=1)
    d = mc.desc
    if me is None:
        me = dict(total=np.zeros(0, np.uint8), cand=np.zeros(0, np.uint8), mv=np.zeros(0, np.uint32))
    tpl_stats = np.zeros(((W + synth - 1) // synth) * ((H + synth - 1) // synth) + 8, abi.TPL_STATS_DTYPE)
    tpl_stats.view(np.uint8)[:] = 0xA5
    recon = (np.arange(cur.size) * 37 % 251).astype(np.uint8).reshape(cur.shape)
    return dict(width=W, height=H, aligned_width=W, aligned_height=H, pad=PAD, cur=cur, recon=recon, recon_width=W, recon_height=H, refs=refs, me=me,
                n_pu=abi.n_pu(d.enable_me_16x16, d.enable_me_8x8), max_cand=d.max_cand, max_refs=d.max_refs, max_l0=d.max_l0,
                enable_me_16x16=d.enable_me_16x16, level=level, sub=sub, pf=pf, synth=synth, disable_intra_pred=disable_intra_pred, is_ref=is_ref,
                slice_is_i=slice_is_i, tpl_slice_is_i=slice_is_i, src_pass=1, store_src_stats=1, quant=rd.quant_row_from_step(*qstep),
                tpl_stats=tpl_stats, tpl_src_stats=np.zeros(((W + 15) // 16) * ((H + 15) // 16), abi.TPL_SRC_STATS_DTYPE))


def single_case(name, results):
    ctl = {k: v for k, v in SINGLE[name][1].items() if k != "own_planes"}
    return case_dict(me_case(name), me_arrays(results), **ctl)


def window(name, results):
    """The group window (tpl_group_cases layout) of WINDOWS[name]; results: the ME result dicts of pictures 1 .. 3."""
    w = WINDOWS[name]
    mcs = window_me_cases(name)
    W, H, synth = w["width"], w["height"], w["synth"]
    win = dict(width=W, height=H, aligned_width=W, aligned_height=H, synth=synth, sb_size=64, frames=[], kind="dispensed", stages=gc.STAGES_ALL)
    rng = np.random.default_rng(W + synth)
    for i in range(N_WINDOW):
        mc = mcs[max(i, 1) - 1]
        c = case_dict(mc, me_arrays(results[i - 1]) if i else None, synth=synth, slice_is_i=int(i == 0), seed=20 + i)
        if i == 0:
            c["cur"] = mcs[0].refs[(0, 0)].planes[2][0]  # picture 0: the plane picture 1 searches
        win["frames"].append(dict(poc=i, valid=int(i < N_WINDOW - 1), base_rdmult=int(rng.integers(40, 4000)), grid=c["tpl_stats"], r0=0.25 * (i + 1),
                                  outputs=1, case=c))
    return win


@functools.lru_cache(maxsize=None)
def oracle_me(name):
    return me_case(name).run_cpu("oracle")


@functools.lru_cache(maxsize=None)
def oracle_window_me(name):
    return [mc.run_cpu("oracle") for mc in window_me_cases(name)]


@functools.lru_cache(maxsize=None)
def oracle_single(name):
    """(case, restatement) of a single-picture case on the oracle's ME arrays."""
    c = single_case(name, oracle_me(name))
    return c, tc.restate(c)


@functools.lru_cache(maxsize=None)
def oracle_window(name):
    """(window, dispensed grids, recon planes, final grids, outs) of a window on the oracle's ME arrays."""
    win = window(name, oracle_window_me(name))
    d_grids, recons = gc.restate_dispensed(win)
    grids, outs = gc.restate(win, win["stages"], d_grids)
    return win, d_grids, recons, grids, outs


def walk_stats(c, src_stats):
    """What a case exercises, from the ME arrays and the restatement's TplSrcStats alone: blocks at least half inside / skipped (of the
    b64 grid's blocks), the NEWMV share and the winning best_rf_idx values of the former, one-directional candidates evaluated and those
    whose MV the +-32 clamp changes, candidate bytes with bits 6-7 set."""
    S = 16 << c["level"]
    W, H = c["width"], c["height"]
    a16w = (c["aligned_width"] + 15) >> 4
    me, n_pu = c["me"], c["n_pu"]
    inside = skipped = newmv = evaluated = clamped = 0
    winners = set()
    for x, y, b64, me_idx in tc.blocks_in_order(c):
        if x + S // 2 > W or y + S // 2 > H:
            skipped += 1
            continue
        inside += 1
        s = src_stats[(y >> 4) * a16w + (x >> 4)]
        if s["best_mode"] == tc.NEWMV:
            newmv += 1
            winners.add(int(s["best_rf_idx"]))
        pu = b64 * n_pu + me_idx
        for ci in range(int(me["total"][pu])):
            cand = int(me["cand"][pu * c["max_cand"] + ci])
            lst = cand & 3
            if lst > 1:
                continue
            ref = (cand >> 2) & 3 if lst == 0 else (cand >> 4) & 3
            r = c["refs"].get((lst, ref))
            if r is None or not r["usable"]:
                continue
            mv = int(me["mv"][pu * c["max_refs"] + (c["max_l0"] if lst else 0) + ref])
            mx, my = tc.wrap16(mv & 0xFFFF), tc.wrap16(mv >> 16)
            evaluated += 1
            clamped += not (-tc.TPL_PADX <= x + mx and x + S + mx <= tc.TPL_PADX + r["max_width"] - 1 and
                            -tc.TPL_PADX <= y + my and y + S + my <= tc.TPL_PADX + r["max_height"] - 1)
    return dict(inside=inside, skipped=skipped, newmv_share=newmv / inside, winners=winners, evaluated=evaluated, clamped=clamped,
                bits67=int((me["cand"] & 0xC0 != 0).sum()))


def input_checksum(c):
    """sha256 over every input array of a chain case: planes, the three ME arrays, the recon buffer's and the grids' initial contents,
    the quantizer row and the numbers that are not arrays."""
    h = hashlib.sha256()
    arrays = [c["cur"], c["recon"], c["tpl_stats"], c["tpl_src_stats"], c["me"]["total"], c["me"]["cand"], c["me"]["mv"], c["quant"]]
    for k in sorted(c["refs"]):
        arrays += [c["refs"][k]["src"], c["refs"][k]["recon"], np.array([k[0], k[1], c["refs"][k]["poc"]], np.int64)]
    arrays.append(np.array([c[k] for k in ("width", "height", "pad", "n_pu", "max_cand", "max_refs", "max_l0", "enable_me_16x16", "level", "sub", "pf",
                                           "synth", "disable_intra_pred", "is_ref", "slice_is_i")], np.int64))
    for a in arrays:
        h.update(np.ascontiguousarray(a).view(np.uint8).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def window_checksum(win):
    h = hashlib.sha256()
    h.update(np.array([win["width"], win["height"], win["synth"], win["sb_size"], win["stages"]], np.int64).tobytes())
    for f in win["frames"]:
        h.update(np.array([f["poc"], f["valid"], f["base_rdmult"], f["outputs"]], np.int64).tobytes())
        h.update(np.array([f["r0"]], np.float64).tobytes())
        h.update(input_checksum(f["case"]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def plane_sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------------------
# The reference fixture (tools/gen_me_tpl_golden.py): the reference build's ME -> the reference's own dispenser / synthesizer / r0beta
# (not golden/me_*.npz: golden_io.me_fixture_names takes every file of that pattern for an ME fixture)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tpl_me_chain.npz")
FIXTURE_SINGLE = ["232x184_m10_L5_s32", "200x136_m12_L4_s16", "360x200_m3_L4_s32", "352x288_m6_L4_s16", "232x184_m10_L5_s32_intra_off_ref"]
FIXTURE_FULL_RECON = ["232x184_m10_L5_s32", "200x136_m12_L4_s16"]  # the others store a sha256 of the padded recon plane
FIXTURE_WINDOW = "200x136_m12_s16"


def load_fixture():
    """{name: record} of the single-picture cases and the window's record; every array of a record keyed without its index."""
    z = np.load(GOLDEN)
    names = FIXTURE_SINGLE + ["window_" + FIXTURE_WINDOW]
    out = {}
    for i, name in enumerate(names):
        assert str(z[f"name_{i}"]) == name
        out[name] = {k[:-len(f"_{i}")]: z[k] for k in z.files if k.endswith(f"_{i}") and not k.startswith("name_")}
    return out


def assert_equals_fixture(rec, got, what):
    """got = (tpl_stats, tpl_src_stats, padded recon) of a single-picture case against its fixture record, bit for bit: the TplStats
    fields of the written cells, which cells are written, every TplSrcStats field, the whole padded recon (or its sha256)."""
    grid, src, recon = got
    w_grid = rec["tpl_stats"]
    raw = lambda g: g.view(np.uint8).reshape(len(g), -1)
    untouched = (raw(w_grid) == 0xA5).all(1)
    assert np.array_equal((raw(grid) == 0xA5).all(1), untouched), f"{what}: written cells differ"
    for k in FIELDS_S:
        assert np.array_equal(grid[k][~untouched], w_grid[k][~untouched]), f"{what}: tpl_stats.{k}"
    for k in FIELDS_SRC:
        assert np.array_equal(src[k], rec["tpl_src_stats"][k]), f"{what}: tpl_src_stats.{k}"
    if "recon" in rec:
        assert np.array_equal(recon, rec["recon"]), f"{what}: recon"
    assert np.array_equal(plane_sha(recon), rec["recon_sha"]), f"{what}: recon sha256"
