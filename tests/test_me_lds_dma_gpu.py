"""GPU: the LDS fills of the ME chain that go through direct-to-LDS loads (csrc/lds_dma.h): the integer search's reference window in the
tail kernel and the one-kernel form (run_me_searches), and the set-up batch of mid2 / s1 / s2 / tail (the block's record, its requests and
keys, the source views).  Both forms of the launch, bit for bit against the oracle on every result field.

What a case must reach to say anything about those loads, shown on the CPU with the oracle alone before any device run:

  source alignment   a window row starts at plane + (64 * bx + centre_x + area origin) + row * stride: the 16-byte phase of a window is set by
                     the x coordinate of the search centre (hme_sc) and cycles with the stride from row to row.  `noise` 448x136 (stride
                     584 = 8 mod 16, like the bench's planes; every block 64 wide, the last row 8 high) must show at least 12 of the 16
                     residues of hme_sc x (mod 16) and all four (mod 4) among the references still searched; `mixed` 456x136 with pad = 70
                     (stride 596 = 4 mod 16: four phases inside one window; planes only 2-byte aligned) at least 8 and all four; `mixed`
                     448x136 at least 8.
  deferred blocks    `fastpan` 200x136 has a narrow last column: its blocks are deferred, yet the batch of every later kernel was issued
                     for them before the flag was read.
  all rows           me_search_method = 1: the source views keep all 64 rows (cshift = 0), the 64-row view copy.
  four references    FOUR_REFS.
  tiles              the window of a search area W x H has rows of pitch(W) = ((W - 1 + 64 + 15) & ~15) + 16 bytes and H - 1 + 64 of them; a
                     tile is found by halving th (from H, down to 1) and then tw (from W: tw = ((tw >> 1) + 7) & ~7, down to 8) while
                     pitch(tw) * (th - 1 + 64) > 10240 (the arena) or tw * th > 4096.  64x32: 144 * 95 = 13680 > 10240 -> th = 8 (144 * 71 =
                     10224): four row tiles.  200x8: 288 * 64 > 10240 even at th = 1 -> tw = 56 (144 * 64 = 9216): column tiles.  Both
                     asserted from that formula, and the oracle's |a - b| count behind HME must grow against the preset's own area.
The staged runs assert from the launch's kernel list that the tail kernel ran."""
import functools

import numpy as np
import pytest

from me_cases import MeCase, compare

FOUR_REFS = {(0, 0): 1, (0, 1): 0, (1, 0): 3, (1, 1): 4}
ARENA, ORD_BITS = 10240, 12


def _no_exit(cfg):
    cfg.me_early_exit_th = 0


def _area(w, h):
    def edit(cfg):
        cfg.me_early_exit_th = 0
        cfg.me_sa.sa_min.width = cfg.me_sa.sa_max.width = w
        cfg.me_sa.sa_min.height = cfg.me_sa.sa_max.height = h
    return edit


def _all_rows(cfg):
    cfg.me_early_exit_th = 0
    cfg.me_search_method = 1


def tile_of(w, h):
    """(tw, th) of the integer search's tiling of a w x h search area: the formula of the module docstring."""
    def pitch(ww):
        return ((ww - 1 + 64 + 15) & ~15) + 16

    def too_big(tw, th):
        return pitch(tw) * (th - 1 + 64) > ARENA or tw * th > (1 << ORD_BITS)
    tw, th = w, h
    while th > 1 and too_big(tw, th):
        th = (th + 1) >> 1
    while tw > 8 and too_big(tw, th):
        tw = ((tw >> 1) + 7) & ~7
    return tw, th


# name -> (builder, what the CPU test shows: ("residues", mod 16 at least, all four mod 4) / ("deferred",) / ("all_rows",) / ("refs", n) / ("tiles", w, h, "rows" | "cols"))
CASES = {
    "noise_448":      (lambda: MeCase(448, 136, enc_mode=6, kind="noise", cfg_edit=_no_exit), ("residues", 12, True)),
    "mixed_456_pad70": (lambda: MeCase(456, 136, enc_mode=6, kind="mixed", cfg_edit=_no_exit, pad=70), ("residues", 8, True)),
    "mixed_448":      (lambda: MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_no_exit), ("residues", 8, False)),
    "fastpan_narrow": (lambda: MeCase(200, 136, enc_mode=6, kind="fastpan", cfg_edit=_no_exit), ("deferred",)),
    "all_rows":       (lambda: MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_all_rows), ("all_rows",)),
    "four_refs":      (lambda: MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_no_exit, cur=2, refs=FOUR_REFS, n_frames=5), ("refs", 4)),
    "area_64x32":     (lambda: MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_area(64, 32)), ("tiles", 64, 32, "rows")),
    "area_200x8":     (lambda: MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_area(200, 8)), ("tiles", 200, 8, "cols")),
}


def _stage5_ops(case):
    """(oracle results, |a - b| evaluations behind HME) of one oracle run."""
    import pyoracle
    o = pyoracle.load_oracle()
    o.orc_sad_ops_stage.restype = np.ctypeslib.ctypes.c_uint64
    o.orc_sad_ops_stage(5, 1)
    want = case.run_cpu("oracle")
    return want, int(o.orc_sad_ops_stage(5, 1))


def _centre_x(case, want):
    """x coordinates of the search centres of the references a block still searches after the final pruning"""
    sc = want["hme_sc"].reshape(-1, 2, 4, 2).astype(np.int64)
    live = want["do_ref"].reshape(-1, 2, 4) != 0
    exists = np.zeros((2, 4), bool)
    for li, ri in case.refs:
        exists[li, ri] = True
    return sc[..., 0][live & exists[None]]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case and its oracle results (computed once, shared by both forms) -- after the proof that the case reaches what it is named for."""
    build, what = CASES[name]
    case = build()
    want, ops = _stage5_ops(case)
    assert ops > 0, "no integer search at all"
    assert case.cfg.hme_search_method == 0 and case.cfg.me_early_exit_th == 0  # a launch with a pre-pass, and no block leaves before the search
    if what[0] == "residues":
        stride = case.cur.planes[2][1]
        x = _centre_x(case, want)
        r16, r4 = len(set((x % 16).tolist())), len(set((x % 4).tolist()))
        print(f"{name}: stride {stride} = {stride % 16} (mod 16); search centres cover {r16} residues mod 16, {r4} mod 4")
        assert r16 >= what[1]
        if what[2]:
            assert r4 == 4
        if name == "noise_448":
            assert stride % 16 == 8 and case.width % 64 == 0 and case.height % 64 == 8
        if name == "mixed_456_pad70":
            assert stride % 16 == 4 and case.cur.planes[2][2] == 70
    elif what[0] == "deferred":
        # the pre-pass has slots only for blocks 64 wide: the last column's blocks (8 wide here) reach mid1 without them and are deferred.  The
        # oracle shows that those blocks exist and did go through the integer search (a best 64x64 SAD below the initial value for list 0 /
        # reference 0), so the deferred path has results to get right.
        w64 = (case.width + 63) // 64
        narrow = np.arange(len(want["do_ref"].reshape(-1, 2, 4))) % w64 == w64 - 1
        assert case.desc.aligned_width - 64 * (w64 - 1) == 8 and narrow.sum() == (case.height + 63) // 64
        s64 = want["sb_best_sad"].reshape(-1, 2, 4, 85)[:, 0, 0, 0]
        print(f"{name}: {int(narrow.sum())} blocks in the 8-wide last column, best 64x64 SADs {s64[narrow].tolist()}")
        assert (s64[narrow] < 128 * 128 * 255).all() and (s64[~narrow] < 128 * 128 * 255).all()
    elif what[0] == "all_rows":
        # the launcher keeps only the even source rows (cshift = 1) when every picture sub-samples both the HME and the integer search; this
        # one does not, so the views have all 64 rows -- and the oracle compares about twice the samples behind HME that the sub-sampled twin does
        assert case.cfg.hme_search_method == 0 and case.cfg.me_search_method != 0
        _, ops_sub = _stage5_ops(MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_no_exit))
        print(f"{name}: {ops} |a-b| behind HME, {ops_sub} with every other row")
        assert ops > 1.5 * ops_sub
    elif what[0] == "refs":
        live = want["do_ref"].reshape(-1, 2, 4) != 0
        assert len(case.refs) == what[1] and all(live[:, li, ri].any() for li, ri in case.refs)  # each of the four is still searched by some block
    elif what[0] == "tiles":
        _, w, h, axis = what
        tw, th = tile_of(w, h)
        print(f"{name}: {w}x{h} search area in tiles of {tw}x{th}")
        assert (th < h and tw == w) if axis == "rows" else (tw < w)
        _, ops_preset = _stage5_ops(MeCase(448, 136, enc_mode=6, kind="mixed", cfg_edit=_no_exit))
        print(f"{name}: {ops} |a-b| behind HME, {ops_preset} with the preset's own area")
        assert ops > 2 * ops_preset
    return case, want


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_what_it_is_named_for(name):
    """CPU only: the oracle shows that every case of this file has the alignments / blocks / tiles it is named for."""
    reference(name)


def test_tile_formula():
    assert tile_of(64, 32) == (64, 8) and tile_of(200, 8) == (56, 1) and tile_of(32, 16) == (32, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 2], ids=["one-kernel", "staged"])
@pytest.mark.parametrize("name", list(CASES))
def test_lds_dma_matches_oracle(hip_ctx, name, form):
    case, want = reference(name)
    hip_ctx.set_me_staged(form)
    try:
        got = case.run_hip(hip_ctx)
    finally:
        hip_ctx.set_me_staged(1)
    assert not compare(want, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_staged_launch_runs_the_tail(hip_ctx, name):
    """The staged setting really launches the chain (mid1, s1, mid2, s2, tail) for every case, and hands blocks back to the one-kernel form
    exactly when the picture has a narrow last column (the pre-pass counters: see test_me_tail_gpu.py)."""
    import torch
    from svt_av1_psyex_amd import abi
    case, _ = reference(name)
    cur = hip_ctx.upload(case.cur)
    refs = {k: hip_ctx.upload(v) for k, v in case.refs.items()}
    n = abi.n_pu(case.desc.enable_me_16x16, case.desc.enable_me_8x8)
    nb = ((case.desc.aligned_width + 63) // 64) * ((case.desc.aligned_height + 63) // 64)
    res, bufs = abi.MeResults(), {}
    for field, dt, cnt in abi.RESULT_FIELDS:
        bufs[field] = torch.zeros(nb * cnt(n, case.desc.max_refs, case.desc.max_cand) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
        setattr(res, field, bufs[field].data_ptr())
    torch.cuda.synchronize()

    def launch(form):
        hip_ctx.set_me_staged(form)
        hip_ctx.me_pictures_async([(case.cfg, case.desc, cur, refs, res)])
        return hip_ctx.me_launch_times(), hip_ctx.me_dense_counters()
    try:
        hip_ctx.set_me_counting(True)
        hip_ctx.set_me_timing(True)
        hip_ctx.me_dense_counters()
        one_kernels, (taken, own) = launch(0)
        kernels, (taken_s, own_s) = launch(2)
    finally:
        hip_ctx.set_me_staged(1)
        hip_ctx.set_me_timing(False)
        hip_ctx.set_me_counting(False)
        hip_ctx.sync()
        cur.free()
        for r in refs.values():
            r.free()
    print(f"{name}: one-kernel {sorted(one_kernels)} taken {taken} own {own}; staged {sorted(kernels)} taken {taken_s} own {own_s}")
    assert "svt_hip_me_b64_kernel" in one_kernels and "svt_hip_me_tail_kernel" not in one_kernels
    for k in ("svt_hip_me_mid1_kernel", "svt_hip_me_s1_kernel", "svt_hip_me_mid2_kernel", "svt_hip_me_s2_kernel", "svt_hip_me_tail_kernel"):
        assert k in kernels, k
    assert taken > 0 and taken_s == taken, (taken_s, taken)
    narrow = case.width % 64 != 0
    assert (own_s > own) == narrow, (own_s, own)
