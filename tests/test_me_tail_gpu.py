"""GPU: the single-position SADs behind HME -- check_00_center's two SADs per reference and the 1-point probe of the 8x8-variance test --
which the tail kernel of the staged form computes without a search stage (c00_sads / probe_sads, csrc/me_kernel.hip) and the one-kernel
form with its search engines: both forms of the launch, bit for bit against the oracle.  Pictures are 200x136 unless a case says otherwise:
the last column and row of blocks are 8 wide / 8 high, and centres get clipped at the right and bottom edge.

What of that reaches the tail kernel.  The pre-pass fills slots only for blocks 64 wide (me_dense.inl, `active`), and mid1 hands every
block with a search the pre-pass did not make to the one-kernel form, so in the staged form
  - the 8-wide last column is deferred: its blocks check the one-kernel form's search engines, never c00_sads' `x < bw` / half-piece
    arithmetic, which stays unreached in the tail by any picture (it is there because both forms share the function's contract);
  - the 8-high bottom row (64 wide) does go through the tail: `y < bh` of c00_sads and the probe's rows below the block are covered;
  - a picture with hme_search_method != 0 has no pre-pass at all and is never staged: probe_outside_plane (me_cases.probe_outside_case)
    runs the one-kernel form under either setting.  probe_outside_plane_sub is its twin with the sub-sampled HME, which IS staged:
    the edge-clamped slow path of probe_sads runs there.
test_staged_launch_reaches_the_tail asserts all three on the GPU from the launch's own kernel list and the pre-pass counters.

A case that does not reach the new code proves nothing, so every case first shows on the CPU, through the oracle's |a - b| counter
(orc_sad_ops_stage), that its stage did work.  The counter has ONE slot (5) for everything behind HME -- centre checks, probe and integer
search together -- so a stage's own work is the difference to a TWIN case in which only that stage is switched off:
  check-00   is_ref = 0 (check_00_center needs is_ref, motion_estimation.c:1139-1206; with enable_me_sr_adjustment != 2 nothing else behind
             HME reads it).  Besides, the blocks that certainly pushed are counted from the oracle's outputs: a non-zero HME centre of a
             reference that is still searched after the final pruning.
  probe      me_8x8_var_enabled = 0 (only the probe reads it).
The two cases whose point is that the stage does nothing assert the opposite: no pushing block (is_ref = 0), a count equal to the twin's
(search area of 24 positions: no probe).  The two outside-plane cases also count, from the oracle's HME centres, the probes whose 64x64
window leaves the padded plane."""
import functools

import numpy as np
import pytest

from me_cases import MCTF_OUTPUTS, MeCase, compare, probe_outside_case
from svt_av1_psyex_amd import synth

W, H = 200, 136
FOUR_REFS = {(0, 0): 1, (0, 1): 0, (1, 0): 3, (1, 1): 4}


def _stage5_ops(case):
    """(oracle results, |a - b| evaluations behind HME) of one oracle run."""
    import pyoracle
    o = pyoracle.load_oracle()
    o.orc_sad_ops_stage.restype = np.ctypeslib.ctypes.c_uint64
    o.orc_sad_ops_stage(5, 1)
    want = case.run_cpu("oracle")
    return want, int(o.orc_sad_ops_stage(5, 1))


def _half_contrast(case):
    """The synthetic pictures carry noise that keeps every 64x64 SAD above 5000, the threshold enable_me_sr_adjustment == 2 compares list 0 /
    reference 0's SAD with: at half the contrast the blocks the pan predicts fall below it, the others stay above."""
    def half(pyr):
        f = pyr.inner(2).astype(np.int16)
        return synth.HostPyramid(((f - 128) // 2 + 128).astype(np.uint8), pyr.picture_number, pad=pyr.planes[2][2])
    case.cur = half(case.cur)
    case.refs = {k: half(v) for k, v in case.refs.items()}
    return case


def _c00(adj, **kw):
    def edit(cfg):
        cfg.me_early_exit_th = 0
        cfg.enable_me_sr_adjustment = adj
    shape = _half_contrast if adj == 2 else (lambda case: case)
    return lambda: shape(MeCase(W, H, enc_mode=6, kind="fastpan", cfg_edit=edit, **kw))


def _probe(edit=None, **kw):
    def ed(cfg):
        cfg.me_8x8_var_enabled = 1
        if edit:
            edit(cfg)
    kw.setdefault("kind", "fastpan")
    return lambda: MeCase(W, H, enc_mode=6, cfg_edit=ed, **kw)


def _set(**fields):
    def edit(cfg):
        for k, v in fields.items():
            setattr(cfg, k, v)
    return edit


def _small_area(cfg):  # 8 x 3 = 24 positions: not more than 24, no probe
    cfg.me_sa.sa_min.width = cfg.me_sa.sa_max.width = 8
    cfg.me_sa.sa_min.height = cfg.me_sa.sa_max.height = 3


def _outside_sub():
    """probe_outside_case with the sub-sampled HME (hme_search_method = 0), so that the launch has a pre-pass and can be staged.  640 wide:
    every block is 64 wide, none is deferred.  Pre-HME on i.i.d. noise lands anywhere in its strip, and with levels 1 / 2 off the integer
    search takes that centre unrefined; seed 5118 gives, in the last block row, one probe left of the padded plane (block 20, (-152, -8))
    and two below it (found with the oracle alone)."""
    ref = probe_outside_case()

    def edit(cfg):
        for name, _ in cfg._fields_:
            setattr(cfg, name, getattr(ref.cfg, name))
        cfg.hme_search_method = 0
    return MeCase(640, 144, enc_mode=11, cur=4, refs={(0, 0): 2, (0, 1): 3, (0, 2): 1, (1, 0): 0, (1, 1): 7}, n_frames=9, seed=5118, kind="noise",
                  temporal_layer_index=1, cfg_edit=edit)


def _outside_probes(case, want):
    """(block, list, reference) of the still-searched references whose probe window (64x64 at the HME centre) leaves the padded plane"""
    pad = case.cur.planes[2][2]
    sc = want["hme_sc"].reshape(-1, 2, 4, 2).astype(np.int64)
    live = want["do_ref"].reshape(-1, 2, 4) != 0
    by, bx = np.divmod(np.arange(sc.shape[0]), (case.width + 63) // 64)
    x, y = 64 * bx[:, None, None] + sc[..., 0], 64 * by[:, None, None] + sc[..., 1]
    out = (x < -pad) | (x + 63 > case.width + pad - 1) | (y < -pad) | (y + 63 > case.height + pad - 1)
    return [tuple(int(v) for v in i) for i in np.argwhere(out & live)]


def _no_is_ref(case):
    case.desc.is_ref = 0


def _no_probe(case):
    case.cfg.me_8x8_var_enabled = 0


# name -> (builder, stage, the stage works (True) / must not (False), what switches the stage off in the twin, outputs compared)
CASES = {
    "c00_is_ref":          (_c00(1, is_ref=1), "c00", True, _no_is_ref, None),
    "c00_not_ref":         (_c00(1, is_ref=0), "c00", False, None, None),
    "c00_is_ref_adj2":     (_c00(2, is_ref=1), "c00", True, _no_is_ref, None),
    "c00_not_ref_adj2":    (_c00(2, is_ref=0), "c00", False, None, None),
    "probe_mult2":         (_probe(_set(me_sr_mult2_th=0)), "probe", True, _no_probe, None),
    "probe_div4":          (_probe(_set(me_sr_div4_th=0xFFFFFFFF)), "probe", True, _no_probe, None),
    "probe_div2":          (_probe(_set(me_sr_div4_th=0, me_sr_div2_th=0xFFFFFFFF)), "probe", True, _no_probe, None),
    "probe_small_area":    (_probe(_small_area), "probe", False, _no_probe, None),
    "probe_all_rows":      (_probe(_set(me_search_method=1)), "probe", True, _no_probe, None),
    "probe_four_refs":     (_probe(cur=2, refs=FOUR_REFS, n_frames=5), "probe", True, _no_probe, None),
    "probe_one_ref":       (_probe(refs={(0, 0): 0}), "probe", True, _no_probe, None),
    "probe_outside_plane": (probe_outside_case, "probe", True, _no_probe, None),
    "probe_outside_plane_sub": (_outside_sub, "probe", True, _no_probe, None),
    "mctf":                (_probe(refs={(0, 0): 1}, mctf_exit_th=0), "probe", True, _no_probe, MCTF_OUTPUTS),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its oracle results (computed once, shared by both forms) -- after the proof that the case reaches its stage."""
    build, stage, works, switch_off, names = CASES[name]
    case = build()
    want, ops = _stage5_ops(case)
    assert ops > 0, "no integer search at all"
    if stage == "c00":
        assert case.cfg.me_early_exit_th == 0
        sc = want["hme_sc"].reshape(-1, 2, 4, 2)
        live = want["do_ref"].reshape(-1, 2, 4) != 0
        nl = case.desc.num_of_list_to_search
        assert nl == 2
        pushing = int(((sc[:, :nl, :1] != 0).any(-1) & live[:, :nl, :1]).sum()) if case.desc.is_ref else 0
        print(f"{name}: {pushing} (block, reference) pairs push check-00 SADs for certain; {ops} |a-b| behind HME")
        assert (pushing > 0) == works
        if case.cfg.enable_me_sr_adjustment == 2:  # the second group of references depends on list 0 / reference 0's 64x64 SAD: both outcomes
            s00 = want["sb_best_sad"].reshape(-1, 2, 4, 85)[:, 0, 0, 0]
            assert (s00 < 5000).any() and (s00 >= 5000).any()
    if switch_off:
        twin = build()
        switch_off(twin)
        _, ops_off = _stage5_ops(twin)
        print(f"{name}: {ops} |a-b| behind HME, {ops_off} with the stage switched off")
        assert (ops != ops_off) == works
    if name == "probe_outside_plane":
        assert tuple(want["hme_sc"].reshape(-1, 2, 4, 2)[22, 1, 0]) == (16, 184)  # 184 rows below a 16-row block of a 144-row picture
    if name.startswith("probe_outside_plane"):
        outside = _outside_probes(case, want)
        print(f"{name}: probes outside the padded plane at (block, list, reference) {outside}")
        assert outside and case.cfg.me_8x8_var_enabled
        if name == "probe_outside_plane_sub":
            assert case.cfg.hme_search_method == 0 and case.width % 64 == 0
            assert (20, 1, 0) in outside and len(outside) == 3  # left of the plane and below it
    return case, want, names


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_stage(name):
    """CPU only: every case of this file makes the oracle do (or, for two of them, not do) the work it is named for."""
    reference(name)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 2], ids=["one-kernel", "staged"])
@pytest.mark.parametrize("name", list(CASES))
def test_tail_matches_oracle(hip_ctx, name, form):
    case, want, names = reference(name)
    hip_ctx.set_me_staged(form)
    try:
        got = case.run_hip(hip_ctx)
    finally:
        hip_ctx.set_me_staged(1)
    assert not compare(want, got, names)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_staged_launch_reaches_the_tail(hip_ctx, name):
    """Which kernels the staged setting really launches, and which blocks it hands back to the one-kernel form.  The pre-pass counters
    (taken, own) count, in mid1 and in the one-kernel form, the searches a block took from the pre-pass / had to make itself; a deferred
    block is counted in mid1 up to the search that deferred it and then again, in full, by the one-kernel form.  So against the counters of
    the one-kernel setting:
      own grows    <=> a block was deferred for a search the pre-pass did not make (the only blocks without a slot are the narrow ones);
      taken grows  <=> a deferred block had taken slots before: a 64-wide one.
    Asserted: the tail kernel ran; no 64-wide block was deferred (the 8-high bottom row included); blocks were deferred exactly when the
    picture has a narrow last column.  With hme_search_method != 0 there is no pre-pass and the launch is not staged at all."""
    import torch
    from svt_av1_psyex_amd import abi
    case, _, _ = reference(name)
    cur = hip_ctx.upload(case.cur)
    refs = {k: hip_ctx.upload(v) for k, v in case.refs.items()}
    n = abi.n_pu(case.desc.enable_me_16x16, case.desc.enable_me_8x8)
    nb = ((case.desc.aligned_width + 63) // 64) * ((case.desc.aligned_height + 63) // 64)
    res, bufs = abi.MeResults(), {}
    for field, dt, cnt in abi.RESULT_FIELDS:
        bufs[field] = torch.zeros(nb * cnt(n, case.desc.max_refs, case.desc.max_cand) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
        setattr(res, field, bufs[field].data_ptr())
    torch.cuda.synchronize()

    def launch(form):  # the asynchronous entry: the launch on the context stream is the one svt_hip_me_launch_times reports
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
    if case.cfg.hme_search_method != 0:
        assert "svt_hip_me_tail_kernel" not in kernels and (taken, own, taken_s, own_s) == (0, 0, 0, 0)
        return
    assert "svt_hip_me_tail_kernel" in kernels and taken > 0
    assert taken_s == taken, (taken_s, taken)
    narrow = case.width % 64 != 0
    assert (own_s > own) == narrow and (own > 0) == narrow, (own_s, own)
