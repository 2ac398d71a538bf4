"""GPU: the direct HME level-1 / level-2 searches (run_small_searches_direct, csrc/me_kernel.hip) in their two layouts -- the ring form
(lane = request x slice of the block rows; requests that are alike) and the general item form (everything else: edge blocks whose
regions are clipped one by one) -- in both launch forms, bit for bit against the oracle.  The staged form reaches the function through
svt_hip_me_s1_kernel / svt_hip_me_s2_kernel, the one-kernel form through its HME stages.

Pictures are a few b64 blocks.  256 x 192 has two interior blocks (all requests 8 x 3: the ring form) inside a frame of edge blocks
(regions clipped to different sizes: the general form), so both forms run side by side in one kernel.  The exit thresholds in front of the
levels are switched off, so that every region of every reference pushes its search: nreq = 4 x the references.

What a case is for:
  refs_*      1 / 2 / 4 / 8 references: nreq = 4, 8, 16, 32, the lanes per request go 16 -> 2
  one_block   one b64 block, picture edge all around: four regions clipped to different widths and heights
  flat        constant luma: every position of every request ties; the first in raster order must win in each request
  shift_*     the reference is the source moved by a whole number of samples: exact matches (SAD 0 against the noise around them) at the
              first and at the last position of an 8 x 3 area around the level's centre
  rows_*      168 rows: the last block row is 40 high, 20 compared rows at level 2 and 10 at level 1 -- not a multiple of the slice count;
              200 x 136 adds 8-high and 8-wide blocks.  `allrows`: hme_search_method = 1, no row sub-sampling; such a picture has no
              pre-pass and runs the one-kernel form under either setting, which keeps the general layout -- the same
              requests through the other layout, against the same oracle
  extremes_*  samples 0 against 255 throughout, 8 references: 2 lanes per request, 16 block rows per lane -- a packed 16-bit sum holds
              4 rows of a 64-wide block, so a missed flush overflows it"""
import functools

import numpy as np
import pytest

from me_cases import MeCase, compare
from svt_av1_psyex_amd import synth

EIGHT_REFS = {(0, 0): 3, (0, 1): 2, (0, 2): 1, (0, 3): 0, (1, 0): 5, (1, 1): 6, (1, 2): 7, (1, 3): 8}
ODD_REFS = {(0, 0): 3, (0, 1): 1, (0, 2): 5, (0, 3): 7, (1, 0): 5, (1, 1): 7, (1, 2): 9, (1, 3): 3}  # `extremes`: odd frames are 255, frame 4 is 0


def _push_all(cfg):
    cfg.me_early_exit_th = 0
    cfg.prev_me_stage_based_exit_th = 0


def _all_rows(cfg):
    _push_all(cfg)
    cfg.hme_search_method = 1


def _case(w, h, edit=_push_all, **kw):
    return lambda: MeCase(w, h, enc_mode=6, cfg_edit=edit, **kw)


def _shifted(dx, dy):
    """noise; every reference is the source moved by (dx, dy)"""
    def build():
        case = MeCase(256, 192, enc_mode=6, kind="noise", cfg_edit=_push_all)
        f = case.cur.inner(2)
        pad = case.cur.planes[2][2]
        moved = np.roll(f, (dy, dx), (0, 1))
        case.refs = {k: synth.HostPyramid(moved, v.picture_number, pad=pad) for k, v in case.refs.items()}
        return case
    return build


CASES = {
    "refs_1_0":      _case(256, 192, refs={(0, 0): 0}),
    "refs_1_1":      _case(256, 192),
    "refs_2_2":      _case(256, 192, cur=2, refs={(0, 0): 1, (0, 1): 0, (1, 0): 3, (1, 1): 4}, n_frames=5),
    "refs_4_4":      _case(256, 192, cur=4, refs=EIGHT_REFS, n_frames=9),
    "one_block":     _case(64, 64),
    "flat":          _case(256, 192, kind="flat"),
    "shift_first":   _shifted(-4, -1),
    "shift_last":    _shifted(3, 1),
    "rows_168":      _case(256, 168),
    "rows_168_allrows": _case(256, 168, edit=_all_rows),
    "rows_136":      _case(200, 136, kind="fastpan"),
    "extremes":      _case(256, 192, cur=4, refs=ODD_REFS, n_frames=10, kind="extremes"),
    "extremes_allrows": _case(256, 192, cur=4, refs=ODD_REFS, n_frames=10, kind="extremes", edit=_all_rows),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case and its oracle results: computed once, shared by both launch forms"""
    case = CASES[name]()
    return case, case.run_cpu("oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 2], ids=["one-kernel", "staged"])
@pytest.mark.parametrize("name", list(CASES))
def test_direct_searches_match_oracle(hip_ctx, name, form):
    case, want = reference(name)
    hip_ctx.set_me_staged(form)
    try:
        got = case.run_hip(hip_ctx)
    finally:
        hip_ctx.set_me_staged(1)
    assert not compare(want, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_staged_launch_goes_through_the_search_kernels(hip_ctx, name):
    """From the launch's own kernel list: with the staged setting a picture with the sub-sampled HME runs s1 and s2 (and the one-kernel
    setting does not); without sub-sampling there is no pre-pass and the launch is never staged."""
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
        return hip_ctx.me_launch_times()
    try:
        hip_ctx.set_me_timing(True)
        one_kernels, kernels = launch(0), launch(2)
    finally:
        hip_ctx.set_me_staged(1)
        hip_ctx.set_me_timing(False)
        hip_ctx.sync()
        cur.free()
        for r in refs.values():
            r.free()
    print(f"{name}: one-kernel {sorted(one_kernels)}; staged {sorted(kernels)}")
    search = {"svt_hip_me_s1_kernel", "svt_hip_me_s2_kernel"}
    assert "svt_hip_me_b64_kernel" in one_kernels and not (search & set(one_kernels))
    if case.cfg.hme_search_method != 0:
        assert not (search & set(kernels))
        return
    assert search <= set(kernels)
