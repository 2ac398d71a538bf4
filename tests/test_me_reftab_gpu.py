"""GPU: the per-wave reference table of the ME chain's control code (csrc/me_kernel.hip: RefTab).  A wave keeps, in LDS, what its
lane-parallel stages want to know about the eight (list, reference) slots of the picture it works on -- planes, distances, live / searched
bits, pre-HME strip sizes -- and refills it when a job belongs to another picture than its previous job.  What can go wrong is a STALE or
half-filled table when a wave moves from one picture to the next, so every case here is ONE launch of several small pictures with
different reference structures, walked by so few waves that each wave sees them all.

How a wave is made to walk several pictures.  A launch starts min(waves per CU x CUs, blocks) persistent waves, and the limit per CU
(set_me_waves_per_cu) cannot go below one wave on each of the 256 CUs -- more than the 16 x 12 blocks a launch of sixteen 256 x 192
pictures has, so with that limit alone every wave would still get a single block.  The launches here also take set_me_max_waves(3): three
waves for the whole launch.  The staged kernels then deal the launch's job range round-robin (wave w: jobs w, w + 3, ...), the one-kernel
form's waves drain the eight band queues one after the other: either way every wave crosses every picture boundary of the launch.

Pictures (configurations of tests/me_cases.py, none larger than 256 x 192):
  base      temporal layer 0 with two lists: list 1 is not searched -- prehme_final mirrors list 0's strips into it and the search centre's
            hme_sad carries over from list 0's last reference
  one_one   1 + 1 references, temporal layer 1
  mrp       preset 0, 3 + 2 references: the general candidate path; prune_me_candidates_th and use_best_unipred_cand_only set
  gm        temporal layer 2, distances 4 / 4, gm_enabled; 200 wide: a narrow last column, whose blocks the staged form defers
  far       preset 4, temporal layer 3, 2 + 1 references at distances 1, 3 / 5
  single    one reference, one list
Every result field of every picture is compared with the oracle AND with the same picture launched alone; the reversed and the
interleaved (A B A B ...: a picture's table is refilled after another picture's overwrote it) orders must give each picture the results
of the forward order.  Edge shapes: a 64 x 64 picture (one block), the narrow last column, bands of one block row (b64_row_start /
b64_row_count).  Both forms: set_me_staged(2) and set_me_staged(0)."""
import functools

import numpy as np
import pytest

from me_cases import MeCase, compare, fill_unsearched


def _mrp_edit(cfg):
    cfg.prune_me_candidates_th = 30
    cfg.use_best_unipred_cand_only = 1


PICTURES = {
    "base":    lambda: MeCase(256, 192, enc_mode=6, cur=2, refs={(0, 0): 0, (1, 0): 4}, n_frames=5, temporal_layer_index=0, seed=11),
    "one_one": lambda: MeCase(192, 128, enc_mode=6, seed=12),
    "mrp":     lambda: MeCase(256, 192, enc_mode=0, cur=3, refs={(0, 0): 2, (0, 1): 1, (0, 2): 0, (1, 0): 4, (1, 1): 5}, n_frames=6, seed=13,
                              kind="mixed", cfg_edit=_mrp_edit),
    "gm":      lambda: MeCase(200, 136, enc_mode=4, cur=4, refs={(0, 0): 0, (1, 0): 8}, n_frames=9, temporal_layer_index=2, gm_enabled=1,
                              seed=14, kind="fastpan"),
    "far":     lambda: MeCase(256, 128, enc_mode=4, cur=3, refs={(0, 0): 2, (0, 1): 0, (1, 0): 8}, n_frames=9, temporal_layer_index=3, seed=15),
    "single":  lambda: MeCase(128, 192, enc_mode=9, cur=1, refs={(0, 0): 0}, seed=16, kind="noise"),
    "one_block": lambda: MeCase(64, 64, enc_mode=6, seed=17),
    "band_row1": lambda: _band(MeCase(192, 192, enc_mode=6, seed=18), 1),
    "band_row2": lambda: _band(MeCase(192, 192, enc_mode=2, cur=2, refs={(0, 0): 1, (0, 1): 0, (1, 0): 3}, n_frames=4, seed=19), 2),
}
FORWARD = ["base", "one_one", "mrp", "gm", "far", "single"]
ORDERS = {
    "forward": FORWARD,
    "reversed": FORWARD[::-1],
    "interleaved": ["base", "mrp", "base", "mrp", "gm", "single", "gm", "single", "one_one", "far", "one_one", "far"],
}
EDGES = ["one_block", "gm", "band_row1", "one_one", "band_row2", "one_block"]


def _band(case, row):
    case.desc.b64_row_start, case.desc.b64_row_count = row, 1
    return case


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, oracle results) of one picture: computed once, shared by every launch it takes part in."""
    case = PICTURES[name]()
    assert case.width <= 256 and case.height <= 192 and case.cfg.hme_search_method == 0  # small, and a launch with a pre-pass: it can be staged
    return case, case.run_cpu("oracle")


def _rows(case):
    """the b64 rows of the picture's band, as a slice of block indices"""
    d = case.desc
    w64, h64 = (d.aligned_width + 63) // 64, (d.aligned_height + 63) // 64
    r0 = d.b64_row_start
    r1 = r0 + (d.b64_row_count or (h64 - r0))
    return slice(r0 * w64, r1 * w64), w64 * h64


def _same(case, a, b):
    rows, nb = _rows(case)
    return compare({k: np.asarray(v).reshape(nb, -1)[rows] for k, v in a.items()}, {k: np.asarray(b[k]).reshape(nb, -1)[rows] for k in a})


def _launch(ctx, names, form, max_waves=3):
    """one svt_hip_me_pictures_async launch of the named pictures in this order (a name may come twice: every entry has result buffers of
    its own) -> the list of their result dicts"""
    import torch
    from svt_av1_psyex_amd import abi
    uploaded, jobs, keep = {}, [], []
    try:
        for name in names:
            case, _ = reference(name)
            if name not in uploaded:
                uploaded[name] = (ctx.upload(case.cur), {k: ctx.upload(v) for k, v in case.refs.items()})
            cur, refs = uploaded[name]
            d = case.desc
            n, nb = abi.n_pu(d.enable_me_16x16, d.enable_me_8x8), _rows(case)[1]
            res, bufs = abi.MeResults(), {}
            for field, dt, cnt in abi.RESULT_FIELDS:
                bufs[field] = torch.zeros(nb * cnt(n, d.max_refs, d.max_cand) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
                setattr(res, field, bufs[field].data_ptr())
            jobs.append((case.cfg, d, cur, refs, res))
            keep.append((case, bufs, nb))
        torch.cuda.synchronize()
        ctx.set_me_staged(form)
        ctx.set_me_waves_per_cu(1)
        ctx.set_me_max_waves(max_waves)
        ctx.set_me_timing(True)
        ctx.me_pictures_async(jobs)
        kernels = ctx.me_launch_times()
        ctx.sync()
        assert ("svt_hip_me_tail_kernel" in kernels) == (form == 2) and "svt_hip_me_b64_kernel" in kernels, kernels
        return [fill_unsearched(case.desc, {f: bufs[f].cpu().numpy().view(dt).reshape(nb, -1).copy() for f, dt, _ in abi.RESULT_FIELDS})
                for case, bufs, nb in keep]
    finally:
        ctx.set_me_timing(False)
        ctx.set_me_max_waves(0)
        ctx.set_me_waves_per_cu(0)
        ctx.set_me_staged(1)
        ctx.sync()
        for cur, refs in uploaded.values():
            cur.free()
            for r in refs.values():
                r.free()


def _alone(ctx, name, form):
    """the picture in a launch of its own (the synchronous entry), every wave the launch would normally get"""
    case, _ = reference(name)
    ctx.set_me_staged(form)
    try:
        return case.run_hip(ctx)
    finally:
        ctx.set_me_staged(1)


def test_pictures_differ_in_what_the_table_holds():
    """CPU only: the pictures of the launches really have different reference structures -- list and reference counts, searched lists,
    distances, temporal layers, GM -- so a table left over from the neighbour is a wrong table."""
    cases = [reference(n)[0] for n in FORWARD]
    shape = lambda c: (c.desc.num_of_list_to_search, tuple(c.desc.num_of_ref_pic_to_search))
    dists = lambda c: tuple(sorted(abs(int(c.desc.picture_number) - int(c.desc.ref_picture_number[li][ri])) for li, ri in c.refs))
    assert len({shape(c) for c in cases}) >= 4 and len({dists(c) for c in cases}) == len(cases)
    assert len({c.desc.temporal_layer_index for c in cases}) >= 4
    base, mrp, gm = reference("base")[0], reference("mrp")[0], reference("gm")[0]
    assert base.desc.temporal_layer_index == 0 and base.desc.num_of_list_to_search == 2  # list 1 exists and is not searched
    assert min(mrp.desc.num_of_ref_pic_to_search) >= 2 and mrp.cfg.prune_me_candidates_th and mrp.cfg.use_best_unipred_cand_only
    assert gm.desc.gm_enabled and gm.width % 64 == 8
    assert sum(_rows(c)[1] for c in cases) > 3 * 8  # more blocks than three waves can take one each, whatever the order
    for n in ("band_row1", "band_row2"):
        assert reference(n)[0].desc.b64_row_count == 1 and reference(n)[0].desc.b64_row_start > 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", [2, 0], ids=["staged", "one-kernel"])
def test_one_launch_of_different_pictures(hip_ctx, form):
    got = _launch(hip_ctx, FORWARD, form)
    for name, g in zip(FORWARD, got):
        case, want = reference(name)
        assert not _same(case, want, g), name
        assert not _same(case, _alone(hip_ctx, name, form), g), name


@pytest.mark.gpu
@pytest.mark.parametrize("form", [2, 0], ids=["staged", "one-kernel"])
@pytest.mark.parametrize("order", ["reversed", "interleaved"])
def test_order_of_the_pictures_does_not_matter(hip_ctx, order, form):
    forward = dict(zip(FORWARD, _launch(hip_ctx, FORWARD, form)))
    got = _launch(hip_ctx, ORDERS[order], form)
    for name, g in zip(ORDERS[order], got):
        case, want = reference(name)
        assert not _same(case, forward[name], g), name
        assert not _same(case, want, g), name


@pytest.mark.gpu
@pytest.mark.parametrize("form", [2, 0], ids=["staged", "one-kernel"])
@pytest.mark.parametrize("max_waves", [1, 3])
def test_edge_shapes(hip_ctx, form, max_waves):
    """one block, a narrow last column (deferred blocks in the staged form), bands of one block row -- with one wave for the whole launch
    and with three"""
    got = _launch(hip_ctx, EDGES, form, max_waves)
    for name, g in zip(EDGES, got):
        case, want = reference(name)
        assert not _same(case, want, g), name
        assert not _same(case, _alone(hip_ctx, name, form), g), name
