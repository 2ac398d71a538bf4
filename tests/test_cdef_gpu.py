"""GPU: svt_hip_cdef_search_batch, svt_hip_cdef_pick_batch and svt_hip_cdef_apply_batch on the MI355X, every comparison exact -- against the
restatements (tests/cdef_cases.py) and the reference's own results (golden/cdef.npz): 8x8, 64x64, 72x40 and 136x72 pictures at 8 and 10 bits, noise,
gratings, flat and saturated steps, full, empty, one-block, checkerboard and random masks with stray bits, every subsampling factor, up to 64
strengths.  Outputs start as the byte 0xA5 with spare slots and are compared whole; input planes are checked unchanged.  The chain runs the three
on one stream with no host read in between."""
import numpy as np
import pytest

import cdef_cases as cc
from svt_av1_psyex_amd import api, cdef

pytestmark = pytest.mark.gpu

FILL = cc.FILL
SPARE = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(cc.GOLDEN)


def filled(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def run_search(ctx, c, with_block_dist=True):
    out = cdef.run_cdef_search_hip(ctx, c["recon"], c["src"], c["bd"], c["base_q_idx"], c["sf"], c["sy"], c["suv"], c["masks"], with_block_dist, SPARE, FILL)
    n_fb = cc.n_fb_of(c["w"], c["h"])
    names = ("dir", "var", "block_dist") if with_block_dist else ("dir", "var")
    assert filled(out["mse_spare"]) and len(out["mse_spare"]) == 2 * SPARE * 64, "spare mse slots written"
    for k in names:
        assert len(out[k]) == n_fb + SPARE and filled(out[k][n_fb:]), f"spare {k} slots written"
    assert all(np.array_equal(g, p) for g, p in zip(out["recon"] + out["src"], list(c["recon"]) + list(c["src"]))), "a plane changed"
    return {"mse": out["mse"], **{k: out[k][:n_fb] for k in names}}


@pytest.mark.parametrize("name", list(cc.SEARCH_CASES))
def test_search_equals_the_restatement_and_the_reference(hip_ctx, golden, name):
    """device == restatement on every byte of every output, block_dist per block among them (so what a skipped filter block, an unlisted block or an
    index past n_strengths leaves untouched is still 0xA5) == the fixture"""
    c, (want, _) = cc.search_case(name), cc.restated_search(name)
    got = run_search(hip_ctx, c)
    for k in ("dir", "var", "block_dist", "mse"):
        assert got[k].tobytes() == want[k].tobytes(), (name, k, np.argwhere(got[k] != want[k])[:6].tolist())
    n = len(c["sy"])
    assert np.array_equal(got["mse"][:, :, :n], golden[f"search_{name}_mse"]) and np.array_equal(got["dir"], golden[f"search_{name}_dir"])
    assert np.array_equal(got["var"], golden[f"search_{name}_var"])


def test_a_search_run_twice_gives_identical_bytes(hip_ctx):
    c = cc.search_case("noise_136x72_10")
    first, second = run_search(hip_ctx, c), run_search(hip_ctx, c)
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)


def test_block_dist_is_optional(hip_ctx):
    c, (want, _) = cc.search_case("grating_72x40_10"), cc.restated_search("grating_72x40_10")
    got = run_search(hip_ctx, c, with_block_dist=False)
    assert "block_dist" not in got and got["mse"].tobytes() == want["mse"].tobytes() and got["dir"].tobytes() == want["dir"].tobytes()


def run_pick(ctx, c):
    out = cdef.run_cdef_pick_hip(ctx, c["w"], c["h"], c["mse"], c["masks"], c["n"], c["is_hbd"], c["bias"], c["lam"], c["map_y"], c["map_uv"], SPARE, FILL)
    n_fb = len(c["masks"])
    assert filled(out["tail"]) and len(out["tail"]) == SPARE and filled(out["fb_strength"][n_fb:]) and len(out["fb_strength"]) == n_fb + SPARE
    r = out["result"]
    rec = {k: (r[k].tolist() if r[k].ndim else int(r[k])) for k in ("cdef_bits", "nb_strengths", "y_strength", "uv_strength", "best_cost", "zero_cost", "cdef_dist_dev")}
    assert int(r["reserved"]) == 0
    return {**rec, "fb_strength": out["fb_strength"][:n_fb], "mse": out["mse"]}


@pytest.mark.parametrize("name", list(cc.PICK_CASES))
def test_pick_equals_the_restatement_and_the_reference(hip_ctx, golden, name):
    """the result struct with both costs, the per-block indices (0xA5 where skipped) and mse as the bias left it"""
    c, (want, _) = cc.pick_case(name), cc.restated_pick(name)
    got = run_pick(hip_ctx, c)
    assert np.array_equal(cc.pick_record(got), cc.pick_record(want)), (name, cc.pick_record(got).tolist(), cc.pick_record(want).tolist())
    assert got["fb_strength"].tobytes() == want["fb_strength"].tobytes() and got["mse"].tobytes() == want["mse"].tobytes()
    assert np.array_equal(cc.pick_record(got, False), golden[f"pick_{name}_result"]) and np.array_equal(got["fb_strength"], golden[f"pick_{name}_fb_strength"])
    assert np.array_equal(got["mse"][:, :, 0], golden[f"pick_{name}_mse0"])


def test_a_pick_run_twice_gives_identical_bytes(hip_ctx):
    c = cc.pick_case("eight_clusters")
    first, second = run_pick(hip_ctx, c), run_pick(hip_ctx, c)
    assert np.array_equal(cc.pick_record(first), cc.pick_record(second)) and first["fb_strength"].tobytes() == second["fb_strength"].tobytes()


def run_apply(ctx, c):
    out = cdef.run_cdef_apply_hip(ctx, c["planes"], c["bd"], c["damping"], c["n_planes"], c["masks"], c["fb_strength"], c["y_strength"], c["uv_strength"], SPARE, FILL)
    assert all(np.array_equal(g, p) for g, p in zip(out["in"], c["planes"])), "an input plane changed"
    planes = []
    for flat, p in zip(out["planes"], c["planes"]):
        assert len(flat) == p.nbytes + SPARE and filled(flat[p.nbytes:]), "bytes behind an output plane written"
        planes.append(flat[:p.nbytes].view(p.dtype).reshape(p.shape))
    return planes


@pytest.mark.parametrize("name", list(cc.APPLY_CASES))
def test_apply_equals_the_restatement_and_the_reference(hip_ctx, golden, name):
    c, (want, _) = cc.apply_case(name), cc.restated_apply(name)
    got = run_apply(hip_ctx, c)
    assert len(got) == c["n_planes"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (name, i, np.argwhere(g != w)[:6].tolist())
        assert np.array_equal(g, golden[f"apply_{name}_plane{i}"])


def test_an_apply_run_twice_gives_identical_bytes(hip_ctx):
    c = cc.apply_case("chroma_zero")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(run_apply(hip_ctx, c), run_apply(hip_ctx, c)))


@pytest.mark.parametrize("name", list(cc.SEARCH_CASES))
def test_the_chain_runs_on_one_stream_without_a_host_read(hip_ctx, golden, name):
    """search, pick on the search's mse and masks where they lie, apply with the pick's strengths and indices where they lie; one wait at the end"""
    c = cc.search_case(name)
    s, p, planes, _ = cc.restated_chain(name)
    a = cc.chain_pick_args(name)
    dt = api.sample_dtype(c["bd"])
    t_recon, t_src = [api.to_device(x, dt) for x in c["recon"]], [api.to_device(x, dt) for x in c["src"]]
    t_masks = api.records_to_device(c["masks"], "<u8")
    so = cdef.run_cdef_search_device(hip_ctx, t_recon, t_src, c["w"], c["h"], c["bd"], c["base_q_idx"], c["sf"], c["sy"], c["suv"], t_masks, False, 0, FILL)
    po, work = cdef.run_cdef_pick_device(hip_ctx, c["w"], c["h"], a["n"], a["is_hbd"], a["bias"], a["lam"], a["map_y"], a["map_uv"], t_masks, so["mse"], 0, FILL)
    ao = cdef.run_cdef_apply_device(hip_ctx, t_recon, c["w"], c["h"], c["bd"], c["damping"], 3, t_masks, po["fb_strength"], po["result"], 0, FILL)
    hip_ctx.sync()
    del work
    n_fb = cc.n_fb_of(c["w"], c["h"])
    assert api.to_host(so["mse"], "<u8", (2, n_fb, 64)).tobytes() == p["mse"].tobytes(), "mse behind the bias"
    assert api.to_host(so["dir"], np.uint8, (n_fb, 64)).tobytes() == s["dir"].tobytes() and api.to_host(so["var"], "<i4", (n_fb, 64)).tobytes() == s["var"].tobytes()
    r = api.to_host(po["result"]).view(cdef.PICK_DTYPE)[0]
    got = {k: (r[k].tolist() if r[k].ndim else int(r[k])) for k in ("cdef_bits", "nb_strengths", "y_strength", "uv_strength", "best_cost", "zero_cost", "cdef_dist_dev")}
    assert np.array_equal(cc.pick_record(got), cc.pick_record(p)), (cc.pick_record(got).tolist(), cc.pick_record(p).tolist())
    assert np.array_equal(cc.pick_record(got, False), golden[f"chain_{name}_pick"])
    assert api.to_host(po["fb_strength"], np.int8).tobytes() == p["fb_strength"].tobytes()
    for i, (t, want) in enumerate(zip(ao, planes)):
        g = api.to_host(t, dt, want.shape)
        assert np.array_equal(g, want), (name, i, np.argwhere(g != want)[:6].tolist())
        assert np.array_equal(g, golden[f"chain_{name}_plane{i}"])
    assert all(np.array_equal(api.to_host(t, dt, x.shape), x) for t, x in zip(t_recon + t_src, list(c["recon"]) + list(c["src"]))), "a plane changed"
