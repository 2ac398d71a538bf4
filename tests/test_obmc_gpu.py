"""GPU: svt_hip_obmc_neighbour_batch, svt_hip_obmc_blend_batch and svt_hip_obmc_target_batch against the restatement of tests/obmc_cases.py (which
golden/obmc.npz pins on the reference block by block), bit for bit.  Every buffer a launch writes starts as the byte 0xA5 or as known content and is
compared whole, so a sample outside a job's region must come back untouched; the per-job refusals run in batches that also hold valid jobs."""
import numpy as np
import pytest

import inter_pred_cases as ip
import obmc_cases as oc
from svt_av1_psyex_amd import obmc

pytestmark = pytest.mark.gpu


def run_batch(ctx, b, name=None, jobs=None, pred=None, offsets=None):
    """every launch of a batch on the device, each on the restatement's inputs of that step: {"above", "left", "blend": {plane: plane}, "wsrc", "mask",
    "status": {(entry, plane): bytes}, "planes_ok"}"""
    dt = np.uint16 if b["bit_depth"] > 8 else np.uint8
    jobs = oc.all_jobs(b) if jobs is None else jobs
    above, left = oc.fill_array(b["strip_samples"], dt), oc.fill_array(b["strip_samples"], dt)
    out = {"blend": {}, "status": {}, "planes_ok": True}
    for plane in b["run_planes"]:
        planes = oc.ref_planes(b, plane)
        r = obmc.run_neighbour_hip(ctx, b["bit_depth"], oc.SS[plane], oc.SS[plane], plane, planes, b["blocks"], jobs, above, left, mv_array=b["mv_array"],
                                   spare_jobs=3, fill=oc.FILL)
        above, left, out["status"][("neighbour", plane)] = r["above"], r["left"], r["status"]
        out["planes_ok"] = out["planes_ok"] and all(np.array_equal(a, p) for a, (p, _, _) in zip(r["planes"], planes))
    out["above"], out["left"] = above, left
    for plane in b["run_planes"]:
        j = jobs.copy()
        j["offset"] = offsets[plane] if offsets else oc.pred_layout(name, plane)[0]
        dst = pred[plane] if pred else oc.pred_plane(name, plane)
        r = obmc.run_blend_hip(ctx, b["bit_depth"], oc.SS[plane], oc.SS[plane], plane, b["blocks"], j, above, left, dst, spare_jobs=3, fill=oc.FILL)
        out["blend"][plane], out["status"][("blend", plane)] = r["dst"], r["status"]
        out["planes_ok"] = out["planes_ok"] and np.array_equal(r["above"], above) and np.array_equal(r["left"], left)
    if 0 in b["run_planes"]:
        off, n = oc.target_offsets(b)
        j = jobs.copy()
        j["offset"][:len(off)] = off
        r = obmc.run_target_hip(ctx, b["bit_depth"], b["blocks"], j, above, left, oc.src_plane(b["src"]), n, spare_jobs=3, fill=oc.FILL)
        out["wsrc"], out["mask"], out["status"][("target", 0)] = r["wsrc"], r["mask"], r["status"]
    return out


@pytest.mark.parametrize("name", oc.batch_names())
def test_every_entry_equals_the_restatement_bit_for_bit(hip_ctx, name):
    b = oc.batch(name)
    got, want = run_batch(hip_ctx, b, name), oc.restated(name)
    n = len(b["blocks"])
    for key, st in got["status"].items():
        assert np.all(st[:n] == oc.ST_OK) and np.all(st[n:] == oc.FILL), key  # the spare status slots are untouched
    assert got["planes_ok"]  # the inputs are untouched
    assert np.array_equal(got["above"], want["above"]) and np.array_equal(got["left"], want["left"])
    for plane in b["run_planes"]:
        assert np.array_equal(got["blend"][plane], want["blend"][plane]), plane
    if 0 in b["run_planes"]:
        assert np.array_equal(got["wsrc"], want["wsrc"]) and np.array_equal(got["mask"], want["mask"])


@pytest.mark.parametrize("bd", [8, 10])
def test_target_reduces_10_bit_strips_to_their_8_bit_part_on_the_same_blocks(hip_ctx, bd):
    """the same blocks and strips read as 8-bit and as 10-bit buffers: the 10-bit launch sees (sample >> 2) & 0xFF"""
    b = oc.batch(f"sizes_32x32_{bd}")
    want = oc.restated(b["name"])
    off, n = oc.target_offsets(b)
    jobs = oc.all_jobs(b, off)
    got = obmc.run_target_hip(hip_ctx, bd, b["blocks"], jobs, want["above"], want["left"], oc.src_plane("noise"), n, fill=oc.FILL)
    assert np.array_equal(got["wsrc"], want["wsrc"]) and np.array_equal(got["mask"], want["mask"])
    if bd == 10:
        a8, l8 = (((x >> 2) & 0xFF).astype(np.uint8) for x in (want["above"], want["left"]))
        got8 = obmc.run_target_hip(hip_ctx, 8, b["blocks"], jobs, a8, l8, oc.src_plane("noise"), n, fill=oc.FILL)
        assert np.array_equal(got8["wsrc"], want["wsrc"]) and np.array_equal(got8["mask"], want["mask"])


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_get_status_ff_and_write_nothing_else(hip_ctx, bd):
    b, bad = oc.undefined_batch(bd)
    n = len(b["blocks"])
    jobs = np.zeros(n + 2, oc.JOB_DTYPE)
    jobs["block"] = list(range(n)) + [n, 0xFFFFFFFF]  # block indices outside the array
    offsets, pred = {}, {}
    rng = np.random.default_rng([8, bd])
    dt, mx = (np.uint16 if bd > 8 else np.uint8), (1 << bd) - 1
    for plane in range(3):
        ss = oc.SS[plane]
        fake = np.zeros(n + 2, ip.JOB_DTYPE)
        fake["width"][:n], fake["height"][:n] = np.minimum(b["blocks"]["width"], 64) >> ss, np.minimum(b["blocks"]["height"], 64) >> ss
        fake["width"][n:], fake["height"][n:] = 8, 8
        packed, rows = ip.pack(list(fake), oc.PRED_STRIDE)
        offsets[plane] = packed["dst_offset"].astype(np.uint32)
        pred[plane] = rng.integers(0, mx + 1, (rows, oc.PRED_STRIDE)).astype(dt)
    # one blend job whose block does not end inside the prediction plane, one target job whose values do not end inside wsrc / mask
    last_ok = next(i for i in reversed(range(n)) if oc.block_ok(b["blocks"][i]) and i not in bad.values())
    blk = b["blocks"][last_ok]
    for plane in range(3):
        offsets[plane][last_ok] = pred[plane].size - ((int(blk["height"]) >> oc.SS[plane]) - 1) * oc.PRED_STRIDE - (int(blk["width"]) >> oc.SS[plane]) + 1
    got = run_batch(hip_ctx, b, jobs=jobs, pred=pred, offsets=offsets)
    above, left, _ = oc.restate_neighbours(b, {p: jobs for p in range(3)})
    assert np.array_equal(got["above"], above) and np.array_equal(got["left"], left)
    for plane in range(3):
        j = jobs.copy()
        j["offset"] = offsets[plane]
        want_st = [oc.ST_OK if oc.neighbour_job_defined(b, x, plane) else oc.ST_UNDEFINED for x in jobs]
        assert list(got["status"][("neighbour", plane)][:n + 2]) == want_st and np.all(got["status"][("neighbour", plane)][n + 2:] == oc.FILL)
        want_st = [oc.ST_OK if oc.blend_job_defined(b, x, plane, oc.PRED_STRIDE, pred[plane].size) else oc.ST_UNDEFINED for x in j]
        assert list(got["status"][("blend", plane)][:n + 2]) == want_st and want_st[last_ok] == oc.ST_UNDEFINED
        assert np.array_equal(got["blend"][plane], oc.restate_blend(b, plane, above, left, pred[plane], j)), plane
    off, n_out = oc.target_offsets(b)
    j = jobs.copy()
    j["offset"][:n] = off
    want_st = [oc.ST_OK if oc.target_job_defined(b, x, (ip.PIC_H, ip.PIC_W), n_out) else oc.ST_UNDEFINED for x in j]
    assert list(got["status"][("target", 0)][:n + 2]) == want_st
    wsrc, mask = oc.restate_target(b, above, left, j, n_out)
    assert np.array_equal(got["wsrc"], wsrc) and np.array_equal(got["mask"], mask)
    # the kinds each entry refuses, and that valid jobs ran among them
    for plane in range(3):
        st = got["status"][("neighbour", plane)]
        assert {i for i in range(n) if st[i]} == {i for k, i in bad.items() if k != "strip_end" or plane == 2}
    assert sum(s == oc.ST_OK for s in want_st) >= 2 * len(bad)


@pytest.mark.parametrize("bd", [8, 10])
def test_buffer_ends_are_refused_per_job(hip_ctx, bd):
    """a target job whose values end one past wsrc / mask, a source block that ends one sample past the source, a block of negative origin"""
    b = oc.batch(f"sizes_16x16_{bd}")
    want = oc.restated(b["name"])
    off, n_out = oc.target_offsets(b)
    jobs = oc.all_jobs(b, off)
    jobs["offset"][3] = n_out - 16 * 16 + 1
    blocks = b["blocks"].copy()
    blocks[5]["org_x"], blocks[5]["org_y"] = ip.PIC_W - 15, ip.PIC_H - 16
    blocks[6]["org_x"] = -4
    bb = dict(b, blocks=blocks)
    got = obmc.run_target_hip(hip_ctx, bd, blocks, jobs, want["above"], want["left"], oc.src_plane("noise"), n_out, fill=oc.FILL)
    assert [i for i, s in enumerate(got["status"]) if s] == [3, 5, 6] and set(got["status"]) == {oc.ST_OK, oc.ST_UNDEFINED}
    wsrc, mask = oc.restate_target(bb, want["above"], want["left"], jobs, n_out)
    assert np.array_equal(got["wsrc"], wsrc) and np.array_equal(got["mask"], mask)


def test_an_empty_batch_enqueues_nothing(hip_ctx):
    b = oc.batch("sizes_8x8_8")
    none = np.zeros(0, oc.JOB_DTYPE)
    above = oc.fill_array(b["strip_samples"], np.uint8)
    r = obmc.run_neighbour_hip(hip_ctx, 8, 0, 0, 0, oc.ref_planes(b, 0), b["blocks"], none, above, above, spare_jobs=2, fill=oc.FILL)
    assert np.all(r["status"] == oc.FILL) and np.array_equal(r["above"], above) and np.array_equal(r["left"], above)
