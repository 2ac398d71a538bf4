"""GPU: svt_hip_masked_pred_batch, svt_hip_interintra_blend_batch and svt_hip_mask_search_batch on the MI355X, every comparison exact -- against the
restatement (tests/mask_cases.py) on every sample of every destination, mask buffer, result record and status slot (so what a job must not touch
is still the fill byte), and against the reference's own results (golden/mask.npz)."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
import mask_cases as mc
from svt_av1_psyex_amd import abi, api, mask, pred

pytestmark = pytest.mark.gpu

FILL = 0xA5
SPARE = 5
JOBS_PER_WORKGROUP = 4  # kWaves of csrc/mask_kernel.hip
COUNTS = [1, JOBS_PER_WORKGROUP - 1, JOBS_PER_WORKGROUP, JOBS_PER_WORKGROUP + 1, 65]


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.GOLDEN)


# ---- prediction ------------------------------------------------------------------------------------------------------------------------------
def run_pred(ctx, b, jobs=None, mask_in="own", planes=None):
    """the batch (or `jobs` of it) on a destination, a status array and a mask buffer pre-filled with 0xA5 (mask_in: "own" the batch's own buffer,
    None no buffer, or the bytes a chroma batch finds): checks the spare status slots and the reference planes; returns (plane, status, mask buffer)"""
    jobs = b["jobs"] if jobs is None else jobs
    planes = mc.pred_planes(b) if planes is None else planes
    if isinstance(mask_in, str):
        mask_in = np.full(b["mask_bytes"], FILL, np.uint8) if b["mask_bytes"] is not None else None
    out = mask.run_masked_pred_hip(ctx, b["bit_depth"], b["ss_x"], b["ss_y"], b["plane"], planes, jobs, b["dst_shape"], b["dst_stride"], mv_array=b["mv_array"],
                                   results=b["results"], mask_buf=mask_in, spare_jobs=SPARE, fill=FILL)
    n = len(jobs)
    assert len(out["status"]) == n + SPARE and np.all(out["status"][n:] == FILL), "spare status slots written"
    for got, (p, _, _) in zip(out["planes"], planes):
        assert np.array_equal(got, p), "a reference plane changed"
    return out["dst"], out["status"][:n], out["mask_buf"]


def check_pred(ctx, golden, name):
    """device == restatement on every sample of the destination and every byte of the mask buffer, == the fixture"""
    b = mc.pred_batch(name)
    want, defined, want_mask, _ = mc.pred_restated(name)
    mask_in = mc.pred_restated(b["mask_from"])[2] if b["mask_from"] else "own"
    img, status, got_mask = run_pred(ctx, b, mask_in=mask_in)
    assert all(defined) and np.all(status == mc.ST_OK), name
    assert np.array_equal(img, mc.pred_expected_image(b, want, FILL)), name
    if want_mask is not None:
        assert np.array_equal(got_mask, want_mask), f"{name}: the mask buffer"
    crcs = []
    for j in b["jobs"]:
        y, x = divmod(int(j["pred"]["dst_offset"]), b["dst_stride"])
        crcs.append(ip.crc(img[y:y + int(j["pred"]["height"]), x:x + int(j["pred"]["width"])].astype(np.uint16)))
    assert np.array_equal(np.array(crcs, np.uint32), golden[f"crc_{name}"]), name
    return img


@pytest.mark.parametrize("size", mc.WEDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_wedge_index_and_sign_on_luma_and_three_chroma_subsamplings(hip_ctx, golden, size):
    for bd in (8, 10):
        for sx, sy in mc.SUBSAMPLINGS:
            check_pred(hip_ctx, golden, f"wedge_{size[0]}x{size[1]}_{bd}_ss{sx}{sy}")


@pytest.mark.parametrize("size", mc.DIFFWTD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_diffwtd_both_mask_types_luma_then_the_chroma_that_reads_its_masks(hip_ctx, golden, size):
    """the luma batch's mask bytes are compared too (and with the fixture's CRCs); the chroma batches leave the buffer as they found it"""
    for bd in (8, 10):
        names = [n for n in mc.pred_batch_names() if n.startswith(f"diffwtd_{size[0]}x{size[1]}_{bd}_")]
        assert names[0].endswith("ss00") and len(names) >= 2
        for name in names:
            check_pred(hip_ctx, golden, name)
        b = mc.pred_batch(names[0])
        masks = mc.pred_restated(names[0])[2]
        crcs = [mc.crc8(masks[int(j["mask_offset"]):int(j["mask_offset"]) + size[0] * size[1]]) for j in b["jobs"]]
        assert np.array_equal(np.array(crcs, np.uint32), golden[f"maskcrc_{names[0]}"])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", ["variants", "geometry_stride203", "geometry_stride204", "fromarray"])
def test_variant_pairs_unaligned_destinations_and_parameters_from_the_arrays(hip_ctx, golden, group, bd):
    kind, _, rest = group.partition("_")
    check_pred(hip_ctx, golden, f"{kind}_{bd}" + (f"_{rest}" if rest else ""))


def test_sample_blocks_equal_the_fixture(hip_ctx, golden):
    for key, name, i in mc.pred_sample_jobs()[::5]:
        b = mc.pred_batch(name)
        img = run_pred(hip_ctx, b)[0]
        j = b["jobs"][i]
        y, x = divmod(int(j["pred"]["dst_offset"]), b["dst_stride"])
        assert np.array_equal(img[y:y + int(j["pred"]["height"]), x:x + int(j["pred"]["width"])], golden[key]), key


def test_a_luma_diffwtd_batch_without_a_mask_buffer_predicts_the_same(hip_ctx):
    b = mc.pred_batch("diffwtd_16x16_10_ss00")
    img, status, got_mask = run_pred(hip_ctx, b, mask_in=None)
    assert got_mask is None and np.all(status == mc.ST_OK)
    assert np.array_equal(img, mc.pred_expected_image(b, mc.pred_restated(b["name"])[0], FILL))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("dims", [(40, 24), (37, 21)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_blocks_over_each_edge_and_corner_of_a_small_plane_take_the_clamp_path(hip_ctx, dims, bd):
    b, planes = mc.edge_batch(bd, *dims)
    want, defined, want_mask, events = mc.run_pred_restated(b, planes=planes)
    assert all(defined) and not any(e["inside"] for e in events) and len(b["jobs"]) == 24
    img, status, got_mask = run_pred(hip_ctx, b, planes=planes)
    assert np.all(status == mc.ST_OK)
    assert np.array_equal(img, mc.pred_expected_image(b, want, FILL)) and np.array_equal(got_mask, want_mask)


@pytest.mark.parametrize("n,name", [(n, "variants_8" if n & 1 else "variants_10") for n in COUNTS] + [(1, "diffwtd_128x128_10_ss00"), (3, "diffwtd_128x128_8_ss00")])
def test_job_counts_around_a_workgroup(hip_ctx, n, name):
    b = mc.pred_batch(name)
    first = 0 if name.startswith("diffwtd") else 7
    jobs = list(np.concatenate([b["jobs"], b["jobs"]])[first:first + n])  # packed anew: every job has a block and a mask of its own
    sub = mc.finish_pred(f"{name}_{n}", b["bit_depth"], (0, 0), 0, mc.NOISE2, jobs, mask_bytes=mc.diffwtd_offsets(jobs))
    want, defined, want_mask, _ = mc.run_pred_restated(sub)
    img, status, got_mask = run_pred(hip_ctx, sub)
    assert len(sub["jobs"]) == n and all(defined) and np.all(status == mc.ST_OK)
    assert np.array_equal(img, mc.pred_expected_image(sub, want, FILL)) and np.array_equal(got_mask, want_mask)
    assert np.any(img != (FILL * 0x0101 if b["bit_depth"] > 8 else FILL))


def test_no_jobs_enqueue_nothing(hip_ctx):
    b = mc.pred_batch("variants_8")
    img, status, got_mask = run_pred(hip_ctx, b, b["jobs"][:0])
    assert np.all(img == FILL) and len(status) == 0 and np.all(got_mask == FILL)
    sb = mc.ties_batch(8)
    out = mask.run_mask_search_hip(hip_ctx, 8, 0, sb.planes["src"], sb.planes["pred0"], sb.planes["pred1"], sb.planes["intra"], sb.jobs[:0], spare_jobs=2, fill=FILL)
    assert np.all(out["results"].view(np.uint8) == FILL) and np.all(out["status"] == FILL)
    bb = mc.blend_batch(8, 0, 0)
    out = mask.run_interintra_blend_hip(hip_ctx, 8, bb["intra"], bb["inter"], bb["jobs"][:0], dst_shape=bb["dst_shape"], fill=FILL)
    assert np.all(out["dst"] == FILL)


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_report_0xff_write_nothing_else_and_leave_their_neighbours(hip_ctx, bd):
    b, bad, kinds = mc.undefined_pred_batch(bd)
    want, defined, want_mask, _ = mc.run_pred_restated(b)
    assert [i for i, ok in enumerate(defined) if not ok] == bad and len(bad) == len(kinds) + 1
    img, status, got_mask = run_pred(hip_ctx, b)
    assert np.array_equal(status, np.where(defined, mc.ST_OK, mc.ST_UNDEFINED))
    # the whole plane and the whole mask buffer: the ordinary jobs exact, the undefined jobs' blocks, masks and everything else still 0xA5
    assert np.array_equal(img, mc.pred_expected_image(b, want, FILL))
    assert np.array_equal(got_mask, want_mask)


@pytest.mark.parametrize("bd", [8, 10])
def test_chroma_diffwtd_without_a_mask_buffer_and_parameters_without_an_array_are_undefined(hip_ctx, bd):
    b = dict(mc.pred_batch(f"diffwtd_16x16_{bd}_ss11"))
    jobs = b["jobs"].copy()
    jobs[1]["comp_type"], jobs[1]["luma_width"], jobs[1]["luma_height"] = mc.WEDGE, 16, 16  # a wedge job needs no mask buffer
    jobs[2]["pred"]["flags"] = mc.PARAMS_FROM_ARRAY  # no result array
    b["jobs"] = jobs
    want, defined, _, _ = mc.run_pred_restated(b, mask_in=None)
    assert defined == [False, True, False, False]
    img, status, _ = run_pred(hip_ctx, b, mask_in=None)
    assert np.array_equal(status, np.where(defined, mc.ST_OK, mc.ST_UNDEFINED))
    assert np.array_equal(img, mc.pred_expected_image(b, want, FILL))


@pytest.mark.parametrize("bad", ["bit_depth_12", "ss_x_2", "n_refs_9", "zero_stride", "null_plane", "no_status", "no_jobs", "zero_dst_stride", "plane_3", "luma_with_ss",
                                 "mask_bytes_without_mask_buf", "n_results_without_results"])
def test_rejected_descriptor_returns_non_zero_and_leaves_the_buffers_as_filled(hip_ctx, bad):
    import torch
    fill = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    bufs = {"plane": fill(2 * 512 * 448), "dst": fill(2 * 256 * 64), "jobs": fill(72 * 6), "status": fill(6), "mask": fill(4096)}
    d = abi.MaskedPredDesc(bit_depth=10, ss_x=1, ss_y=1, n_refs=2, n_jobs=6, dst=bufs["dst"].data_ptr(), dst_stride=256, plane=1, dst_samples=256 * 64,
                           jobs=bufs["jobs"].data_ptr(), status=bufs["status"].data_ptr(), mask_buf=bufs["mask"].data_ptr(), mask_bytes=4096)
    for i in range(2):
        d.refs[i] = pred.plane_ref(bufs["plane"], 512, 160, 160, 512, 448)
    mc.spoil_pred_desc(d, bad)
    torch.cuda.synchronize()
    assert api.lib().svt_hip_masked_pred_batch(hip_ctx._h, C.byref(d)) == 2
    assert b"svt_hip_masked_pred_check_desc" in api.lib().svt_hip_last_error(None)
    hip_ctx.sync()
    for name, t in bufs.items():
        assert bool(torch.all(t == FILL)), name


# ---- blend -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.blend_batch_names())
def test_blend_seven_sizes_four_modes_sixteen_wedges_out_of_place_and_in_place(hip_ctx, golden, name):
    b = mc.blend_by_name(name)
    want = mc.blend_restated(name)
    dt = b["inter"].dtype
    for in_place in (False, True):
        out = mask.run_interintra_blend_hip(hip_ctx, b["bit_depth"], b["intra"], b["inter"], b["jobs"], dst_shape=None if in_place else b["dst_shape"],
                                            spare_jobs=SPARE, fill=FILL)
        n = len(b["jobs"])
        assert np.all(out["status"][:n] == mc.ST_OK) and np.all(out["status"][n:] == FILL)
        base = b["inter"] if in_place else np.full(b["dst_shape"], FILL * 0x0101 if b["bit_depth"] > 8 else FILL, dt)
        assert np.array_equal(out["dst"], mc.blend_expected_image(b, want, base)), (name, in_place)
        assert np.array_equal(out["intra"], b["intra"]) and (in_place or np.array_equal(out["inter"], b["inter"]))
    crcs = [ip.crc(mc.block_of(out["dst"], j["dst_offset"], int(j["width"]), int(j["height"])).astype(np.uint16)) for j in b["jobs"]]
    assert np.array_equal(np.array(crcs, np.uint32), golden[f"crc_{name}"])


@pytest.mark.parametrize("bd", [8, 10])
def test_blend_parameters_from_the_array_undefined_jobs_and_job_counts(hip_ctx, bd):
    b = dict(mc.blend_batch(bd, 1, 1))
    results = np.zeros(4, mc.RESULT_DTYPE)
    results["interintra_mode"], results["use_wedge_interintra"], results["wedge_index"] = [3, 0, 0xEE, 1], [0, 1, 1, 0], [-1, 11, -1, 0]
    jobs = b["jobs"][20:60].copy()
    for i, j in enumerate(jobs[:12]):
        j["flags"], j["result_index"] = mc.PARAMS_FROM_ARRAY, i % 6  # records 0, 1, 3 defined; 2 has wedge_index -1; 4, 5 are outside the array
        j["intra_offset"] = j["intra_offset"][int(j["interintra_mode"])]  # whichever mode the record names: the same block
        j["wedge_sign"] = 0
    jobs[12]["use_wedge"], jobs[12]["interintra_mode"], jobs[13]["luma_width"], jobs[14]["width"], jobs[15]["wedge_sign"] = 0, 4, 64, 12, 2
    jobs[16]["use_wedge"], jobs[17]["dst_offset"], jobs[18]["intra_offset"] = 2, b["inter"].size - 3, b["intra"].size - 3
    jobs[19]["use_wedge"], jobs[19]["wedge_index"] = 1, 16
    defined = [mc.blend_job_defined(b, j, results) for j in jobs]
    assert defined[:12] == [True, True, False, True, False, False] * 2 and not any(defined[12:20]) and all(defined[20:])
    for n in COUNTS[:-1] + [len(jobs)]:
        sub = dict(b, jobs=jobs[:n])
        want = [mc.restate_blend_job(b, b["intra"], b["inter"], j, results) if ok else None for j, ok in zip(sub["jobs"], defined)]
        out = mask.run_interintra_blend_hip(hip_ctx, bd, b["intra"], b["inter"], sub["jobs"], dst_shape=b["dst_shape"], results=results, fill=FILL)
        assert np.array_equal(out["status"], np.where(defined[:n], mc.ST_OK, mc.ST_UNDEFINED))
        base = np.full(b["dst_shape"], FILL * 0x0101 if bd > 8 else FILL, b["inter"].dtype)
        assert np.array_equal(out["dst"], mc.blend_expected_image(sub, want, base)), n


# ---- searches --------------------------------------------------------------------------------------------------------------------------------
def run_search(ctx, sb, jobs=None, planes=None):
    """(result records, status) on arrays pre-filled with 0xA5; the spare slots are checked"""
    jobs = sb.jobs if jobs is None else jobs
    p = sb.planes if planes is None else planes
    out = mask.run_mask_search_hip(ctx, sb.bit_depth, sb.mult, p["src"], p.get("pred0"), p["pred1"], p.get("intra"), jobs, spare_jobs=SPARE, fill=FILL)
    n = len(jobs)
    assert np.all(out["status"][n:] == FILL) and np.all(out["results"][n:].view(np.uint8) == FILL), "spare slots written"
    return out["results"][:n], out["status"][:n]


def filled_record():
    return np.frombuffer(bytes([FILL]) * np.dtype(mc.RESULT_DTYPE).itemsize, mc.RESULT_DTYPE)[0]


def restated_records(sb, jobs, planes=None):
    """what every defined job leaves of a record that starts as 0xA5 bytes (a job that exits writes `exit` alone); None for an undefined job"""
    p = sb.planes if planes is None else planes
    return [mc.restate_search_job(p, sb.bit_depth, sb.mult, j, before=filled_record())[0] if mc.search_job_defined(p, j) else None for j in jobs]


def check_search(ctx, sb, jobs=None, planes=None):
    jobs = sb.jobs if jobs is None else jobs
    want = restated_records(sb, jobs, planes)
    got, status = run_search(ctx, sb, jobs, planes)
    assert np.array_equal(status, [mc.ST_OK if w is not None else mc.ST_UNDEFINED for w in want])
    bad = [i for i, w in enumerate(want) if (w if w is not None else filled_record()).tobytes() != got[i].tobytes()]
    assert not bad, (sb.name, bad[:8], [(got[i], want[i]) for i in bad[:2]])
    return got


@pytest.mark.parametrize("name", sorted(mc.search_batches()))
def test_search_batches_equal_the_restatement_and_the_reference(hip_ctx, golden, name):
    """planted wedges (four ranges: the int16 clamp and the delta-square saturation fire or cannot), planted DIFFWTD masks and the job of the largest
    sums, ties, the gate at its threshold for multipliers 0 / 1 / 4, inter-intra modes and wedge modes; unequal strides and odd offsets throughout"""
    sb = mc.search_batches()[name]
    got = check_search(hip_ctx, sb)
    assert np.array_equal(mc.reference_outputs(sb, got), golden[f"search_{name}"])
    assert len({p.shape[1] for p in sb.planes.values()}) == 4 and {int(o) % 531 % 2 for o in sb.jobs["src_offset"]} == {0, 1}


@pytest.mark.parametrize("n", COUNTS)
def test_search_job_counts_around_a_workgroup(hip_ctx, n):
    for sb in (mc.planted_wedge_batch("full10")[0], mc.planted_seg_batch(8)[0], mc.ii_batch(10)[0]):
        check_search(hip_ctx, sb, sb.jobs[3:3 + n])


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_search_jobs_report_0xff_and_leave_their_records(hip_ctx, bd):
    sb = mc.ii_batch(bd)[0]
    wb = mc.planted_wedge_batch("full8" if bd == 8 else "full10")[0]
    jobs = np.concatenate([sb.jobs[:14], sb.jobs[:2]])
    jobs[1]["kind"], jobs[3]["ii_wedge_mode"], jobs[5]["width"], jobs[7]["kind"], jobs[9]["kind"] = 3, 3, 64, mc.KIND_WEDGE, mc.KIND_DIFFWTD
    jobs[7]["width"], jobs[7]["height"], jobs[9]["width"] = 16, 64, 4  # sizes outside the kind's
    jobs[11]["src_offset"], jobs[13]["intra_offset"][2] = sb.planes["src"].size - 8, sb.planes["intra"].size - 8
    jobs[14]["pred1_offset"] = sb.planes["pred1"].size - 1
    want = restated_records(sb, jobs)
    assert [w is None for w in want] == [False, True] * 7 + [True, False]
    check_search(hip_ctx, sb, jobs)
    # kinds 0 / 1 without a pred0 plane, kind 2 without an intra plane
    for planes, jobs in (({k: v for k, v in wb.planes.items() if k != "pred0"}, wb.jobs[:5]), ({k: v for k, v in sb.planes.items() if k != "intra"}, sb.jobs[:5])):
        got, status = run_search(hip_ctx, sb if planes.get("pred0") is not None else wb, jobs, planes)
        assert np.all(status == mc.ST_UNDEFINED) and np.all(got.view(np.uint8) == FILL)


@pytest.mark.parametrize("bad", ["use_rate", "use_rd_model", "bit_depth_12", "no_results", "zero_src_stride"])
def test_rejected_search_descriptor_enqueues_nothing(hip_ctx, bad):
    import torch
    fill = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    bufs = {k: fill(4096) for k in ("src", "pred0", "pred1", "intra", "jobs", "results", "status")}
    d = abi.MaskSearchDesc(bit_depth=8, pred0_to_pred1_mult=1, n_jobs=6, src_stride=64, pred0_stride=64, pred1_stride=64, intra_stride=64, src_samples=4096,
                           pred0_samples=4096, pred1_samples=4096, intra_samples=4096, **{k: t.data_ptr() for k, t in bufs.items()})
    mc.spoil_search_desc(d, bad)
    torch.cuda.synchronize()
    assert api.lib().svt_hip_mask_search_batch(hip_ctx._h, C.byref(d)) == 2
    assert b"svt_hip_mask_search_check_desc" in api.lib().svt_hip_last_error(None)
    hip_ctx.sync()
    for name, t in bufs.items():
        assert bool(torch.all(t == FILL)), name
