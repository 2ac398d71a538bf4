"""CPU: the restatement of the masked predictions and their searches (tests/mask_cases.py) against the reference's own results (golden/mask.npz), the
library's wedge tables against the fixture's CRCs, the conditions of the planted search inputs recomputed from the restatement, the struct
lay-outs of abi.py against the library's, and the three check_desc functions (validation needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
import mask_cases as mc
from abi_mirror import check_layout
from batch_entry_cases import good_interintra_blend_desc as good_blend_desc, good_mask_search_desc as good_search_desc, good_masked_pred_desc as good_pred_desc
from svt_av1_psyex_amd import abi, api, mask

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.GOLDEN)


def test_the_library_tables_have_the_reference_crcs(golden):
    prim, flip = mask.wedge_tables()
    assert mc.crc8(prim) == golden["primaries_crc"][0] and mc.crc8(flip) == golden["signflip_crc"][0]
    assert np.array_equal(prim, mc.primaries()) and np.array_equal(flip, mc.signflip())
    assert mc.crc8(mc.contiguous_masks()) == golden["contiguous_crc"][0]
    assert mask.WEDGE_SIZES == mc.WEDGE_SIZES and len(mc.DIFFWTD_SIZES) == 17
    assert np.array_equal(prim[1], 64 - prim[0])  # what lets a search form the other sign's mask in registers


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", ["wedge", "diffwtd", "variants", "geometry", "fromarray"])
def test_prediction_restatement_equals_the_reference_on_every_job(golden, group, bd):
    names = [n for n in mc.pred_batch_names() if n.startswith(group) and mc.pred_batch(n)["bit_depth"] == bd]
    assert names
    for name in names:
        b = mc.pred_batch(name)
        blocks, defined, masks, events = mc.pred_restated(name)
        assert all(defined) and all(e["inside"] for e in events), name
        assert np.array_equal(np.array([ip.crc(x) for x in blocks], np.uint32), golden[f"crc_{name}"]), name
        if b["plane"] == 0:
            dw = [j for j in b["jobs"] if j["comp_type"] == mc.DIFFWTD]
            crcs = [mc.crc8(masks[int(j["mask_offset"]):int(j["mask_offset"]) + int(j["luma_width"]) * int(j["luma_height"])]) for j in dw]
            assert (f"maskcrc_{name}" in golden.files) == bool(dw)
            if dw:
                assert np.array_equal(np.array(crcs, np.uint32), golden[f"maskcrc_{name}"]), name


def test_sample_blocks_equal_the_reference_sample_by_sample(golden):
    for key, name, i in mc.pred_sample_jobs():
        assert np.array_equal(mc.pred_restated(name)[0][i], golden[key]), key


def test_the_prediction_cases_are_what_the_issue_lists():
    for bd in (8, 10):
        for w, h in mc.WEDGE_SIZES:
            for sx, sy in mc.SUBSAMPLINGS:
                b = mc.pred_batch(f"wedge_{w}x{h}_{bd}_ss{sx}{sy}")
                assert {(int(j["wedge_index"]), int(j["wedge_sign"])) for j in b["jobs"]} == {(k, s) for k in range(16) for s in (0, 1)}
                assert (b["plane"] == 0) == ((sx, sy) == (0, 0)) and {(int(j["pred"]["width"]), int(j["pred"]["height"])) for j in b["jobs"]} == {(w >> sx, h >> sy)}
        for w, h in mc.DIFFWTD_SIZES:
            luma, chroma = mc.pred_batch(f"diffwtd_{w}x{h}_{bd}_ss00"), mc.pred_batch(f"diffwtd_{w}x{h}_{bd}_ss11")
            assert {int(j["mask_type"]) for j in luma["jobs"]} == {0, 1} and chroma["mask_from"] == luma["name"] and chroma["plane"] != 0
            assert np.array_equal(luma["jobs"]["mask_offset"], chroma["jobs"]["mask_offset"])
        v = mc.pred_batch(f"variants_{bd}")
        ev = mc.pred_restated(v["name"])[3]
        for size in ((8, 8), (32, 16)):
            got = {tuple(e["variants"]) for j, e in zip(v["jobs"], ev) if (int(j["luma_width"]), int(j["luma_height"])) == size}
            assert got == {(a, b) for a in range(4) for b in range(4)}
        for stride in (203, 204):
            g = mc.pred_batch(f"geometry_{bd}_stride{stride}")
            assert {int(j["pred"]["dst_offset"]) % stride % 8 for j in g["jobs"]} == set(range(8))
    # both ends of the output range are reached: the clip runs
    ev = [e for n in mc.pred_batch_names() for e in mc.pred_restated(n)[3]]
    assert any(e["clip_lo"] for e in ev) and any(e["clip_hi"] for e in ev)


@pytest.mark.parametrize("name", mc.blend_batch_names())
def test_blend_restatement_equals_the_reference_on_every_job(golden, name):
    b = mc.blend_by_name(name)
    assert len(b["jobs"]) == 7 * 20 and all(mc.blend_job_defined(b, j, None) for j in b["jobs"])
    assert np.array_equal(np.array([ip.crc(x) for x in mc.blend_restated(name)], np.uint32), golden[f"crc_{name}"])
    assert b["intra"].shape[1] != b["inter"].shape[1] and {int(o) & 1 for o in b["jobs"]["inter_offset"]} == {0, 1}


@pytest.mark.parametrize("name", sorted(mc.search_batches()))
def test_search_restatement_equals_the_reference_on_every_job(golden, name):
    sb = mc.search_batches()[name]
    assert all(mc.search_job_defined(sb.planes, j) for j in sb.jobs)
    assert np.array_equal(mc.reference_outputs(sb, mc.search_restated(name)[0]), golden[f"search_{name}"]), name


def test_the_fixture_holds_every_batch_and_nothing_else(golden):
    keys = {"primaries_crc", "signflip_crc", "contiguous_crc"} | {f"crc_{n}" for n in mc.pred_batch_names()} | {k for k, _, _ in mc.pred_sample_jobs()}
    keys |= {f"crc_{n}" for n in mc.blend_batch_names()} | {f"search_{n}" for n in mc.search_batches()}
    keys |= {f"maskcrc_{n}" for n in mc.pred_batch_names() if mc.pred_batch(n)["plane"] == 0 and (mc.pred_batch(n)["jobs"]["comp_type"] == mc.DIFFWTD).any()}
    assert set(golden.files) == keys


def test_the_planted_search_inputs_meet_their_conditions():
    """the issue's recipes, on the restatement (the generator asserts them on the reference's results, which the restatement equals job by job)"""
    for r in mc.RANGES:
        sb, planted = mc.planted_wedge_batch(r)
        res, ev = mc.search_restated(sb.name)
        won = sum((int(a["wedge_index"]), int(a["wedge_sign"])) == p for a, p in zip(res, planted))
        assert len(planted) == 288 == len({(int(j["width"]), int(j["height"]), p) for j, p in zip(sb.jobs, planted)})
        if r != "full10":
            assert won == 288, r  # every (size, index, sign) wins its job
        clamp, sat = sum(e["clamp"] for e in ev), sum(e["ds_saturated"] for e in ev)
        assert {"full8": clamp == 0 and sat >= 280, "mid8": sat == 0 and clamp == 0, "full10": clamp == 288, "mid10": clamp == 0}[r], (r, clamp, sat)
    for bd in (8, 10):
        sb, planted = mc.planted_seg_batch(bd)
        res, _ = mc.search_restated(sb.name)
        assert [int(v) for v in res["mask_type"][:-1]] == planted and len(planted) == 34
        j, mx = sb.jobs[-1], (1 << bd) - 1  # the issue's job of the largest sums: 128 x 128, src = p0 = 0, p1 = max: m = 53, t = -11 max on every sample
        assert (int(j["width"]), int(j["height"])) == (128, 128) and int(res["best_rd"][-1]) == (16384 * (11 * mx) ** 2 + 2048) >> 12
        res, _ = mc.search_restated(f"ties_{bd}")
        for k in range(3):
            assert (res[3 * k]["wedge_index"], res[3 * k]["wedge_sign"], res[3 * k + 1]["mask_type"], res[3 * k + 2]["interintra_mode"]) == (0, 0, 0, 0)
        sb, info = mc.ii_batch(bd)
        res, _ = mc.search_restated(sb.name)
        for a, (what, v, wm) in zip(res, info):
            if what == "mode":
                assert a["interintra_mode"] == v and (a["wedge_index"] >= 0) == (wm != 0) and (wm != 1 or a["use_wedge_interintra"] == 1)
                assert (a["rd_wedge"] == mc.NO_RD) == (wm == 0) and (wm != 0 or a["use_wedge_interintra"] == 0)
            elif what == "wedge":
                assert a["use_wedge_interintra"] == 1 and a["wedge_index"] == v and a["rd_wedge"] < a["best_rd"]
            else:
                assert a["use_wedge_interintra"] == 0 and a["rd_wedge"] == a["best_rd"] == 0
        assert {w for _, _, w in info} == {0, 1, 2} and {i[0] for i in info} == {"mode", "wedge", "equal"}
        for mult in (0, 1, 4):
            sb, want = mc.gate_batch(bd, mult)
            res, ev = mc.search_restated(sb.name)
            assert [bool(v) for v in res["exit"]] == want and (mult == 0) == (not any(want))
            for j, e, less in zip(sb.jobs, ev, want):
                assert e["sad"] == int(j["width"]) * int(j["height"]) * mult - less


def test_struct_layouts_match_the_library():
    check_layout("svt_hip_masked_pred_layout", (abi.MaskedPredDesc, abi.MaskedPredJob, abi.MaskSearchResult), multiple_of_8=True)
    check_layout("svt_hip_interintra_blend_layout", (abi.InterIntraDesc, abi.InterIntraJob), multiple_of_8=True)
    check_layout("svt_hip_mask_search_layout", (abi.MaskSearchDesc, abi.MaskSearchJob), multiple_of_8=True)
    for dtype, t, mine in ((abi.MASKED_PRED_JOB_DTYPE, abi.MaskedPredJob, mc.PRED_JOB_DTYPE), (abi.INTERINTRA_JOB_DTYPE, abi.InterIntraJob, mc.BLEND_JOB_DTYPE),
                           (abi.MASK_SEARCH_JOB_DTYPE, abi.MaskSearchJob, mc.SEARCH_JOB_DTYPE), (abi.MASK_SEARCH_RESULT_DTYPE, abi.MaskSearchResult, mc.RESULT_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(t) and dtype == mine
        for name, *_ in t._fields_:
            assert dt.fields[name][1] == getattr(t, name).offset, name
    assert (abi.MASK_WEDGE, abi.MASK_DIFFWTD, abi.MASK_PARAMS_FROM_ARRAY, abi.MASK_OK, abi.MASK_UNDEFINED) == (mc.WEDGE, mc.DIFFWTD, mc.PARAMS_FROM_ARRAY, mc.ST_OK,
                                                                                                             mc.ST_UNDEFINED)
    assert (abi.MASK_SEARCH_WEDGE, abi.MASK_SEARCH_DIFFWTD, abi.MASK_SEARCH_INTERINTRA, abi.MASK_NO_RD) == (mc.KIND_WEDGE, mc.KIND_DIFFWTD, mc.KIND_INTERINTRA, mc.NO_RD)


P = 0x1000  # never dereferenced: the validation reads the descriptor alone


def test_check_desc_accepts_good_descriptors():
    mask.check_pred_desc(good_pred_desc())
    mask.check_pred_desc(good_pred_desc(0))
    d = good_pred_desc(2)
    d.ss_x, d.ss_y, d.mask_buf, d.mask_bytes, d.results, d.n_results = 0, 0, None, 0, P, 5  # 4:4:4 chroma; wedge jobs need no mask buffer
    mask.check_pred_desc(d)
    mask.check_blend_desc(good_blend_desc())
    mask.check_search_desc(good_search_desc())
    d = good_search_desc()
    d.pred0, d.pred0_stride, d.pred0_samples, d.intra, d.pred0_to_pred1_mult = None, 0, 0, None, 0
    mask.check_search_desc(d)


PRED_BAD = ["no_dst", "no_jobs", "no_status", "bit_depth_12", "bit_depth_9", "ss_x_2", "ss_y_2", "n_refs_9", "n_refs_0", "null_plane", "zero_stride",
            "stride_below_width", "zero_width", "org_outside", "zero_dst_stride", "zero_dst_samples", "n_mvs_without_mv_array", "plane_3", "luma_with_ss",
            "n_results_without_results", "mask_bytes_without_mask_buf"]
BLEND_BAD = ["no_intra", "no_inter", "no_dst", "no_jobs", "no_status", "bit_depth_12", "bit_depth_0", "zero_inter_stride", "zero_dst_samples",
             "n_results_without_results"]
SEARCH_BAD = ["no_src", "no_pred1", "no_jobs", "no_results", "no_status", "bit_depth_12", "bit_depth_9", "use_rate", "use_rd_model", "zero_src_stride",
              "zero_pred1_samples", "pred0_zero_stride", "intra_zero_samples"]
CASES = [("svt_hip_masked_pred", good_pred_desc, mc.spoil_pred_desc, b) for b in PRED_BAD] + \
        [("svt_hip_interintra_blend", good_blend_desc, mc.spoil_blend_desc, b) for b in BLEND_BAD] + \
        [("svt_hip_mask_search", good_search_desc, mc.spoil_search_desc, b) for b in SEARCH_BAD]


@pytest.mark.parametrize("entry,good,spoil,bad", CASES, ids=[f"{c[0][8:]}-{c[3]}" for c in CASES])
def test_check_desc_and_batch_refuse_with_an_error_text(entry, good, spoil, bad):
    L = api.lib()
    d = spoil(good(), bad)
    assert getattr(L, entry + "_check_desc")(C.byref(d)) == BAD_PARAM
    text = L.svt_hip_last_error(None)
    assert (entry + "_check_desc").encode() in text
    if bad in ("use_rate", "use_rd_model"):
        assert b"stays on the host" in text
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    assert getattr(L, entry + "_batch")(ctx, C.byref(d)) == BAD_PARAM


@pytest.mark.parametrize("entry", ["svt_hip_masked_pred", "svt_hip_interintra_blend", "svt_hip_mask_search"])
def test_null_descriptor_and_null_context_are_refused(entry):
    L = api.lib()
    assert getattr(L, entry + "_check_desc")(None) == BAD_PARAM
    assert getattr(L, entry + "_batch")(None, None) == BAD_PARAM
    assert entry.encode() in L.svt_hip_last_error(None)


def test_job_defined_names_every_undefined_kind():
    for bd in (8, 10):
        b, bad, kinds = mc.undefined_pred_batch(bd)
        defined = mc.run_pred_restated(b)[1]
        assert [i for i, ok in enumerate(defined) if not ok] == bad and len(bad) == len(kinds) + 1 == 19
