"""CPU: the restatement of the OBMC entries (tests/obmc_cases.py) against the reference's own results (golden/obmc.npz), the library's mask rows
against the fixture's CRC, the conditions of the case list recomputed from the restatement, the struct lay-outs of abi.py against the library's, and
the three check_desc functions (validation needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import inter_pred_cases as ip
import obmc_cases as oc
from abi_mirror import check_layout
from batch_entry_cases import good_obmc_blend_desc as good_blend_desc, good_obmc_neighbour_desc as good_neighbour_desc, good_obmc_target_desc as good_target_desc
from svt_av1_psyex_amd import abi, api, obmc

BAD_PARAM = 2


@pytest.fixture(scope="module")
def golden():
    return np.load(oc.GOLDEN)


def test_the_library_mask_rows_have_the_reference_crc(golden):
    rows = obmc.masks()
    assert oc.crc(rows, "u1") == golden["masks_crc"][0] and np.array_equal(rows, oc.MASKS)
    for n in (1, 2, 4, 8, 16, 32):  # every row ends at the full weight and rises to it
        assert rows[2 * n - 1] == 64 and np.all(np.diff(rows[n:2 * n].astype(int)) >= 0)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("group", ["sizes", "phases", "clamp", "plane_edge", "extremes"])
def test_restatement_equals_the_reference_on_every_block(golden, group, bd):
    names = [n for n in oc.batch_names() if n.startswith(group) and oc.batch(n)["bit_depth"] == bd]
    assert names
    for name in names:
        want = oc.restated(name)
        assert all(e["inside"] for evs in want["events"].values() for _, e in evs), name
        mine = oc.fixture_arrays(name, want)
        assert set(mine) == {k for k in golden.files if k.endswith("_" + name) and not k.startswith(("sample", "search"))}, name
        for k, v in mine.items():
            assert v.dtype == golden[k].dtype and np.array_equal(v, golden[k]), k


def test_sample_blocks_equal_the_reference_value_by_value(golden):
    keys = oc.sample_blocks()
    assert len(keys) == 2 * len(oc.SIZES) == 28
    for key, name, i in keys:
        assert np.array_equal(oc.sample_arrays(name, i, oc.restated(name)), golden[key]), key


def test_the_fixture_holds_every_batch_and_nothing_else(golden):
    keys = {"masks_crc"} | {k for k, _, _ in oc.sample_blocks()}
    for n in oc.batch_names():
        keys |= {f"{k}_{n}" for k in ("above", "left", "blend")} | ({f"wsrc_{n}", f"mask_{n}"} if 0 in oc.batch(n)["run_planes"] else set())
    import obmc_search_cases as sc
    keys |= {f"{k}_{n}" for n in sc.batches() for k in ("search", "searchmv")}
    assert set(golden.files) == keys


def test_the_cases_are_what_the_issue_lists():
    assert oc.coverage_missing() == []
    assert len(oc.SIZES) == 14 and all(min(s) >= 8 and max(s) <= 64 and s in ip.BLOCK_SIZES for s in oc.SIZES)
    assert {s for s in ip.BLOCK_SIZES if min(s) >= 8 and max(s) <= 64} == set(oc.SIZES)
    cap = {8: 1, 16: 2, 32: 3, 64: 4}  # max_neighbor_obmc
    for bd in (8, 10):
        for w, h in oc.SIZES:
            b = oc.batch(f"sizes_{w}x{h}_{bd}")
            spans = lambda blk, side: tuple((int(r["rel_pos"]), int(r["size"])) for r in blk[side][:int(blk["n_above" if side == "above" else "n_left"])])
            above, left = {spans(x, "above") for x in b["blocks"]}, {spans(x, "left") for x in b["blocks"]}
            for got, n4 in ((above, w >> 2), (left, h >> 2)):
                assert {(), ((0, n4),)} <= got and max(len(s) for s in got) == cap[n4 * 4]  # none, one over the whole side, as many as the cap allows
                if n4 >= 8:  # a gap in the middle, at the start, at the end, at both ends
                    q = n4 // 4
                    assert {((0, q), (3 * q, q)), ((n4 // 2, n4 // 2),), ((0, n4 // 2),), ((q, q), (2 * q, q))} <= got
                if n4 == 16:
                    assert tuple((4 * k, 4) for k in range(4)) in got  # four of a quarter each
            assert any(x["n_above"] and not x["n_left"] for x in b["blocks"]) and any(x["n_left"] and not x["n_above"] for x in b["blocks"])
            assert {int(r["ref"]) for x in b["blocks"] for r in list(x["above"][:int(x["n_above"])]) + list(x["left"][:int(x["n_left"])])} == {0, 1}
        # the chroma of 8x8 / 8x16 / 16x8 has no above strips and keeps its left ones; 64x16 / 16x64 give 64x8 / 8x64 and 32x4 / 4x32 strips
        for (w, h), skipped in (((8, 8), True), ((8, 16), True), ((16, 8), True), ((16, 16), False)):
            blk = next(x for x in oc.batch(f"sizes_{w}x{h}_{bd}")["blocks"] if x["n_above"] and x["n_left"])
            dirs = [d for d, _, _, _ in oc.strip_jobs(blk, 1)]
            assert (0 not in dirs) == skipped and 1 in dirs and 0 in [d for d, _, _, _ in oc.strip_jobs(blk, 0)]
        for (w, h), luma, chroma in (((64, 16), (64, 8), (32, 4)), ((16, 64), (8, 64), (4, 32))):
            blk = next(x for x in oc.batch(f"sizes_{w}x{h}_{bd}")["blocks"] if x["n_above"] == 1 and x["n_left"] == 1)
            d = 0 if w == 64 else 1
            for plane, want in ((0, luma), (1, chroma)):
                j = next(j for dd, j, _, _ in oc.strip_jobs(blk, plane) if dd == d)
                assert (int(j["width"]), int(j["height"])) == want
        assert sum(int(r["flags"]) for x in oc.batch(f"clamp_{bd}")["blocks"] for r in list(x["above"]) + list(x["left"])) >= 4  # MVs from mv_array
        # the extremes of wsrc: a source of 255 under strips of 0, a source of 0 under strips of 255 (the largest weight a strip gets is 4096 - 33 * 33)
        hi = oc.restated(f"extremes_{bd}_zero_max")["wsrc"]
        lo = oc.restated(f"extremes_{bd}_max_zero")["wsrc"]
        assert hi.max() == 255 * 4096 and lo[lo != oc.fill_i32(1)[0]].min() == -255 * (4096 - 33 * 33)


def test_struct_layouts_match_the_library():
    structs = (abi.ObmcNeighbourDesc, abi.ObmcBlendDesc, abi.ObmcTargetDesc, abi.ObmcBlock, abi.ObmcNeighbour, abi.ObmcJob, abi.ObmcSearchDesc, abi.ObmcSearchJob,
               abi.ObmcSearchResult)
    check_layout("svt_hip_obmc_layout", structs, only=range(6), multiple_of_8=True)  # 6 .. 8 are the search's (tests/test_obmc_search.py)
    for dtype, t, mine in ((abi.OBMC_BLOCK_DTYPE, abi.ObmcBlock, oc.BLOCK_DTYPE), (abi.OBMC_NEIGHBOUR_DTYPE, abi.ObmcNeighbour, oc.NB_DTYPE),
                           (abi.OBMC_JOB_DTYPE, abi.ObmcJob, oc.JOB_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(t) and np.dtype(mine) == dt
        for name, *_ in t._fields_:
            assert dt.fields[name][1] == getattr(t, name).offset, name
    assert (abi.OBMC_MAX_NEIGHBOURS, abi.OBMC_MV_FROM_ARRAY, abi.OBMC_OK, abi.OBMC_UNDEFINED) == (oc.MAX_NB, oc.MV_FROM_ARRAY, oc.ST_OK, oc.ST_UNDEFINED)


P = 0x1000  # never dereferenced: the validation reads the descriptor alone


def test_check_desc_accepts_good_descriptors():
    obmc.check_neighbour_desc(good_neighbour_desc())
    obmc.check_neighbour_desc(good_neighbour_desc(0))
    d = good_neighbour_desc(2)
    d.ss_x, d.ss_y, d.mv_array, d.n_mvs = 0, 0, P, 7  # 4:4:4 chroma
    obmc.check_neighbour_desc(d)
    obmc.check_blend_desc(good_blend_desc())
    obmc.check_blend_desc(good_blend_desc(0))
    obmc.check_target_desc(good_target_desc())
    d = good_target_desc()
    d.strip_bit_depth = 8
    obmc.check_target_desc(d)


NEIGHBOUR_BAD = ["no_blocks", "no_jobs", "no_above", "no_left", "no_status", "bit_depth_12", "bit_depth_9", "ss_x_2", "ss_y_2", "plane_3", "luma_with_ss", "n_refs_0",
                 "n_refs_9", "null_plane", "zero_ref_stride", "stride_below_width", "org_outside", "zero_n_blocks", "zero_strip_samples", "n_mvs_without_mv_array"]
BLEND_BAD = ["no_blocks", "no_jobs", "no_above", "no_left", "no_dst", "no_status", "bit_depth_12", "bit_depth_0", "ss_x_2", "ss_y_2", "plane_3", "luma_with_ss",
             "zero_n_blocks", "zero_strip_samples", "zero_dst_stride", "zero_dst_samples"]
TARGET_BAD = ["no_blocks", "no_jobs", "no_above", "no_left", "no_src", "no_wsrc", "no_mask", "no_status", "strip_bit_depth_12", "strip_bit_depth_9", "zero_n_blocks",
              "zero_strip_samples", "zero_src_stride", "zero_src_samples", "zero_out_values"]
CASES = [("svt_hip_obmc_neighbour", good_neighbour_desc, b) for b in NEIGHBOUR_BAD] + [("svt_hip_obmc_blend", good_blend_desc, b) for b in BLEND_BAD] + \
        [("svt_hip_obmc_target", good_target_desc, b) for b in TARGET_BAD]


@pytest.mark.parametrize("entry,good,bad", CASES, ids=[f"{c[0][13:]}-{c[2]}" for c in CASES])
def test_check_desc_and_batch_refuse_with_an_error_text(entry, good, bad):
    L = api.lib()
    d = oc.spoil_desc(good(), bad)
    assert getattr(L, entry + "_check_desc")(C.byref(d)) == BAD_PARAM
    assert (entry + "_check_desc").encode() in L.svt_hip_last_error(None)
    ctx = C.create_string_buffer(4096)  # a stand-in handle: validation comes first, and a rejected call enqueues nothing
    assert getattr(L, entry + "_batch")(ctx, C.byref(d)) == BAD_PARAM


@pytest.mark.parametrize("entry", ["svt_hip_obmc_neighbour", "svt_hip_obmc_blend", "svt_hip_obmc_target"])
def test_null_descriptor_and_null_context_are_refused(entry):
    L = api.lib()
    assert getattr(L, entry + "_check_desc")(None) == BAD_PARAM
    assert getattr(L, entry + "_batch")(None, None) == BAD_PARAM
    assert entry.encode() in L.svt_hip_last_error(None)


def test_job_defined_names_every_undefined_kind():
    for bd in (8, 10):
        b, bad = oc.undefined_batch(bd)
        assert list(bad) == oc.UNDEFINED_KINDS and len(b["blocks"]) == 3 * len(bad)
        jobs = oc.all_jobs(b)
        for plane in range(3):
            undefined = {i for i, j in enumerate(jobs) if not oc.neighbour_job_defined(b, j, plane)}
            assert undefined == {i for k, i in bad.items() if k != "strip_end" or plane == 2}, plane
            undefined = {i for i, j in enumerate(jobs) if not oc.blend_job_defined(b, j, plane, oc.PRED_STRIDE, 1 << 20)}
            assert undefined == {i for k, i in bad.items() if k not in oc.NEIGHBOUR_ONLY and (k != "strip_end" or plane == 2)}, plane
        undefined = {i for i, j in enumerate(jobs) if not oc.target_job_defined(b, j, (ip.PIC_H, ip.PIC_W), 1 << 20)}
        assert undefined == {i for k, i in bad.items() if k not in oc.NEIGHBOUR_ONLY and k != "strip_end"}
