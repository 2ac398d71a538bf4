"""CPU: the restatement of tests/palette_cases.py against golden/palette.npz (the reference's own search_palette_luma, palette rate and palette
prediction, job by job), the struct layouts of the library against their mirrors, every refusal of svt_hip_palette_check_desc and
svt_hip_palette_pred_check_desc, and the conditions a fixture must meet to be worth anything.  Nothing here needs a GPU: the library is only asked
for host-side answers."""
import ctypes as C

import numpy as np
import pytest

import palette_cases as pc
from abi_mirror import check_layout
from batch_entry_cases import good_palette_desc as valid_desc, good_palette_pred_desc as valid_pred_desc
from svt_av1_psyex_amd import abi, api, palette


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN)


def test_the_fixture_holds_every_batch_and_nothing_else(golden):
    keys = {k for name in pc.batch_names() for k in pc.fixture_arrays(name, pc.restated(name))}
    assert set(golden.files) == keys


@pytest.mark.parametrize("name", pc.batch_names())
def test_restatement_equals_the_reference_on_every_output(golden, name):
    for key, mine in pc.fixture_arrays(name, pc.restated(name)).items():
        assert golden[key].dtype == mine.dtype and np.array_equal(golden[key], mine), (key, np.argwhere(golden[key] != mine)[:4].tolist())


def test_the_fixture_meets_its_conditions(golden):
    """every allowed size at both depths; 1, 2, 3, 8, 9, 64, 65 and far more colours; a 10-bit sample >= 1024; an empty k-means cluster; a snap
    that changes a centroid; a de-duplication that lowers the size, and one that drops the candidate; dominant and k-means palettes of one n that
    differ; equal counts among the top colours; a sample equidistant from two centroids; n_cache 0, in between and 16 with colours found and not
    found; step 1 and 2; cost precision 0 and 1; rows, columns and both cropped; values 0 and 255 / 1023; data[0] == 0; 8-bit planes of a
    10-bit encode with cache colours above 255, and a centroid at the maximum drawn to maximum + 1 at both depths; the k-means restore never
    fires; the most candidates kept is what the fixture records"""
    assert pc.coverage_missing() == []
    assert sorted(pc.SIZES) == sorted(set(pc.SIZES)) and len(pc.SIZES) == 16
    most = max(int(golden[f"{name}_max_cands"][0]) for name in pc.batch_names())
    assert most == pc.max_cands() == 12 <= pc.MAX_CANDS  # sizes 8..3, twice
    for name in pc.batch_names():
        assert int(golden[f"{name}_n_cands"].max()) == int(golden[f"{name}_max_cands"][0])


def test_candidates_are_compacted_sorted_and_consistent():
    for name in pc.batch_names():
        b = pc.batch(name)
        for j, r in zip(b["jobs"], pc.restated(name)):
            assert (r["n_cands"] == 0) or 2 < r["n_colors"] <= 64
            for c in r["cands"]:
                assert 3 <= c["size"] <= 8 and c["colors"] == sorted(set(c["colors"])) and c["first_index"] == c["map"][0, 0]
                assert c["rate"] == int(b["tables"]["ymode"][j["bsize_ctx"]][j["mode_ctx"]][1]) + sum(c[k] for k in pc.COSTS[:4])
                assert (c["map_cost"] == 0) == bool(b["params"]["reduce_palette_cost_precision"])
                assert c["map"].shape == (j["height"], j["width"]) and int(c["map"].max()) < c["size"]
                rows, cols = int(j["rows"]), int(j["cols"])
                assert np.all(c["map"][rows:] == c["map"][rows - 1]) and np.all(c["map"][:, cols:] == c["map"][:, cols - 1:cols])  # the extension


def test_palette_cache_merge():
    assert pc.palette_cache(None, None) == [] and pc.palette_cache([], [3]) == [3]
    assert pc.palette_cache([1, 5, 9], [2, 5, 7, 9, 30]) == [1, 2, 5, 7, 9, 30]
    assert len(pc.palette_cache(list(range(0, 16, 2)), list(range(1, 16, 2)))) == 16


STRUCTS = [abi.PaletteDesc, abi.PaletteJob, abi.PaletteCand, abi.PaletteResult, abi.PalettePredJob, abi.PalettePredDesc]


@pytest.mark.parametrize("what,struct", enumerate(STRUCTS))
def test_struct_layouts_equal_the_librarys(what, struct):
    check_layout("svt_hip_palette_layout", STRUCTS, only=(what,))


def test_record_dtypes_equal_the_structs():
    for dtype, struct in ((abi.PALETTE_JOB_DTYPE, abi.PaletteJob), (abi.PALETTE_CAND_DTYPE, abi.PaletteCand), (abi.PALETTE_RESULT_DTYPE, abi.PaletteResult),
                          (abi.PALETTE_PRED_JOB_DTYPE, abi.PalettePredJob)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(struct)
        for name, *_ in struct._fields_:
            assert dt.fields[name][1] == getattr(struct, name).offset, name
    assert np.dtype(pc.JOB_DTYPE) == np.dtype(abi.PALETTE_JOB_DTYPE) and np.dtype(pc.RESULT_DTYPE) == np.dtype(abi.PALETTE_RESULT_DTYPE)
    assert np.dtype(pc.PRED_JOB_DTYPE) == np.dtype(abi.PALETTE_PRED_JOB_DTYPE) and np.dtype(pc.CAND_DTYPE) == np.dtype(abi.PALETTE_CAND_DTYPE)
    assert (abi.PALETTE_MAX_CANDS, abi.PALETTE_MAX_SIZE, abi.PALETTE_MAX_CACHE) == (pc.MAX_CANDS, pc.MAX_SIZE, pc.MAX_CACHE)


def test_check_desc_accepts_and_refuses():
    palette.check_desc(valid_desc())
    d = valid_desc()
    d.color_maps, d.map_bytes, d.n_jobs = None, 0, 0  # the optional output left out
    palette.check_desc(d)
    for bad in pc.SPOILS:
        with pytest.raises(api.SvtHipError):
            palette.check_desc(pc.spoil_desc(valid_desc(), bad))
    assert api.lib().svt_hip_palette_check_desc(None) == 2


def test_pred_check_desc_accepts_and_refuses():
    palette.check_pred_desc(valid_pred_desc())
    d = valid_pred_desc()
    d.color_map, d.map_bytes = None, 0
    palette.check_pred_desc(d)
    for bad in pc.PRED_SPOILS:
        with pytest.raises(api.SvtHipError):
            palette.check_pred_desc(pc.spoil_pred_desc(valid_pred_desc(), bad))
    assert api.lib().svt_hip_palette_pred_check_desc(None) == 2
