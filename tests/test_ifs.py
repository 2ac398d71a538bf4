"""CPU: the restatement of tests/ifs_cases.py against golden/ifs.npz (the reference's own interpolation_filter_search, job by job), the model tables
and struct layouts of the library against their mirrors, every refusal of svt_hip_ifs_check_desc, and the conditions a fixture must meet to be
worth anything.  Nothing here needs a GPU: the library is only asked for host-side answers."""
import ctypes as C

import numpy as np
import pytest

import ifs_cases as ic
from abi_mirror import check_layout
from batch_entry_cases import good_ifs_desc as valid_desc
from svt_av1_psyex_amd import abi, api, ifs


@pytest.fixture(scope="module")
def golden():
    return np.load(ic.GOLDEN)


def test_the_fixture_holds_every_batch_and_nothing_else(golden):
    keys = {k for name in ic.batch_names() for k in ic.fixture_arrays(name, ic.restated(name))}
    assert set(golden.files) == keys


@pytest.mark.parametrize("name", ic.batch_names())
def test_restatement_equals_the_reference_on_every_output(golden, name):
    for key, mine in ic.fixture_arrays(name, ic.restated(name)).items():
        assert golden[key].dtype == mine.dtype and np.array_equal(golden[key], mine), (key, np.argwhere(golden[key] != mine)[:4].tolist())


def test_the_fixture_meets_its_conditions():
    """every pair wins (dual filter on), every equal pair wins (off), a tie of all nine costs picks pair 0, sse == 0, the MAX_XSQ_Q10 clamp, every
    bias flips a winner against the unbiased costs, every variant and a compound of two variants"""
    assert ic.coverage_missing() == []
    for name in ic.batch_names():
        b = ic.batch(name)
        for r in ic.restated(name):
            assert b["edge_planes"] or r["events"]["inside"]  # only the edge batches read past their planes


def test_skipped_pairs_and_the_first_minimum():
    for name in ("nodual_8", "exact_8"):
        for r in ic.restated(name):
            visited = r["rd"] != ic.SKIPPED
            assert visited.sum() == (3 if name.startswith("nodual") else 9) and np.array_equal(visited, r["sse"] != ic.SKIPPED)
            assert r["winner"] == int(np.argmin(np.where(visited, r["rd"], ic.SKIPPED))) and r["best_rd"] == int(r["rd"][r["winner"]])
            assert r["interp_filters"] == ic.FILTER_SETS[r["winner"]][0] | (ic.FILTER_SETS[r["winner"]][1] << 16)


def test_model_tables_equal_the_librarys():
    got = ifs.model_tables()
    assert got.shape == (3, abi.IFS_MODEL_ENTRIES) and np.array_equal(got, ic.MODEL_TABLES)
    L = api.lib()
    L.svt_hip_ifs_model_table.restype = C.c_void_p
    assert L.svt_hip_ifs_model_table(3) is None and L.svt_hip_ifs_model_table(-1) is None


STRUCTS = [abi.IfsDesc, abi.IfsJob, abi.IfsResult, abi.IfsPatch, abi.IfsScatterDesc]


@pytest.mark.parametrize("what,struct", enumerate(STRUCTS))
def test_struct_layouts_equal_the_librarys(what, struct):
    check_layout("svt_hip_ifs_layout", STRUCTS, only=(what,))


def test_record_dtypes_equal_the_structs():
    for dtype, struct in ((abi.IFS_JOB_DTYPE, abi.IfsJob), (abi.IFS_RESULT_DTYPE, abi.IfsResult), (abi.IFS_PATCH_DTYPE, abi.IfsPatch)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(struct)
        for name, *_ in struct._fields_:
            assert dt.fields[name][1] == getattr(struct, name).offset, name
    assert np.dtype(ic.JOB_DTYPE) == np.dtype(abi.IFS_JOB_DTYPE) and np.dtype(ic.RESULT_DTYPE) == np.dtype(abi.IFS_RESULT_DTYPE)


def test_check_desc_accepts_and_refuses():
    ifs.check_desc(valid_desc())
    d = valid_desc()
    d.dst, d.dst_stride, d.dst_samples, d.rd, d.sse, d.mv_array, d.n_mvs = None, 0, 0, None, None, None, 0  # everything optional left out
    ifs.check_desc(d)
    for bad in ic.SPOILS:
        with pytest.raises(api.SvtHipError):
            ifs.check_desc(ic.spoil_desc(valid_desc(), bad))
    assert api.lib().svt_hip_ifs_check_desc(None) == 2
