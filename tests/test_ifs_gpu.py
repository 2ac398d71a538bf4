"""GPU: svt_hip_ifs_batch and svt_hip_ifs_scatter_filters against the restatement of tests/ifs_cases.py (which golden/ifs.npz pins on the reference
job by job), bit for bit.  Every buffer a launch writes starts as the byte 0xA5 and is compared whole, so a byte outside a job's outputs must come
back untouched; the per-job refusals run in a batch that also holds valid jobs.  No tolerance: every output is an integer."""
import ctypes as C

import numpy as np
import pytest

import ifs_cases as ic
import inter_pred_cases as ip
from svt_av1_psyex_amd import abi, api, ifs

pytestmark = pytest.mark.gpu
FILL = 0xA5


def launch(ctx, b, with_dst=True, want_arrays=True, spare=3):
    return ifs.run_ifs_hip(ctx, b["bit_depth"], ic.batch_planes(b), b["src"], b["jobs"], b["fac_bits"], b["params"], dst_shape=b["dst_shape"] if with_dst else None,
                           dst_stride=b["dst_stride"], mv_array=b["mv_array"], spare_jobs=spare, fill=FILL, want_arrays=want_arrays)


def check(got, name, results, n, defined=None, with_dst=True):
    """every output of a launch against `results`; jobs that are not `defined` left every byte of theirs as it was"""
    defined = np.ones(n, bool) if defined is None else defined
    rec, rd, sse, img = ic.expected_outputs(name, results, FILL, with_dst)
    filled = np.frombuffer(bytes([FILL]) * np.dtype(ic.RESULT_DTYPE).itemsize, ic.RESULT_DTYPE)[0]
    assert np.array_equal(got["status"][:n], np.where(defined, ic.ST_OK, ic.ST_UNDEFINED)) and np.all(got["status"][n:] == FILL)
    for i in range(n):
        assert got["results"][i].tobytes() == (rec[i] if defined[i] else filled).tobytes(), (name, i)
    assert all(r.tobytes() == filled.tobytes() for r in got["results"][n:])
    for key, want in (("rd", rd), ("sse", sse)):
        if got[key] is not None:
            want = np.where(defined[:, None], want, np.uint64(0xA5A5A5A5A5A5A5A5))
            assert np.array_equal(got[key][:n], want), (name, key, np.argwhere(got[key][:n] != want)[:4].tolist())
            assert np.all(got[key][n:] == np.uint64(0xA5A5A5A5A5A5A5A5))
    if with_dst:
        assert np.array_equal(got["dst"], img), (name, np.argwhere(got["dst"] != img)[:4].tolist())  # the winners' samples and the bytes around them


@pytest.mark.parametrize("name", ic.batch_names())
def test_every_output_equals_the_restatement_bit_for_bit(hip_ctx, name):
    b = ic.batch(name)
    check(launch(hip_ctx, b), name, ic.restated(name), len(b["jobs"]))


@pytest.mark.parametrize("name", ["main_8", "nodual_10"])
def test_search_only_and_without_the_optional_arrays(hip_ctx, name):
    """dst == NULL: the same results; rd / sse null: the same results and samples"""
    b = ic.batch(name)
    check(launch(hip_ctx, b, with_dst=False), name, ic.restated(name), len(b["jobs"]), with_dst=False)
    check(launch(hip_ctx, b, want_arrays=False), name, ic.restated(name), len(b["jobs"]))


@pytest.mark.parametrize("bd", [8, 10])
def test_undefined_jobs_write_their_status_and_nothing_else(hip_ctx, bd):
    b, bad = ic.undefined_batch(bd)
    n = len(b["jobs"])
    planes = ic.batch_planes(b)
    samples = b["dst_shape"][0] * b["dst_stride"]
    defined = np.array([ic.job_defined(j, 2, b["mv_array"], samples, 256, samples, 256) for j in b["jobs"]])
    assert sorted(np.flatnonzero(~defined)) == bad
    dummy = ic.restated(f"main_{bd}")[0]
    results = [ic.restate_job(planes, b["src"], bd, j, b["params"], b["fac_bits"], b["mv_array"]) if ok else dummy for j, ok in zip(b["jobs"], defined)]
    got = launch(hip_ctx, b)
    rec, rd, sse, _ = ic.expected_outputs(f"main_{bd}", results, FILL, with_dst=False)
    filled = np.frombuffer(bytes([FILL]) * np.dtype(ic.RESULT_DTYPE).itemsize, ic.RESULT_DTYPE)[0]
    assert np.array_equal(got["status"][:n], np.where(defined, ic.ST_OK, ic.ST_UNDEFINED)) and np.all(got["status"][n:] == FILL)
    for i in range(n):
        assert got["results"][i].tobytes() == (rec[i] if defined[i] else filled).tobytes(), i
        assert np.array_equal(got["rd"][i], rd[i] if defined[i] else np.full(9, 0xA5A5A5A5A5A5A5A5, np.uint64)), i
        assert np.array_equal(got["sse"][i], sse[i] if defined[i] else np.full(9, 0xA5A5A5A5A5A5A5A5, np.uint64)), i
    img = ip.expected_image({"bit_depth": bd, "dst_shape": b["dst_shape"], "dst_stride": 256, "jobs": b["jobs"]["pred"]}, [r["pred"] for r in results], FILL, defined)
    assert np.array_equal(got["dst"], img)
    # dst == NULL: the destination is not checked, so the job past its end is defined
    defined2 = np.array([ic.job_defined(j, 2, b["mv_array"], samples, 256) for j in b["jobs"]])
    assert defined2.sum() == defined.sum() + 1
    got = launch(hip_ctx, b, with_dst=False)
    assert np.array_equal(got["status"][:n], np.where(defined2, ic.ST_OK, ic.ST_UNDEFINED))


def test_an_empty_batch_and_a_refused_descriptor_enqueue_nothing(hip_ctx):
    b = dict(ic.batch("smooth_8"))
    n = len(b["jobs"])
    b["jobs"] = b["jobs"][:0]
    got = launch(hip_ctx, b, spare=n)
    assert np.all(got["status"] == FILL) and np.all(got["dst"] == FILL) and np.all(got["rd"] == np.uint64(0xA5A5A5A5A5A5A5A5))
    assert np.all(got["results"].view(np.uint8) == FILL)
    b = dict(ic.batch("smooth_8"))
    b["params"] = dict(b["params"], quantizer=0)
    with pytest.raises(api.SvtHipError, match="quantizer"):
        launch(hip_ctx, b)


def test_scatter_patches_the_filters_of_both_record_kinds(hip_ctx):
    """the result's two bytes go to filter_x / filter_y of an SvtHipInterPredJob array and of an SvtHipMaskedPredJob array; a patch with an index out
    of range or a failed result leaves its record as it was and gets 0xFF"""
    rng = np.random.default_rng(41)
    results = np.zeros(7, abi.IFS_RESULT_DTYPE)
    results["filter_x"], results["filter_y"] = rng.integers(0, 3, 7), rng.integers(0, 3, 7)
    results["filter_x"][2], results["filter_y"][2] = 2, 1
    rstatus = np.zeros(7, np.uint8)
    rstatus[4] = ic.ST_UNDEFINED
    patches = np.array([(0, 0), (2, 1), (3, 5), (4, 2), (7, 3), (1, 6), (0xFFFFFFFF, 4), (5, 0xFFFFFFFF), (6, 4)], abi.IFS_PATCH_DTYPE)
    bad = np.array([0, 0, 0, 1, 1, 1, 1, 1, 0], bool)
    for dtype, off in ((abi.INTER_PRED_JOB_DTYPE, abi.InterPredJob.filter_x.offset), (abi.MASKED_PRED_JOB_DTYPE, abi.MaskedPredJob.pred.offset + abi.InterPredJob.filter_x.offset)):
        records = np.frombuffer(rng.integers(0, 256, 6 * np.dtype(dtype).itemsize).astype(np.uint8).tobytes(), dtype).copy()
        want = records.copy()
        for p, b in zip(patches, bad):
            if not b:
                rec = want[int(p["record_index"])]["pred"] if dtype is abi.MASKED_PRED_JOB_DTYPE else want[int(p["record_index"])]
                rec["filter_x"], rec["filter_y"] = results[int(p["result_index"])]["filter_x"], results[int(p["result_index"])]["filter_y"]
        got, status = ifs.run_scatter_hip(hip_ctx, patches, results, rstatus, records, off, fill=FILL)
        assert np.array_equal(status, np.where(bad, ic.ST_UNDEFINED, ic.ST_OK))
        assert got.tobytes() == want.tobytes()
        assert want.tobytes() != records.tobytes()
    # no patches: nothing runs; refusals
    got, status = ifs.run_scatter_hip(hip_ctx, patches[:0], results, rstatus, records, off, fill=FILL)
    assert got.tobytes() == records.tobytes() and len(status) == 0
    d = abi.IfsScatterDesc(n_patches=1, n_results=1, n_records=1, record_stride=8, filter_x_offset=7, patches=1, results=1, result_status=1, base=1, status=1)
    assert api.lib().svt_hip_ifs_scatter_filters(hip_ctx._h, C.byref(d)) == 2
    d.filter_x_offset, d.base = 0, None
    assert api.lib().svt_hip_ifs_scatter_filters(hip_ctx._h, C.byref(d)) == 2
