"""What every asynchronous batch entry does before it enqueues anything (csrc/batch_host.h owns the sequence): null arguments and a refused descriptor
come back as BAD_PARAM with the entry's name in the text, and an empty batch returns OK without touching the context.  The prediction families first, then
the older entries, whose checks each keep their own order against an empty batch, then the two full-pel prediction entries that take arguments.  No GPU."""
import ctypes as C

import pytest

from batch_entry_cases import BIT_DEPTH_THEN_EMPTY, CHECK_FIRST, EMPTY_FIRST, ENTRIES, OLDER, P
from svt_av1_psyex_amd import abi, api

OK, BAD_PARAM = 0, 2
IDS = [e[0] for e in ENTRIES]
OLDER_IDS = [e[0] for e in OLDER]


def stand_in_context():
    return C.create_string_buffer(4096)  # not a context: an entry that read its device, mutex or stream would not return normally


def test_every_batch_entry_of_the_eight_families_is_listed():
    assert len(ENTRIES) == len(set(IDS)) == 18
    assert all(hasattr(api.lib(), name) for name in IDS)


@pytest.mark.parametrize("entry,good,count", ENTRIES, ids=IDS)
def test_null_arguments_are_refused_in_the_entrys_own_name(entry, good, count):
    L = api.lib()
    f = getattr(L, entry)
    for ctx, d in ((None, None), (stand_in_context(), None), (None, C.byref(good()))):
        L.svt_hip_inter_pred_check_desc(None)  # leaves another entry's text behind
        assert f(ctx, d) == BAD_PARAM
        assert entry.encode() in L.svt_hip_last_error(None)


@pytest.mark.parametrize("entry,good,count", ENTRIES, ids=IDS)
def test_an_empty_batch_returns_ok_before_the_context_is_touched(entry, good, count):
    d = good()
    assert getattr(d, count) != 0
    setattr(d, count, 0)
    assert getattr(api.lib(), entry)(stand_in_context(), C.byref(d)) == OK


@pytest.mark.parametrize("entry,good,count", ENTRIES, ids=IDS)
def test_a_spoiled_descriptor_is_refused_before_the_context_is_touched(entry, good, count):
    L = api.lib()
    d = good()
    d.status = None  # mandatory in every descriptor
    assert getattr(L, entry)(stand_in_context(), C.byref(d)) == BAD_PARAM
    assert b"svt_hip_" in L.svt_hip_last_error(None) and b"null" in L.svt_hip_last_error(None)
    setattr(d, count, 0)  # the check comes before the early return
    assert getattr(L, entry)(stand_in_context(), C.byref(d)) == BAD_PARAM


# ---- the older entries: RD, the transforms alone, the MD searches, PME, statistics, SSIM, rate, RDOQ ----
def emptied(d, counts):
    for c in counts:
        assert getattr(d, c) != 0
        setattr(d, c, 0)
    return d


def test_every_older_entry_is_listed():
    assert len(OLDER) == len(set(OLDER_IDS)) == 10 and not set(OLDER_IDS) & set(IDS)
    assert all(hasattr(api.lib(), name) for name in OLDER_IDS)
    assert [e[4] for e in OLDER] == [EMPTY_FIRST] * 7 + [BIT_DEPTH_THEN_EMPTY] + [CHECK_FIRST] * 2


@pytest.mark.parametrize("entry,good,counts,pointer,order", OLDER, ids=OLDER_IDS)
def test_an_older_entry_refuses_null_arguments_in_its_own_name(entry, good, counts, pointer, order):
    L = api.lib()
    f = getattr(L, entry)
    for ctx, d in ((None, None), (stand_in_context(), None), (None, C.byref(good()))):
        L.svt_hip_inter_pred_check_desc(None)  # leaves another entry's text behind
        assert f(ctx, d) == BAD_PARAM
        assert entry.encode() in L.svt_hip_last_error(None)


@pytest.mark.parametrize("entry,good,counts,pointer,order", OLDER, ids=OLDER_IDS)
def test_an_older_entry_returns_ok_for_an_empty_batch_before_the_context_is_touched(entry, good, counts, pointer, order):
    f = getattr(api.lib(), entry)
    assert f(stand_in_context(), C.byref(emptied(good(), counts))) == OK
    for zero, other in ((counts, counts[::-1]) if len(counts) == 2 else ()):  # one zero count of two is not "nothing to do": the other's array is asked for
        d = good()
        setattr(d, zero, 0)
        setattr(d, {"n_jobs": "jobs", "n_pyramids": "pyramids", "n_groups": "group_start"}[other], None)
        assert f(stand_in_context(), C.byref(d)) == BAD_PARAM


@pytest.mark.parametrize("entry,good,counts,pointer,order", OLDER, ids=OLDER_IDS)
def test_an_older_entry_refuses_a_spoiled_descriptor_before_the_context_is_touched(entry, good, counts, pointer, order):
    L = api.lib()
    d = good()
    assert getattr(d, pointer)
    setattr(d, pointer, None)
    assert getattr(L, entry)(stand_in_context(), C.byref(d)) == BAD_PARAM
    assert b"null" in L.svt_hip_last_error(None)


@pytest.mark.parametrize("entry,good,counts,pointer,order", OLDER, ids=OLDER_IDS)
def test_an_older_entry_keeps_its_order_of_check_and_empty(entry, good, counts, pointer, order):
    f = getattr(api.lib(), entry)
    d = emptied(good(), counts)
    setattr(d, pointer, None)
    assert f(stand_in_context(), C.byref(d)) == (BAD_PARAM if order == CHECK_FIRST else OK)
    if hasattr(d, "bit_depth"):
        d.bit_depth = 9
        assert f(stand_in_context(), C.byref(d)) == (OK if order == EMPTY_FIRST else BAD_PARAM)


# ---- the two full-pel prediction entries: an argument list, no descriptor ----
def fullpel_pred(ctx, ref=P, width=128, height=128, bit_depth=8, mv=P, lst=0, ref_idx=0, row_start=0, pred=P):
    return api.lib().svt_hip_fullpel_pred(ctx, C.c_void_p(ref), 128, width, height, bit_depth, C.c_void_p(mv), lst, ref_idx, row_start, 0, C.c_void_p(pred), 128)


def fullpel_pred_batch(ctx, jobs, n_jobs=None, width=128, height=128, bit_depth=8):
    arr = (abi.PredJob * max(len(jobs), 1))(*jobs)
    return api.lib().svt_hip_fullpel_pred_batch(ctx, 128, width, height, bit_depth, 128, len(jobs) if n_jobs is None else n_jobs, arr)


def good_pred_job(**over):
    return abi.PredJob(**{**dict(ref=P, sb_best_mv=P, pred=P, b64_row_start=0, b64_row_count=0, list=0, ref_idx=0), **over})


def test_fullpel_pred_refuses_a_null_context_and_bad_arguments_before_the_context_is_touched():
    L = api.lib()
    assert fullpel_pred(None) == BAD_PARAM
    for bad in (dict(ref=None), dict(mv=None), dict(pred=None), dict(lst=2), dict(ref_idx=4), dict(bit_depth=9), dict(width=0), dict(height=0), dict(row_start=2)):
        L.svt_hip_inter_pred_check_desc(None)
        assert fullpel_pred(stand_in_context(), **bad) == BAD_PARAM, bad
        assert b"svt_hip_fullpel_pred:" in L.svt_hip_last_error(None)


def test_fullpel_pred_batch_refuses_a_null_context_no_jobs_and_bad_arguments_before_the_context_is_touched():
    L = api.lib()
    assert fullpel_pred_batch(None, [good_pred_job()]) == BAD_PARAM
    calls = [dict(jobs=[good_pred_job()], n_jobs=0), dict(jobs=[good_pred_job()], n_jobs=17), dict(jobs=[good_pred_job()], bit_depth=12),
             dict(jobs=[good_pred_job()], width=0)]
    calls += [dict(jobs=[good_pred_job(), good_pred_job(**bad)])
              for bad in (dict(ref=None), dict(sb_best_mv=None), dict(pred=None), dict(list=2), dict(ref_idx=4), dict(b64_row_start=2))]
    for call in calls:
        L.svt_hip_inter_pred_check_desc(None)
        assert fullpel_pred_batch(stand_in_context(), **call) == BAD_PARAM, call
        assert b"svt_hip_fullpel_pred_batch:" in L.svt_hip_last_error(None)
    assert L.svt_hip_fullpel_pred_batch(stand_in_context(), 128, 128, 128, 8, 128, 1, None) == BAD_PARAM
