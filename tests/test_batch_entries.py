"""What every asynchronous batch entry of the prediction families does before it enqueues anything (csrc/batch_host.h owns the sequence): null arguments
and a refused descriptor come back as BAD_PARAM with the entry's name in the text, and an empty batch returns OK without touching the context.  No GPU."""
import ctypes as C

import pytest

from batch_entry_cases import ENTRIES
from svt_av1_psyex_amd import api

OK, BAD_PARAM = 0, 2
IDS = [e[0] for e in ENTRIES]


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
