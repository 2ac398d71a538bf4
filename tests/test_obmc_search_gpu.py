"""GPU: svt_hip_obmc_search_batch against the restatement of tests/obmc_search_cases.py (which golden/obmc.npz pins on the reference's
single_motion_search job by job), bit for bit: best_mv, every field of the result record, the status bytes; the output slots of undefined and of
spare jobs come back untouched."""
import numpy as np
import pytest

import obmc_cases as oc
import obmc_search_cases as sc
from svt_av1_psyex_amd import obmc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(sc.batches()))
def test_search_equals_the_restatement_bit_for_bit(hip_ctx, name):
    b = sc.batches()[name]
    tables = None if b["params"]["approx_inter_rate"] else sc.cost_tables()
    got = obmc.run_search_hip(hip_ctx, b["params"], sc.ref_plane(b["ref"]), b["wsrc"], b["mask"], b["jobs"], tables=tables, spare_jobs=2, fill=oc.FILL)
    mv, res, _ = sc.restated(name)
    n = len(mv)
    assert np.all(got["status"][:n] == oc.ST_OK) and np.all(got["status"][n:] == oc.FILL)
    assert np.array_equal(got["best_mv"][:n], mv), (got["best_mv"][:n].tolist(), mv.tolist())
    assert got["results"][:n].tobytes() == res.tobytes(), (got["results"][:n].tolist(), res.tolist())
    assert np.all(got["best_mv"][n:].view(np.uint8) == oc.FILL) and np.all(got["results"][n:].view(np.uint8) == oc.FILL)


def test_undefined_jobs_get_status_ff_and_write_nothing_else(hip_ctx):
    b, bad = sc.undefined_batch()
    ref, tables = sc.ref_plane(b["ref"]), sc.cost_tables()
    got = obmc.run_search_hip(hip_ctx, b["params"], ref, b["wsrc"], b["mask"], b["jobs"], tables=tables, fill=oc.FILL)
    for i, j in enumerate(b["jobs"]):
        want = sc.restate_job(b["params"], ref, b["wsrc"], b["mask"], j, tables)
        if want is None:
            assert i in bad.values() and got["status"][i] == oc.ST_UNDEFINED
            assert np.all(got["best_mv"][i].view(np.uint8) == oc.FILL) and np.all(got["results"][i:i + 1].view(np.uint8) == oc.FILL)
        else:
            assert got["status"][i] == oc.ST_OK and tuple(got["best_mv"][i]) == want[0] and got["results"][i].tobytes() == want[1].tobytes()
    assert sum(s == oc.ST_OK for s in got["status"]) == 2 * len(bad)
