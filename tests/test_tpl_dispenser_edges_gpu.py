"""GPU: svt_hip_tpl_dispense on the edge cases of tests/tpl_dispenser_cases.py (zero-eob blocks, every transform size and shape, ties,
MV clamps, range limits, grid writes past a row and past the grid, stored stats the reference never produces, diagonals longer than the
intra kernel's waves) -- device == restatement == the reference's own dispenser (tests/golden/tpl_dispenser_edges.npz), bit for bit: the
whole padded recon plane, every written cell's nine fields, the set of untouched cells, the TplSrcStats.  Group G has no reference: the
restatement states the header's definition.  test_tpl_dispenser_edges.py (CPU) asserts that each case reaches the path it is built for."""
import ctypes as C

import numpy as np
import pytest

from svt_av1_psyex_amd import api, tpl
from test_tpl_dispenser_edges import FIXTURE_NAMES, NAMES, assert_equals_fixture, edge_fixture, restated
from tpl_dispenser_cases import assert_same
from tpl_dispenser_cases import PAD, exact_cells, restate

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES)
def test_edge_case_vs_restatement_and_reference(hip_ctx, name):
    c, want, _ = restated(name)
    got = tpl.run_tpl_hip(hip_ctx, c, PAD)
    assert_same(c, got, want, f"{name} (restatement)")
    if name in FIXTURE_NAMES:
        assert_equals_fixture(name, want)  # so the recon plane below is the reference's, also where the fixture stores its sha256
        f = edge_fixture()[name]
        assert_same(c, got, (f["tpl_stats"], f["tpl_src_stats"], want[2]), f"{name} (reference)")


def test_exact_cell_count_leaves_the_cells_behind_untouched(hip_ctx):
    """n_tpl_stats names the grid's cells exactly while the buffer is longer: the 2x2 writes below the grid's last row are dropped."""
    import torch
    c = exact_cells(restated("F_grid_below_last_row")[0])
    n = c["n_tpl_stats"]
    assert n == 13 * 9 < len(c["tpl_stats"])
    t = tpl.upload_case(c)
    torch.cuda.synchronize()
    d = tpl.make_desc(c, PAD, t["cur"].data_ptr(), t["recon"].data_ptr(), {k: (v[0].data_ptr(), v[1].data_ptr()) for k, v in t["refs"].items()},
                      tuple(x.data_ptr() for x in t["me"]), t["tpl_stats"].data_ptr(), t["tpl_src_stats"].data_ptr())
    d.n_tpl_stats = n
    hip_ctx.check(api.lib().svt_hip_tpl_dispense(hip_ctx._h, C.byref(d)), "svt_hip_tpl_dispense")
    hip_ctx.sync()
    got = tpl.download(c, t)
    assert_same(c, got, restate(c), "exact n_tpl_stats")
    assert (got[0][n:].view(np.uint8) == 0xA5).all()
    f = edge_fixture()["F_grid_below_last_row"]  # the reference's cells inside the grid
    for k in got[0].dtype.names:
        if k != "reserved":
            np.testing.assert_array_equal(got[0][k][:n], f["tpl_stats"][k][:n], err_msg=k)
