"""CPU: the dispenser's edge cases (tests/tpl_dispenser_cases.py:edge_cases).  The restatement equals the reference's own dispenser on
every one (tests/golden/tpl_dispenser_edges.npz, tools/gen_tpl_golden.py; group G, stored stats the reference never produces, is the
project's definition and has no fixture), and each case still reaches the path of the kernel it was built for: the conditions are
asserted on the counters restate() fills.  They are conditions on the inputs, not measurements of the kernel.

The int16 clamp of quantize_fp's t needs |coeff| + round_fp > 32767.  The largest |coeff| of a +-255 flat residual is 32637 (16x16),
32625 (32x32) and 32648 (32x8), so the clamp fires once the DC step is at least 262 (with step 1336 it leaves the quantized value as it is, with step 300 it
changes it: both are cases); with TX_16X8 / TX_32X16 (sub 1) it is 23091 and with
TX_16X4 16327: the clamp cannot fire there, and no case pretends to.  recon_clamp_* is a proxy (see restate)."""
import functools

import numpy as np
import pytest

from svt_av1_psyex_amd import tpl
from test_tpl_dispenser import FIELDS_S, FIELDS_SRC, fake_desc
from tpl_dispenser_cases import (EDGE_FIXTURE_GROUPS, EDGE_PLANES_STORED, GOLDEN_EDGES, NEWMV, PAD, edge_case, edge_case_names, exact_cells,
                                 input_checksum, plane_checksum, restate)

NAMES = edge_case_names()
FIXTURE_NAMES = edge_case_names(EDGE_FIXTURE_GROUPS)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(case, restatement, counters) of an edge case, computed once and shared (nobody changes them)."""
    c = edge_case(name)
    st = {}
    return c, restate(c, st), st


@functools.lru_cache(maxsize=None)
def edge_fixture():
    z = np.load(GOLDEN_EDGES)
    out = {}
    for i, name in enumerate(FIXTURE_NAMES):
        assert str(z[f"name_{i}"]) == name
        out[name] = dict(checksum=z[f"checksum_{i}"], tpl_stats=z[f"tpl_stats_{i}"], tpl_src_stats=z[f"tpl_src_stats_{i}"],
                         recon=z[f"recon_{i}"] if f"recon_{i}" in z.files else None, recon_sha=z[f"recon_sha_{i}"] if f"recon_sha_{i}" in z.files else None)
    assert f"name_{len(FIXTURE_NAMES)}" not in z.files
    return out


def assert_equals_fixture(name, got):
    """Every field of (tpl_stats, tpl_src_stats, recon) against the fixture's entry, all cells (untouched ones included)."""
    f = edge_fixture()[name]
    g, s, r = got
    if f["recon"] is not None:
        assert name[0] in EDGE_PLANES_STORED
        np.testing.assert_array_equal(r, f["recon"], err_msg=f"{name}: recon")
    else:
        np.testing.assert_array_equal(plane_checksum(r), f["recon_sha"], err_msg=f"{name}: recon (sha256)")
    assert len(g) == len(f["tpl_stats"])
    for k in FIELDS_S:
        np.testing.assert_array_equal(g[k], f["tpl_stats"][k], err_msg=f"{name}: tpl_stats.{k}")
    for k in FIELDS_SRC:
        np.testing.assert_array_equal(s[k], f["tpl_src_stats"][k], err_msg=f"{name}: tpl_src_stats.{k}")


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_restatement_equals_the_reference_on_edge_cases(name):
    c, got, _ = restated(name)
    np.testing.assert_array_equal(input_checksum(c), edge_fixture()[name]["checksum"], err_msg=f"{name}: the case's inputs changed")
    assert_equals_fixture(name, got)


@pytest.mark.parametrize("name", NAMES)
def test_check_desc_accepts_the_edge_cases(name):
    tpl.check_desc(fake_desc(restated(name)[0]))


def stats_of(name):
    return restated(name)[2]


@pytest.mark.parametrize("name", edge_case_names("A"))
def test_group_a_reaches_eob_zero_and_full_eob(name):
    st, c = stats_of(name), restated(name)[0]
    if "fine" in name:
        assert st["max_eob"] == 256 and st["rec_eob0_newmv"] == st["rec_eob0_dc"] == st["src_eob0"] == 0
        return
    assert st["rec_eob0_newmv"] >= 3 and st["src_eob0"] >= 1
    assert st["rec_eob_pos_newmv"] >= 3 and st["rec_eob_pos_dc"] >= 3 and st["src_eob_pos"] >= 3
    if c["sub"] == 2:  # duplicated rows instead of the prediction's own rows would show
        assert st["eob0_newmv_rows_differ"] >= 1
    if "no_inverse" in name:
        assert c["disable_intra_pred"] and not c["is_ref"]


@pytest.mark.parametrize("name", edge_case_names("B"))
def test_group_b_has_both_kinds_of_block(name):
    st = stats_of(name)
    assert st["newmv_blocks"] >= 1 and st["dc_blocks"] >= 1


def test_group_b_covers_every_size_and_shape():
    seen = {(c["level"], c["sub"], c["pf"]) for c in (restated(n)[0] for n in edge_case_names("B"))}
    assert seen >= {(l, s, pf) for l in (0, 1) for s in (0, 1, 2) for pf in (0, 1, 2)} | {(0, 0, 3), (1, 2, 3)}
    # the encoder's pairs with N2
    assert {(0, 0, 1), (1, 2, 1)} <= seen


@pytest.mark.parametrize("name", edge_case_names("C"))
def test_group_c_ties(name):
    st, c = stats_of(name), restated(name)[0]
    if c["level"] == 0:
        assert st["cand_ties"] >= 10 and st["inter_intra_ties"] >= 10 and st["cand_ties_rf"] >= 3 and st["re_is_1"] >= 3
    else:
        assert st["cand_ties"] >= 3 and st["inter_intra_ties"] >= 3


def test_group_c_has_a_tie_across_the_lists():
    c, (_, s, _), st = restated("C_ties_L0_list0_list1")
    assert np.array_equal(c["refs"][(0, 0)]["src"], c["refs"][(1, 0)]["src"]) and st["cand_ties_rf"] >= 3
    assert (s["best_rf_idx"] == 0).any()  # a list-0 winner that a later list-1 candidate (best_rf_idx 4) equals


@pytest.mark.parametrize("name", edge_case_names("D"))
def test_group_d_clamps_on_all_four_sides(name):
    st = stats_of(name)
    for k in ("clamp_x_lo", "clamp_x_hi", "clamp_y_lo", "clamp_y_hi"):
        assert st[k] >= 3, k
    if "intra_on" not in name:
        assert st["winner_clamped_y"] >= 1


E_T_CLAMP = {"E_halves_L0_coarse_inter": 32637, "E_halves_L1_sub0_coarse_inter": 32625, "E_halves_L1_sub2_coarse_inter": 32648,
             "E_halves_L0_step300_inter": 32637, "E_halves_L1_sub0_step300_inter": 32625, "E_halves_L1_sub2_step300_inter": 32648}


@pytest.mark.parametrize("name", edge_case_names("E"))
def test_group_e_range_limits(name):
    st, c = stats_of(name), restated(name)[0]
    step_dc, round_dc = int(c["quant"]["dequant"].reshape(-1)[0]), int(c["quant"]["round_fp"].reshape(-1)[0])
    if name in E_T_CLAMP:  # from the oracle's coeff: the flat +-255 residual's DC coefficient, past int16 with the rounding term
        assert st["max_abs_coeff"] == E_T_CLAMP[name] and step_dc >= 262
        assert st["max_abs_coeff"] + round_dc > 32767 and st["t_clamped"] >= 3
        # step 1336: the clamped and the unclamped t quantize alike; step 300: a kernel without the clamp gives another qcoeff
        assert (st["t_clamp_changes_q"] >= 3) == ("step300" in name) and (st["t_clamp_changes_q"] == 0) == ("coarse" in name)
    else:
        assert st["t_clamped"] == 0 and st["t_clamp_changes_q"] == 0
    if name == "E_halves_L0_sub1_coarse_inter":
        assert st["max_abs_coeff"] == 23091  # TX_16X8: out of the clamp's reach whatever the step
    if "fine" in name:
        assert step_dc == 4 and st["max_abs_coeff"] + round_dc <= 32767
    assert st["recon_clamp_blocks"] >= 3
    if "intra" in name:
        assert st["dc_blocks"] >= 3 and not c["disable_intra_pred"]
    else:
        assert st["newmv_blocks"] >= 3 and c["disable_intra_pred"]


def test_group_e_patterns():
    c = restated("E_halves_L0_coarse_inter")[0]
    inner = c["cur"][PAD:PAD + c["height"], PAD:PAD + c["width"]]
    assert (inner[:, :64] == 255).all() and (inner[:, 64:] == 0).all()
    assert all(((r["src"].astype(int) + c["cur"]) == 255).all() for r in c["refs"].values())
    c = restated("E_checker_L0_coarse_inter")[0]
    inner = c["cur"][PAD:PAD + c["height"], PAD:PAD + c["width"]].astype(int)
    assert set(np.unique(inner)) == {0, 255} and (np.abs(np.diff(inner, axis=0)) == 255).all() and (np.abs(np.diff(inner, axis=1)) == 255).all()


def test_group_f_grid_writes_past_a_row_and_past_the_grid():
    c, (g, _, _), st = restated("F_grid_row_wrap")
    gs, rows = 15, 8
    assert (c["aligned_width"] + 15) // 16 == gs and (c["aligned_height"] + 15) // 16 == rows
    assert st["grid_wrap_row"] >= 3 and st["grid_cells_past_grid"] == 1
    touched = ~(g.view(np.uint8).reshape(len(g), -1) == 0xA5).all(1)
    assert touched[gs * rows] and not touched[gs * rows + 1:].any()  # the last block's base + gs + 1: the first cell past the grid
    c, (g, _, _), st = restated("F_grid_below_last_row")
    gs, rows = 13, 9
    assert (c["aligned_width"] + 15) // 16 == gs and (c["aligned_height"] + 15) // 16 == rows
    assert st["grid_below_last_row"] >= 3 and st["grid_wrap_row"] >= 3 and st["grid_cells_past_grid"] == gs + 1
    assert len(g) >= gs * rows + gs + 2  # the reference writes up to gs + 1 cells past the grid
    touched = ~(g.view(np.uint8).reshape(len(g), -1) == 0xA5).all(1)
    assert touched[gs * rows:gs * rows + gs + 1].all() and not touched[gs * rows + gs + 1:].any()


def test_group_f_exact_cell_count_drops_the_writes_past_the_grid():
    c, (g, _, r), _ = restated("F_grid_below_last_row")
    n = 13 * 9
    g2, _, r2 = restate(exact_cells(c))
    np.testing.assert_array_equal(r2, r)
    assert g2[:n].tobytes() == g[:n].tobytes() and (g2[n:].view(np.uint8) == 0xA5).all()
    for k in FIELDS_S:
        np.testing.assert_array_equal(g2[k][:n], edge_fixture()["F_grid_below_last_row"]["tpl_stats"][k][:n], err_msg=k)


@pytest.mark.parametrize("name", edge_case_names("H"))
def test_group_h_diagonals_longer_than_the_intra_waves(name):
    st = stats_of(name)
    assert st["longest_dc_diagonal"] > 16 and st["dc_blocks_past_16_on_diagonal"] >= 3


def test_group_g_far_stored_vectors_are_clamped_on_every_side():
    for name in ("G_far_stored_mvs_L0", "G_far_stored_mvs_L1"):
        c, _, st = restated(name)
        s = c["tpl_src_stats"][c["tpl_src_stats"]["best_mode"] == NEWMV]
        assert (s["mv_col"] < -2000).sum() >= 1 and (s["mv_col"] > 2000).sum() >= 1 and (s["mv_row"] < -2000).sum() >= 1 and (s["mv_row"] > 2000).sum() >= 1
        assert st["stored_mv_clamped"] >= 4 and st["stored_mv_clamped"] == st["newmv_blocks"]


@pytest.mark.parametrize("name,values", [("G_newmv_without_planes", (3, 6)), ("G_rf_idx_out_of_range", (9, -1))])
def test_group_g_skipped_blocks_keep_the_buffers(name, values):
    """A stored NEWMV naming no usable planes: the block's recon samples keep the buffer's pattern and its cell stays 0xA5, the others
    are dispensed."""
    c, (g, _, r), st = restated(name)
    s = c["tpl_src_stats"]
    a16w = (c["aligned_width"] + 15) >> 4
    n = {v: 0 for v in values}
    for i in np.flatnonzero((s["best_mode"] == NEWMV) & np.isin(s["best_rf_idx"], values)):
        x, y = (i % a16w) * 16, (i // a16w) * 16
        if x + 8 > c["width"] or y + 8 > c["height"]:
            continue
        # samples inside the picture (the padding pass replicates over what lies outside it)
        h, w = min(16, c["height"] - y), min(16, c["width"] - x)
        np.testing.assert_array_equal(r[PAD + y:PAD + y + h, PAD + x:PAD + x + w], c["recon"][PAD + y:PAD + y + h, PAD + x:PAD + x + w])
        assert (g[i:i + 1].view(np.uint8) == 0xA5).all()  # synth 16, 16x16 blocks: cell index == block index
        n[int(s["best_rf_idx"][i])] += 1
    assert all(v >= 3 for v in n.values()) and sum(n.values()) == st["stored_skipped"]
    assert st["blocks"] >= 50
