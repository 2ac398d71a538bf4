"""CPU: the ME -> TPL chain cases (tests/me_tpl_cases.py).  The dispenser's restatement fed with the oracle's ME arrays equals the
reference fixture tests/golden/tpl_me_chain.npz (tools/gen_me_tpl_golden.py: the reference build's ME -> the reference's own dispenser,
synthesizer and r0 / beta); the reference build's ME equals the oracle's on every chain case; the cases exercise what they are for
(both dispenser paths, both lists, the MV clamp, skipped blocks, the ME layouts of real pictures) -- asserted on the oracle and the
restatement, never on device output."""
import numpy as np
import pytest

import me_tpl_cases as mt
import tpl_group_cases as gc
from me_cases import compare
from svt_av1_psyex_amd import tpl

SINGLE = list(mt.SINGLE)
WINDOWS = list(mt.WINDOWS)


def fake_desc(case):
    """A descriptor of the case with host addresses as stand-ins: svt_hip_tpl_check_desc reads no sample."""
    refs = {k: (r["src"].ctypes.data, r["recon"].ctypes.data) for k, r in case["refs"].items()}
    me = None if case["slice_is_i"] else tuple(case["me"][k].ctypes.data for k in ("total", "mv", "cand"))
    return tpl.make_desc(case, case["pad"], case["cur"].ctypes.data, case["recon"].ctypes.data, refs, me, case["tpl_stats"].ctypes.data,
                         case["tpl_src_stats"].ctypes.data)


@pytest.fixture(scope="module")
def fixture():
    return mt.load_fixture()


@pytest.mark.parametrize("name", mt.FIXTURE_SINGLE)
def test_restatement_on_oracle_me_equals_the_reference_fixture(fixture, name):
    c, got = mt.oracle_single(name)
    rec = fixture[name]
    np.testing.assert_array_equal(mt.input_checksum(c), rec["checksum"], err_msg=f"{name}: the inputs (the oracle's ME arrays among them) are not the fixture's")
    mt.assert_equals_fixture(rec, got, name)


def test_window_restatement_on_oracle_me_equals_the_reference_fixture(fixture):
    win, _, recons, grids, outs = mt.oracle_window(mt.FIXTURE_WINDOW)
    rec = fixture["window_" + mt.FIXTURE_WINDOW]
    np.testing.assert_array_equal(mt.window_checksum(win), rec["checksum"], err_msg="the window's inputs are not the fixture's")
    want = gc.outputs_record(win, grids, outs, full_grids=True)
    assert set(want) | {"checksum", "recon_sha"} == set(rec)
    for k in win["frames"][0]["grid"].dtype.names:
        np.testing.assert_array_equal(want["grids"][k], rec["grids"][k], err_msg=f"grids.{k}")
    assert want["grids"].tobytes() == rec["grids"].tobytes()
    for k in ("r0", "tpl_is_valid", "beta", "scaling"):
        np.testing.assert_array_equal(want[k], rec[k], err_msg=k)
    np.testing.assert_array_equal(np.stack([mt.plane_sha(r) for r in recons]), rec["recon_sha"], err_msg="recon planes")


@pytest.mark.parametrize("name", SINGLE)
def test_reference_me_equals_oracle_me(ref, fixture, name):
    """Ties the fixture's inputs to ME output: the reference build's ME arrays are the oracle's, and their checksum is the stored one."""
    got = mt.me_case(name).run_cpu("ref")
    assert not compare(mt.oracle_me(name), got), name
    if name in fixture:
        np.testing.assert_array_equal(mt.input_checksum(mt.single_case(name, got)), fixture[name]["checksum"], err_msg=name)


@pytest.mark.parametrize("name", WINDOWS)
def test_reference_me_equals_oracle_me_on_the_windows(ref, fixture, name):
    got = [mc.run_cpu("ref") for mc in mt.window_me_cases(name)]
    for i, (a, b) in enumerate(zip(mt.oracle_window_me(name), got)):
        assert not compare(a, b), f"{name}: picture {i + 1}"
    if name == mt.FIXTURE_WINDOW:
        np.testing.assert_array_equal(mt.window_checksum(mt.window(name, got)), fixture["window_" + name]["checksum"], err_msg=name)


@pytest.mark.parametrize("name", SINGLE)
def test_single_cases_exercise_the_dispenser(name):
    c, (_, src_stats, _) = mt.oracle_single(name)
    st = mt.walk_stats(c, src_stats)
    assert st["skipped"] >= 1 and st["evaluated"] >= st["inside"] // 2, st
    if not c["disable_intra_pred"]:
        assert 0.05 <= st["newmv_share"] <= 0.95, st   # both the NEWMV and the DC path of the recon pass
    else:
        assert st["newmv_share"] == 1.0, st            # every block has at least one candidate
    if not name.startswith("232x184"):
        assert st["clamped"] >= 1, st                  # the +-32 clamp changes an evaluated MV
    two_lists = any(k[0] == 1 for k in c["refs"])
    if two_lists:
        assert {w >> 2 for w in st["winners"]} == {0, 1}, st
        assert st["bits67"] > 0, st                    # the candidate byte's upper bits are set (the synthetic cases never do that)
    if "_m3_" in name:
        assert {1, 5} & st["winners"], st              # a winner with ref index 1: the max_l0 term of the MV slot matters
    mv = c["me"]["mv"]
    assert (np.abs((mv & 0xFFFF).astype(np.uint16).view(np.int16)) > 32).any() or (np.abs((mv >> 16).astype(np.uint16).view(np.int16)) > 32).any()


def test_the_grid_covers_the_me_layouts():
    layouts = {(c["n_pu"], c["max_cand"], c["max_refs"], c["max_l0"]) for c in (mt.oracle_single(n)[0] for n in SINGLE)}
    assert {l[0] for l in layouts} == {85, 21}
    assert len({l[1:] for l in layouts}) >= 3, layouts
    assert {(85, 3, 2, 1), (85, 9, 4, 2), (21, 1, 1, 1)} <= layouts


@pytest.mark.parametrize("name", WINDOWS)
def test_windows_exercise_the_group(name):
    win, d_grids, recons, grids, outs = mt.oracle_window(name)
    assert [f["valid"] for f in win["frames"]] == [1, 1, 1, 0] and win["frames"][0]["case"]["slice_is_i"]
    assert gc.stride_alias(win) == (name == "360x200_m3_s32")
    for i in (1, 2):  # the inter pictures take both dispenser paths and something propagates back from them
        c = dict(win["frames"][i]["case"])
        st = mt.walk_stats(c, _src_stats_of(win, i, recons))
        assert 0.05 <= st["newmv_share"] <= 0.95 and st["skipped"] >= 1, (i, st)
    for i in (0, 1):
        assert (grids[i]["mc_dep_dist"][:gc.geometry(win)["alloc"]] != 0).any(), i
    assert [o[1] for o in outs] == [1, 1, 1, 0]
    assert n_pu_of(win) == (21 if "m12" in name else 85)


def n_pu_of(win):
    return win["frames"][1]["case"]["n_pu"]


def _src_stats_of(win, i, recons):
    """The TplSrcStats of picture i of a window as the group dispenses it (its list-0 recon-path reference = the TPL recon before it)."""
    import tpl_dispenser_cases as tc
    return tc.restate(gc.chained_cases(win, recons)[i])[1]


@pytest.mark.parametrize("name", SINGLE)
def test_check_desc_accepts_the_chain_cases(name):
    tpl.check_desc(fake_desc(mt.oracle_single(name)[0]))


@pytest.mark.parametrize("name", WINDOWS)
def test_check_desc_accepts_the_windows(name):
    """svt_hip_tpl_check_desc on every picture and svt_hip_tpl_group_check_desc on the group with its dispenser descriptors."""
    import ctypes as C
    from test_tpl_group import fake_group
    win, _, recons, _, _ = mt.oracle_window(name)
    d = fake_group(win, gc.STAGES_ALL)
    disp = []
    for i, c in enumerate(gc.chained_cases(win, recons)):
        t = fake_desc(c)
        tpl.check_desc(t)
        t.tpl_stats = d.frames[i].tpl_stats
        disp.append(t)
        d.frames[i].dispense = C.pointer(t)
    d._disp = disp
    tpl.group_check_desc(d)
