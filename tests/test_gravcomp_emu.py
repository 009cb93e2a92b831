"""not-gpu: the gravity-compensation build of the redistribution kernel (libdwbc_amd/csrc/dwbc_redistribute.h, GRAV = true) in host
emulation (tests/emu/emu_gravcomp.cpp: one "thread" per workgroup, LDS of exactly LdsGc<N, NB>::total doubles NaN-poisoned before every
instance, a guard behind it, outputs pre-filled with NaN) against the numpy restatement: on TopoGeneric at the pack sizes (23, 18),
(37, 32), (43, 38) and TOCABI's (39, 34), and on TOCABI's constant tree.  Both forms: gravity only, and the redistribution of
torque_grav_ + torque_input.

References, premises and bars: tests/gravcomp_cases.py (1e-6 Nm, 1e-5 N, status identical)."""
import numpy as np
import pytest

from tests import cases
from tests import gravcomp_cases as gc
from tests import redist_cases as rc
from tests import redist_pack_cases as pc
from tests.emu import emu_gravcomp as eg

# LdsGc<N, NB>::total_bytes as DESIGN.md section 5 lists them ("Gravity compensation"): the gravity stage adds tenants, no bytes
LDS_BYTES = {23: 12880, 37: 19488, 39: 20432, 43: 22320, 50: 26792}
CASES = [("fixed_arms", 16), ("fixed_head", 16), ("surgery_43", 8), ("tocabi", 16)]


def _mass(mo):
    return float(np.sum(mo["mass"]))


@pytest.mark.parametrize("name,B", CASES, ids=[c[0] for c in CASES])
def test_gravity_only_matches_restatement_at_pack_sizes(name, B):
    ref = pc.state_set(name, B)
    g = gc.pack_grav(name, B)
    gc.check_grav_premise(g, ref["flags"])
    mo, links = pc.model(name)
    rd, got = eg.run(mo, pc.contacts_of(links), np.full(mo["ndof"] - 6, pc.TAU_LIM), ref["q"], ref["flags"])
    assert np.isfinite(got["tau"]).all() and np.isfinite(got["wrench"]).all()
    gc.compare_grav(got, g)
    gc.check_free_instances(got, ref["flags"])
    gc.check_vertical_force(got, ref["flags"], _mass(mo))
    # without a torque input the redistribution's outputs are not touched
    assert np.isnan(rd["tau"]).all() and np.isnan(rd["cf"]).all() and np.isnan(rd["wrench"]).all() and (rd["status"] == -1).all()


@pytest.mark.parametrize("name,B", CASES, ids=[c[0] for c in CASES])
def test_option_matches_restatement_at_pack_sizes(name, B):
    ref = pc.state_set(name, B)
    rc.check_premises(ref)
    g = gc.pack_grav(name, B)
    gc.check_grav_premise(g, ref["flags"])
    mo, links = pc.model(name)
    rd, got = eg.run(mo, pc.contacts_of(links), np.full(mo["ndof"] - 6, pc.TAU_LIM), ref["q"], ref["flags"], tau_in=ref["tau_in"] - g["tau"])
    for k in ("tau", "cf", "wrench"):
        assert np.isfinite(rd[k]).all(), k
    rc.compare(rd, ref)
    pc.check_flag_mix_outputs(rd, ref)
    gc.compare_grav(got, g)  # torque_grav_ is written to the gravity outputs as well


@pytest.mark.parametrize("tree", [True, False], ids=["tocabi_tree", "generic_tree"])
def test_tocabi_both_forms(tree):
    ref = rc.state_set(32, True, "mixed")
    rc.check_premises(ref)
    g = gc.tocabi_grav(32, True, "mixed")
    gc.check_grav_premise(g, ref["flags"])
    mo = cases.tocabi_model()
    _, got = eg.run(mo, cases.CONTACTS_2, cases.TAU_LIM, ref["q"], ref["flags"], tree=tree)
    gc.compare_grav(got, g)
    gc.check_vertical_force(got, ref["flags"], _mass(mo))
    rd, got2 = eg.run(mo, cases.CONTACTS_2, cases.TAU_LIM, ref["q"], ref["flags"], tau_in=ref["tau_in"] - g["tau"], tree=tree)
    rc.compare(rd, ref)
    assert (got2["tau"] == got["tau"]).all() and (got2["wrench"] == got["wrench"]).all() and (got2["status"] == got["status"]).all()


def test_free_and_overflagged_instances():
    """no contact: exact zeros, status 1; three flags raised on a three-contact set-up: zeros, status 0"""
    g = gc.tocabi_grav(32, True, "mixed", free_every=3)
    ref = rc.state_set(32, True, "mixed")
    mo = cases.tocabi_model()
    _, got = eg.run(mo, cases.CONTACTS_2, cases.TAU_LIM, ref["q"], g["flags"], tree=True)
    gc.compare_grav(got, g)
    gc.check_free_instances(got, g["flags"])
    three = cases.CONTACTS_4[:3]  # both feet and a hand
    flags = np.ones((4, 3), np.uint8)
    flags[1, 2] = 0
    _, over = eg.run(mo, three, cases.TAU_LIM, ref["q"][:4], flags, tree=True)
    assert list(over["status"]) == [0, 1, 0, 0]
    assert np.abs(over["tau"][[0, 2, 3]]).max() == 0.0 and np.abs(over["wrench"][[0, 2, 3]]).max() == 0.0
    assert np.abs(over["tau"][1]).max() > gc.MIN_GRAV


def test_generic_tree_agrees_with_the_constant_tree_on_tocabi():
    ref = rc.state_set(32, True, "mixed")
    g = gc.tocabi_grav(32, True, "mixed")
    mo = cases.tocabi_model()
    tin = ref["tau_in"] - g["tau"]
    rd_t, gr_t = eg.run(mo, cases.CONTACTS_2, cases.TAU_LIM, ref["q"], ref["flags"], tau_in=tin, tree=True)
    rd_g, gr_g = eg.run(mo, cases.CONTACTS_2, cases.TAU_LIM, ref["q"], ref["flags"], tau_in=tin, tree=False)
    assert (gr_t["status"] == gr_g["status"]).all() and (rd_t["status"] == rd_g["status"]).all() and rd_t["status"].sum() >= 0.9 * 32
    e_g = float(np.abs(gr_t["tau"] - gr_g["tau"]).max())
    e_r = float(np.abs(rd_t["tau"] - rd_g["tau"]).max())
    print(f"worst |torque_grav_ generic - tree| = {e_g:.3e} Nm, worst |redist tau generic - tree| = {e_r:.3e} Nm")
    assert e_g <= 1e-9 and e_r <= 1e-9


@pytest.mark.parametrize("n", sorted(LDS_BYTES))
def test_lds_bytes_are_the_documented_ones(n):
    assert eg.lds_bytes(n) == LDS_BYTES[n]
