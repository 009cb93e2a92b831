"""not-gpu: the dynamics kernel (libdwbc_amd/csrc/dwbc_dynamics.h) in host emulation (tests/emu/emu_dynamics.cpp: one "thread" per
workgroup, LDS of exactly LdsDyn<N, NB>::total doubles NaN-poisoned before every instance, a guard behind it, every output buffer
pre-filled with NaN) against the numpy restatement: on TOCABI's constant tree (B = 4), and on TopoGeneric at the pack sizes (37, 32),
(23, 18), (43, 38) (B = 3).

Inputs, references, premises and bars: tests/dynamics_cases.py."""
import numpy as np
import pytest

from tests import cases
from tests import dynamics_cases as dc
from tests import redist_pack_cases as pc
from tests.emu import emu_dynamics as ed

# LdsDyn<N, NB>::total_bytes as DESIGN.md lists them ("Dynamics of UpdateKinematics")
LDS_BYTES = {23: 8336, 37: 14448, 39: 15536, 43: 17824, 50: 22144}
PACKS = ["fixed_head", "fixed_arms", "surgery_43"]
MASKS = [("G",), ("A_inv",), ("B",)]


def _all_written(got):
    for k in dc.NAMES:
        assert np.isfinite(got[k]).all(), k
    assert (got["status"] == 1).all()


def _check_masks(mo, s, full, tree):
    """one output alone: bit-equal to the same output of the all-outputs run, every other buffer keeps its sentinel"""
    for names in MASKS:
        got = ed.run(mo, s["q"], s["qd"], outputs=names, tree=tree)
        assert (got["status"] == 1).all(), names
        for k in dc.NAMES:
            if k in names:
                assert (got[k] == full[k]).all(), (names, k)
            else:
                assert np.isnan(got[k]).all(), (names, k)


def _check_no_qdot(mo, s, full, tree):
    """without a qdot B_ is G_ to the bit, and nothing else moves"""
    got = ed.run(mo, s["q"], None, tree=tree)
    _all_written(got)
    assert (got["B"] == got["G"]).all()
    for k in ("A", "A_inv", "G", "CMM", "com"):
        assert (got[k] == full[k]).all(), k
    assert np.abs(full["B"] - full["G"]).max() > 1.0  # (with the velocities of the set B_ is not G_: the comparison above is not idle)


def test_restatement_residual_premise():
    dc.check_residual_premise(dc.tocabi_set(4)["ref"], ("tocabi", 4))
    for name in PACKS:
        dc.check_residual_premise(dc.pack_set(name, 3)["ref"], (name, 3))
    g = dc.golden_set()
    dc.check_residual_premise(dc.reference(cases.tocabi_model(), g["q"], None), ("golden", 2))


@pytest.mark.parametrize("tree", [True, False], ids=["tocabi_tree", "generic_tree"])
def test_tocabi_all_outputs_match_restatement(tree):
    s = dc.tocabi_set(4)
    mo = cases.tocabi_model()
    full = ed.run(mo, s["q"], s["qd"], tree=tree)
    _all_written(full)
    dc.compare(full, s["ref"], ("tocabi", 4), "emulation, " + ("constant tree" if tree else "generic tree"))
    _check_no_qdot(mo, s, full, tree)
    _check_masks(mo, s, full, tree)


def test_tocabi_goldens_at_case_states():
    g = dc.golden_set()
    got = ed.run(cases.tocabi_model(), g["q"], None, outputs=("A", "A_inv"), tree=True)
    assert (got["status"] == 1).all()
    e_a, e_i = float(np.abs(got["A"] - g["A"]).max()), float(np.abs(got["A_inv"] - g["A_inv"]).max())
    r = dc.residual(got["A"], got["A_inv"])
    print(f"goldens: |A - Acontact_mat| = {e_a:.2e}, |A_inv - A_inv_| = {e_i:.2e}, max|A A_inv - I| = {r:.2e}")
    assert e_a <= dc.BARS["A"] and e_i <= dc.BARS["A_inv"] and r <= dc.bar_residual(("golden", 2))


def test_generic_tree_agrees_with_the_constant_tree_on_tocabi():
    """the leaves-first dense sweep keeps the entries outside the tree's pattern exact zeros: the two builds agree to the bit"""
    s = dc.tocabi_set(4)
    mo = cases.tocabi_model()
    t, g = ed.run(mo, s["q"], s["qd"], tree=True), ed.run(mo, s["q"], s["qd"], tree=False)
    for k in dc.NAMES:
        assert (t[k] == g[k]).all(), k


@pytest.mark.parametrize("name", PACKS)
def test_pack_sizes_match_restatement(name):
    s = dc.pack_set(name, 3)
    mo, _ = pc.model(name)
    assert (mo["ndof"], mo["nb"]) == pc.SIZES[name]
    full = ed.run(mo, s["q"], s["qd"])
    _all_written(full)
    dc.compare(full, s["ref"], (name, 3), "emulation")
    _check_no_qdot(mo, s, full, False)
    _check_masks(mo, s, full, False)


@pytest.mark.parametrize("n", sorted(LDS_BYTES))
def test_lds_bytes_are_the_documented_ones(n):
    assert ed.lds_bytes(n) == LDS_BYTES[n]
