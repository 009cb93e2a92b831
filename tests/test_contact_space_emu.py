"""not-gpu: the contact-space kernel (libdwbc_amd/csrc/dwbc_contact_space.h) in host emulation (tests/emu/emu_contact_space.cpp: one
"thread" per workgroup, LDS of exactly LdsCs<N, NB>::total doubles NaN-poisoned before every instance, a guard behind it, every output
buffer pre-filled with NaN) against the numpy restatement and the reference's goldens: on TOCABI on both tree rows (B = 4), and on
TopoGeneric at the pack sizes (37, 32), (23, 18), (43, 38) (B = 3).  Every batch mixes the support: both feet, left only, right only, none.

Inputs, references, premises and bars: tests/contact_space_cases.py."""
import numpy as np
import pytest

from tests import cases
from tests import contact_space_cases as cc
from tests import redist_pack_cases as pc
from tests.emu import emu_contact_space as ec

# LdsCs<N, NB>::total_bytes as DESIGN.md lists them ("Contact space of CalcContactConstraint")
LDS_BYTES = {23: 12880, 37: 19488, 39: 20432, 43: 22320, 50: 26792}
PACKS = ["fixed_head", "fixed_arms", "surgery_43"]
MASKS = [("J_C",), ("Lambda_c", "J_C_INV_T"), ("NwJw",), ("W_inv",), ("N_C",), ("contact_pos", "contact_rot"), ("A_inv_N_C", "W")]


def _check_masks(mo, s, full, tree):
    """a few outputs alone: bit-equal to the same outputs of the all-outputs run, every other buffer keeps its sentinel"""
    for names in MASKS:
        got = ec.run(mo, s["contacts"], s["q"], s["flags"], outputs=names, tree=tree)
        assert (got["status"] == full["status"]).all(), names
        for k in cc.NAMES:
            if k in names:
                assert (got[k] == full[k]).all(), (names, k)
            else:
                assert np.isnan(got[k]).all(), (names, k)


def _check_support(got, s):
    """every support case is in the batch; no contact: N_C = I exactly, A_inv_N_C is symmetric positive (A^-1), W its joint block"""
    nact = s["flags"].sum(axis=1)
    assert set(nact.tolist()) >= {0, 1, 2}
    assert (got["status"] == 1).all()
    for b in np.nonzero(nact == 0)[0]:
        n = got["N_C"].shape[-1]
        assert (got["N_C"][b] == np.eye(n)).all()
        assert (got["W"][b] == got["A_inv_N_C"][b][6:, 6:]).all()
        for k in ("J_C", "Lambda_c", "J_C_INV_T", "NwJw", "contact_pos", "contact_rot"):
            assert not got[k][b].any(), k
    for b in np.nonzero(nact == 1)[0]:
        assert not got["NwJw"][b].any()
        assert np.abs(got["W"][b] @ got["W_inv"][b] - np.eye(got["W"].shape[-1])).max() < 1e-9  # (k = 0: W_inv is W's inverse)


def test_restatement_residual_premise():
    cc.check_residual_premise(cc.tocabi_set(4)["ref"], ("tocabi", 4))
    cc.check_residual_premise(cc.golden_set()["ref"], ("golden", 2))
    for name in PACKS:
        cc.check_residual_premise(cc.pack_set(name, 3)["ref"], (name, 3))


@pytest.mark.parametrize("tree", [True, False], ids=["tocabi_tree", "generic_tree"])
def test_tocabi_all_outputs_match_restatement(tree):
    s = cc.tocabi_set(4)
    mo = cases.tocabi_model()
    full = ec.run(mo, s["contacts"], s["q"], s["flags"], tree=tree)
    what = "emulation, " + ("constant tree" if tree else "generic tree")
    cc.compare(full, s["ref"], what, w_inv_bar=cc.BAR_W_INV_EMU)
    cc.check_identities(full, s["ref"], ("tocabi", 4), what)
    _check_support(full, s)
    _check_masks(mo, s, full, tree)


@pytest.mark.parametrize("tree", [True, False], ids=["tocabi_tree", "generic_tree"])
def test_tocabi_goldens_at_case_states(tree):
    g = cc.golden_set()
    got = ec.run(cases.tocabi_model(), g["contacts"], g["q"], g["flags"], tree=tree)
    cc.compare(got, g["ref"], "emulation, CASE states", w_inv_bar=cc.BAR_W_INV_EMU)
    cc.compare_goldens(got, g, "emulation", w_inv_bar=cc.BAR_W_INV_EMU)
    cc.check_identities(got, g["ref"], ("golden", 2), "emulation, CASE states")


def test_generic_tree_agrees_with_the_constant_tree_on_tocabi():
    """the leaves-first dense sweep keeps the entries outside the tree's pattern exact zeros: the two builds agree to the bit"""
    s = cc.tocabi_set(4)
    mo = cases.tocabi_model()
    t = ec.run(mo, s["contacts"], s["q"], s["flags"], tree=True)
    g = ec.run(mo, s["contacts"], s["q"], s["flags"], tree=False)
    for k in cc.NAMES:
        assert (t[k] == g[k]).all(), k


def test_three_flags_fail_the_instance_and_leave_its_neighbours_alone():
    s = cc.too_many_set()
    mo = cases.tocabi_model()
    got = ec.run(mo, s["contacts"], s["q"], s["flags"])
    assert got["status"].tolist() == [1, 0, 1]
    cc.compare(got, s["ref"], "emulation, three flags in instance 1", w_inv_bar=cc.BAR_W_INV_EMU)
    for k in cc.NAMES:
        assert not got[k][1].any(), k
    # the neighbours alone, in a batch of their own: the same bits
    keep = [0, 2]
    alone = ec.run(mo, s["contacts"], s["q"][keep], s["flags"][keep])
    for k in cc.NAMES:
        assert (alone[k] == got[k][keep]).all(), k
    # one output alone: the failed instance is zero there too, nothing else is written
    one = ec.run(mo, s["contacts"], s["q"], s["flags"], outputs=("N_C",))
    assert one["status"].tolist() == [1, 0, 1] and not one["N_C"][1].any() and np.isnan(one["J_C"]).all()


@pytest.mark.parametrize("name", PACKS)
def test_pack_sizes_match_restatement(name):
    s = cc.pack_set(name, 3)
    mo, _ = pc.model(name)
    assert (mo["ndof"], mo["nb"]) == pc.SIZES[name]
    full = ec.run(mo, s["contacts"], s["q"], s["flags"])
    cc.compare(full, s["ref"], "emulation, " + name, w_inv_bar=cc.BAR_W_INV_EMU)
    cc.check_identities(full, s["ref"], (name, 3), "emulation, " + name)
    _check_masks(mo, s, full, False)


@pytest.mark.parametrize("n", sorted(LDS_BYTES))
def test_lds_bytes_are_the_documented_ones(n):
    assert ec.lds_bytes(n) == LDS_BYTES[n]
