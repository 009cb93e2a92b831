"""not-gpu: the task-space kernel (libdwbc_amd/csrc/dwbc_task_space.h) in host emulation (tests/emu/emu_task_space.cpp: one "thread" per
workgroup, LDS of exactly LdsTs<N, NB>::total doubles NaN-poisoned before every instance, a guard behind it, every output buffer pre-filled
with NaN) against the numpy restatement: H4, HCOM, HPOS (the position and COM-frame modes, two links on a level) and the one- and two-level prefixes of H4 on TOCABI on both tree rows, and the first three
levels of H4 at the generic (37, 32) size, B = 8, every mask tier.

Inputs, references, premises and bars: tests/task_space_cases.py."""
import numpy as np
import pytest

from tests import cases
from tests import redist_pack_cases as pc
from tests import task_space_cases as tc
from tests.emu import emu_contact_space as ec
from tests.emu import emu_task_space as et

B = 8
# LdsTs<N, NB>::total_bytes as DESIGN.md lists them ("Task space of CalcTaskSpace")
LDS_BYTES = {23: 24960, 37: 36944, 39: 38656, 43: 53032, 50: 64736}
# (the empty tier is a request of the status alone: every output buffer keeps its sentinel)
TIERS = [(), ("J_task",), ("J_task", "Lambda_task"), ("Lambda_task",), ("J_task", "Lambda_task", "J_kt"), ("J_kt",), ("Null_task",)]


def _a_inv_n_c(mo, s, tree):
    """A_inv_N_C of the contact-space kernel's emulation on the same inputs: the front end the levels were formed from"""
    return ec.run(mo, s["contacts"], s["q"], s["flags"], outputs=("A_inv_N_C",), tree=tree)["A_inv_N_C"]


def _check_tiers(mo, s, full, tree):
    """every mask tier: bit-equal to the same outputs of the all-outputs run, every other buffer keeps its sentinel"""
    for names in TIERS:
        got = et.run(mo, s["contacts"], s["tasks"], s["q"], s["flags"], outputs=names, tree=tree)
        assert (got["status"] == full["status"]).all(), names
        for k in tc.NAMES:
            for l, a in enumerate(got[k]):
                if k in names:
                    assert (a == full[k][l]).all(), (names, k, l)
                else:
                    assert np.isnan(a).all(), (names, k, l)


@pytest.mark.parametrize("hier", ["H4", "HCOM", "HPOS", "H4_1", "H4_2"])
def test_restatement_residual_premise(hier):
    tc.check_residual_premise(tc.tocabi_set(hier, B)["ref"], (hier, B))


def test_restatement_residual_premise_generic_size():
    tc.check_residual_premise(tc.pack_set("fixed_head", B)["ref"], ("fixed_head", B))


@pytest.mark.parametrize("tree", [True, False], ids=["tocabi_tree", "generic_tree"])
@pytest.mark.parametrize("hier", ["H4", "HCOM", "HPOS", "H4_1", "H4_2"])
def test_tocabi_matches_restatement(hier, tree):
    s = tc.tocabi_set(hier, B)
    mo = cases.tocabi_model()
    full = et.run(mo, s["contacts"], s["tasks"], s["q"], s["flags"], tree=tree)
    what = f"emulation, {hier}, " + ("constant tree" if tree else "generic tree")
    assert (full["status"] == 1).all()
    assert set(s["flags"].sum(axis=1).tolist()) >= ({1, 2} if hier == "HCOM" else {0, 1, 2})  # every support is in the batch
    tc.compare(full, s["ref"], s["tasks"], s["nb"], what, w_bar=tc.BAR_W_EMU)
    tc.check_identities(full, _a_inv_n_c(mo, s, tree), s["ref"], (hier, B), what)
    _check_tiers(mo, s, full, tree)


def test_generic_size_matches_restatement():
    s = tc.pack_set("fixed_head", B)
    mo, _ = pc.model("fixed_head")
    assert (mo["ndof"], mo["nb"]) == (37, 32)
    full = et.run(mo, s["contacts"], s["tasks"], s["q"], s["flags"])
    tc.compare(full, s["ref"], s["tasks"], s["nb"], "emulation, fixed_head (37, 32)", w_bar=tc.BAR_W_EMU)
    tc.check_identities(full, _a_inv_n_c(mo, s, False), s["ref"], ("fixed_head", B), "emulation, fixed_head (37, 32)")
    _check_tiers(mo, s, full, False)


def test_generic_tree_agrees_with_the_constant_tree_on_tocabi():
    """the leaves-first dense sweep keeps the entries outside the tree's pattern exact zeros: the two builds agree to the bit"""
    s = tc.tocabi_set("H4", B)
    mo = cases.tocabi_model()
    t = et.run(mo, s["contacts"], s["tasks"], s["q"], s["flags"], tree=True)
    g = et.run(mo, s["contacts"], s["tasks"], s["q"], s["flags"], tree=False)
    for k in tc.NAMES:
        for a, b in zip(t[k], g[k]):
            assert (a == b).all(), k


def test_three_flags_fail_the_instance_and_leave_its_neighbours_alone():
    q, _, _ = cases.synth_batch(3, seed=tc.SEED, yaw=True)
    fl = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    mo = cases.tocabi_model()
    ref = tc.reference(mo, cases.CONTACTS_4, tc.H4, q, fl)
    got = et.run(mo, cases.CONTACTS_4, tc.H4, q, fl)
    assert got["status"].tolist() == [1, 0, 1]
    tc.compare(got, ref, tc.H4, tc.NB_TOCABI, "emulation, three flags in instance 1", w_bar=tc.BAR_W_EMU)
    keep = [0, 2]
    alone = et.run(mo, cases.CONTACTS_4, tc.H4, q[keep], fl[keep])
    for k in tc.NAMES:
        for a, b in zip(alone[k], got[k]):
            assert (a == b[keep]).all(), k
    # J_task alone: the failed instance is zero there too, nothing else is written
    one = et.run(mo, cases.CONTACTS_4, tc.H4, q, fl, outputs=("J_task",))
    assert one["status"].tolist() == [1, 0, 1] and not any(a[1].any() for a in one["J_task"]) and all(np.isnan(a).all() for a in one["J_kt"])
    # the status alone: it says the same, and no output buffer is touched
    none = et.run(mo, cases.CONTACTS_4, tc.H4, q, fl, outputs=())
    assert none["status"].tolist() == [1, 0, 1] and all(np.isnan(a).all() for k in tc.NAMES for a in none[k])


@pytest.mark.parametrize("n", sorted(LDS_BYTES))
def test_lds_bytes_are_the_documented_ones(n):
    assert et.lds_bytes(n) == LDS_BYTES[n]
