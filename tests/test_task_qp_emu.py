"""not-gpu: the single-level task-QP kernel (libdwbc_amd/csrc/dwbc_task_qp.h) in host emulation (tests/emu/emu_task_qp.cpp: one "thread" per
workgroup, LDS of exactly LdsTq<N, NB>::total doubles NaN-poisoned before every instance, a guard behind it, every output buffer pre-filled
with NaN / -1) against the numpy restatement, on TOCABI's constant tree and on TopoGeneric: sets P (B = 12), Q, F and S3 on every level of
their hierarchies, a no-contact support and a set-up without torque limit, a level on the COM link, per-instance torque limits, three
flags, and the mask tiers.

Inputs, references, premises and bars: tests/task_qp_cases.py.  A numeric comparison leaves out only instances whose restatement status is 0
(tests/task_qp_cases.compare asserts exact zeros there); each test asserts how many those were."""
import numpy as np
import pytest

from tests import cases
from tests import task_qp_cases as qc
from tests.emu import emu_task_qp as eq

BARS = qc.bars(qc.MEASURED_EMU)
# LdsTq<N, NB>::total_bytes as the header and DESIGN.md list them
LDS_BYTES = {23: 24048, 37: 36144, 39: 37872, 43: 52280, 50: 64032}
TIERS = [(), ("f_star_qp",), ("contact_qp", "torque_contact"), ("torque_h",), ("torque_null_h", "f_star_qp"), ("torque_contact",)]
trees = pytest.mark.parametrize("tree", [True, False], ids=["tocabi_tree", "generic_tree"])


def _run(s, level, lv, tree, **kw):
    return eq.run(cases.tocabi_model(), s["contacts"], s["tasks"], s["q"], s["flags"], s["fstar"], level, lv["torque_prev"], lv["null"],
                  tau_lim=kw.pop("tau_lim", s["tau_lim"]), tree=tree, **kw)


def _chain(s, tree, what, **kw):
    """every level of the set with the restatement's chained inputs; returns the instances left out per level"""
    left = []
    for l, lv in enumerate(s["levels"]):
        got = _run(s, l, lv, tree, **kw)
        left.append(qc.compare(got, lv["ref"], BARS, f"emulation, {what}, level {l}, " + ("constant tree" if tree else "generic tree"))[1])
    return left


@pytest.mark.parametrize("yaw", [False, True])
@pytest.mark.parametrize("B", [12, 130])
def test_premises_P(B, yaw):
    qc.check_premises_P(B, yaw)


@pytest.mark.parametrize("yaw", [False, True])
def test_premises_Q(yaw):
    qc.check_premises_Q(yaw)


def test_premises_F_S3_and_instance_limits():
    qc.check_premises_F()
    qc.check_premises_S3()
    qc.check_premises_inst_lim()


def test_bars_are_ten_times_the_measured_figures():
    assert BARS["f_star_qp"] == pytest.approx(6.3e-11) and BARS["contact_qp"] == pytest.approx(4.9e-8)
    assert all(BARS[k] == 1e-6 for k in qc.TORQUES)


@trees
@pytest.mark.parametrize("yaw", [False, True])
def test_P_every_level(yaw, tree):
    assert _chain(qc.set_P(12, yaw), tree, f"P B=12 yaw={yaw}") == [0, 0, 0, 0]


@trees
@pytest.mark.parametrize("yaw", [False, True])
def test_Q_a_level_beneath_a_foreign_torque(yaw, tree):
    s, r = qc.set_P(130, yaw), qc.set_Q(130, yaw)
    got = _run(s, r["level"], r, tree)
    assert qc.compare(got, r["ref"], BARS, f"emulation, Q yaw={yaw}")[1] == 0


@trees
def test_F_failure_is_status_zero_and_exact_zeros(tree):
    s, r = qc.set_P(12, True), qc.set_F()
    got = _run(s, r["level"], r, tree)
    assert (got["status"] == 0).all()
    assert qc.compare(got, r["ref"], BARS, "emulation, F")[1] == 12  # (every instance: compare asserts exact zeros on them)
    for k in qc.NAMES:
        assert not got[k].any(), k


@trees
def test_S3_single_support_has_no_contact_variables(tree):
    s = qc.set_S3()
    assert _chain(s, tree, "S3") == [0, 0, 0]
    for l, lv in enumerate(s["levels"]):
        got = _run(s, l, lv, tree)
        assert not got["contact_qp"].any() and not got["torque_contact"].any(), l


@trees
@pytest.mark.parametrize("kind", ["free", "free_nolim", "nolim"])
def test_supports_and_setups_without_rows(kind, tree):
    s = qc.set_variant(kind)
    assert _chain(s, tree, kind) == [0, 0, 0, 0]
    if kind == "free_nolim":  # no rows at all: x = 0, status 1
        for l, lv in enumerate(s["levels"]):
            got = _run(s, l, lv, tree)
            assert (got["status"] == 1).all() and not got["f_star_qp"].any() and not got["contact_qp"].any() and (lv["ref"]["nact"] == 0).all(), l


@trees
def test_a_level_on_the_com_link(tree):
    s = qc.set_HCOM()
    assert all((lv["ref"]["status"] == 1).all() for lv in s["levels"])
    assert set(s["flags"].sum(axis=1).tolist()) == {1, 2}
    assert _chain(s, tree, "HCOM") == [0, 0, 0, 0]


@trees
def test_per_instance_torque_limits(tree):
    s = qc.set_inst_lim()
    left = _chain(s, tree, "per-instance limits", tau_lim=None, inst_par=qc.inst_par_record(s))
    assert left == [int((lv["ref"]["status"] == 0).sum()) for lv in s["levels"]]
    # the record takes the place of a batch-wide limit that is set as well
    for l, lv in enumerate(s["levels"]):
        a = _run(s, l, lv, tree, tau_lim=None, inst_par=qc.inst_par_record(s))
        b = _run(s, l, lv, tree, inst_par=qc.inst_par_record(s))
        for k in qc.NAMES + ("status",):
            assert (a[k] == b[k]).all(), (l, k)


def test_outputs_not_asked_for_stay_nan():
    s = qc.set_P(12, True)
    for l in (0, 2):
        lv = s["levels"][l]
        full = _run(s, l, lv, True)
        for names in TIERS:
            got = _run(s, l, lv, True, outputs=names)
            assert (got["status"] == full["status"]).all(), names
            for k in qc.NAMES:
                if k in names:
                    assert (got[k] == full[k]).all(), (names, k)
                else:
                    assert np.isnan(got[k]).all(), (names, k)


def test_generic_tree_agrees_with_the_constant_tree_on_tocabi():
    s = qc.set_P(12, True)
    for l, lv in enumerate(s["levels"]):
        t, g = _run(s, l, lv, True), _run(s, l, lv, False)
        for k in qc.NAMES:
            assert (t[k] == g[k]).all(), (l, k)


def test_three_flags_fail_the_instance_and_leave_its_neighbours_alone():
    s = qc.set_P(12, True)
    q, fstar = s["q"][:3], s["fstar"][:3]
    fl = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    mo = cases.tocabi_model()
    ref = qc.chain_reference(mo, cases.CONTACTS_4, s["tasks"], q, fl, fstar, s["tau_lim"])["levels"][0]
    got = eq.run(mo, cases.CONTACTS_4, s["tasks"], q, fl, fstar, 0, ref["torque_prev"], None, tau_lim=s["tau_lim"])
    assert got["status"].tolist() == [1, 0, 1]
    assert qc.compare(got, ref["ref"], BARS, "emulation, three flags in instance 1")[1] == 1
    keep = [0, 2]
    alone = eq.run(mo, cases.CONTACTS_4, s["tasks"], q[keep], fl[keep], fstar[keep], 0, ref["torque_prev"][keep], None, tau_lim=s["tau_lim"])
    for k in qc.NAMES:
        assert (alone[k] == got[k][keep]).all(), k


@pytest.mark.parametrize("n", sorted(LDS_BYTES))
def test_lds_bytes_are_the_documented_ones(n):
    assert eq.lds_bytes(n) == LDS_BYTES[n]


def test_one_live_level_fits_the_task_space_kernels_map():
    from tests.emu import emu_task_space as et

    assert eq.lds_bytes(39) <= et.lds_bytes(39) == 38656
