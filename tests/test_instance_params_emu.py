"""not-gpu: per-instance torque limits and contact cone constants (BatchIO::inst_par) in host emulation of the one-wave cycle and of the
redistribution kernel (tests/emu/emu_cycle.cpp: one "thread" per workgroup, LDS NaN-poisoned before every instance) against the
restatement with one set-up per instance.

Inputs and bars: tests/inst_par_cases.py (states of synth_batch seed 7, yaw, mixed support; limits TAU_LIM * U(0.15, 0.5), contact
constants times U(0.4, 1.0)); 1e-6 Nm, 1e-5 N, status identical.  Every comparison first asserts on the reference alone that it solves
at least 90 % of the instances and that the record moves at least half of them by more than 1e-3 Nm."""
import numpy as np
import pytest

from tests import cases
from tests import inst_par_cases as ic
from tests import redist_cases as rc
from tests.emu.emu import Emu

B = 48


@pytest.fixture(scope="module")
def emu():
    return Emu(cases.URDF, cases.CONTACTS_2, cases.TASKS_2LEVEL, cases.TAU_LIM)


@pytest.mark.parametrize("compact", [False, True], ids=["extras", "compact_lean"])
@pytest.mark.parametrize("lim,con", [(True, False), (False, True), (True, True)], ids=["limits", "contacts", "both"])
def test_cycle_matches_restatement(emu, lim, con, compact):
    q, flags, fstar = ic.states(B)
    ref = ic.reference(B, lim, con)
    ic.check_premises(ref, ic.reference(B, False, False), f"lim={lim} con={con}")
    got = emu.run(q, flags, fstar, inst_par=ic.record(B, ic.limits(B) if lim else None, ic.contact_consts(B) if con else None), compact=compact)
    ic.compare(got["tau"], got["wrench"], got["status"], ref, f"lim={lim} con={con} compact={compact}")


def test_record_without_a_batch_wide_limit(emu):
    """the torque rows exist exactly as after SetTorqueLimit: a set-up that never had a limit gives the same bits under the same record"""
    q, flags, fstar = ic.states(B)
    rec = ic.record(B, ic.limits(B), ic.contact_consts(B))
    nolim = Emu(cases.URDF, cases.CONTACTS_2, cases.TASKS_2LEVEL, None)
    a, b = emu.run(q, flags, fstar, inst_par=rec), nolim.run(q, flags, fstar, inst_par=rec)
    for k in ("tau", "wrench", "status"):
        assert (a[k] == b[k]).all(), k
    ra, rb = emu.run_redist(q, flags, rc.state_set(B, True, "mixed")["tau_in"], rec), nolim.run_redist(q, flags, rc.state_set(B, True, "mixed")["tau_in"], rec)
    for k in ("tau", "cf", "wrench", "status"):
        assert (ra[k] == rb[k]).all(), k


@pytest.mark.parametrize("compact", [False, True], ids=["extras", "compact_lean"])
def test_batch_wide_record_is_bit_equal_to_none(emu, compact):
    q, flags, fstar = ic.states(B)
    plain = emu.run(q, flags, fstar, inst_par=None, compact=compact)
    same = emu.run(q, flags, fstar, inst_par=ic.record(B, None, None), compact=compact)
    assert (plain["status"] == 1).mean() >= 0.9
    for k in ("tau", "wrench", "status"):
        assert (plain[k] == same[k]).all(), k


def test_redistribution_matches_restatement(emu):
    ref = ic.redist_reference(B)
    rc.check_premises(ref)
    ic.redist_moved(ref)
    got = emu.run_redist(ref["q"], ref["flags"], ref["tau_in"], ic.record(B, None, ref["con"]))
    rc.compare(got, ref)


def test_redistribution_batch_wide_record_is_bit_equal_to_none(emu):
    base = rc.state_set(B, True, "mixed")
    plain = emu.run_redist(base["q"], base["flags"], base["tau_in"], None)
    same = emu.run_redist(base["q"], base["flags"], base["tau_in"], ic.record(B, None, None))
    for k in ("tau", "cf", "wrench", "status"):
        assert (plain[k] == same[k]).all(), k
    rc.compare(plain, base)
