"""Restatement references of the gravity-compensation tests (tests/test_gravcomp_*.py), computed once per state set and left unchanged.

The reference is the oracle's call sequence update_kinematics, set_contact, calc_contact_constraint, calc_grav, contact_force(tau_grav)
(reference src/wbd.cpp:186-192, 268-271).  The state sets are the redistribution tests' own (tests/redist_cases.py, tests/redist_pack_cases.py):
with the option on, the kernel is fed torque_input = ref["tau_in"] - torque_grav_(restatement), so that the torque it redistributes is
ref["tau_in"] and redist_cases.compare applies to its outputs as it stands.  Bars: redist_cases' (1e-6 Nm, 1e-5 N), status identical."""
import functools

import numpy as np

from tests import redist_cases as rc
from tests import redist_pack_cases as pc

MIN_GRAV = 10.0  # Nm: premise -- |torque_grav_| exceeds this in some joint of every instance with a contact (measured: 34 - 126 Nm)


def grav_ref(cyc, q, flags):
    """(status, torque_grav_, getContactForce(torque_grav_) padded to 12) of one instance"""
    m = cyc.m
    w = np.zeros(12)
    if not any(flags):
        return 1, np.zeros(m), w
    cyc.update_kinematics(q)
    cyc.set_contact([bool(f) for f in flags])
    ok = cyc.calc_contact_constraint()
    tg = cyc.calc_grav().copy()
    w[: cyc.cdof] = cyc.contact_force(tg)
    return int(bool(ok)), tg, w


def _grav_of(cyc, q, flags):
    B = len(q)
    out = dict(status=np.zeros(B, np.int32), tau=np.zeros((B, cyc.m)), wrench=np.zeros((B, 12)))
    for b in range(B):
        out["status"][b], out["tau"][b], out["wrench"][b] = grav_ref(cyc, q[b], flags[b])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tocabi_grav(B, yaw, mode, free_every=0):
    """restatement of the gravity-only launch on redist_cases.state_set(B, yaw, mode); free_every = 3: every third instance in the air
    (the flags come back with it)"""
    ref = rc.state_set(B, yaw, mode)
    flags = ref["flags"].copy()
    if free_every:
        flags[::free_every] = 0
    out = dict(_grav_of(rc._cycle(), ref["q"], flags), flags=flags)
    out["flags"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pack_grav(name, B):
    """restatement of the gravity-only launch on redist_pack_cases.state_set(name, B)"""
    ref = pc.state_set(name, B)
    mo, links = pc.model(name)
    return _grav_of(pc.cycle_of(mo, links), ref["q"], ref["flags"])


def check_grav_premise(g, flags):
    """the comparison cannot pass idle: torque_grav_ is tens of Nm wherever there is a contact, and the restatement solved those"""
    on = np.asarray(flags).sum(axis=1) > 0
    assert on.sum() >= 0.5 * len(on)
    assert (g["status"][on] == 1).all()
    big = np.abs(g["tau"][on]).max(axis=1)
    assert big.min() > MIN_GRAV, big.min()


def compare_grav(got, g):
    """status identical everywhere; torque and wrench on the instances the restatement solved.  Returns (worst |d tau|, worst |d wrench|)."""
    assert (got["status"] == g["status"]).all(), np.nonzero(got["status"] != g["status"])[0]
    okm = g["status"] == 1
    e_tau = float(np.abs(got["tau"][okm] - g["tau"][okm]).max())
    e_wr = float(np.abs(got["wrench"][okm] - g["wrench"][okm]).max())
    print(f"gravity: worst |d tau| = {e_tau:.3e} Nm, worst |d wrench| = {e_wr:.3e} N over {int(okm.sum())} instances")
    assert e_tau <= rc.TOL_TAU, e_tau
    assert e_wr <= rc.TOL_WRENCH, e_wr
    return e_tau, e_wr


def check_free_instances(got, flags):
    """no contact: exact zeros and status 1"""
    free = np.asarray(flags).sum(axis=1) == 0
    assert free.sum() >= 1
    assert (got["status"][free] == 1).all()
    assert np.abs(got["tau"][free]).max() == 0.0 and np.abs(got["wrench"][free]).max() == 0.0


def check_vertical_force(got, flags, total_mass):
    """needs no restatement: wherever there is a contact the vertical contact forces of getContactForce(torque_grav_) carry the weight
    (wrench rows are [f; m] per contact, and the sign is the reference's: P_C enters with a minus, src/wbd.cpp:268-271)"""
    on = np.asarray(flags).sum(axis=1) > 0
    fz = got["wrench"][:, 2] + got["wrench"][:, 8]
    e = float(np.abs(fz[on] + 9.81 * total_mass).max())
    print(f"gravity: worst |sum f_z + 9.81 m| = {e:.3e} N (m = {total_mass:.3f} kg)")
    assert e <= rc.TOL_WRENCH, e
    return e
