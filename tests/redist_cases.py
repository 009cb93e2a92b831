"""Inputs and restatement references of the redistribution tests (tests/test_redistribute_*.py), computed once per state set.

A state set is `cases.synth_batch(B, seed=7, yaw=.., contact_mode=..)`.  tau_feasible is the restatement's full-cycle torque for
TASKS_2LEVEL with TAU_LIM; tau_in = tau_feasible + NwJw d with d = s N(0, I6) from default_rng(11) pushes the contact wrenches out of
their cones along the contact null space, so the redistribution QP has work to do (s = 10) or none (s = 0).  The reference follows the
oracle's call sequence: update_kinematics, set_contact, calc_contact_constraint, calc_grav, then tau_grav = tau_in,
tau_task = tau_contact = 0 and calc_contact_redistribute(); contact_force(tau) gives the wrenches."""
import functools

import numpy as np

from tests import cases

TOL_TAU = 1e-6     # Nm: the project's bar of the cycle kernels against the restatement
TOL_WRENCH = 1e-5  # N


def _cycle():
    from oracle.dwbc_np import Cycle

    cyc = Cycle(cases.tocabi_model())
    for c in cases.CONTACTS_2:
        cyc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(cases.TASKS_2LEVEL):
        for mode, link, pt in links:
            cyc.add_task(lv, mode, link, pt)
    cyc.set_torque_limit(cases.TAU_LIM)
    return cyc


def redistribute_ref(cyc, q, flags, tau_in):
    """(status, NwJw c, c padded to 6, [wrench(tau_in), wrench(tau_in + NwJw c)] padded to 12, NwJw) of one instance"""
    m = cyc.m
    out_w = np.zeros((2, 12))
    if not any(flags):
        return 1, np.zeros(m), np.zeros(6), out_w, np.zeros((m, 0))
    cyc.update_kinematics(q)
    cyc.set_contact([bool(f) for f in flags])
    ok = cyc.calc_contact_constraint()
    cyc.calc_grav()
    cyc.tau_grav = np.asarray(tau_in, float).copy()
    cyc.tau_task = np.zeros(m)
    cyc.tau_contact = np.zeros(m)
    cyc.cf_redis = np.zeros(max(cyc.cdof - 6, 0))
    st = int(bool(ok) and bool(cyc.calc_contact_redistribute()))
    dt = cyc.tau_contact.copy() if st else np.zeros(m)
    c = np.zeros(6)
    if st:
        c[: len(cyc.cf_redis)] = cyc.cf_redis
    out_w[0, : cyc.cdof] = cyc.contact_force(tau_in)
    out_w[1, : cyc.cdof] = cyc.contact_force(tau_in + dt)
    return st, dt, c, out_w, cyc.NwJw.copy()


@functools.lru_cache(maxsize=None)
def state_set(B, yaw, mode, scale=10.0):
    """dict(q, flags, tau_feasible, tau_in, status, tau, cf, wrench, nwjw): inputs and the restatement's answers; read-only arrays"""
    q, flags, fstar = cases.synth_batch(B, seed=7, yaw=yaw, contact_mode=mode)
    d = scale * np.random.default_rng(11).standard_normal((B, 6))
    cyc = _cycle()
    m = cyc.m
    out = dict(q=q, flags=flags, tau_feasible=np.zeros((B, m)), tau_in=np.zeros((B, m)), status=np.zeros(B, np.int32), tau=np.zeros((B, m)),
               cf=np.zeros((B, 6)), wrench=np.zeros((B, 2, 12)), nwjw=np.zeros((B, m, 6)))
    for b in range(B):
        tf = cyc.run(q[b], [bool(f) for f in flags[b]], [fstar[b, :6], fstar[b, 6:9]])
        out["tau_feasible"][b] = tf
        out["tau_in"][b] = tf + (cyc.NwJw @ d[b] if cyc.NwJw.shape[1] == 6 else 0.0)
        st, dt, c, w, nw = redistribute_ref(cyc, q[b], flags[b], out["tau_in"][b])
        out["status"][b], out["tau"][b], out["cf"][b], out["wrench"][b] = st, dt, c, w
        out["nwjw"][b, :, : nw.shape[1]] = nw
    for v in out.values():
        v.setflags(write=False)
    return out


def check_premises(ref):
    """the two conditions every comparison asserts on its own inputs first, so that it cannot pass on idle QPs"""
    B = len(ref["status"])
    double = ref["flags"].sum(axis=1) == 2
    assert ref["status"].sum() >= 0.9 * B, f"restatement status 1 on {ref['status'].sum()} of {B}"
    busy = np.linalg.norm(ref["cf"][double], axis=1) > 1e-3
    assert busy.sum() >= 0.5 * double.sum(), f"|c| > 1e-3 on {busy.sum()} of {double.sum()} double-support instances"


def compare(got, ref):
    """status identical everywhere; torque, c (through NwJw) and both wrench rows on the instances the restatement solved.
    Returns (worst |d tau|, worst |d wrench|)."""
    assert (got["status"] == ref["status"]).all(), np.nonzero(got["status"] != ref["status"])[0]
    okm = ref["status"] == 1
    e_tau = float(np.abs(got["tau"][okm] - ref["tau"][okm]).max())
    e_wr = float(np.abs(got["wrench"][okm] - ref["wrench"][okm]).max())
    print(f"worst |d tau| = {e_tau:.3e} Nm, worst |d wrench| = {e_wr:.3e} N over {int(okm.sum())} instances")
    assert e_tau <= TOL_TAU, e_tau
    assert e_wr <= TOL_WRENCH, e_wr
    e_cf = float(np.abs(np.einsum("bij,bj->bi", ref["nwjw"][okm], got["cf"][okm]) - ref["tau"][okm]).max())  # DWBC_REDIST_CF . NwJw: the same torque
    print(f"worst |NwJw cf - tau_ref| = {e_cf:.3e} Nm")
    assert e_cf <= TOL_TAU, e_cf
    return e_tau, e_wr
