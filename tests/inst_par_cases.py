"""Inputs and restatement references of the per-instance parameter tests (tests/test_instance_params_*.py), computed once.

States: `cases.synth_batch(B, seed=7, yaw=True, contact_mode="mixed")` with TASKS_2LEVEL on CONTACTS_2.  Per-instance torque limits:
TAU_LIM * U(0.15, 0.5) per joint from default_rng(29); per-instance contact constants: the batch-wide lx, ly, mu, mu_z times U(0.4, 1.0)
from default_rng(23).  The reference is the C restatement (oracle.orc) with one set-up per instance; the record layout is the
library's: [tau_lim[m] | lx ly mu muz of every registered contact]."""
import functools

import numpy as np

from tests import cases

TOL_TAU = 1e-6     # Nm: the project's bars against the restatement
TOL_WRENCH = 1e-5  # N
MOVED = 1e-3       # Nm: an instance whose torque differs from the batch-wide answer by more than this was moved by its record


def consts(contacts):
    """(n_contacts, 4): lx, ly, mu, mu_z as registered"""
    return np.array([[c["lx"], c["ly"], c.get("mu", 0.2), c.get("muz", 0.2)] for c in contacts], float)


@functools.lru_cache(maxsize=None)
def states(B):
    out = cases.synth_batch(B, seed=7, yaw=True, contact_mode="mixed")
    for a in out:
        a.setflags(write=False)
    return out


def limits(B, m=33):
    v = np.asarray(cases.TAU_LIM, float)[:m] * np.random.default_rng(29).uniform(0.15, 0.5, size=(B, m))
    v.setflags(write=False)
    return v


def contact_consts(B, contacts=cases.CONTACTS_2):
    v = consts(contacts) * np.random.default_rng(23).uniform(0.4, 1.0, size=(B, len(contacts), 4))
    v.setflags(write=False)
    return v


def record(B, lim, con, contacts=cases.CONTACTS_2, tau_lim=cases.TAU_LIM):
    """(B, m + 4 n_contacts): the halves given, the others the batch-wide values"""
    m = len(tau_lim)
    lim_ = np.broadcast_to(np.asarray(tau_lim, float), (B, m)) if lim is None else lim
    con_ = np.broadcast_to(consts(contacts), (B, len(contacts), 4)) if con is None else con
    return np.ascontiguousarray(np.concatenate([lim_, con_.reshape(B, -1)], axis=1))


def with_consts(contacts, con_i):
    return [dict(c, lx=v[0], ly=v[1], mu=v[2], muz=v[3]) for c, v in zip(contacts, con_i)]


def orc_reference(q, flags, fstar, lim, con, contacts=cases.CONTACTS_2, tasks=cases.TASKS_2LEVEL, tau_lim=cases.TAU_LIM, model=None):
    """(tau (B, 3, m), wrench (B, 6 n_contacts), status) of the C restatement, one set-up per instance; lim / con None: batch-wide"""
    from oracle import orc

    M = orc.make_model(cases.tocabi_model() if model is None else model)
    B = len(q)
    if lim is None and con is None:
        return orc.cycle_batch(M, orc.make_setup(contacts, tasks, tau_lim), q, flags, fstar, 0)[:3]
    outs = []
    for i in range(B):
        S = orc.make_setup(contacts if con is None else with_consts(contacts, con[i]), tasks, tau_lim if lim is None else lim[i])
        outs.append(orc.cycle_batch(M, S, q[i : i + 1], flags[i : i + 1], fstar[i : i + 1], 1)[:3])
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(3))


@functools.lru_cache(maxsize=None)
def reference(B, lim, con):
    """lim / con: booleans -- which halves are randomised.  Read-only arrays."""
    q, flags, fstar = states(B)
    out = orc_reference(q, flags, fstar, limits(B) if lim else None, contact_consts(B) if con else None)
    for a in out:
        a.setflags(write=False)
    return out


def check_premises(ref, base, what=""):
    """what every comparison asserts on the reference alone first: the restatement solves the instances, and the record moves them"""
    st = ref[2]
    B = len(st)
    assert (st == 1).sum() >= 0.9 * B, f"{what}: restatement status 1 on {(st == 1).sum()} of {B}"
    moved = np.abs(ref[0].sum(axis=1) - base[0].sum(axis=1)).max(axis=1) > MOVED
    print(f"{what}: status 1 on {(st == 1).sum()} of {B}, moved by more than {MOVED} Nm: {moved.sum()} of {B}")
    assert moved.sum() >= 0.5 * B, f"{what}: only {moved.sum()} of {B} instances differ from the batch-wide answer"


def compare(got_tau, got_wr, got_st, ref, what=""):
    tau_r, wr_r, st_r = ref
    assert (got_st == st_r).all(), (what, np.nonzero(got_st != st_r)[0])
    ok = st_r == 1
    e_tau = float(np.abs(got_tau[ok] - tau_r[ok]).max())
    e_wr = float(np.abs(got_wr[ok] - wr_r[ok]).max())
    print(f"{what}: worst |d tau| = {e_tau:.3e} Nm, worst |d wrench| = {e_wr:.3e} N over {int(ok.sum())} instances")
    assert np.isfinite(got_tau).all(), what
    assert e_tau <= TOL_TAU, (what, e_tau)
    assert e_wr <= TOL_WRENCH, (what, e_wr)


# ---- the redistribution of a supplied torque: the recipe of tests/redist_cases.py, contact constants per instance
@functools.lru_cache(maxsize=None)
def redist_reference(B, yaw=True, mode="mixed"):
    """dict like redist_cases.state_set: the numpy restatement's redistribution with instance i's contact constants.  tau_in is built as
    redist_cases builds it -- the cycle's torque pushed along the contact null space by NwJw d, d = 10 N(0, I6) from default_rng(11) --
    with the cycle run under the instance's own constants.  (The batch-wide cycle's torque leaves the narrower cones of most instances
    by more than the six contact-null variables can mend: the restatement fails 122 of 127 double-support instances at B = 250, and a
    comparison over the rest would be idle.)"""
    from tests import redist_cases as rc

    base = rc.state_set(B, yaw, mode)
    assert yaw and mode == "mixed" and (base["q"] == states(B)[0]).all()
    con = contact_consts(B)
    tau_in = reference(B, False, True)[0].sum(axis=1) + (base["tau_in"] - base["tau_feasible"])  # (NwJw does not depend on the constants)
    cyc = rc._cycle()
    m = cyc.m
    out = dict(q=base["q"], flags=base["flags"], tau_in=tau_in, status=np.zeros(B, np.int32), tau=np.zeros((B, m)), cf=np.zeros((B, 6)),
               wrench=np.zeros((B, 2, 12)), nwjw=np.zeros((B, m, 6)), con=con)
    for b in range(B):
        for cc, v in zip(cyc.contacts, con[b]):
            cc["lx"], cc["ly"], cc["mu"], cc["muz"] = v
        st, dt, c, w, nw = rc.redistribute_ref(cyc, base["q"][b], base["flags"][b], tau_in[b])
        out["status"][b], out["tau"][b], out["cf"][b], out["wrench"][b] = st, dt, c, w
        out["nwjw"][b, :, : nw.shape[1]] = nw
    for v in out.values():
        v.setflags(write=False)
    return out


def redist_moved(ref):
    """the record moves the redistribution: against the batch-wide constants on the same inputs, at least half the double-support
    instances differ by more than MOVED (asserted on the restatement alone)"""
    from tests import redist_cases as rc

    cyc = rc._cycle()
    double = np.nonzero(ref["flags"].sum(axis=1) == 2)[0]
    moved = sum(np.abs(rc.redistribute_ref(cyc, ref["q"][b], ref["flags"][b], ref["tau_in"][b])[1] - ref["tau"][b]).max() > MOVED for b in double)
    print(f"redistribution: moved by more than {MOVED} Nm: {moved} of {len(double)} double-support instances")
    assert moved >= 0.5 * len(double), (moved, len(double))
