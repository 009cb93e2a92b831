"""Cases of the two-wave kernel's request phase (libdwbc_amd/csrc/dwbc_cycle2p.h: the contact flags of an instance, q, f* and the
lane's model record are requested at the top of the kernel): one, two and three declared contacts (feet, feet + left hand) and every
flag pattern of each on a handful of yawed states -- three flags raised on this two-contact kernel among them, which it answers
with status 0 and zero outputs.  The reference is the oracle, computed once per number of declared contacts and shared read-only
by tests/test_pair_prologue_emu.py and tests/test_pair_prologue_gpu.py."""
import functools
import itertools

import numpy as np

from tests import cases

TOL, WTOL = 1e-6, 1e-5  # |d tau|, |d wrench| against the oracle: the bar of tests/test_launch_flavours.py for this kernel
DECLARED = (1, 2, 3)
NSTATES = 5
MAX_ACTIVE = 2  # kMaxActiveContacts of the product kernels


def patterns(n):
    return np.array(list(itertools.product((0, 1), repeat=n)), np.uint8)


@functools.lru_cache(maxsize=None)
def states():
    q, _, fstar = cases.synth_batch(NSTATES, seed=20261020, yaw=True)
    q.setflags(write=False)
    fstar.setflags(write=False)
    return q, fstar


@functools.lru_cache(maxsize=None)
def reference(n):
    """the oracle on every (pattern, state) of n declared contacts: tau (P, NSTATES, 3, m), wrench (P, NSTATES, 6 n), status (P, NSTATES)"""
    from oracle import orc

    q, fstar = states()
    pat = patterns(n)
    P = len(pat)
    M = orc.make_model(cases.tocabi_model())
    S = orc.make_setup(cases.CONTACTS_4[:n], cases.TASKS_2LEVEL, cases.TAU_LIM)
    tau, wr, st, _ = orc.cycle_batch(M, S, np.tile(q, (P, 1)), np.repeat(pat, NSTATES, axis=0), np.tile(fstar, (P, 1)), 0)
    ref = dict(tau=tau.reshape((P, NSTATES) + tau.shape[1:]), wrench=wr.reshape(P, NSTATES, -1), status=st.reshape(P, NSTATES))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def check(label, n, pi, si, tau, wrench, status):
    """instance i ran pattern pi[i] of n declared contacts on state si[i]"""
    ref = reference(n)
    pi, si = np.asarray(pi), np.asarray(si)
    many = patterns(n)[pi].sum(axis=1) > MAX_ACTIVE
    tau_r, wr_r, st_r = ref["tau"][pi, si], ref["wrench"][pi, si], ref["status"][pi, si]
    assert (st_r[~many] == 1).all(), (label, st_r)  # the oracle solves every case that is compared
    w = min(6 * MAX_ACTIVE, 6 * n)
    dt = float(np.abs(tau[~many] - tau_r[~many]).max()) if (~many).any() else 0.0
    dw = float(np.abs(wrench[~many][:, :w] - wr_r[~many][:, :w]).max()) if (~many).any() else 0.0
    print(f"{label}: instances {len(pi)} (refused {int(many.sum())})  max|dtau| {dt:.3e}  max|dwrench| {dw:.3e}")
    assert np.isfinite(tau).all() and np.isfinite(wrench).all(), label
    assert (status[~many] == 1).all() and (status[many] == 0).all(), (label, status)
    assert dt < TOL and dw < WTOL, (label, dt, dw)
    assert np.abs(tau[many]).max(initial=0.0) == 0.0 and np.abs(wrench[many]).max(initial=0.0) == 0.0, label
    assert np.abs(tau[~many]).max(initial=1.0) > 0.5, label  # (torques of tens of Nm: the comparison is not between zeros)
