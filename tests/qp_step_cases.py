"""Batches for the active-set step tests (tests/test_qp_step_emu.py, tests/test_qp_step_gpu.py): the smallest batch that still holds
every class of path the wave QP solver takes on the bench's states, with the oracle's answer and its step counts, computed once.

"paths": 64 instances of synth_batch(1024, seed = 20251226 + 2) -- the states `bench.py` runs -- chosen by the oracle's own step counts:
    level 0 takes 7, 9 or 11 steps (9 and 11: a row is added and dropped again), level 1 takes 4, 5 or 6.  Of every one of the six
    classes the first PER_CLASS instances are taken (all of a class that has fewer in this seed), the rest is filled up in index order.
"tilted": 32 states with a rolled / pitched / yawed base: feet tilted against the ground, where the second projection of the step
    ("twice is enough") is taken.
"gc": feet + left hand through the general-contact kernel (18 variables, slot lanes 32..49), the shape of its smallest emulation test."""
import functools

import numpy as np

from oracle import orc
from tests import cases

SEED = 20251226 + 2
PER_CLASS = 4
L0_STEPS, L1_STEPS = (7, 9, 11), (4, 5, 6)


def oracle_batch(q, fl, fs, contacts=cases.CONTACTS_2, tasks=cases.TASKS_2LEVEL, lim=cases.TAU_LIM):
    """every instance through the C restatement, one by one: tau (B, 3, m), wrench, status and the steps of every QP (B, levels + 1:
    the task levels, then the redistribution)"""
    M = orc.make_model(cases.tocabi_model())
    S = orc.make_setup(contacts, tasks, lim)
    tau, wr, st, _ = orc.cycle_batch(M, S, q, fl, fs, 0)
    nl = len(tasks)
    dofs = [sum(6 if mode == 0 else 3 for mode, _, _ in links) for links in tasks]
    offs = np.concatenate([[0], np.cumsum(dofs)])
    steps = np.zeros((len(q), nl + 1), np.int32)
    for i in range(len(q)):
        out, _ = orc.cycle(M, S, q[i], fl[i], [fs[i, offs[l] : offs[l + 1]] for l in range(nl)])
        steps[i] = [out.qp_iter[l] for l in range(nl + 1)]
    return dict(tau=tau, wrench=wr, status=st, steps=steps)


@functools.lru_cache(maxsize=None)
def paths_batch():
    q, fl, fs = cases.synth_batch(1024, seed=SEED)
    full = oracle_batch(q, fl, fs)
    s0, s1 = full["steps"][:, 0], full["steps"][:, 1]
    assert set(np.unique(s0)) == set(L0_STEPS) and set(np.unique(s1)) == set(L1_STEPS), (np.unique(s0), np.unique(s1))
    pick = []
    for col, counts in ((s0, L0_STEPS), (s1, L1_STEPS)):
        for c in counts:
            pick += list(np.flatnonzero(col == c)[:PER_CLASS])
    pick = sorted(set(int(i) for i in pick))
    pick = sorted(pick + [i for i in range(1024) if i not in pick][: 64 - len(pick)])
    idx = np.array(pick)
    assert len(idx) == 64
    for col, counts in ((s0, L0_STEPS), (s1, L1_STEPS)):
        for c in counts:
            assert (col[idx] == c).sum() >= min(PER_CLASS, (col == c).sum()) > 0, (c, (col == c).sum())
    ref = {k: v[idx].copy() for k, v in full.items()}
    for v in (q, fl, fs, *ref.values()):
        v.setflags(write=False)
    return (q[idx], fl[idx], fs[idx]), ref, {"level0": {c: int((s0 == c).sum()) for c in L0_STEPS}, "level1": {c: int((s1 == c).sum()) for c in L1_STEPS}}


@functools.lru_cache(maxsize=None)
def tilted_batch():
    q, fl, fs = cases.synth_batch(32, seed=SEED, yaw=True)
    return (q, fl, fs), oracle_batch(q, fl, fs)


GC_FLAGS = [1, 1, 1, 0]  # both feet and the left hand


@functools.lru_cache(maxsize=None)
def gc_batch(B):
    q, _, fs = cases.synth_batch(B, seed=11, yaw=True)
    fl = np.tile(np.array(GC_FLAGS, np.uint8), (B, 1))
    return (q, fl, fs), oracle_batch(q, fl, fs, contacts=cases.CONTACTS_4)


def check(name, got, ref, ncols=12, tol_tau=1e-6, tol_wr=1e-5):
    """tau, wrench and status against the oracle at the tolerances of tests/test_gpu_parity.py for this kernel, and the steps of every QP
    (diag: DG_QP_ITER at 4, the redistribution in slot kMaxLevels = 4) against the oracle's"""
    st, ok = got["status"], ref["status"] == 1
    nl = ref["steps"].shape[1] - 1
    steps = np.concatenate([got["diag"][:, 4 : 4 + nl], got["diag"][:, 8:9]], axis=1)
    dt = float(np.abs(got["tau"][ok] - ref["tau"][ok]).max())
    dw = float(np.abs(got["wrench"][ok][:, :ncols] - ref["wrench"][ok][:, :ncols]).max())
    ds = int((steps[ok] != ref["steps"][ok]).any(axis=1).sum())
    print(f"{name}: ok {int(ok.sum())}/{len(ok)} max|dtau| {dt:.3e} max|dwrench| {dw:.3e} instances with other step counts {ds}")
    assert (st == ref["status"]).all()
    assert dt < tol_tau and dw < tol_wr
    assert ds == 0, (steps[ok][(steps[ok] != ref["steps"][ok]).any(axis=1)], ref["steps"][ok][(steps[ok] != ref["steps"][ok]).any(axis=1)])
