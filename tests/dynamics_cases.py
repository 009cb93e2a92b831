"""Inputs, restatement references and bars of the dynamics-launch tests (tests/test_dynamics_emu.py, tests/test_dynamics_gpu.py),
computed once per state set and left unchanged.

States: TOCABI -- cases.synth_batch(B, SEED, yaw=True); the pack models of tests/redist_pack_cases.model -- their own state recipe
(redist_pack_cases.states); the reference's CASE 1 and CASE 2 states for the goldens.  Velocities: default_rng(SEED).uniform(-1, 1, (B, n)).
Reference: the restatement, oracle.dwbc_np.Cycle.update_kinematics (A, A_inv, G, CMM, com) and nonlinear_effects (B).

Bars, all the project's own for these quantities: A 1e-9 and A_inv 1e-8 (tests/test_gpu_parity.py:63-64), G 1e-8 (9.81 x the bar of A's
row 2), B 1e-9 (tests/test_velocity_outputs.py:78), CMM 1e-10 and com 1e-12 (tests/test_gpu_parity.py:234-235).  One bar is not in the
project: the kernel's own max|A A_inv - I|.  It is ten times the restatement's own residual on the same states (RESIDUAL_RESTATEMENT,
measured by check_residual_premise, which the tests run and print first): the kernel's sweep eliminates in another order than the
restatement's LLT, but the conditioning of A is the same.  State sets are named by (model, B): "tocabi", "golden" (the two CASE states),
"fixed_head", "fixed_arms", "surgery_43"."""
import functools

import numpy as np

from tests import cases

SEED = 7
BARS = {"A": 1e-9, "A_inv": 1e-8, "G": 1e-8, "B": 1e-9, "CMM": 1e-10, "com": 1e-12}
NAMES = ("A", "A_inv", "B", "G", "CMM", "com")
# max|A A_inv - I| of the restatement (numpy: LLT inverse, float64 product) on each state set the tests use, measured by
# check_residual_premise and recorded here, rounded up.  The kernel's bar on a set is ten times the figure of that set.  (The reference's own
# dumped A_inv_ at the CASE states has 1.7e-14.)
RESIDUAL_RESTATEMENT = {
    ("tocabi", 4): 2.8e-14, ("tocabi", 8): 2.7e-14, ("golden", 2): 1.9e-14,
    ("fixed_head", 3): 2.5e-14, ("fixed_head", 8): 3.0e-14, ("fixed_arms", 3): 1.5e-14, ("fixed_arms", 8): 1.9e-14,
    ("surgery_43", 3): 9.3e-14, ("surgery_43", 8): 1.4e-13,
}


def bar_residual(key):
    return 10.0 * RESIDUAL_RESTATEMENT[key]


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def reference(mo, q, qd):
    """dict of A (B, n, n), A_inv, B, G (B, n), CMM (B, 6, n), com (B, 3) of the restatement; qd None: B = G"""
    from oracle.dwbc_np import Cycle, nonlinear_effects

    n = mo["ndof"]
    B = len(q)
    cyc = Cycle(mo)
    out = dict(A=np.zeros((B, n, n)), A_inv=np.zeros((B, n, n)), B=np.zeros((B, n)), G=np.zeros((B, n)), CMM=np.zeros((B, 6, n)), com=np.zeros((B, 3)))
    for b in range(B):
        cyc.update_kinematics(q[b])
        out["A"][b], out["A_inv"][b], out["G"][b], out["CMM"][b], out["com"][b] = cyc.A, cyc.A_inv, cyc.G, cyc.CMM, cyc.com
        out["B"][b] = nonlinear_effects(mo, q[b], qd[b]) if qd is not None else cyc.G
    return out


def velocities(B, n):
    return np.random.default_rng(SEED).uniform(-1, 1, (B, n))


@functools.lru_cache(maxsize=None)
def tocabi_set(B):
    """q (B, 40), qd (B, 39) and the restatement's answers"""
    q, _, _ = cases.synth_batch(B, seed=SEED, yaw=True)
    qd = velocities(B, 39)
    return _freeze(dict(q=q, qd=qd, ref=_freeze(reference(cases.tocabi_model(), q, qd))))


@functools.lru_cache(maxsize=None)
def golden_set():
    """the reference's CASE 1 and CASE 2 states (tests/dwbc_test.cpp) with the dumped Acontact_mat and A_inv_"""
    q = np.array([cases.Q_CASE[1], cases.Q_CASE[2]], dtype=np.float64)
    return _freeze(dict(q=q, A=np.array([cases.golden(c, "Acontact_mat") for c in (1, 2)]), A_inv=np.array([cases.golden(c, "A_inv_") for c in (1, 2)])))


@functools.lru_cache(maxsize=None)
def pack_set(name, B):
    """the same for a model of tests/redist_pack_cases.model ("fixed_head", "fixed_arms", "surgery_43")"""
    from tests import redist_pack_cases as pc

    mo, _ = pc.model(name)
    q, _ = pc.states(name, mo, B)
    qd = velocities(B, mo["ndof"])
    return _freeze(dict(q=q, qd=qd, ref=_freeze(reference(mo, q, qd))))


def residual(A, A_inv):
    """max |A A_inv - I| over the batch"""
    n = A.shape[-1]
    return float(np.abs(A @ A_inv - np.eye(n)).max())


def check_residual_premise(ref, key):
    """the restatement's own residual on this state set: printed, and the recorded figure the kernel's bar is ten times of -- within a
    factor of 1.5 either way (the figure is a maximum over a few thousand rounding errors, and the summation order of the float64
    product behind it is the BLAS build's)"""
    r = residual(ref["A"], ref["A_inv"])
    rec = RESIDUAL_RESTATEMENT[key]
    print(f"{key}: restatement max|A A_inv - I| = {r:.3e} (recorded {rec:.1e}, bar for the kernel {bar_residual(key):.1e})")
    assert rec / 1.5 <= r <= 1.5 * rec, (key, r, rec)
    return r


def compare(got, ref, key, what="", names=NAMES):
    """every named output against the restatement at its bar, the kernel's own residual at the bar of the state set `key`; prints and
    returns the errors"""
    errs = {}
    for k in names:
        assert np.isfinite(got[k]).all(), k
        errs[k] = float(np.abs(got[k] - ref[k]).max())
    if "A" in names and "A_inv" in names:
        errs["residual"] = residual(got["A"], got["A_inv"])
    print(f"{key} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + (f" (residual bar {bar_residual(key):.1e})" if "residual" in errs else ""))
    for k in names:
        assert errs[k] <= BARS[k], (k, errs[k])
    if "residual" in errs:
        assert errs["residual"] <= bar_residual(key), (errs["residual"], bar_residual(key))
    return errs
