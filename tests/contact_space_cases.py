"""Inputs, restatement references, premises and bars of the contact-space tests (tests/test_contact_space_emu.py,
tests/test_contact_space_gpu.py), computed once per state set and left unchanged.

States: TOCABI -- cases.synth_batch(B, SEED, yaw=True) with the support mixed inside the batch (flag_mix: both feet, left only, right
only, none, in turn); the reference's CASE 1 and CASE 2 states with four registered contacts and two enabled (cases.CONTACTS_4) for the
goldens; the pack models of tests/redist_pack_cases.model with their own state recipe and the same flag mix.
Reference: the restatement, oracle.dwbc_np.Cycle.update_kinematics, set_contact, calc_contact_constraint, every output padded with zeros to
the launch's fixed shapes; the contact frames are the link rotation and link position + R point of the active contacts, in their order.

Bars against the restatement and the goldens: the ones the project holds its dump record to on a device (tests/test_gpu_parity.py:63-70,
tests/test_facade_cpp.py:43): J_C 1e-12, Lambda_c 1e-8, J_C_INV_T 1e-9, N_C 1e-9, A_inv_N_C and W 1e-8, W_inv 1e-7 on the device and 1e-8 in
host emulation (tests/test_kernel_emulation.py:33), NwJw 1e-9, contact position and rotation the link query's (tests/link_query_cases.py).

Identities: J_C_INV_T J_C^T = I on cd x cd, J_C (A_inv_N_C) = 0, N_C N_C = N_C, W W_inv W = W, trace(W_inv W) = m - k (rounded).  Each bar
is ten times the restatement's own residual on the same state set (RESIDUAL_RESTATEMENT, measured by check_residual_premise, which the
tests run and print first), the rule of tests/dynamics_cases.py.  State sets are named by (model, B)."""
import functools

import numpy as np

from tests import cases
from tests import link_query_cases as lq

SEED = 7
NAMES = ("J_C", "Lambda_c", "J_C_INV_T", "N_C", "A_inv_N_C", "W", "W_inv", "NwJw", "contact_pos", "contact_rot")
BARS = {"J_C": 1e-12, "Lambda_c": 1e-8, "J_C_INV_T": 1e-9, "N_C": 1e-9, "A_inv_N_C": 1e-8, "W": 1e-8, "W_inv": 1e-7, "NwJw": 1e-9,
        "contact_pos": lq.TOL_POS, "contact_rot": lq.TOL_ROT}
BAR_W_INV_EMU = 1e-8
GOLDEN_NAMES = {"J_C": "J_C", "Lambda_c": "Lambda_contact", "J_C_INV_T": "J_C_INV_T", "N_C": "N_C", "W": "W", "W_inv": "W_inv", "NwJw": "NwJw"}
IDENTITIES = ("JbT_JT", "J_AiNc", "NN", "WWiW")
# the restatement's own residuals (numpy float64) of the four identities on each state set the tests use, measured by
# check_residual_premise and recorded here, rounded up.  The kernel's bar on a set is ten times the figure of that set.
RESIDUAL_RESTATEMENT = {
    ("tocabi", 4): dict(JbT_JT=2.7e-15, J_AiNc=2.5e-15, NN=4.7e-15, WWiW=1.6e-12),
    ("tocabi", 8): dict(JbT_JT=5.6e-15, J_AiNc=1.8e-15, NN=4.5e-15, WWiW=1.6e-12),
    ("golden", 2): dict(JbT_JT=1.1e-14, J_AiNc=1.9e-15, NN=9.4e-15, WWiW=1.6e-12),
    ("fixed_head", 3): dict(JbT_JT=6.3e-15, J_AiNc=1.9e-15, NN=4.3e-15, WWiW=1.2e-12),
    ("fixed_head", 8): dict(JbT_JT=9.4e-15, J_AiNc=1.9e-15, NN=5.8e-15, WWiW=1.9e-12),
    ("fixed_arms", 3): dict(JbT_JT=5.9e-15, J_AiNc=2.6e-15, NN=3.9e-15, WWiW=2.5e-14),
    ("fixed_arms", 8): dict(JbT_JT=7.2e-15, J_AiNc=2.6e-15, NN=8.5e-15, WWiW=2.5e-14),
    ("surgery_43", 3): dict(JbT_JT=5.8e-15, J_AiNc=3.2e-15, NN=4.5e-15, WWiW=2.8e-12),
    ("surgery_43", 8): dict(JbT_JT=4.1e-15, J_AiNc=2.8e-15, NN=4.8e-15, WWiW=8.7e-12),
}


def flag_mix(B, nreg=2):
    """both feet, left only, right only, none, in turn"""
    fl = np.zeros((B, nreg), np.uint8)
    fl[0::4, :2] = 1
    fl[1::4, 0] = 1
    fl[2::4, 1] = 1
    return fl


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def shapes(B, n):
    m = n - 6
    return {"J_C": (B, 12, n), "Lambda_c": (B, 12, 12), "J_C_INV_T": (B, 12, n), "N_C": (B, n, n), "A_inv_N_C": (B, n, n), "W": (B, m, m), "W_inv": (B, m, m),
            "NwJw": (B, m, 6), "contact_pos": (B, 2, 3), "contact_rot": (B, 2, 3, 3)}


def reference(mo, contacts, q, flags):
    """the restatement's outputs in the launch's shapes, ``status``, and cd / k per instance.  More than two flags: status 0, zeros."""
    from oracle.dwbc_np import Cycle

    n = mo["ndof"]
    B = len(q)
    cyc = Cycle(mo)
    for c in contacts:
        cyc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    out = {k: np.zeros(s) for k, s in shapes(B, n).items()}
    out["status"] = np.zeros(B, np.int32)
    out["cd"] = np.zeros(B, np.int64)
    for b in range(B):
        on = [bool(f) for f in flags[b]]
        if sum(on) > 2:
            continue
        cyc.update_kinematics(q[b])
        cyc.set_contact(on)
        out["status"][b] = cyc.calc_contact_constraint()
        cd = cyc.cdof
        out["cd"][b] = cd
        out["J_C"][b, :cd] = cyc.J_C
        out["Lambda_c"][b, :cd, :cd] = cyc.Lambda_c
        out["J_C_INV_T"][b, :cd] = cyc.J_C_INV_T
        out["N_C"][b], out["A_inv_N_C"][b], out["W"][b], out["W_inv"][b] = cyc.N_C, cyc.A_inv_N_C, cyc.W, cyc.W_inv
        out["NwJw"][b, :, : cyc.NwJw.shape[1]] = cyc.NwJw
        for a, c in enumerate(cyc.act_contacts):
            R = cyc.R[c["link"]]
            out["contact_rot"][b, a] = R
            out["contact_pos"][b, a] = cyc.p[c["link"]] + R @ c["point"]
    return out


@functools.lru_cache(maxsize=None)
def tocabi_set(B):
    """q (B, 40), flags (B, 2) and the restatement's answers, contacts CONTACTS_2"""
    q, _, _ = cases.synth_batch(B, seed=SEED, yaw=True)
    fl = flag_mix(B)
    return _freeze(dict(q=q, flags=fl, contacts=cases.CONTACTS_2, ref=_freeze(reference(cases.tocabi_model(), cases.CONTACTS_2, q, fl))))


@functools.lru_cache(maxsize=None)
def golden_set():
    """the reference's CASE 1 and CASE 2 states (tests/dwbc_test.cpp) with four registered contacts, two enabled, and the dumped matrices"""
    q = np.array([cases.Q_CASE[1], cases.Q_CASE[2]], dtype=np.float64)
    fl = np.array([[1, 1, 0, 0]] * 2, np.uint8)
    d = dict(q=q, flags=fl, contacts=cases.CONTACTS_4, ref=_freeze(reference(cases.tocabi_model(), cases.CONTACTS_4, q, fl)))
    for k, g in GOLDEN_NAMES.items():
        d["golden_" + k] = np.array([cases.golden(c, g) for c in (1, 2)])
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def too_many_set():
    """B = 3 on CONTACTS_4: both feet / three flags set (status 0, zeros) / left foot"""
    q, _, _ = cases.synth_batch(3, seed=SEED, yaw=True)
    fl = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    return _freeze(dict(q=q, flags=fl, contacts=cases.CONTACTS_4, ref=_freeze(reference(cases.tocabi_model(), cases.CONTACTS_4, q, fl))))


@functools.lru_cache(maxsize=None)
def pack_set(name, B):
    """the same for a model of tests/redist_pack_cases.model ("fixed_head", "fixed_arms", "surgery_43")"""
    from tests import redist_pack_cases as pc

    mo, links = pc.model(name)
    q, _ = pc.states(name, mo, B)
    con = pc.contacts_of(links)
    fl = flag_mix(B)
    return _freeze(dict(q=q, flags=fl, contacts=con, ref=_freeze(reference(mo, con, q, fl))))


def residuals(o, cd):
    """the four identity residuals (max abs over the batch) and trace(W_inv W) per instance"""
    r = dict.fromkeys(IDENTITIES, 0.0)
    tr = np.zeros(len(cd))
    for b in range(len(cd)):
        c = int(cd[b])
        J, Jb, N, Ai, W, Wi = o["J_C"][b], o["J_C_INV_T"][b], o["N_C"][b], o["A_inv_N_C"][b], o["W"][b], o["W_inv"][b]
        if c:
            r["JbT_JT"] = max(r["JbT_JT"], float(np.abs(Jb[:c] @ J[:c].T - np.eye(c)).max()))
            r["J_AiNc"] = max(r["J_AiNc"], float(np.abs(J[:c] @ Ai).max()))
        r["NN"] = max(r["NN"], float(np.abs(N @ N - N).max()))
        r["WWiW"] = max(r["WWiW"], float(np.abs(W @ Wi @ W - W).max()))
        tr[b] = np.trace(Wi @ W)
    return r, tr


def bar_residual(key, ident):
    return 10.0 * RESIDUAL_RESTATEMENT[key][ident]


def check_residual_premise(ref, key):
    """the restatement's own residuals on this state set: printed, and the recorded figures the kernel's bars are ten times of -- within a
    factor of 1.5 either way (each is a maximum over a few thousand rounding errors, and the summation order of the float64 products
    behind it is the BLAS build's); its trace(W_inv W) rounds to m - k"""
    r, tr = residuals(ref, ref["cd"])
    rec = RESIDUAL_RESTATEMENT[key]
    print(f"{key}: restatement residuals " + ", ".join(f"{k} {v:.3e} (recorded {rec[k]:.1e})" for k, v in r.items()))
    for k in IDENTITIES:
        assert rec[k] / 1.5 <= r[k] <= 1.5 * rec[k], (key, k, r[k], rec[k])
    m = ref["W"].shape[-1]
    kk = np.maximum(ref["cd"] - 6, 0)
    assert (np.rint(tr) == m - kk).all(), (tr, m - kk)
    return r


def check_identities(got, ref, key, what=""):
    """the kernel's outputs against the identity bars of the state set `key`, on the instances the restatement solved; prints and returns
    the residuals"""
    okm = ref["status"] == 1
    sub = {k: got[k][okm] for k in ("J_C", "J_C_INV_T", "N_C", "A_inv_N_C", "W", "W_inv")}
    r, tr = residuals(sub, ref["cd"][okm])
    print(f"{key} {what}: identities " + ", ".join(f"{k} {v:.2e} (bar {bar_residual(key, k):.1e})" for k, v in r.items()) +
          f", |trace(W_inv W) - (m - k)| {np.abs(tr - np.rint(tr)).max():.1e}")
    m = ref["W"].shape[-1]
    assert (np.rint(tr) == m - np.maximum(ref["cd"][okm] - 6, 0)).all(), tr
    for k in IDENTITIES:
        assert r[k] <= bar_residual(key, k), (k, r[k], bar_residual(key, k))
    return r


def compare(got, ref, what="", names=NAMES, w_inv_bar=None):
    """status identical; every named output against the restatement at its bar; exact zeros beyond cd and on failed instances; prints and
    returns the errors"""
    assert (got["status"] == ref["status"]).all(), (got["status"], ref["status"])
    bars = dict(BARS)
    if w_inv_bar is not None:
        bars["W_inv"] = w_inv_bar
    errs = {}
    for k in names:
        assert np.isfinite(got[k]).all(), k
        errs[k] = float(np.abs(got[k] - ref[k]).max())
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for b in range(len(ref["status"])):
        cd = int(ref["cd"][b])
        for k in names:
            if ref["status"][b] == 0:
                assert not got[k][b].any(), (k, b)
        if "J_C" in names:
            assert not got["J_C"][b, cd:].any()
        if "J_C_INV_T" in names:
            assert not got["J_C_INV_T"][b, cd:].any()
        if "Lambda_c" in names:
            assert not got["Lambda_c"][b, cd:].any() and not got["Lambda_c"][b, :, cd:].any()
        if "NwJw" in names and cd <= 6:
            assert not got["NwJw"][b].any()
        if "contact_pos" in names:
            assert not got["contact_pos"][b, cd // 6:].any()
        if "contact_rot" in names:
            assert not got["contact_rot"][b, cd // 6:].any()
    for k in names:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
    return errs


def compare_goldens(got, g, what="", w_inv_bar=None):
    """against the reference's dumped matrices at the CASE states (cd = 12)"""
    errs = {}
    for k in GOLDEN_NAMES:
        gold = g["golden_" + k]
        errs[k] = float(np.abs(got[k][: len(gold)].reshape(gold.shape) - gold).max())
    print(f"{what} goldens: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= (w_inv_bar if (k == "W_inv" and w_inv_bar is not None) else BARS[k]), (k, v)
    return errs
