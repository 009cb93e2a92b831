"""Inputs, restatement references, premises and bars of the task-space tests (tests/test_task_space_emu.py, tests/test_task_space_gpu.py),
computed once per state set and left unchanged.

Hierarchies: H4 = cases.TASKS_4LEVEL (pelvis 6D, upper-body rotation, left hand 6D, right hand 6D) and its one- and two-level prefixes;
HCOM = COM link 6D, pelvis rotation, upper-body rotation, left hand TASK_LINK_6D_CUSTOM_FRAME with point (0.01, 0.02, -0.03); HPOS (host
emulation) = pelvis TASK_LINK_POSITION_COM_FRAME, upper body TASK_LINK_6D_COM_FRAME, both hands' positions on one level (TASK_LINK_POSITION and
TASK_LINK_POSITION_CUSTOM_FRAME) -- every task dof (6, 3), every mode's row selection and every Jacobian source (link origin, the link's centre
of mass, custom point, rotation rows, the COM link) occurs.
States: cases.synth_batch(B, SEED, yaw=True); supports from contact_space_cases.flag_mix (both feet, left, right, none, in turn).  HCOM runs
on the three supports with a contact only: with no active contact the reference's complete orthogonal decomposition of Q W^+ Q^T truncates
there (Y X - I is 11 in the restatement itself), and the device's SPD route does not reproduce a truncation.
Reference: the restatement, oracle.dwbc_np.Cycle: J_task, Lambda_t, J_kt and Null after calc_task_torque.

Bars against the restatement (max abs): J_task of link levels 1e-12 and of a COM level 1e-10 (the link query's), Lambda_task 1e-8 (the
project's bar for Lambda_c and between its two CPU implementations, tests/test_oracle_golden.py), J_kt and Null_task 1e-7 on the device and
1e-8 in host emulation (both are linear in W^+ and carry its bars, contact_space_cases.BARS["W_inv"] and BAR_W_INV_EMU).

Identities, with X = J_kt Lambda and Y = (J_task A^-1 N_c)[:, 6:] of the outputs and A^-1 N_c of the same source as they -- the
restatement's for the restatement, the contact-space launch's on the same batch for the kernel (the same front end): Lambda (J_task A^-1 N_c
J_task^T) = I, Y X = I, (I - X Y)^2 = I - X Y, Y_0 Null_0 = 0.  Each bar is ten times the restatement's own residual on the same state set
(RESIDUAL_RESTATEMENT, measured by check_residual_premise, which the tests run and print first), the rule of tests/contact_space_cases.py."""
import functools

import numpy as np

from tests import cases
from tests import contact_space_cases as cs

SEED = 7
NAMES = ("J_task", "Lambda_task", "J_kt", "Null_task")
BAR_J_LINK, BAR_J_COM, BAR_LAMBDA = 1e-12, 1e-10, 1e-8
BAR_W_DEVICE, BAR_W_EMU = cs.BARS["W_inv"], cs.BAR_W_INV_EMU
TASK_LINK_6D_CUSTOM_FRAME = 2
H4 = cases.TASKS_4LEVEL
NB_TOCABI = 34
HCOM = [[(cases.TASK_LINK_6D, NB_TOCABI, (0, 0, 0))], [(cases.TASK_LINK_ROTATION, 0, (0, 0, 0))], [(cases.TASK_LINK_ROTATION, 15, (0, 0, 0))],
        [(TASK_LINK_6D_CUSTOM_FRAME, 23, (0.01, 0.02, -0.03))]]
# the position modes and the COM-frame points (rows [0:3] of the point Jacobian; the link's own centre of mass as the point), with two links
# on one level: pelvis position at its COM, upper body 6D at its COM, both hands' positions (left: link origin, right: a custom point)
TASK_LINK_6D_COM_FRAME, TASK_LINK_POSITION, TASK_LINK_POSITION_COM_FRAME, TASK_LINK_POSITION_CUSTOM_FRAME = 1, 3, 4, 5
HPOS = [[(TASK_LINK_POSITION_COM_FRAME, 0, (0, 0, 0))], [(TASK_LINK_6D_COM_FRAME, 15, (0, 0, 0))],
        [(TASK_LINK_POSITION, 23, (0, 0, 0)), (TASK_LINK_POSITION_CUSTOM_FRAME, 33, (0.02, -0.01, 0.03))]]
HIERARCHIES = {"H4": H4, "H4_1": H4[:1], "H4_2": H4[:2], "H4_3": H4[:3], "HCOM": HCOM, "HPOS": HPOS}
IDENTITIES = ("LL", "YX", "PP", "Y0N0")
# the restatement's own residuals (numpy float64) of the four identities on each state set the tests use, measured by
# check_residual_premise and recorded here, rounded up.  The kernel's bar on a set is ten times the figure of that set.
RESIDUAL_RESTATEMENT = {
    ("H4", 8): dict(LL=6.6e-13, YX=4.8e-14, PP=5.2e-14, Y0N0=1.3e-14),
    ("HCOM", 8): dict(LL=8.4e-13, YX=1.1e-13, PP=6.7e-14, Y0N0=1.6e-15),
    ("H4_1", 8): dict(LL=1.1e-14, YX=4.8e-14, PP=2.8e-14, Y0N0=0.0),  # (one level: no Null_task)
    ("H4_2", 8): dict(LL=1.1e-14, YX=4.8e-14, PP=2.8e-14, Y0N0=1.3e-14),
    ("H4", 7): dict(LL=8.8e-13, YX=7.3e-14, PP=4.1e-14, Y0N0=1.7e-14),
    ("H4", 130): dict(LL=4.4e-12, YX=1.3e-13, PP=6.0e-14, Y0N0=2.4e-14),
    ("HCOM", 7): dict(LL=2.0e-13, YX=7.3e-14, PP=5.1e-14, Y0N0=8.8e-16),
    ("HPOS", 8): dict(LL=5.1e-15, YX=2.6e-14, PP=2.7e-14, Y0N0=4.1e-16),
    ("fixed_head", 8): dict(LL=2.1e-14, YX=7.2e-14, PP=2.5e-14, Y0N0=1.1e-14),
}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, list):
            for a in v:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return d


def task_dofs(tasks):
    return [sum(6 if mode <= 2 else 3 for mode, _, _ in lv) for lv in tasks]


def com_levels(tasks, nb):
    return [any(link == nb for _, link, _ in lv) for lv in tasks]


def contact_mix(B):
    """both feet, left only, right only, in turn: the supports with a contact"""
    fl = np.zeros((B, 2), np.uint8)
    fl[0::3, :2] = 1
    fl[1::3, 0] = 1
    fl[2::3, 1] = 1
    return fl


def reference(mo, contacts, tasks, q, flags):
    """the restatement's outputs per level in the launch's shapes, ``status``, and A_inv_N_C.  More than two flags: status 0, zeros."""
    from oracle.dwbc_np import Cycle

    n = mo["ndof"]
    m = n - 6
    B = len(q)
    ts = task_dofs(tasks)
    L = len(tasks)
    cyc = Cycle(mo)
    for c in contacts:
        cyc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for l, lv in enumerate(tasks):
        for mode, link, pt in lv:
            cyc.add_task(l, mode, link, pt)
    cyc.set_torque_limit(np.full(m, 300.0))  # (the QPs behind the matrices need a row when no contact is active; f* = 0 is feasible)
    out = {"J_task": [np.zeros((B, t, n)) for t in ts], "Lambda_task": [np.zeros((B, t, t)) for t in ts], "J_kt": [np.zeros((B, m, t)) for t in ts],
           "Null_task": [np.zeros((B, m, m)) for _ in ts[:-1]], "status": np.zeros(B, np.int32), "A_inv_N_C": np.zeros((B, n, n))}
    for b in range(B):
        on = [bool(f) for f in flags[b]]
        if sum(on) > 2:
            continue
        cyc.update_kinematics(q[b])
        cyc.set_contact(on)
        out["status"][b] = cyc.calc_contact_constraint()
        cyc.calc_grav()
        cyc.calc_task_torque([np.zeros(t) for t in ts])
        out["A_inv_N_C"][b] = cyc.A_inv_N_C
        for l in range(L):
            out["J_task"][l][b], out["Lambda_task"][l][b], out["J_kt"][l][b] = cyc.J_task[l], cyc.Lambda_t[l], cyc.J_kt[l]
            if l < L - 1:
                out["Null_task"][l][b] = cyc.Null[l]
    return out


@functools.lru_cache(maxsize=None)
def tocabi_set(hier, B):
    """q (B, 40), flags (B, 2) and the restatement's answers on TOCABI, contacts CONTACTS_2"""
    q, _, _ = cases.synth_batch(B, seed=SEED, yaw=True)
    fl = contact_mix(B) if hier == "HCOM" else cs.flag_mix(B)
    tasks = HIERARCHIES[hier]
    return _freeze(dict(q=q, flags=fl, contacts=cases.CONTACTS_2, tasks=tasks, nb=NB_TOCABI,
                        ref=_freeze(reference(cases.tocabi_model(), cases.CONTACTS_2, tasks, q, fl))))


def pack_tasks(mo):
    """the first three levels of H4 on a model of tests/redist_pack_cases.model: every link is looked up by its TOCABI name in the edited model"""
    tocabi = list(cases.tocabi_model()["names"])
    names = list(mo["names"])
    return [[(mode, names.index(tocabi[link]), pt) for mode, link, pt in lv] for lv in H4[:3]]


@functools.lru_cache(maxsize=None)
def pack_set(name, B):
    """the same for a model of tests/redist_pack_cases.model ("fixed_head": 37 dof / 32 bodies), supports from flag_mix"""
    from tests import redist_pack_cases as pc

    mo, links = pc.model(name)
    q, _ = pc.states(name, mo, B)
    con = pc.contacts_of(links)
    fl = cs.flag_mix(B)
    tasks = pack_tasks(mo)
    return _freeze(dict(q=q, flags=fl, contacts=con, tasks=tasks, nb=mo["nb"], ref=_freeze(reference(mo, con, tasks, q, fl))))


def residuals(o, AiNc, okm=None):
    """the four identity residuals (max abs over the batch) of per-level outputs"""
    r = dict.fromkeys(IDENTITIES, 0.0)
    L = len(o["J_task"])
    for b in range(len(AiNc)):
        if okm is not None and not okm[b]:
            continue
        for l in range(L):
            J, Lam, Jk = o["J_task"][l][b], o["Lambda_task"][l][b], o["J_kt"][l][b]
            T1 = J @ AiNc[b]
            X, Y = Jk @ Lam, T1[:, 6:]
            t = len(J)
            r["LL"] = max(r["LL"], float(np.abs(Lam @ (T1 @ J.T) - np.eye(t)).max()))
            r["YX"] = max(r["YX"], float(np.abs(Y @ X - np.eye(t)).max()))
            P = np.eye(X.shape[0]) - X @ Y
            r["PP"] = max(r["PP"], float(np.abs(P @ P - P).max()))
            if l == 0 and L > 1:
                r["Y0N0"] = max(r["Y0N0"], float(np.abs(Y @ o["Null_task"][0][b]).max()))
    return r


def bar_residual(key, ident):
    return 10.0 * RESIDUAL_RESTATEMENT[key][ident]


def check_residual_premise(ref, key):
    """the restatement's own residuals on this state set: printed, and the recorded figures the kernel's bars are ten times of -- within a
    factor of 1.5 either way (each is a maximum over a few thousand rounding errors, and the summation order of the float64 products
    behind it is the BLAS build's)"""
    r = residuals(ref, ref["A_inv_N_C"], ref["status"] == 1)
    rec = RESIDUAL_RESTATEMENT.get(key)
    print(f"{key}: restatement residuals " + ", ".join(f"{k} {v:.3e}" + (f" (recorded {rec[k]:.1e})" if rec else "") for k, v in r.items()))
    assert rec is not None, (key, r)
    for k in IDENTITIES:
        assert rec[k] / 1.5 <= r[k] <= 1.5 * rec[k] or (r[k] == 0.0 and rec[k] == 0.0), (key, k, r[k], rec[k])
    return r


def check_identities(got, A_inv_N_C, ref, key, what=""):
    """the kernel's outputs, with A_inv_N_C of the contact-space launch on the same batch (the same front end: what the levels were formed
    from), against the identity bars of the state set `key`, on the instances the restatement solved; prints and returns the residuals"""
    assert np.abs(A_inv_N_C - ref["A_inv_N_C"]).max() <= cs.BARS["A_inv_N_C"]
    r = residuals(got, A_inv_N_C, ref["status"] == 1)
    print(f"{key} {what}: identities " + ", ".join(f"{k} {v:.2e} (bar {bar_residual(key, k):.1e})" for k, v in r.items()))
    for k in IDENTITIES:
        assert r[k] <= bar_residual(key, k), (k, r[k], bar_residual(key, k))
    return r


def compare(got, ref, tasks, nb, what="", names=NAMES, w_bar=BAR_W_DEVICE):
    """status identical; every named output of every level against the restatement at its bar; exact zeros on failed instances; prints and
    returns the worst error per output"""
    assert (got["status"] == ref["status"]).all(), (got["status"], ref["status"])
    com = com_levels(tasks, nb)
    L = len(tasks)
    errs, over = {}, []
    for k in names:
        worst = 0.0
        for l in range(L - 1 if k == "Null_task" else L):
            g, r = got[k][l], ref[k][l]
            assert g.shape == r.shape, (k, l, g.shape, r.shape)
            assert np.isfinite(g).all(), (k, l)
            e = float(np.abs(g - r).max())
            bar = {"J_task": BAR_J_COM if com[l] else BAR_J_LINK, "Lambda_task": BAR_LAMBDA}.get(k, w_bar)
            if e > bar:
                over.append((k, l, e, bar))
            worst = max(worst, e)
            for b in np.nonzero(ref["status"] == 0)[0]:
                assert not g[b].any(), (k, l, b)
        errs[k] = worst
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert not over, over
    return errs
