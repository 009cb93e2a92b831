"""Inputs, restatement references, premises and bars of the single-level task-QP tests (tests/test_task_qp_emu.py, tests/test_task_qp_gpu.py),
computed once per state set and left unchanged.

Reference: the restatement, oracle.dwbc_np -- per instance Cycle.build_task_qp(N J_kt Lambda, f*, torque_prev) and solve_qp(A, ub, t), the two
functions CalcSingleTaskTorqueWithQP is restated as; f_star_qp = x[:t], contact_qp = x[t:], torque_h = J_kt Lambda (f* + f_star_qp),
torque_null_h = N torque_h, torque_contact = NwJw contact_qp.  A failed QP, a failed contact stage or more than two flags: status 0 and zeros.

State sets (contacts cases.CONTACTS_2, torque limit cases.TAU_LIM unless stated):
  P   cases.hierarchy_batch(B, 4, seed=SEED, yaw=Y, mixed=True), B in {12, 130}, Y in {False, True}: four levels (pelvis 6D, upper-body rotation,
      both hands 6D), supports LR / L / R in turn.  Level l runs with N = Null[l - 1] (identity at level 0) and torque_prev = tau_grav + the
      torque_null_h of the levels above: the chain of CalcTaskControlTorque.
  Q   "a level beneath a foreign torque": on P, level 1 with N = Null[0] and torque_prev = tau_grav + default_rng(5).uniform(-40, 40, 33),
      drawn per instance in batch order.
  F   failure: on P at B = 12, level 0, identity, torque_prev = tau_grav + 1000: every torque row is violated by more than the task can give up.
  S3  cases.hierarchy_batch(6, 3, seed=SEED): swing foot, single support, k = 0.
Premises (check_premises, run and printed by the tests first): the restatement's four-level cascade returns status 1 on every instance of
the four P sets; at B = 12 the level QPs carry between 0 and 8 active rows (0 .. 7 at Y = False, 0 .. 8 at Y = True); solving level by level as above reproduces
Cycle.calc_task_torque's fstar_qp exactly (difference 0.0); Q: status 1 on 130 of 130 for both Y, at least one active row on 68 % (Y = False)
and 75 % (Y = True) of the instances; F: status 0 and x = 0 on all 12; S3: status 1 on all 6.

Bars against the restatement (max abs):
  torques (torque_h, torque_null_h, torque_contact, and the chained sum)   TOL = 1e-6 Nm, the project's bar for every torque against the oracle
  f_star_qp, contact_qp                                                     ten times what the full cycle's own QPs show against the
      restatement on sets P (B = 130, both Y), the rule of tests/contact_space_cases.py and tests/task_space_cases.py (the new front sums in
      another order): MEASURED_DEVICE from Batch.solve() with the dump record on an MI355X, MEASURED_EMU from tests/emu's cycle emulation
      (extras build), both on the commit before this launch existed; max |dump - restatement| over every level and instance, rounded up.
      The bars: f_star_qp 6.8e-11 (device) / 6.3e-11 (emulation), contact_qp 2.0e-7 / 4.9e-8.  (What the launch itself shows on the device on
      P at B = 130, Y = True: 1.2e-12 and 4.9e-9; the chained sum of torque_null_h against the restatement 1.1e-11 Nm, against tau_task of
      solve() 7.0e-11 Nm.)"""
import functools

import numpy as np

from tests import cases

SEED = 20261021
TOL = 1e-6
NAMES = ("f_star_qp", "contact_qp", "torque_h", "torque_null_h", "torque_contact")
TORQUES = ("torque_h", "torque_null_h", "torque_contact")
# max |fstar_qp / contact_qp of the dump record - restatement| of the full cycle on sets P, B = 130, Y in {False, True} (see above)
MEASURED_DEVICE = {"f_star_qp": 6.8e-12, "contact_qp": 2.0e-8}  # (6.72e-12 and 1.93e-8, both at Y = True; Y = False alone: 1.1e-12, 9.8e-11)
MEASURED_EMU = {"f_star_qp": 6.3e-12, "contact_qp": 4.9e-9}  # (Y = False alone: 2.0e-12, 1.1e-10)


def _round_up(x):
    """to two significant digits, upwards"""
    from math import ceil, floor, log10

    if x == 0.0:
        return 0.0
    e = floor(log10(x)) - 1
    return ceil(x / 10.0 ** e) * 10.0 ** e


def bars(measured):
    b = {k: TOL for k in TORQUES}
    for k in ("f_star_qp", "contact_qp"):
        b[k] = _round_up(10.0 * measured[k])
    return b


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, list):
            for a in v:
                if isinstance(a, dict):
                    _freeze(a)
        elif isinstance(v, dict):
            _freeze(v)
    return d


def task_dofs(tasks):
    return [sum(6 if mode <= 2 else 3 for mode, _, _ in lv) for lv in tasks]


def split_fstar(tasks, fstar_row):
    out, o = [], 0
    for t in task_dofs(tasks):
        out.append(np.asarray(fstar_row[o : o + t], float))
        o += t
    return out


def make_cycle(mo, contacts, tasks, tau_lim):
    from oracle.dwbc_np import Cycle

    cyc = Cycle(mo)
    for c in contacts:
        cyc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for l, lv in enumerate(tasks):
        for mode, link, pt in lv:
            cyc.add_task(l, mode, link, pt)
    if tau_lim is not None:
        cyc.set_torque_limit(np.asarray(tau_lim, float))
    return cyc


def prepare(cyc, q, flags, fstars):
    """the restatement up to and including CalcTaskSpace (and its own cascade, whose answers the premises read).  Returns the status of the
    contact stage; more than two flags: 0, nothing computed"""
    on = [bool(f) for f in flags]
    if sum(on) > 2:
        return 0
    cyc.update_kinematics(q)
    cyc.set_contact(on)
    st = cyc.calc_contact_constraint()
    cyc.calc_grav()
    try:
        cyc.cascade_status = cyc.calc_task_torque(fstars)
    except ValueError:  # no torque limit and no active contact: the cascade's solve_qp takes no QP without rows; the matrices stand before it
        if cyc.tau_lim is not None or cyc.cdof:
            raise
        cyc.cascade_status, cyc.fstar_qp = 1, []
    return st


def single_level(cyc, level, fstar, N, torque_prev):
    """one call of the reference method on the restatement's state.  Returns dict(status, the five outputs, nact)"""
    from oracle.dwbc_np import solve_qp

    m = cyc.m
    k = max(cyc.cdof - 6, 0)
    X = cyc.J_kt[level] @ cyc.Lambda_t[level]
    t = X.shape[1]
    Nm = np.eye(m) if N is None else N
    A, ub = cyc.build_task_qp(Nm @ cyc.J_kt[level] @ cyc.Lambda_t[level], fstar, torque_prev)  # (the cascade's order of the products)
    if A.shape[0]:
        st, x, act = solve_qp(A, ub, t, 1000)
    else:  # no torque limit and no active contact: no row at all, and the least-norm point of an unconstrained problem is x = 0 (solve_qp takes none)
        st, x, act = 1, np.zeros(A.shape[1]), []
    out = dict(status=st, nact=len(act), f_star_qp=np.zeros(6), contact_qp=np.zeros(6), torque_h=np.zeros(m), torque_null_h=np.zeros(m), torque_contact=np.zeros(m))
    if st:
        out["f_star_qp"][:t] = x[:t]
        out["contact_qp"][:k] = x[t:]
        out["torque_h"] = X @ (fstar + x[:t])
        out["torque_null_h"] = Nm @ out["torque_h"]
        if k:
            out["torque_contact"] = cyc.NwJw @ x[t:]
    return out


def _empty(B, m):
    d = {k: np.zeros((B, 6 if k in ("f_star_qp", "contact_qp") else m)) for k in NAMES}
    d["status"] = np.zeros(B, np.int32)
    d["nact"] = np.zeros(B, np.int32)
    return d


def _store(d, b, r):
    for k in NAMES:
        d[k][b] = r[k]
    d["status"][b] = r["status"]
    d["nact"][b] = r["nact"]


def chain_reference(mo, contacts, tasks, q, flags, fstar, tau_lim, inst_lim=None):
    """every level in turn, as CalcTaskControlTorque chains them.  Returns per level dict(null (B, m, m) or None at level 0, torque_prev
    (B, m), ref = outputs), tau_grav (B, m), null (the restatement's Null per level), exact (max |level-by-level f_star_qp - the cascade's|),
    cascade (status of the restatement's own cascade per instance).  inst_lim: (B, m) torque limits per instance instead of tau_lim.  A level
    below a failed one: status 0, zeros (the reference never reaches it)."""
    m = mo["ndof"] - 6
    B = len(q)
    L = len(tasks)
    cyc = make_cycle(mo, contacts, tasks, tau_lim)
    levels = [dict(null=None if l == 0 else np.zeros((B, m, m)), torque_prev=np.zeros((B, m)), ref=_empty(B, m)) for l in range(L)]
    tau_grav = np.zeros((B, m))
    cascade = np.zeros(B, np.int32)
    exact = 0.0
    for b in range(B):
        if inst_lim is not None:
            cyc.set_torque_limit(inst_lim[b])
        fs = split_fstar(tasks, fstar[b])
        if not prepare(cyc, q[b], flags[b], fs):
            continue
        cascade[b] = cyc.cascade_status
        tau_grav[b] = cyc.tau_grav
        tau_task = np.zeros(m)
        for l in range(L):
            N = None if l == 0 else cyc.Null[l - 1]
            if l:
                levels[l]["null"][b] = N
            levels[l]["torque_prev"][b] = cyc.tau_grav + tau_task
            r = single_level(cyc, l, fs[l], N, cyc.tau_grav + tau_task)
            _store(levels[l]["ref"], b, r)
            if not r["status"]:
                break
            t = len(fs[l])
            if l < len(cyc.fstar_qp):
                exact = max(exact, float(np.abs(r["f_star_qp"][:t] - cyc.fstar_qp[l]).max()))
            tau_task = tau_task + r["torque_null_h"]
    return dict(levels=levels, tau_grav=tau_grav, cascade=cascade, exact=exact)


def one_level_reference(mo, contacts, tasks, q, flags, fstar, tau_lim, level, null_of, torque_prev_of, inst_lim=None):
    """one level with inputs of the caller's choice: null_of(cyc) -> (m, m) or None, torque_prev_of(cyc, b) -> (m,), both called per instance in
    batch order on the prepared restatement.  Returns dict(null, torque_prev, ref)"""
    m = mo["ndof"] - 6
    B = len(q)
    cyc = make_cycle(mo, contacts, tasks, tau_lim)
    out = dict(null=None, torque_prev=np.zeros((B, m)), ref=_empty(B, m))
    for b in range(B):
        if inst_lim is not None:
            cyc.set_torque_limit(inst_lim[b])
        fs = split_fstar(tasks, fstar[b])
        if not prepare(cyc, q[b], flags[b], fs):
            continue
        N = null_of(cyc)
        if N is not None:
            if out["null"] is None:
                out["null"] = np.zeros((B, m, m))
            out["null"][b] = N
        tp = torque_prev_of(cyc, b)
        out["torque_prev"][b] = tp
        _store(out["ref"], b, single_level(cyc, level, fs[level], N, tp))
    return out


@functools.lru_cache(maxsize=None)
def set_P(B, yaw):
    tasks, q, flags, fstar = cases.hierarchy_batch(B, 4, seed=SEED, yaw=yaw, mixed=True)
    ch = chain_reference(cases.tocabi_model(), cases.CONTACTS_2, tasks, q, flags, fstar, cases.TAU_LIM)
    return _freeze(dict(tasks=tasks, q=q, flags=flags, fstar=fstar, contacts=cases.CONTACTS_2, tau_lim=np.array(cases.TAU_LIM, float), **ch))


@functools.lru_cache(maxsize=None)
def set_Q(B, yaw):
    s = set_P(B, yaw)
    rng = np.random.default_rng(5)
    r = one_level_reference(cases.tocabi_model(), s["contacts"], s["tasks"], s["q"], s["flags"], s["fstar"], s["tau_lim"], 1, lambda cyc: cyc.Null[0],
                            lambda cyc, b: cyc.tau_grav + rng.uniform(-40, 40, 33))
    return _freeze(dict(level=1, **r))


@functools.lru_cache(maxsize=None)
def set_F():
    s = set_P(12, True)
    r = one_level_reference(cases.tocabi_model(), s["contacts"], s["tasks"], s["q"], s["flags"], s["fstar"], s["tau_lim"], 0, lambda cyc: None,
                            lambda cyc, b: cyc.tau_grav + 1000.0)
    return _freeze(dict(level=0, **r))


@functools.lru_cache(maxsize=None)
def set_S3():
    tasks, q, flags, fstar = cases.hierarchy_batch(6, 3, seed=SEED)
    ch = chain_reference(cases.tocabi_model(), cases.CONTACTS_2, tasks, q, flags, fstar, cases.TAU_LIM)
    return _freeze(dict(tasks=tasks, q=q, flags=flags, fstar=fstar, contacts=cases.CONTACTS_2, tau_lim=np.array(cases.TAU_LIM, float), **ch))


@functools.lru_cache(maxsize=None)
def set_variant(kind):
    """P at B = 12, Y = True with another support or no torque limit, every level chained: "free" -- no active contact, torque rows alone;
    "free_nolim" -- no active contact and no torque limit: no rows at all, x = 0 and status 1; "nolim" -- P's supports, cone rows alone"""
    s = set_P(12, True)
    flags = s["flags"] if kind == "nolim" else np.zeros_like(s["flags"])
    tau_lim = s["tau_lim"] if kind == "free" else None
    ch = chain_reference(cases.tocabi_model(), s["contacts"], s["tasks"], s["q"], flags, s["fstar"], tau_lim)
    return _freeze(dict(tasks=s["tasks"], q=s["q"], flags=flags, fstar=s["fstar"], contacts=s["contacts"], tau_lim=tau_lim, **ch))


@functools.lru_cache(maxsize=None)
def set_HCOM():
    """a hierarchy whose level 0 is on the COM link (tests/task_space_cases.HCOM: COM 6D, pelvis rotation, upper-body rotation, left hand 6D at
    a custom point) on P's states at B = 12, Y = True, the supports with a contact in turn (both feet, left, right: with no active contact
    the reference's complete orthogonal decomposition truncates on this hierarchy, see tests/task_space_cases.py), f* a seeded uniform of
    +- 0.5, every level chained"""
    from tests import task_space_cases as tc

    s = set_P(12, True)
    flags = tc.contact_mix(12)
    fstar = 0.5 * np.random.default_rng(SEED + 2).uniform(-1, 1, size=(12, sum(task_dofs(tc.HCOM))))
    ch = chain_reference(cases.tocabi_model(), s["contacts"], tc.HCOM, s["q"], flags, fstar, s["tau_lim"])
    return _freeze(dict(tasks=tc.HCOM, q=s["q"], flags=flags, fstar=fstar, contacts=s["contacts"], tau_lim=s["tau_lim"], **ch))


# of cases.TAU_LIM, on every second instance of set_inst_lim: P's chained torque reaches 0.21 to 0.54 of the limit on some joint of every
# instance at B = 12, Y = True, so a fifth of the limit puts torque rows into every such instance's working sets
TIGHT = 0.2


@functools.lru_cache(maxsize=None)
def set_inst_lim():
    """per-instance torque limits on P at B = 12, Y = True: cases.TAU_LIM on the even instances, TIGHT times it on the odd ones, every level
    chained with each instance's own limit.  ``nact_batch_wide``: the active rows per level with cases.TAU_LIM on every instance."""
    s = set_P(12, True)
    lim = np.tile(s["tau_lim"], (12, 1))
    lim[1::2] *= TIGHT
    ch = chain_reference(cases.tocabi_model(), s["contacts"], s["tasks"], s["q"], s["flags"], s["fstar"], None, inst_lim=lim)
    wide = np.stack([lv["ref"]["nact"] for lv in s["levels"]])
    return _freeze(dict(tasks=s["tasks"], q=s["q"], flags=s["flags"], fstar=s["fstar"], contacts=s["contacts"], tau_lim=s["tau_lim"], inst_lim=lim,
                        nact_batch_wide=wide, **ch))


def inst_par_record(s):
    """the per-instance record [tau_lim[m] | lx ly mu muz of every registered contact] of set_inst_lim for the emulation"""
    con = np.array([[c["lx"], c["ly"], c["mu"], c["muz"]] for c in s["contacts"]], float).reshape(-1)
    return np.concatenate([s["inst_lim"], np.tile(con, (len(s["inst_lim"]), 1))], axis=1)


def check_premises_inst_lim():
    s = set_inst_lim()
    nact = np.stack([lv["ref"]["nact"] for lv in s["levels"]])
    st = np.stack([lv["ref"]["status"] for lv in s["levels"]])
    differ = int((nact[:, 1::2] != s["nact_batch_wide"][:, 1::2]).sum())
    print(f"per-instance limits: status 1 on {int(st.sum())} of {st.size} level solves; active rows differ from the batch-wide limit's on {differ} level "
          f"solves of the tight instances")
    assert (nact[:, 0::2] == s["nact_batch_wide"][:, 0::2]).all()
    assert differ > 0
    return st


def check_premises_P(B, yaw):
    s = set_P(B, yaw)
    nact = np.stack([lv["ref"]["nact"] for lv in s["levels"]])
    print(f"P B={B} yaw={yaw}: cascade status 1 on {int(s['cascade'].sum())} of {B}; active rows per level QP {nact.min()} .. {nact.max()}; "
          f"level by level against the cascade: {s['exact']:.1e}")
    assert (s["cascade"] == 1).all()
    assert all((lv["ref"]["status"] == 1).all() for lv in s["levels"])
    assert s["exact"] == 0.0
    if B == 12:  # the QPs bite: 0 .. 7 active rows at Y = False, 0 .. 8 at Y = True
        assert nact.min() == 0 and nact.max() == (8 if yaw else 7), (nact.min(), nact.max())
    assert set(s["flags"].sum(axis=1).tolist()) == {1, 2}
    return nact


def check_premises_Q(yaw):
    s = set_Q(130, yaw)
    share = float((s["ref"]["nact"] > 0).mean())
    print(f"Q yaw={yaw}: status 1 on {int(s['ref']['status'].sum())} of 130; at least one active row on {100 * share:.0f} %")
    assert (s["ref"]["status"] == 1).all()
    assert round(100 * share) == (75 if yaw else 68), share


def check_premises_F():
    s = set_F()
    print(f"F: status {s['ref']['status'].tolist()}")
    assert (s["ref"]["status"] == 0).all()
    assert not any(s["ref"][k].any() for k in NAMES)


def check_premises_S3():
    s = set_S3()
    assert all((lv["ref"]["status"] == 1).all() for lv in s["levels"])
    assert (s["flags"].sum(axis=1) == 1).all()  # single support: k = 0


def compare(got, ref, bar, what="", names=NAMES):
    """status agreement exact; every named output against the restatement at its bar on the instances the restatement solved -- every other
    instance must be exact zeros; prints each figure before it asserts; returns (worst error per output, instances left out)"""
    assert (got["status"] == ref["status"]).all(), (what, got["status"], ref["status"])
    ok = ref["status"] == 1
    left_out = int((~ok).sum())
    errs, over = {}, []
    for k in names:
        g, r = got[k], ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.isfinite(g).all(), (what, k)
        assert not g[~ok].any(), (what, k)
        e = float(np.abs(g[ok] - r[ok]).max()) if ok.any() else 0.0
        errs[k] = e
        if e > bar[k]:
            over.append((k, e, bar[k]))
    print(f"{what}: " + ", ".join(f"{k} {v:.2e} (bar {bar[k]:.1e})" for k, v in errs.items()) + f"; left out {left_out}")
    assert not over, (what, over)
    return errs, left_out
