"""-m gpu: every launch flavour of the full-model cycle kernel against the oracle.

dwbc_batch_solve picks one of several builds of the same cycle (the planner of dwbc_launch_plan.h over the rows dwbc_kernels.h emits;
tests/test_launch_plan.py checks the decision itself without a device):
each build has its own register budget and some their own LDS map, so lane ownership, LDS races and register-capped code generation can
differ between builds that share every line of arithmetic -- the host emulation (tests/emu) cannot see those.  The launcher's own
switches force each route at a batch the oracle finishes in well under a second:

  route           switches                     build (kernel_name())
  two_wave        --                           dwbc_cycle_kernel_v2p<.., L, TopoTocabi>           (1 - 2 levels only)
  wide_lean       DWBC_NO_PAIR                 dwbc_cycle_kernel_v2w<.., L, 64, false, TopoTocabi>
  compact_lean    DWBC_NO_WIDE                 dwbc_cycle_kernel_v2<.., L, 64, false, TopoTocabi, true>   (Lds3)
  wide_extras     DWBC_NO_LEAN                 dwbc_cycle_kernel_v2w<.., L, 64, true, TopoTocabi>         (Lds2)
  capped_extras   DWBC_NO_LEAN + DWBC_NO_WIDE  dwbc_cycle_kernel_v2<.., L, 64, true, TopoTocabi>          (Lds2)
  generic         DWBC_DENSE_SWEEP (creation)  dwbc_cycle_kernel_v2<.., L, 64, true, TopoGeneric>

The natural boundary (B = 4 CU vs 4 CU + 1, no switches) is checked on its own below.
"""
import functools

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

TOL, WTOL, XTOL = 1e-6, 1e-5, 1e-8  # |d tau| / |d wrench| vs the oracle (the suite's bars); between routes on flat feet
B = 250  # not a power of two, at most 4 instances per CU: the B > 4 CU builds are forced by DWBC_NO_WIDE
SWITCHES = ("DWBC_NO_WIDE", "DWBC_NO_PAIR", "DWBC_NO_LEAN", "DWBC_DENSE_SWEEP", "DWBC_PAIR_ALWAYS")
ROUTES = {
    "two_wave": ({}, "dwbc::dwbc_cycle_kernel_v2p<39, 34, {L}, dwbc::TopoTocabi>", 128),
    "wide_lean": ({"DWBC_NO_PAIR": "1"}, "dwbc::dwbc_cycle_kernel_v2w<39, 34, {L}, 64, false, dwbc::TopoTocabi>", 64),
    "compact_lean": ({"DWBC_NO_WIDE": "1"}, "dwbc::dwbc_cycle_kernel_v2<39, 34, {L}, 64, false, dwbc::TopoTocabi, true>", 64),
    "wide_extras": ({"DWBC_NO_LEAN": "1"}, "dwbc::dwbc_cycle_kernel_v2w<39, 34, {L}, 64, true, dwbc::TopoTocabi>", 64),
    "capped_extras": ({"DWBC_NO_LEAN": "1", "DWBC_NO_WIDE": "1"}, cases.CAPPED_EXTRAS, 64),
    "generic": ({"DWBC_DENSE_SWEEP": "1"}, "dwbc::dwbc_cycle_kernel_v2<39, 34, {L}, 64, true, dwbc::TopoGeneric>", 64),
}
# states: flat feet (double support; left-foot support under the 3-level swing-foot hierarchy), yaw / tilted bases, per-instance
# LR / L / R flags (not with a swing-foot level: that foot cannot be a contact too), a third of the instances with no contact
STATES = {"flat": {}, "yaw": dict(yaw=True), "mixed": dict(mixed=True), "free": dict(mixed=True, free=True)}
FLAT = ("flat", "mixed", "free")


def _exists(route, levels, state):
    return not (route == "two_wave" and levels > 2) and not (state == "mixed" and levels == 3)


def _cells(states):
    return [(r, lv, s) for r in ROUTES for lv in (1, 2, 3, 4) for s in states if _exists(r, lv, s)]


@functools.lru_cache(maxsize=None)
def _case(levels, state):
    tasks, q, flags, fstar = cases.hierarchy_batch(B, levels, seed=20261016 + 10 * levels + list(STATES).index(state), **STATES[state])
    return tasks, q, flags, fstar


@functools.lru_cache(maxsize=None)
def _oracle(levels, state):
    from oracle import orc

    tasks, q, flags, fstar = _case(levels, state)
    M = orc.make_model(cases.tocabi_model())
    S = orc.make_setup(cases.CONTACTS_2, tasks, cases.TAU_LIM)
    return orc.cycle_batch(M, S, q, flags, fstar, 0)


def _make(nb, tasks, tau_lim=cases.TAU_LIM):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), nb, device=0)
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(tasks):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(None if tau_lim is None else np.array(tau_lim))
    return wbc


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _solve_route(monkeypatch, route, tasks, q, flags, fstar):
    """one solve through `route` (its switches set around batch creation and solve); asserts the launcher reports that build.
    Returns (tau, wrench, status, diag, lds, batch)."""
    env, name, threads = ROUTES[route]
    _set_env(monkeypatch, env)
    wbc = _make(len(q), tasks)
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    wbc.solve()
    nt, lds = wbc.launch_info()
    assert wbc.kernel_name() == name.format(L=len(tasks)), (route, wbc.kernel_name())
    assert nt == threads and lds > 0, (route, nt, lds)
    return wbc.get("tau"), wbc.get("wrench"), wbc.get("status"), wbc.get("diag"), lds, wbc


@pytest.mark.parametrize("route,levels,state", _cells(STATES))
def test_launch_flavour_vs_oracle(route, levels, state, monkeypatch):
    """one build x one hierarchy x one state distribution, every instance against the oracle"""
    tasks, q, flags, fstar = _case(levels, state)
    tau_r, wr_r, st_r, _ = _oracle(levels, state)
    tau, wr, st, diag, lds, wbc = _solve_route(monkeypatch, route, tasks, q, flags, fstar)
    assert (st == st_r).all()
    ok = st_r == 1
    assert ok.mean() > (0.5 if levels == 3 else 0.9)
    assert np.isfinite(tau).all()
    assert np.abs(tau[ok] - tau_r[ok]).max() < TOL
    assert np.abs(wr[ok] - wr_r[ok]).max() < WTOL
    # the cell tests something: task torques, active QP rows, and the lowest-priority level moves the answer
    assert np.abs(tau[ok, 1]).max() > 1.0
    assert diag[:, 9:12].sum() > 0
    fs2 = fstar.copy()
    fs2[:, sum(wbc.task_dof(lv) for lv in range(levels - 1)):] += 0.2
    wbc.set_fstar_all(fs2)
    wbc.solve()
    st2 = wbc.get("status")
    both = ok & (st2 == 1)
    assert both.mean() > 0.5 and np.abs(wbc.get("tau")[both, 1] - tau[both, 1]).max() > 1e-3


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_launch_flavours_agree_on_flat_feet(levels, monkeypatch):
    """Every build gives the same flat-footed states the same answer to 1e-8 (the bar between the wide and the compact build of
    test_full_size_configs_3_and_4); tilted bases keep the oracle bar only.  The compact map is the smaller LDS footprint, and the
    extras builds of both topologies share the Lds2 map."""
    for state in FLAT:
        if not _exists("wide_lean", levels, state):
            continue
        tasks, q, flags, fstar = _case(levels, state)
        res = {r: _solve_route(monkeypatch, r, tasks, q, flags, fstar) for r in ROUTES if _exists(r, levels, state)}
        tau0, wr0, st0 = res["capped_extras"][:3]
        ok = st0 == 1
        for r, (tau, wr, st, _, _, _) in res.items():
            assert (st == st0).all(), (r, state)
            assert np.abs(tau[ok] - tau0[ok]).max() < XTOL, (r, state)
            assert np.abs(wr[ok] - wr0[ok]).max() < 1e3 * XTOL, (r, state)  # wrench ~ 1e3 N
        lds = {r: v[4] for r, v in res.items()}
        assert lds["compact_lean"] < lds["capped_extras"] == lds["wide_extras"] == lds["generic"], lds


def _n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def test_natural_boundary_lean_and_warm_start(monkeypatch):
    """No switches: the same seeded states at B = 4 CU and 4 CU + 1.  A cold lean solve runs the two-wave kernel, then the compact
    one; warm-started solves (init = false) the wide, then the capped extras build.  Every instance against the oracle, and the
    instances both batches share agree to 1e-8."""
    from oracle import orc

    _set_env(monkeypatch, {})
    n_lo = 4 * _n_cu()
    n_hi = n_lo + 1
    tasks, q, flags, fstar = cases.hierarchy_batch(n_hi, 2, seed=20261017, mixed=True)
    q2 = q.copy()
    q2[:, 6:39] += 0.002 * np.random.default_rng(5).standard_normal((n_hi, 33))
    fstar2 = fstar + 0.01
    M = orc.make_model(cases.tocabi_model())
    S = orc.make_setup(cases.CONTACTS_2, tasks, cases.TAU_LIM)
    ref1 = orc.cycle_batch(M, S, q, flags, fstar, 0)
    ref2 = orc.cycle_batch(M, S, q2, flags, fstar2, 0)
    names, out = {}, {}
    for nb in (n_lo, n_hi):
        wbc = _make(nb, tasks)
        wbc.set_contact(flags[:nb])
        wbc.set_state(q[:nb])
        wbc.set_fstar_all(fstar[:nb])
        wbc.solve()  # cold, lean
        names[nb, "lean"] = wbc.kernel_name()
        out[nb, "lean"] = wbc.get("tau"), wbc.get("wrench"), wbc.get("status")
        wbc.solve(init=False)  # extras build, no working set yet (the lean build keeps none): cold
        wbc.set_state(q2[:nb])
        wbc.set_fstar_all(fstar2[:nb])
        wbc.solve(init=False)  # extras build, warm from the previous solve's working sets
        names[nb, "warm"] = wbc.kernel_name()
        out[nb, "warm"] = wbc.get("tau"), wbc.get("wrench"), wbc.get("status")
    assert names[n_lo, "lean"] == ROUTES["two_wave"][1].format(L=2), names
    assert names[n_hi, "lean"] == ROUTES["compact_lean"][1].format(L=2), names
    assert names[n_lo, "warm"] == ROUTES["wide_extras"][1].format(L=2), names
    assert names[n_hi, "warm"] == ROUTES["capped_extras"][1].format(L=2), names
    for kind, (tau_r, wr_r, st_r, _) in (("lean", ref1), ("warm", ref2)):
        ok = st_r == 1
        assert ok.mean() > 0.9
        for nb in (n_lo, n_hi):
            tau, wr, st = out[nb, kind]
            k = ok[:nb]
            assert (st == st_r[:nb]).all(), (kind, nb)
            assert np.abs(tau[k] - tau_r[:nb][k]).max() < TOL, (kind, nb)
            assert np.abs(wr[k] - wr_r[:nb][k]).max() < WTOL, (kind, nb)
        k = ok[:n_lo]
        assert np.abs(out[n_hi, kind][0][:n_lo][k] - out[n_lo, kind][0][k]).max() < XTOL, kind


def test_natural_boundary_hqp_false():
    """hqp = false beyond 4 CU (the RL bridge's default at more than 4 CU envs): the capped extras build.  A seeded sample of
    128 instances against the per-instance numpy restatement, and the same states in a small batch (the wide extras build)
    agree to 1e-8."""
    from tests.test_kernel_emulation import _no_hqp_oracle

    nb = 4 * _n_cu() + 1
    q, fl, fs = cases.synth_batch(nb, seed=20261018, yaw=True)
    idx = np.sort(np.random.default_rng(3).choice(nb, size=128, replace=False))
    res = {}
    for n, (qq, ff, ss) in ((nb, (q, fl, fs)), (128, (q[idx], fl[idx], fs[idx]))):
        wbc = _make(n, cases.TASKS_2LEVEL, tau_lim=None)
        wbc.set_state(qq)
        wbc.set_contact(ff)
        wbc.set_fstar_all(ss)
        wbc.solve(hqp=False)
        res[n] = wbc.kernel_name(), wbc.get("tau"), wbc.get("status")
    assert res[nb][0] == cases.CAPPED_EXTRAS.format(L=2), res[nb][0]
    assert res[128][0] == ROUTES["wide_extras"][1].format(L=2), res[128][0]
    tau_r, st_r = _no_hqp_oracle(q[idx], fl[idx], fs[idx])
    tau, st = res[nb][1][idx], res[nb][2][idx]
    assert (st == st_r).all() and st_r.mean() > 0.9
    assert np.abs(tau - tau_r).max() < TOL
    assert np.abs(tau[:, 2]).max() > 1.0
    assert (res[128][2] == st).all()
    assert np.abs(res[128][1] - tau).max() < XTOL


LDS4_2LEVEL = 39152  # Lds4<39, 34, 2>::total_bytes (dwbc_cycle2p.h): dynamic LDS of the two-wave kernel for two task levels


def test_pair_always_is_reported_as_launched(monkeypatch):
    """DWBC_PAIR_ALWAYS=1 beyond 4 CU: the two-wave kernel runs and kernel_name() / launch_info() say so (they are the plan of the
    launch); the answer is the compact build's on the same flat-footed states."""
    nb = 4 * _n_cu() + 1
    tasks, q, flags, fstar = cases.hierarchy_batch(nb, 2, seed=20261019)
    res = {}
    for env in ({}, {"DWBC_PAIR_ALWAYS": "1"}):
        _set_env(monkeypatch, env)
        wbc = _make(nb, tasks)
        wbc.set_state(q)
        wbc.set_contact(flags)
        wbc.set_fstar_all(fstar)
        wbc.solve()
        res[len(env)] = wbc.kernel_name(), wbc.launch_info(), wbc.get("tau"), wbc.get("status")
    assert res[0][0] == ROUTES["compact_lean"][1].format(L=2) and res[0][1][0] == 64, res[0][:2]
    assert res[1][0] == ROUTES["two_wave"][1].format(L=2), res[1][0]
    assert tuple(res[1][1]) == (128, LDS4_2LEVEL), res[1][1]
    ok = res[0][3] == 1
    assert (res[1][3] == res[0][3]).all() and ok.mean() > 0.9
    assert np.abs(res[1][2][ok] - res[0][2][ok]).max() < XTOL


def test_fp32_report_does_not_depend_on_a_solve(monkeypatch):
    """kernel_name() / launch_info() of an fp32 batch before its first solve are those of the launch that follows"""
    import libdwbc_amd as D

    _set_env(monkeypatch, {})
    nb = 64
    tasks, q, flags, fstar = cases.hierarchy_batch(nb, 2, seed=20261020)
    wbc = D.Batch(D.Model.from_urdf(cases.URDF), nb, device=0, dtype="f32")
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(tasks):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    before = wbc.kernel_name(), tuple(wbc.launch_info())
    wbc.solve()
    assert wbc.get("status").mean() > 0.9
    after = wbc.kernel_name(), tuple(wbc.launch_info())
    assert before == after, (before, after)
    assert after[0].startswith("dwbc_f32::") and after[1][0] == 64 and after[1][1] > 0, after
