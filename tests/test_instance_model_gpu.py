"""gpu: one body table per instance (dwbc_batch_set_instance_model / dwbc_batch_bind_instance_model -> the dwbc_im:: build of the kernels,
libdwbc_amd/csrc/dwbc_kernels_im.h).  B = 24, every link of every instance randomised; recipe, references, premises and bars:
tests/instance_model_cases.py.  On the parent of the change that added the record every test here fails for lack of the entry points.

The full-model cycle on each launch route against the restatement with instance i's own model (all 18 cycle kernels of the build are
launched), against single-model batches of the default build, with the base table broadcast, with hqp = false, beside its dump record; the
six lean launches at the bars of their own test files; a bound tensor rewritten in place; the refusals.  A launcher that uploads the first
instance's table only fails every comparison against the restatement here (instances 1 .. 23 would read unwritten memory)."""
import numpy as np
import pytest

from tests import cases
from tests import instance_model_cases as im

pytestmark = pytest.mark.gpu

B = im.B
SWITCHES = ("DWBC_NO_WIDE", "DWBC_NO_PAIR", "DWBC_NO_LEAN", "DWBC_DENSE_SWEEP", "DWBC_PAIR_ALWAYS")
ROUTES = {
    "two_wave": ({}, "dwbc_cycle_kernel_v2p<39, 34, {L}, {ns}TopoTocabi>", 128),
    "wide_lean": ({"DWBC_NO_PAIR": "1"}, "dwbc_cycle_kernel_v2w<39, 34, {L}, 64, false, {ns}TopoTocabi>", 64),
    "compact_lean": ({"DWBC_NO_WIDE": "1"}, "dwbc_cycle_kernel_v2<39, 34, {L}, 64, false, {ns}TopoTocabi, true>", 64),
    "wide_extras": ({"DWBC_NO_LEAN": "1"}, "dwbc_cycle_kernel_v2w<39, 34, {L}, 64, true, {ns}TopoTocabi>", 64),
    "capped_extras": ({"DWBC_NO_LEAN": "1", "DWBC_NO_WIDE": "1"}, "dwbc_cycle_kernel_v2<39, 34, {L}, 64, true, {ns}TopoTocabi>", 64),
}
CELLS = [(r, lv) for r in ROUTES for lv in (1, 2, 3, 4) if not (r == "two_wave" and lv > 2)]


def _name(route, levels, ns):
    return ns + ROUTES[route][1].format(L=levels, ns=ns)


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _model(arrs=None):
    import libdwbc_amd as D

    return D.Model.from_urdf(cases.URDF) if arrs is None else D.Model.from_arrays(arrs)


def _make(n, tasks, model=None, tau_lim=cases.TAU_LIM, contacts=True, dtype="f64"):
    import libdwbc_amd as D

    wbc = D.Batch(model or _model(), n, device=0, dtype=dtype)
    for c in cases.CONTACTS_2 if contacts else ():
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(tasks):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(None if tau_lim is None else np.array(tau_lim))
    return wbc


def _load(wbc, q, flags, fstar):
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)


def _results(wbc):
    return wbc.get("tau"), wbc.get("wrench"), wbc.get("status")


def _solve_with_record(monkeypatch, route, levels, state, tables=None, **solve):
    tasks, q, flags, fstar = im.states(levels, state)
    _set_env(monkeypatch, ROUTES[route][0])
    wbc = _make(B, tasks, tau_lim=None if solve.get("hqp") is False else cases.TAU_LIM)
    wbc.set_instance_model(im.tables() if tables is None else tables)
    _load(wbc, q, flags, fstar)
    wbc.solve(**solve)
    return wbc


@pytest.mark.parametrize("route,levels", CELLS)
def test_route_matches_the_restatement(route, levels, monkeypatch):
    for state in im.SETS:
        if not im.exists(levels, state):
            continue
        ref = im.reference(levels, state)
        im.check_premises(ref, im.shared_reference(levels, state), f"L = {levels}, {state}")
        wbc = _solve_with_record(monkeypatch, route, levels, state)
        assert wbc.kernel_name() == _name(route, levels, "dwbc_im::"), (route, wbc.kernel_name())
        assert wbc.launch_info()[0] == ROUTES[route][2]
        im.compare(*_results(wbc), ref, f"{route}, L = {levels}, {state}")
        wbc.close()


@pytest.mark.parametrize("route,levels", [("two_wave", 2), ("wide_lean", 3), ("compact_lean", 4), ("wide_extras", 1), ("capped_extras", 2)])
def test_single_model_batches_agree(route, levels, monkeypatch):
    """three instances as Model.from_arrays models in B = 1 batches through the default build's kernel of the same route"""
    state = "yaw"
    tasks, q, flags, fstar = im.states(levels, state)
    wbc = _solve_with_record(monkeypatch, route, levels, state)
    tau, wr, st = _results(wbc)
    wbc.close()
    for i in (0, 7, B - 1):
        one = _make(1, tasks, model=_model(im.arrays(i)))
        _load(one, q[i : i + 1], flags[i : i + 1], fstar[i : i + 1])
        one.solve()
        assert one.kernel_name() == _name(route, levels, "dwbc::"), one.kernel_name()
        t1, w1, s1 = _results(one)
        one.close()
        assert s1[0] == st[i] == 1
        e = float(np.abs(t1[0] - tau[i]).max())
        print(f"{route}, L = {levels}, instance {i}: |d tau| to its single-model batch = {e:.3e} Nm, bit-equal: {bool((t1[0] == tau[i]).all() and (w1[0] == wr[i]).all())}")
        assert e <= im.XTOL, (i, e)
        assert np.abs(w1[0] - wr[i]).max() <= 1e3 * im.XTOL


@pytest.mark.parametrize("route,levels", [("two_wave", 1), ("compact_lean", 2), ("capped_extras", 4)])
def test_broadcast_base_table_is_the_batch_without_a_record(route, levels, monkeypatch):
    state = "mixed"
    tasks, q, flags, fstar = im.states(levels, state)
    base = _model()
    wbc = _solve_with_record(monkeypatch, route, levels, state, tables=base.instance_model(B))
    assert wbc.kernel_name().startswith("dwbc_im::")
    tau, wr, st = _results(wbc)
    wbc.set_instance_model(None)
    wbc.solve()
    assert wbc.kernel_name() == _name(route, levels, "dwbc::"), wbc.kernel_name()
    tau0, wr0, st0 = _results(wbc)
    wbc.close()
    assert (st == st0).all() and (st0 == 1).sum() >= 0.9 * B
    ok = st0 == 1
    e = float(np.abs(tau[ok] - tau0[ok]).max())
    print(f"{route}, L = {levels}: base table broadcast vs no record: |d tau| = {e:.3e} Nm, bit-equal: {bool((tau == tau0).all() and (wr == wr0).all())}")
    assert e <= im.XTOL and np.abs(wr[ok] - wr0[ok]).max() <= 1e3 * im.XTOL


@pytest.mark.parametrize("route", ["wide_extras", "capped_extras"])
def test_hqp_false_matches_the_restatement(route, monkeypatch):
    """the RL bridge's configuration (closed-form redistribution, no torque limit): per instance the numpy restatement of hqp = false"""
    from oracle import dwbc_np as Dn

    tasks, q, flags, fstar = im.states(2, "yaw")  # (double support: the closed form is written for two contacts)
    wbc = _solve_with_record(monkeypatch, route, 2, "yaw", hqp=False)
    assert wbc.kernel_name() == _name(route, 2, "dwbc_im::")
    tau, _, st = _results(wbc)
    wbc.close()
    tau_r, st_r, tau_s = np.zeros((B, 3, 33)), np.zeros(B, np.int32), np.zeros((B, 3, 33))
    for i in range(B):
        for mo, out in ((im.arrays(i), tau_r), (im.base_arrays(), tau_s)):
            cyc = Dn.Cycle(mo)
            for c in cases.CONTACTS_2:
                cyc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
            for lv, links in enumerate(tasks):
                for mode, link, pt in links:
                    cyc.add_task(lv, mode, link, pt)
            Dn.run_no_hqp(cyc, q[i], list(flags[i]), [fstar[i, :6], fstar[i, 6:]])
            out[i] = [cyc.tau_grav, cyc.tau_task, cyc.tau_contact]
            if out is tau_r:
                st_r[i] = cyc.status
    assert (st_r == 1).sum() >= 0.9 * B
    assert (np.abs(tau_r.sum(axis=1) - tau_s.sum(axis=1)).max(axis=1) > im.MOVED).sum() >= 0.5 * B
    assert (st == st_r).all()
    ok = st_r == 1
    e = float(np.abs(tau[ok] - tau_r[ok]).max())
    print(f"{route}, hqp = false: worst |d tau| = {e:.3e} Nm")
    assert e <= im.TOL_TAU, e


def _dynamics_reference(qd):
    from tests import dynamics_cases as dc

    _, q, _, _ = im.states(2, "yaw")
    outs = [dc.reference(im.arrays(i), q[i : i + 1], qd[i : i + 1]) for i in range(B)]
    return {k: np.concatenate([o[k] for o in outs]) for k in dc.NAMES}


def test_dump_record_agrees_with_the_dynamics_launch(monkeypatch):
    """A of the dump record (the extras build of the cycle) and A of the dynamics launch, both under the record, on the same batch"""
    _set_env(monkeypatch, {})
    tasks, q, flags, fstar = im.states(2, "yaw")
    wbc = _make(B, tasks)
    wbc.set_instance_model(im.tables())
    wbc.enable_dump(True)
    _load(wbc, q, flags, fstar)
    wbc.solve()
    assert wbc.kernel_name() == _name("wide_extras", 2, "dwbc_im::")
    A_dump = wbc.get("A")
    wbc.set_dynamics_outputs(["A"])
    wbc.update_dynamics()
    assert wbc.dynamics_kernel_name() == "dwbc_im::dwbc_dynamics_kernel<39, 34, dwbc_im::TopoTocabi>"
    A_dyn = wbc.dynamics()["A"]
    wbc.close()
    e = float(np.abs(A_dump - A_dyn).max())
    shared = float(np.abs(A_dyn - A_dyn[0]).max())
    print(f"A: dump record vs dynamics launch {e:.3e}; instances differ from instance 0 by up to {shared:.3e}")
    assert e <= 1e-9 and shared > 1e-3  # (the project's bar for A)


def test_dynamics_and_link_query_launches():
    from oracle.dwbc_np import Cycle, forward_kinematics, link_velocities, point_jacobian
    from tests import dynamics_cases as dc
    from tests import link_query_cases as lq

    _, q, _, _ = im.states(2, "yaw")
    qd = dc.velocities(B, 39)
    wbc = _make(B, [], contacts=False)
    wbc.set_instance_model(im.tables())
    wbc.set_state(q, qd)
    wbc.set_dynamics_outputs(list(dc.NAMES))
    wbc.update_dynamics()
    got = wbc.dynamics()
    assert (got["status"] == 1).all()
    ref = _dynamics_reference(qd)
    errs = {k: float(np.abs(got[k] - ref[k]).max()) for k in dc.NAMES}
    print("dynamics: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in dc.NAMES:
        assert errs[k] <= dc.BARS[k], (k, errs[k])
    # link query: the pelvis, a foot and a hand with points, and the COM link
    links, points = [0, 6, 23, lq.COM], [(0.0, 0.0, 0.0), cases.FOOT_POINT, (0.01, 0.02, -0.03), (0.0, 0.0, 0.0)]
    wbc.set_link_query(links, points, jacobians=True)
    wbc.update_kinematics()
    assert wbc.link_query_kernel_name() == "dwbc_im::dwbc_link_query_kernel<39, 34>"
    st = wbc.link_states()
    wbc.close()
    want = dict(pos=np.zeros((B, 4, 3)), rot=np.zeros((B, 4, 3, 3)), vel=np.zeros((B, 4, 6)), jac=np.zeros((B, 4, 6, 39)))
    for b in range(B):
        mo = im.arrays(b)
        R, p = forward_kinematics(mo, q[b])
        v0, w0, _ = link_velocities(mo, R, p, qd[b])
        cyc = Cycle(mo)
        cyc.update_kinematics(q[b])
        for e, (l, pt) in enumerate(zip(links, points)):
            pt = np.asarray(pt, float)
            if l == lq.COM:
                want["pos"][b, e], want["rot"][b, e], want["jac"][b, e], want["vel"][b, e] = cyc.com, R[0], cyc.J_com, cyc.J_com @ qd[b]
                continue
            want["pos"][b, e], want["rot"][b, e], want["jac"][b, e] = p[l] + R[l] @ pt, R[l], point_jacobian(mo, R, p, l, pt)
            want["vel"][b, e, :3], want["vel"][b, e, 3:] = v0[l] + np.cross(w0[l], R[l] @ pt), w0[l]
    lq.compare(st, want, links)
    assert np.abs(want["pos"][:, 2] - want["pos"][0, 2]).max() > 1e-3  # (the link lengths moved the hand)


def test_contact_space_task_space_and_gravity_launches():
    from tests import contact_space_cases as cs
    from tests import gravcomp_cases as gv
    from tests import task_space_cases as ts

    tasks, q, flags, _ = im.states(4, "mixed")
    wbc = _make(B, tasks)
    wbc.set_instance_model(im.tables())
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_contact_space_outputs(list(cs.NAMES))
    wbc.calc_contact_constraint()
    assert wbc.contact_space_kernel_name() == "dwbc_im::dwbc_contact_space_kernel<39, 34, dwbc_im::TopoTocabi>"
    got_cs = wbc.contact_space()
    wbc.set_task_space_outputs(list(ts.NAMES))
    wbc.calc_task_space()
    assert wbc.task_space_kernel_name() == "dwbc_im::dwbc_task_space_kernel<39, 34, dwbc_im::TopoTocabi>"
    levels, ts_status = wbc.task_space()
    wbc.grav_compensation()
    assert wbc.grav_kernel_name() == "dwbc_im::dwbc_gravcomp_kernel<39, 34, dwbc_im::TopoTocabi>"
    got_gv = wbc.grav_outputs()
    wbc.close()
    refs_cs = [cs.reference(im.arrays(i), cases.CONTACTS_2, q[i : i + 1], flags[i : i + 1]) for i in range(B)]
    cs.compare(got_cs, {k: np.concatenate([r[k] for r in refs_cs]) for k in refs_cs[0]}, "contact space")
    refs_ts = [ts.reference(im.arrays(i), cases.CONTACTS_2, tasks, q[i : i + 1], flags[i : i + 1]) for i in range(B)]
    ref_ts = {k: [np.concatenate([r[k][l] for r in refs_ts]) for l in range(len(refs_ts[0][k]))] for k in ts.NAMES}
    ref_ts["status"] = np.concatenate([r["status"] for r in refs_ts])
    got_ts = {k: [lv[k] for lv in levels if k in lv] for k in ts.NAMES}
    got_ts["status"] = ts_status
    ts.compare(got_ts, ref_ts, tasks, 34, "task space")
    g = {k: np.zeros(s) for k, s in (("tau", (B, 33)), ("wrench", (B, 12)))}
    g["status"] = np.zeros(B, np.int32)
    for i in range(B):
        g["status"][i], g["tau"][i], g["wrench"][i] = gv.grav_ref(_cycle_of(im.arrays(i)), q[i], flags[i])
    gv.check_grav_premise(g, flags)
    gv.compare_grav(got_gv, g)


def _cycle_of(mo):
    from oracle.dwbc_np import Cycle

    cyc = Cycle(mo)
    for c in cases.CONTACTS_2:
        cyc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    cyc.set_torque_limit(np.array(cases.TAU_LIM))
    return cyc


def test_redistribution_matches_single_model_batches():
    """the redistribution of a supplied torque under the record against B = 1 batches of Model.from_arrays models (the default build)"""
    tasks, q, flags, fstar = im.states(2, "mixed")
    tau_in = im.reference(2, "mixed")[0].sum(axis=1) + 5.0 * np.random.default_rng(11).standard_normal((B, 33))
    wbc = _make(B, tasks)
    wbc.set_instance_model(im.tables())
    _load(wbc, q, flags, fstar)
    wbc.set_torque_input(tau_in)
    wbc.redistribute()
    assert wbc.redistribute_kernel_name() == "dwbc_im::dwbc_redistribute_kernel<39, 34, dwbc_im::TopoTocabi>"
    tau, wr, st = wbc.get("redist_tau"), wbc.get("redist_wrench"), wbc.get("redist_status")
    wbc.close()
    moved = solved = 0
    for i in (0, 5, 11, 17, B - 1):
        res = []
        for mo in (im.arrays(i), None):  # the instance's own model, then the shared one
            one = _make(1, tasks, model=_model(mo))
            _load(one, q[i : i + 1], flags[i : i + 1], fstar[i : i + 1])
            one.set_torque_input(tau_in[i : i + 1])
            one.redistribute()
            assert one.redistribute_kernel_name().startswith("dwbc::")
            res.append((one.get("redist_tau")[0], one.get("redist_wrench")[0], one.get("redist_status")[0]))
            one.close()
        (t1, w1, s1), (_, w0, _) = res
        assert s1 == st[i]
        e = float(np.abs(t1 - tau[i]).max())
        print(f"redistribution, instance {i}: status {s1}, |d tau| to its single-model batch = {e:.3e} Nm, bit-equal: {bool((t1 == tau[i]).all())}")
        assert e <= im.XTOL and np.abs(w1 - wr[i]).max() <= 1e3 * im.XTOL
        solved += int(s1 == 1)
        moved += bool(np.abs(w1[0] - w0[0]).max() > im.MOVED)  # (the wrench of the supplied torque itself depends on the model)
    assert moved >= 3 and solved >= 3, (moved, solved)


def test_bound_tensor_is_read_in_place(monkeypatch):
    import torch

    _set_env(monkeypatch, {})
    tasks, q, flags, fstar = im.states(2, "yaw")
    wbc = _make(B, tasks)
    rec = torch.tensor(np.array(im.tables()), dtype=torch.float64, device="cuda:0")
    wbc.bind_instance_model(rec)
    with pytest.raises(Exception, match="bound to a device buffer"):
        wbc.set_instance_model(im.tables())
    _load(wbc, q, flags, fstar)
    wbc.solve()
    assert wbc.kernel_name().startswith("dwbc_im::")
    first = _results(wbc)
    im.compare(*first, im.reference(2, "yaw"), "bound tensor")
    # instance 3 becomes the model of instance 10, in place on the device
    new = im.arrays(10)
    rec[3] = torch.tensor(im.pack(new), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    wbc.solve()
    tau, wr, st = _results(wbc)
    wbc.close()
    others = np.arange(B) != 3
    assert (tau[others] == first[0][others]).all() and (wr[others] == first[1][others]).all() and (st[others] == first[2][others]).all()
    ref3 = im.orc_cycle([new], tasks, q[3:4], flags[3:4], fstar[3:4])
    assert ref3[2][0] == 1 and np.abs(ref3[0][0] - im.reference(2, "yaw")[0][3]).max() > im.MOVED
    im.compare(tau[3:4], wr[3:4], st[3:4], ref3, "instance 3 after the in-place change")


def test_refusals(monkeypatch):
    import libdwbc_amd as D

    _set_env(monkeypatch, {})
    tasks, q, flags, fstar = im.states(2, "yaw")
    t = np.array(im.tables())
    # batches that cannot carry a record at all: set and bind refuse at once
    f32 = _make(B, tasks, dtype="f32")
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    dense = _make(B, tasks)
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        md = D.Model.from_urdf(cases.variant_urdf(tmp + "/fh.urdf", cases.HEAD_JOINTS))
    cases.ensure_pack(md)
    pack = D.Batch(md, 4, device=0)
    for wbc, rec, msg in ((f32, t, "fp64 batches only"), (dense, t, "TOCABI's constant tree only"), (pack, md.instance_model(4), "kernel-pack models")):
        with pytest.raises(D.DwbcError, match="per-instance model: .*" + msg):
            wbc.set_instance_model(rec)
        assert wbc._L.dwbc_batch_bind_instance_model(wbc._h, 8) == 0 and msg in wbc._L.dwbc_last_error().decode()  # (never dereferenced: refused at once)
        wbc.close()
    wbc = _make(B, tasks, tau_lim=None)
    assert wbc.instance_model_shape == (B, 34, 25) and wbc._L.dwbc_batch_instance_model_stride(wbc._h) == 34 * 25
    # wrong shape; one validation refusal per rule, each naming the instance and the body; the batch keeps what it had
    with pytest.raises(D.DwbcError, match="shape"):
        wbc.set_instance_model(t[:, :-1])
    wbc.set_instance_model(t)
    bad = {"not finite": (2, 5, 17, np.nan), "mass must be > 0": (1, 3, 15, 0.0), "diagonal of the inertia": (4, 9, 22, -1e-3),
           "joint axis must have unit length": (0, 12, 13, 0.5), "R_T must be orthonormal": (7, 20, 4, 0.9)}
    for msg, (i, k, col, v) in bad.items():
        r = t.copy()
        r[i, k, col] = v
        with pytest.raises(D.DwbcError, match=f"instance {i}, body {k}: .*{msg}"):
            wbc.set_instance_model(r)
    _load(wbc, q, flags, fstar)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    wbc.solve()
    im.compare(*_results(wbc), im.reference(2, "yaw"), "after the refused records")
    # what a batch with a record refuses
    wbc.set_torque_limit(None)  # (the reduced path refuses a torque limit before anything else)
    with pytest.raises(D.DwbcError, match="per-instance model: not built on the reduced dynamics path"):
        wbc.solve(reduced=True)
    with pytest.raises(D.DwbcError, match="per-instance model: not built for three active contacts"):
        wbc.set_max_active_contacts(3)
    wbc.close()
    from libdwbc_amd.hqp import HQP

    lq = _make(B, tasks)
    lq.set_instance_model(t)
    lq.enable_dump(True)
    _load(lq, q, flags, fstar)
    lq.solve()
    hq = HQP.for_lqp(lq, contact_dof=12)
    with pytest.raises(D.DwbcError, match="a per-instance model is not built here"):
        hq.configure_lqp(lq)
    with pytest.raises(D.DwbcError, match="a per-instance model is not built here"):
        HQP(B, 39, 0, 12).solve_jacc(lq, 0)
    lq.close()
    # the capacity set first: the solve refuses
    gc = _make(B, tasks)
    gc.set_max_active_contacts(3)
    gc.set_instance_model(t)
    _load(gc, q, flags, fstar)
    with pytest.raises(D.DwbcError, match="per-instance model: not built for three active contacts"):
        gc.solve()
    gc.close()


def test_rl_bridge_takes_a_record():
    """RlWBCBridge.set_instance_model: hqp = false at the bridge's set-up; environment i follows its own model (against a bridge of one
    environment on that model), and None brings the shared model back"""
    from libdwbc_amd.rl_bridge import RlWBCBridge

    n = 6
    rng = np.random.default_rng(3)
    qpos = np.zeros((n, 40))
    qpos[:, 2], qpos[:, 3] = 0.93, 1.0
    qpos[:, 7:] = 0.1 * rng.standard_normal((n, 33))
    br = RlWBCBridge(n, cases.URDF)

    def torque(b, qp):
        b.UpdateKinematics(qp)
        b.SetContact(True, True)
        b.SetTaskSpace(0, np.zeros(6))
        b.SetTaskSpace(1, np.zeros(3))
        b.CalcTorque()
        return b.getTorqueCommand()

    shared = torque(br, qpos)
    br.set_instance_model(im.tables()[:n])
    own = torque(br, qpos)
    assert br.wbc.kernel_name().startswith("dwbc_im::")
    assert (np.abs(own - shared).max(axis=1) > im.MOVED).sum() >= n // 2
    one = RlWBCBridge(1, cases.URDF)
    one.model = _model(im.arrays(4))
    one.set_instance_model(im.tables()[4:5])
    assert np.abs(torque(one, qpos[4:5])[0] - own[4]).max() <= 1e-4  # (float32 torques of some 1e2 Nm)
    br.set_instance_model(None)
    br.Reset()
    assert np.abs(torque(br, qpos) - shared).max() == 0.0
