"""gpu: CalcGravCompensation as a lean launch (dwbc_batch_grav_compensation -> dwbc_gravcomp_kernel, libdwbc_amd/csrc/dwbc_redistribute.h
with GRAV = true), alone and ahead of the redistribution (Batch.redistribute(add_gravity=True)), against the numpy restatement, against
the full cycle's own torque_grav_, and against the plain redistribution.

References, premises and bars (1e-6 Nm, 1e-5 N, status identical): tests/gravcomp_cases.py, tests/redist_cases.py.  On the parent of the
change that added the launch every test here fails for lack of the entry points."""
import numpy as np
import pytest

from tests import cases
from tests import gravcomp_cases as gc
from tests import redist_cases as rc
from tests import redist_pack_cases as pc

pytestmark = pytest.mark.gpu

B = 130
KERNEL = "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoTocabi>"


def _batch(n, tasks=False, dtype="f64"):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), n, device=0, dtype=dtype)
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    if tasks:
        wbc.add_task(0, D.TASK_LINK_6D, 0)
        wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _redist(wbc):
    return dict(tau=wbc.get("redist_tau"), cf=wbc.get("redist_cf"), wrench=wbc.get("redist_wrench"), status=wbc.get("redist_status"))


def _posed(wbc, ref, flags=None, tau_in=None):
    wbc.set_state(ref["q"])
    wbc.set_contact(ref["flags"] if flags is None else flags)
    if tau_in is not None:
        wbc.set_torque_input(tau_in)
    return wbc


def test_gravity_only_matches_restatement_and_carries_the_weight():
    ref = rc.state_set(B, True, "mixed")
    g = gc.tocabi_grav(B, True, "mixed", free_every=3)
    gc.check_grav_premise(g, g["flags"])
    wbc = _posed(_batch(B), ref, flags=g["flags"])  # no task space, no torque input
    assert wbc.grav_kernel_name() == KERNEL
    wbc.grav_compensation()
    got = wbc.grav_outputs()
    gc.compare_grav(got, g)
    gc.check_free_instances(got, g["flags"])
    gc.check_vertical_force(got, g["flags"], wbc.model.total_mass)
    wbc.close()


def test_gravity_only_equals_the_cycles_torque_grav():
    ref = rc.state_set(B, True, "mixed")
    _, _, fstar = cases.synth_batch(B, seed=7, yaw=True, contact_mode="mixed")
    wbc = _posed(_batch(B, tasks=True), ref)
    wbc.set_fstar_all(fstar)
    wbc.solve()
    want = wbc.get("tau_grav")
    ok = wbc.get("status") == 1
    assert ok.sum() >= 0.9 * B and np.abs(want[ok]).max(axis=1).min() > gc.MIN_GRAV
    wbc.grav_compensation()
    got = wbc.grav_outputs()
    assert (got["status"][ok] == 1).all()
    e = float(np.abs(got["tau"][ok] - want[ok]).max())
    print(f"worst |grav_outputs tau - tau_grav of solve()| = {e:.3e} Nm over {int(ok.sum())} instances")
    assert e <= rc.TOL_TAU
    wbc.close()


@pytest.mark.parametrize("case", ["flat_LR", "yaw_mixed"])
def test_option_matches_restatement_and_the_plain_redistribution(case):
    yaw, mode = (True, "mixed") if case == "yaw_mixed" else (False, "LR")
    ref = rc.state_set(B, yaw, mode)
    rc.check_premises(ref)
    g = gc.tocabi_grav(B, yaw, mode)
    gc.check_grav_premise(g, ref["flags"])
    wbc = _posed(_batch(B), ref, tau_in=ref["tau_in"] - g["tau"])
    wbc.redistribute(add_gravity=True)
    got = _redist(wbc)
    rc.compare(got, ref)
    gc.compare_grav(wbc.grav_outputs(), g)
    # the plain redistribution of the summed torque on the same batch
    wbc.set_torque_input(ref["tau_in"])
    wbc.redistribute()
    plain = _redist(wbc)
    assert (plain["status"] == got["status"]).all()
    e = float(np.abs(plain["tau"] - got["tau"]).max())
    print(f"worst |redist tau with the option - plain redistribution of the sum| = {e:.3e} Nm")
    assert e <= rc.TOL_TAU
    wbc.close()


def test_option_leaves_a_feasible_input_alone():
    ref = rc.state_set(B, False, "LR")
    g = gc.tocabi_grav(B, False, "LR")
    wbc = _posed(_batch(B), ref, tau_in=ref["tau_feasible"] - g["tau"])
    wbc.redistribute(init=False, add_gravity=True)  # accepted: runs cold
    got = _redist(wbc)
    assert (got["status"] == 1).all()
    assert np.abs(got["tau"]).max() <= 1e-6
    assert (got["wrench"][:, 0] == got["wrench"][:, 1]).all() and np.abs(got["wrench"][:, 0]).max(axis=1).min() > 100.0
    wbc.close()


def test_independent_of_the_other_launches():
    """DWBC_TAU / DWBC_WRENCH / DWBC_STATUS / DWBC_DIAG of solve(), the plain redistribution's four outputs and a link query's outputs are
    bit-identical with and without the two new launches, run before or after them"""
    ref = rc.state_set(B, True, "mixed")
    g = gc.tocabi_grav(B, True, "mixed")
    _, _, fstar = cases.synth_batch(B, seed=7, yaw=True, contact_mode="mixed")
    only, after, before = _batch(B, tasks=True), _batch(B, tasks=True), _batch(B, tasks=True)
    for w in (only, after, before):
        _posed(w, ref, tau_in=ref["tau_in"])
        w.set_fstar_all(fstar)
        w.set_link_query([0, 6, 15], jacobians=True)

    def old_launches(w):
        w.solve()
        w.redistribute()
        w.update_kinematics()
        return dict({"cyc_" + k: w.get(k) for k in ("tau", "wrench", "status", "diag")}, **{"rd_" + k: v for k, v in _redist(w).items()},
                    **{"lq_" + k: v for k, v in w.link_states().items()})

    def new_launches(w):
        w.grav_compensation()
        alone = w.grav_outputs()
        w.set_torque_input(ref["tau_in"] - g["tau"])
        w.redistribute(add_gravity=True)  # writes the redistribution's outputs: the plain launch below must restore them to the bit
        w.set_torque_input(ref["tau_in"])
        return alone

    want = old_launches(only)
    assert want["cyc_status"].sum() >= 0.9 * B
    new_launches(before)
    got_before = old_launches(before)
    old_launches(after)
    cyc_after = {k: after.get(k) for k in ("tau", "wrench", "status", "diag")}
    lq_after = after.link_states()
    g_after = new_launches(after)
    for k, v in want.items():
        assert (got_before[k] == v).all(), k
        if k.startswith("cyc_"):
            assert (after.get(k[4:]) == v).all() and (cyc_after[k[4:]] == v).all(), k
        if k.startswith("lq_"):
            assert (after.link_states()[k[3:]] == v).all() and (lq_after[k[3:]] == v).all(), k
    after.redistribute()
    for k, v in _redist(after).items():
        assert (v == want["rd_" + k]).all(), k
    # and the gravity launch does not depend on what ran before it
    fresh = _posed(_batch(B), ref)
    fresh.grav_compensation()
    for k, v in fresh.grav_outputs().items():
        assert (g_after[k] == v).all(), k
    # the cycle still starts warm from its own working sets after the new launches ran in between
    after.solve(init=False)
    only.solve(init=False)
    assert (after.get("tau") == only.get("tau")).all() and (after.get("diag") == only.get("diag")).all()
    for w in (only, after, before, fresh):
        w.close()


def test_bound_tensors_match_the_host_path():
    import torch

    ref = rc.state_set(B, False, "LR")
    g = gc.tocabi_grav(B, False, "LR")
    tin = ref["tau_in"] - g["tau"]
    host = _posed(_batch(B), ref, tau_in=tin)
    host.grav_compensation()
    want_g = host.grav_outputs()
    host.redistribute(add_gravity=True)
    want_r = _redist(host)
    dev = _batch(B)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t = dict(in_q=torch.from_numpy(ref["q"].copy()).cuda(), in_contact=torch.from_numpy(ref["flags"].copy()).cuda(), in_torque=torch.from_numpy(tin.copy()).cuda(),
                 redist_tau=torch.full((B, dev.m), float("nan"), dtype=torch.float64, device="cuda:0"),
                 redist_wrench=torch.full((B, 2, 12), float("nan"), dtype=torch.float64, device="cuda:0"))
        gt = dict(tau=torch.full((B, dev.m), float("nan"), dtype=torch.float64, device="cuda:0"),
                  wrench=torch.full((B, 12), float("nan"), dtype=torch.float64, device="cuda:0"), status=torch.full((B,), -1, dtype=torch.int32, device="cuda:0"))
        for k, v in t.items():
            dev.bind_tensor(k, v)
        for k, v in gt.items():
            dev.bind_grav(k, v)
        dev.grav_compensation()
        s.synchronize()
        for k, v in gt.items():
            assert (v.cpu().numpy() == want_g[k]).all(), k
        assert torch.isnan(t["redist_tau"]).all()  # the gravity-only launch writes none of the redistribution's outputs
        for v in gt.values():
            v.fill_(-1)
        dev.redistribute(add_gravity=True)
        s.synchronize()
        for k, v in gt.items():
            assert (v.cpu().numpy() == want_g[k]).all(), k
        assert (t["redist_tau"].cpu().numpy() == want_r["tau"]).all() and (t["redist_wrench"].cpu().numpy() == want_r["wrench"]).all()
        dev.bind_grav("tau", None)  # back to the batch's own buffer
        dev.grav_compensation()
        assert (dev.grav_outputs()["tau"] == want_g["tau"]).all()
    host.close()
    dev.close()


def _pack_model(name, tmp_path):
    import libdwbc_amd as D
    from tests.test_model_packs import VARIANTS

    return D.Model.from_urdf(cases.variant_urdf(tmp_path / f"{name}.urdf", VARIANTS[name][0]))


def _pack_batch(md, links, n):
    import libdwbc_amd as D

    wbc = D.Batch(md, n, device=0)
    for c in pc.contacts_of(links):
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    wbc.set_torque_limit(np.full(md.ndof - 6, pc.TAU_LIM))
    return wbc


def _both_forms(wbc, ref, g, mass):
    _posed(wbc, ref)
    wbc.grav_compensation()
    got = wbc.grav_outputs()
    gc.compare_grav(got, g)
    gc.check_free_instances(got, ref["flags"])
    gc.check_vertical_force(got, ref["flags"], mass)
    wbc.set_torque_input(ref["tau_in"] - g["tau"])
    wbc.redistribute(add_gravity=True)
    rd = _redist(wbc)
    rc.compare(rd, ref)
    pc.check_flag_mix_outputs(rd, ref)
    gc.compare_grav(wbc.grav_outputs(), g)


@pytest.mark.parametrize("name", ["fixed_arms", "fixed_head", "fixed_head_own_tree"])
def test_packs_both_forms(tmp_path, name):
    n = 32
    own = name.endswith("_own_tree")
    name = name.replace("_own_tree", "")
    md = _pack_model(name, tmp_path)
    cases.ensure_pack(md)
    if own:
        cases.ensure_pack(md, tree=True)
    ref = pc.state_set(name, n)
    rc.check_premises(ref)
    g = gc.pack_grav(name, n)
    gc.check_grav_premise(g, ref["flags"])
    _, links = pc.model(name)
    wbc = _pack_batch(md, links, n)
    kn = wbc.grav_kernel_name()
    assert f"dwbc_gravcomp_kernel<{md.ndof}, {md.nb}," in kn
    if own:
        assert "TopoPack" in kn
    _both_forms(wbc, ref, g, md.total_mass)
    wbc.close()


def test_builtin_generic_row(monkeypatch):
    """a TOCABI batch created under DWBC_DENSE_SWEEP (any 34-body tree) takes the built-in TopoGeneric row"""
    n = 32
    ref = rc.state_set(n, True, "mixed")
    rc.check_premises(ref)
    g = gc.tocabi_grav(n, True, "mixed")
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    wbc = _batch(n)
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    assert wbc.grav_kernel_name() == "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoGeneric>"
    _posed(wbc, ref)
    wbc.grav_compensation()
    gc.compare_grav(wbc.grav_outputs(), g)
    wbc.set_torque_input(ref["tau_in"] - g["tau"])
    wbc.redistribute(add_gravity=True)
    rc.compare(_redist(wbc), ref)
    wbc.close()


def instance_limit_case(n):
    """Per-instance torque limits that bind, chosen on the restatement alone: on a double-support instance the joint the contact null space
    moves most (largest row of NwJw) is limited 1 Nm below the batch-wide answer tau_in + NwJw c, every other joint 20 Nm above it, so the
    QP has to move; an instance the restatement cannot solve under that limit keeps the batch-wide 300 Nm.  Returns (lim (n, m), ref)."""
    base = pc.state_set("fixed_head", n)
    mo, links = pc.model("fixed_head")
    m = mo["ndof"] - 6
    tstar = base["tau_in"] + base["tau"]
    lim = np.full((n, m), pc.TAU_LIM)
    ref = {k: np.array(v) for k, v in base.items()}
    for b in range(n):
        if base["flags"][b].sum() < 2:
            continue
        tight = np.abs(tstar[b]) + 20.0
        j0 = int(np.argmax(np.linalg.norm(base["nwjw"][b], axis=1)))
        tight[j0] = abs(tstar[b, j0]) - 1.0
        st, dt, c, w, nw = rc.redistribute_ref(pc.cycle_of(mo, links, tau_lim=tight), base["q"][b], base["flags"][b], base["tau_in"][b])
        if st == 1:
            lim[b] = tight
            ref["tau"][b], ref["cf"][b], ref["wrench"][b] = dt, c, w
    rc.check_premises(ref)
    moved = np.abs(ref["tau"] - base["tau"]).max(axis=1) > 0.5
    assert moved.sum() >= 3, moved  # the record changes answers (asserted on the restatement alone)
    return lim, ref


def test_instance_torque_limits_with_the_option_on_a_pack(tmp_path):
    """Batch.set_instance_params with the option: every instance against the restatement set up with its own limit"""
    n = 16
    md = _pack_model("fixed_head", tmp_path)
    cases.ensure_pack(md)
    base = pc.state_set("fixed_head", n)
    g = gc.pack_grav("fixed_head", n)
    _, links = pc.model("fixed_head")
    lim, ref = instance_limit_case(n)
    wbc = _pack_batch(md, links, n)
    wbc.set_instance_params(tau_lim=lim)
    _posed(wbc, base, tau_in=base["tau_in"] - g["tau"])
    wbc.redistribute(add_gravity=True)
    rc.compare(_redist(wbc), ref)
    gc.compare_grav(wbc.grav_outputs(), g)
    wbc.close()


def test_refusals():
    import libdwbc_amd as D

    ref = rc.state_set(B, False, "LR")
    n = 8

    def posed(**kw):
        w = _batch(n, **kw)
        w.set_state(ref["q"][:n])
        w.set_contact(ref["flags"][:n])
        return w

    w = posed()
    with pytest.raises(D.DwbcError, match="no gravity-compensation output yet"):
        w.grav_outputs()
    with pytest.raises(D.DwbcError, match="no torque input"):
        w.redistribute(add_gravity=True)
    w.set_torque_input(ref["tau_in"][:n])
    with pytest.raises(D.DwbcError, match=r"hqp = true only \(the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque\)"):
        w.redistribute(hqp=False, add_gravity=True)
    with pytest.raises(D.DwbcError, match="no gravity-compensation output yet"):
        w.grav_outputs()  # nothing was launched by the refused calls
    w.grav_compensation()
    assert (w.grav_outputs()["status"] == 1).all()
    w.set_max_active_contacts(3)
    with pytest.raises(D.DwbcError, match=r"gravity compensation: two simultaneously active contacts at most"):
        w.grav_compensation()
    with pytest.raises(D.DwbcError, match=r"gravity compensation: two simultaneously active contacts at most"):
        w.grav_kernel_name()
    with pytest.raises(D.DwbcError, match=r"redistribution of a supplied torque: two simultaneously active contacts at most"):
        w.redistribute(add_gravity=True)  # the redistribution's own refusals come first
    w.close()
    f = posed(dtype="f32")
    with pytest.raises(D.DwbcError, match="gravity compensation: fp64 batches only"):
        f.grav_compensation()
    f.close()
