"""gpu: per-instance torque limits and contact cone constants (dwbc_batch_set_instance_params / bind_instance_params ->
BatchIO::inst_par) through the C-ABI, in every kernel that fills QP rows.

Inputs, premises and bars: tests/inst_par_cases.py (states of synth_batch seed 7, yaw, mixed support; limits TAU_LIM * U(0.15, 0.5) from
default_rng(29), contact constants times U(0.4, 1.0) from default_rng(23); the C restatement with one set-up per instance; 1e-6 Nm,
1e-5 N, status identical).  The six launch routes are those of tests/test_launch_flavours.py, forced by its switches."""
import numpy as np
import pytest

from tests import cases
from tests import inst_par_cases as ic
from tests import redist_cases as rc
from tests.test_launch_flavours import ROUTES, _set_env

pytestmark = pytest.mark.gpu

B = 250
OUT = ("tau", "wrench", "status")


def _make(nb, contacts=cases.CONTACTS_2, tasks=cases.TASKS_2LEVEL, tau_lim=cases.TAU_LIM, dtype="f64", urdf=cases.URDF, model=None):
    import libdwbc_amd as D

    wbc = D.Batch(model or D.Model.from_urdf(urdf), nb, device=0, dtype=dtype)
    for c in contacts:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(tasks):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(None if tau_lim is None else np.array(tau_lim, float))
    return wbc


def _load(wbc, q, flags, fstar):
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)


def _solve(wbc):
    wbc.solve()
    return {k: wbc.get(k) for k in OUT}


def _routed(monkeypatch, route, nb, **kw):
    """a batch created under the switches of `route` (they stay set for the solves of the test)"""
    _set_env(monkeypatch, ROUTES[route][0])
    return _make(nb, **kw)


def _check_route(wbc, route, levels=2):
    env, name, threads = ROUTES[route]
    assert wbc.kernel_name() == name.format(L=levels), (route, wbc.kernel_name())
    assert wbc.launch_info()[0] == threads
    if route == "capped_extras":
        cases.check_route(wbc, "capped", levels)


def _bit_equal(a, b, what, rows=slice(None)):
    for k in OUT:
        assert (a[k][rows] == b[k][rows]).all(), (what, k)


def _moved(ref, base):
    return np.abs(ref[0].sum(axis=1) - base[0].sum(axis=1)).max(axis=1)


def _index_check(make_batchwide, got, lim, con, states, B_, what, moved):
    """(f): a batch whose batch-wide parameters are record i reproduces instance i of the recorded batch bit for bit.  moved[i]: how far
    the restatement's torque of instance i under record i is from its batch-wide answer -- an instance the record does not move would
    pass on a kernel that ignores it"""
    for i in (0, B_ // 2, B_ - 1):
        assert moved[i] > ic.MOVED, (what, i, moved[i])
        w2 = make_batchwide(lim[i], con[i])
        _load(w2, *states)
        r2 = _solve(w2)
        assert r2["status"][i] == 1, (what, i)
        _bit_equal(got, r2, (what, "instance", i), rows=i)
        w2.close()


# ---------------------------------------------------------------- 4. the cycle, every route
@pytest.mark.parametrize("route", list(ROUTES))
def test_cycle_vs_restatement(route, monkeypatch):
    """(a) limits only, (b) contacts only, (c) both: each against the restatement with one set-up per instance"""
    q, flags, fstar = ic.states(B)
    base = ic.reference(B, False, False)
    wbc = _routed(monkeypatch, route, B)
    _load(wbc, q, flags, fstar)
    for lim, con in ((True, False), (False, True), (True, True)):
        what = f"{route} lim={lim} con={con}"
        ref = ic.reference(B, lim, con)
        ic.check_premises(ref, base, what)
        wbc.set_instance_params(ic.limits(B) if lim else None, ic.contact_consts(B) if con else None)
        got = _solve(wbc)
        _check_route(wbc, route)
        ic.compare(got["tau"], got["wrench"], got["status"], ref, what)
    wbc.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_cycle_bit_identities(route, monkeypatch):
    """(d) a record of the batch-wide values, (e) set then drop, (f) indexing"""
    states = ic.states(B)
    lim, con = ic.limits(B), ic.contact_consts(B)
    plain = _routed(monkeypatch, route, B)
    _load(plain, *states)
    never = _solve(plain)
    _check_route(plain, route)
    assert (never["status"] == 1).mean() >= 0.9
    wbc = _make(B)
    _load(wbc, *states)
    assert wbc.instance_param_stride == 33 + 8
    wbc.set_instance_params(np.broadcast_to(np.array(cases.TAU_LIM, float), (B, 33)), np.broadcast_to(ic.consts(cases.CONTACTS_2), (B, 2, 4)))
    _bit_equal(_solve(wbc), never, (route, "batch-wide record"))
    _check_route(wbc, route)
    wbc.set_instance_params(lim, con)
    got = _solve(wbc)
    assert not (got["tau"] == never["tau"]).all()
    wbc.set_instance_params(None, None)
    _bit_equal(_solve(wbc), never, (route, "set then drop"))
    _check_route(wbc, route)
    _index_check(lambda l, c: _make(B, contacts=ic.with_consts(cases.CONTACTS_2, c), tau_lim=l), got, lim, con, states, B, route,
                 _moved(ic.reference(B, True, True), ic.reference(B, False, False)))
    # a record on a batch that never had a batch-wide limit: the torque rows exist as after set_torque_limit
    nolim = _make(B, tau_lim=None)
    _load(nolim, *states)
    nolim.set_instance_params(lim, con)
    _bit_equal(_solve(nolim), got, (route, "no batch-wide limit"))
    for w in (plain, wbc, nolim):
        w.close()


# ---------------------------------------------------------------- 5. the other consumers
def test_bound_tensor_equals_host_record():
    import torch

    states = ic.states(B)
    lim, con = ic.limits(B), ic.contact_consts(B)
    host, bound = _make(B), _make(B)
    for w in (host, bound):
        _load(w, *states)
    host.set_instance_params(lim, con)
    t = torch.from_numpy(ic.record(B, lim, con)).to("cuda:0")
    bound.bind_instance_params(t)
    a, b = _solve(host), _solve(bound)
    _bit_equal(a, b, "bound")
    ic.compare(b["tau"], b["wrench"], b["status"], ic.reference(B, True, True), "bound")
    import libdwbc_amd as D

    with pytest.raises(D.DwbcError, match="bound to a device buffer"):
        bound.set_instance_params(lim, con)
    # the tensor is read in place: what the caller writes into it holds for the next launch
    t.copy_(torch.from_numpy(ic.record(B, None, None)))
    torch.cuda.synchronize()
    never = _make(B)
    _load(never, *states)
    _bit_equal(_solve(bound), _solve(never), "tensor rewritten in place")
    bound.bind_instance_params(None)
    _bit_equal(_solve(bound), _solve(never), "unbound")
    bound.set_instance_params(lim, con)  # accepted again
    _bit_equal(_solve(bound), a, "host record after unbinding")
    for w in (host, bound, never):
        w.close()


def _redist_out(wbc):
    return dict(tau=wbc.get("redist_tau"), cf=wbc.get("redist_cf"), wrench=wbc.get("redist_wrench"), status=wbc.get("redist_status"))


def test_redistribution_kernel():
    ref = ic.redist_reference(B)
    rc.check_premises(ref)
    ic.redist_moved(ref)
    wbc = _make(B, tasks=())
    wbc.set_state(ref["q"])
    wbc.set_contact(ref["flags"])
    wbc.set_torque_input(ref["tau_in"])
    wbc.redistribute()
    plain = _redist_out(wbc)  # the batch-wide constants on the same inputs
    wbc.set_instance_params(None, ref["con"])
    wbc.redistribute()
    rc.compare(_redist_out(wbc), ref)
    wbc.set_instance_params(None, np.broadcast_to(ic.consts(cases.CONTACTS_2), (B, 2, 4)))
    wbc.redistribute()
    same = _redist_out(wbc)
    for k in same:
        assert (same[k] == plain[k]).all(), k
    wbc.close()


def test_general_contact_kernel():
    """feet + left hand of four registered contacts (stride 33 + 16): against the C restatement, (d) and (f)"""
    nb = 64
    q, _, fstar = cases.synth_batch(nb, seed=7, yaw=True)
    flags = np.tile(np.array([1, 1, 1, 0], np.uint8), (nb, 1))
    states = (q, flags, fstar)
    lim, con = ic.limits(nb), ic.contact_consts(nb, cases.CONTACTS_4)
    base = ic.orc_reference(q, flags, fstar, None, None, contacts=cases.CONTACTS_4)
    ref = ic.orc_reference(q, flags, fstar, lim, con, contacts=cases.CONTACTS_4)
    ic.check_premises(ref, base, "general-contact")

    def make(contacts=cases.CONTACTS_4, tau_lim=cases.TAU_LIM):
        w = _make(nb, contacts=contacts, tau_lim=tau_lim)
        w.set_max_active_contacts(3)
        return w

    wbc = make()
    assert wbc.instance_param_stride == 33 + 16
    _load(wbc, *states)
    never = _solve(wbc)
    assert "dwbc_cycle_kernel_gc<39, 34, 64, 6>" in wbc.kernel_name()
    wbc.set_instance_params(None, np.broadcast_to(ic.consts(cases.CONTACTS_4), (nb, 4, 4)))
    _bit_equal(_solve(wbc), never, "gc batch-wide record")
    wbc.set_instance_params(lim, con)
    got = _solve(wbc)
    assert "dwbc_cycle_kernel_gc<39, 34, 64, 6>" in wbc.kernel_name()
    ic.compare(got["tau"], got["wrench"], got["status"], (ref[0], ref[1][:, :18], ref[2]), "general-contact")
    _index_check(lambda l, c: make(ic.with_consts(cases.CONTACTS_4, c), l), got, lim, con, states, nb, "general-contact", _moved(ref, base))
    wbc.close()


def test_kernel_pack_37_dof(tmp_path):
    """(d) and (f) on the 37-dof / 32-body pack (TOCABI with the head fixed)"""
    import libdwbc_amd as D
    from oracle import dwbc_np, urdf_model
    from tests.test_model_packs import variant_states

    nb = 64
    path = cases.variant_urdf(tmp_path / "fixed_head.urdf", cases.HEAD_JOINTS)
    md = D.Model.from_urdf(path)
    cases.ensure_pack(md)
    mo = urdf_model.load_urdf(path)
    q, fstar = variant_states(mo, nb, seed=7)
    states = (q, np.ones((nb, 2), np.uint8), fstar)
    links = [md.link_id("L_AnkleRoll_Link"), md.link_id("R_AnkleRoll_Link"), md.link_id("Upperbody_Link")]
    contacts = [dict(cc, link=l) for cc, l in zip(cases.CONTACTS_2, links[:2])]
    tasks = [[(D.TASK_LINK_6D, 0, (0, 0, 0))], [(D.TASK_LINK_ROTATION, links[2], (0, 0, 0))]]
    m = md.ndof - 6
    lim, con = ic.limits(nb, m), ic.contact_consts(nb)

    def make(contacts_=contacts, tau_lim=np.full(m, 300.0)):
        return _make(nb, contacts=contacts_, tasks=tasks, tau_lim=tau_lim, model=md)

    wbc = make()
    assert wbc.instance_param_stride == m + 8
    _load(wbc, *states)
    never = _solve(wbc)
    assert "<37, 32," in wbc.kernel_name() and (never["status"] == 1).mean() >= 0.9
    wbc.set_instance_params(None, np.broadcast_to(ic.consts(contacts), (nb, 2, 4)))
    _bit_equal(_solve(wbc), never, "pack batch-wide record")
    wbc.set_instance_params(lim, con)
    got = _solve(wbc)

    def restated(i, l, c):  # the numpy restatement (model-generic as written) of instance i under these parameters
        cy = dwbc_np.Cycle(mo)
        for cc in ic.with_consts(contacts, c):
            cy.add_contact(cc["link"], cc["point"], cc["lx"], cc["ly"], cc["mu"], cc["muz"])
        for lv, lks in enumerate(tasks):
            for mode, link, pt in lks:
                cy.add_task(lv, mode, link, pt)
        cy.set_torque_limit(l)
        tau = cy.run(q[i], [1, 1], [fstar[i, :6], fstar[i, 6:9]])
        assert cy.status == 1
        return tau

    moved = {i: np.abs(restated(i, lim[i], con[i]) - restated(i, np.full(m, 300.0), ic.consts(contacts))).max() for i in (0, nb // 2, nb - 1)}
    _index_check(lambda l, c: make(ic.with_consts(contacts, c), l), got, lim, con, states, nb, "pack", moved)
    wbc.close()


def test_fp32():
    """(d) and (f) on flat feet; no fp32 tolerance of its own"""
    nb = 64
    states = cases.synth_batch(nb, seed=7)
    lim, con = ic.limits(nb), ic.contact_consts(nb)
    wbc = _make(nb, dtype="f32")
    _load(wbc, *states)
    never = _solve(wbc)
    assert wbc.kernel_name().startswith("dwbc_f32::") and (never["status"] == 1).mean() >= 0.9
    wbc.set_instance_params(None, np.broadcast_to(ic.consts(cases.CONTACTS_2), (nb, 2, 4)))
    _bit_equal(_solve(wbc), never, "fp32 batch-wide record")
    wbc.set_instance_params(lim, con)
    got = _solve(wbc)
    base, ref = ic.orc_reference(*states, None, None), ic.orc_reference(*states, lim, con)  # (fp64 restatement: the premises only)
    ic.check_premises(ref, base, "flat feet")
    _index_check(lambda l, c: _make(nb, contacts=ic.with_consts(cases.CONTACTS_2, c), tau_lim=l, dtype="f32"), got, lim, con, states, nb, "fp32",
                 _moved(ref, base))
    wbc.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_alone():
    import libdwbc_amd as D

    nb = 64
    states = cases.synth_batch(nb, seed=7)  # flat feet, double support everywhere: the LQP configurator wants uniform flags
    lim, con = ic.limits(nb), ic.contact_consts(nb)
    wbc = _make(nb, tau_lim=None)  # (no batch-wide limit: the reduced path would refuse that first)
    wbc.enable_dump(True)
    _load(wbc, *states)
    wbc.set_instance_params(lim, con)
    before = _solve(wbc)
    diag = wbc.get("diag")
    assert (before["status"] == 1).mean() >= 0.9

    def untouched(what):
        for k in OUT:
            assert (wbc.get(k) == before[k]).all(), (what, k)
        assert (wbc.get("diag") == diag).all(), what

    with pytest.raises(D.DwbcError, match="per-instance parameters: not built on the reduced dynamics path"):
        wbc.solve(reduced=True)
    untouched("reduced")
    with pytest.raises(D.DwbcError, match="per-instance parameters: hqp = true only"):
        wbc.solve(hqp=False)
    untouched("hqp = false")
    hq = D.HQP.for_lqp(wbc, 12)
    with pytest.raises(D.DwbcError, match="LQP / JACC: per-instance parameters"):
        hq.configure_lqp(wbc)
    with pytest.raises(D.DwbcError, match="LQP / JACC: per-instance parameters"):
        hq.solve_jacc(wbc, 0)
    untouched("LQP / JACC")
    # existing refusals keep their precedence
    with pytest.raises(D.DwbcError, match="hqp=false is not built on the reduced dynamics path"):
        wbc.solve(hqp=False, reduced=True)
    # without the record all of them are served again
    wbc.set_instance_params(None, None)
    wbc.solve(hqp=False)
    wbc.solve(reduced=True)
    wbc.solve()
    hq.configure_lqp(wbc)
    wbc.close()


def test_bad_records_are_refused_and_add_contact_drops():
    import libdwbc_amd as D

    nb = 64
    states = cases.synth_batch(nb, seed=7, yaw=True, contact_mode="mixed")
    lim, con = ic.limits(nb), ic.contact_consts(nb)
    wbc = _make(nb)
    _load(wbc, *states)
    wbc.set_instance_params(lim, con)
    good = _solve(wbc)
    for what, (i, j, v) in {"nan": (3, 5, np.nan), "inf": (nb - 1, 32, np.inf), "zero": (0, 0, 0.0), "negative": (7, 1, -1.0)}.items():
        bad = lim.copy()
        bad[i, j] = v
        with pytest.raises(D.DwbcError, match="finite and > 0"):
            wbc.set_instance_params(bad, con)
        _bit_equal(_solve(wbc), good, what)  # the previous record holds
    badc = con.copy()
    badc[nb // 2, 1, 3] = -0.1
    with pytest.raises(D.DwbcError, match="finite and > 0"):
        wbc.set_instance_params(lim, badc)
    _bit_equal(_solve(wbc), good, "negative mu_z")
    nolim = _make(nb, tau_lim=None)
    with pytest.raises(D.DwbcError, match="no batch-wide torque limit"):
        nolim.set_instance_params(None, con)
    nolim.close()
    # add_contact drops the record: the batch-wide values hold again, and the stride has grown
    never = _make(nb)
    _load(never, *states)
    plain = _solve(never)
    c3 = cases.CONTACTS_4[2]
    for w in (wbc, never):
        w.add_contact(c3["link"], c3["point"], c3["lx"], c3["ly"], c3["mu"], c3["muz"])
        w.set_contact(np.concatenate([states[1], np.zeros((nb, 1), np.uint8)], axis=1))
    assert wbc.instance_param_stride == 33 + 12
    _bit_equal(_solve(wbc), _solve(never), "add_contact drops the record")
    _bit_equal(_solve(never), plain, "an inactive third contact changes nothing")
    for w in (wbc, never):
        w.close()
