"""gpu: CalcSingleTaskTorqueWithQP of one task level as a lean launch (dwbc_batch_calc_single_task_torque_qp -> dwbc_task_qp_kernel,
libdwbc_amd/csrc/dwbc_task_qp.h): every level of a hierarchy launched in turn, with Null_task from calc_task_space() and torque_prev
accumulated from grav_outputs()["tau"] and the torque_null_h of the levels above, against the numpy restatement and against tau_task of
solve() on the same batch; a level beneath a foreign torque, the failure, single support, the mask tiers, inputs and outputs bound to torch
tensors, the TopoGeneric row, per-instance torque limits, three flags on the device, the refusals, and solve() beside it.

Inputs, references, premises and bars: tests/task_qp_cases.py.  On the parent of the change that added the launch every test here fails for
lack of the entry points.  The refusal of a model without the kernel (a kernel pack's model: no pack carries one) is pinned by
tests/test_task_qp_plan.py."""
import numpy as np
import pytest

from tests import cases
from tests import task_qp_cases as qc

pytestmark = pytest.mark.gpu

KERNEL = "dwbc::dwbc_task_qp_kernel<39, 34, dwbc::TopoTocabi>"
KERNEL_ANY = "dwbc::dwbc_task_qp_kernel<39, 34, dwbc::TopoGeneric>"
ALL = list(qc.NAMES)


def _bars():
    return qc.bars(qc.MEASURED_DEVICE)


def test_bars_are_ten_times_the_measured_figures():
    b = _bars()
    assert b["f_star_qp"] == pytest.approx(6.8e-11) and b["contact_qp"] == pytest.approx(2.0e-7) and all(b[k] == 1e-6 for k in qc.TORQUES)


def _batch(s, B=None, contacts=None, dtype="f64", tau_lim=True):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B or len(s["q"]), device=0, dtype=dtype)
    for c in contacts or s["contacts"]:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for l, lv in enumerate(s["tasks"]):
        for mode, link, pt in lv:
            wbc.add_task(l, mode, link, pt)
    if tau_lim and s["tau_lim"] is not None:
        wbc.set_torque_limit(s["tau_lim"])
    return wbc


def _pose(wbc, s):
    wbc.set_state(s["q"])
    wbc.set_contact(s["flags"])
    wbc.set_fstar_all(s["fstar"])


def _level(wbc, level, torque_prev, null, names=None):
    wbc.set_task_qp(level, names)
    wbc.set_task_qp_inputs(torque_prev, null)
    wbc.calc_single_task_torque_qp()
    return wbc.task_qp()


def _chain(wbc, s, what, bar):
    """every level in turn from the launches' own outputs; returns (per-level outputs, summed torque_null_h, instances left out per level)"""
    _pose(wbc, s)
    wbc.grav_compensation()
    tau_grav = wbc.grav_outputs()["tau"]
    assert np.abs(tau_grav - s["tau_grav"]).max() <= qc.TOL
    L = len(s["tasks"])
    nulls = []
    if L > 1:
        wbc.set_task_space_outputs(["Null_task"])
        wbc.calc_task_space()
        levels, status = wbc.task_space()
        assert (status == 1).all()
        nulls = [lv["Null_task"] for lv in levels[:-1]]
    tau_task = np.zeros_like(tau_grav)
    outs, left = [], []
    for l in range(L):
        got = _level(wbc, l, tau_grav + tau_task, nulls[l - 1] if l else None)
        left.append(qc.compare(got, s["levels"][l]["ref"], bar, f"{what}, level {l}")[1])
        tau_task = tau_task + got["torque_null_h"]
        outs.append(got)
    return outs, tau_task, left


@pytest.mark.parametrize("B", [12, 130])
def test_P_every_level_in_turn_against_the_restatement_and_solve(B):
    qc.check_premises_P(B, True)
    s = qc.set_P(B, True)
    bar = _bars()
    wbc = _batch(s)
    assert wbc.task_qp_kernel_name() == KERNEL
    outs, tau_task, left = _chain(wbc, s, f"P B={B}", bar)
    assert left == [0, 0, 0, 0]
    ref_sum = sum(lv["ref"]["torque_null_h"] for lv in s["levels"])
    e_ref = float(np.abs(tau_task - ref_sum).max())
    wbc.solve()
    assert (wbc.get("status") == 1).all()
    e_solve = float(np.abs(tau_task - wbc.get("tau_task")).max())
    print(f"P B={B}: chained sum against the restatement {e_ref:.2e}, against tau_task of solve() {e_solve:.2e} (bar {qc.TOL:.0e})")
    assert e_ref <= qc.TOL and e_solve <= qc.TOL
    wbc.close()


def test_Q_a_level_beneath_a_foreign_torque():
    qc.check_premises_Q(True)
    s, r = qc.set_P(130, True), qc.set_Q(130, True)
    wbc = _batch(s)
    _pose(wbc, s)
    got = _level(wbc, r["level"], r["torque_prev"], r["null"])
    assert qc.compare(got, r["ref"], _bars(), "Q B=130")[1] == 0
    wbc.close()


def test_F_failure_is_status_zero_and_exact_zeros():
    qc.check_premises_F()
    s, r = qc.set_P(12, True), qc.set_F()
    wbc = _batch(s)
    _pose(wbc, s)
    got = _level(wbc, r["level"], r["torque_prev"], r["null"])
    assert (got["status"] == 0).all()
    assert qc.compare(got, r["ref"], _bars(), "F")[1] == 12
    for k in ALL:
        assert not got[k].any(), k
    wbc.close()


def test_S3_single_support_has_no_contact_variables():
    qc.check_premises_S3()
    s = qc.set_S3()
    wbc = _batch(s)
    outs, _, left = _chain(wbc, s, "S3", _bars())
    assert left == [0, 0, 0]
    for got in outs:
        assert not got["contact_qp"].any() and not got["torque_contact"].any()
    wbc.close()


def test_mask_tiers_equal_the_full_run():
    s = qc.set_P(12, True)
    lv = s["levels"][2]
    wbc = _batch(s)
    _pose(wbc, s)
    full = _level(wbc, 2, lv["torque_prev"], lv["null"])
    one = _level(wbc, 2, lv["torque_prev"], lv["null"], ["f_star_qp"])
    assert sorted(one) == ["f_star_qp", "status"] and (one["f_star_qp"] == full["f_star_qp"]).all() and (one["status"] == full["status"]).all()
    st = _level(wbc, 2, lv["torque_prev"], lv["null"], ["status"])
    assert sorted(st) == ["status"] and (st["status"] == full["status"]).all()
    assert [wbc._L.dwbc_batch_task_qp_bytes(wbc._h, i) for i in range(7)] == [0, 0, 0, 0, 0, 12 * 4, 0]
    wbc.close()


def test_bound_tensors_give_the_host_paths_numbers():
    import torch

    s = qc.set_P(12, True)
    lv = s["levels"][1]
    host = _batch(s)
    _pose(host, s)
    want = _level(host, 1, lv["torque_prev"], lv["null"])
    dev = _batch(s)
    _pose(dev, s)
    dev.set_task_qp(1)
    tp = torch.tensor(lv["torque_prev"], dtype=torch.float64, device="cuda:0")
    nl = torch.tensor(lv["null"], dtype=torch.float64, device="cuda:0")
    dev.bind_task_qp_input("torque_prev", tp)
    dev.bind_task_qp_input("null", nl)
    t = {k: torch.full(want[k].shape, -1, dtype=torch.int32 if k == "status" else torch.float64, device="cuda:0") for k in want}
    for k in want:
        dev.bind_task_qp(k, t[k])
    dev.calc_single_task_torque_qp()
    dev.sync()
    for k in want:
        assert (t[k].cpu().numpy() == want[k]).all(), k
    got = dev.task_qp()
    for k in want:
        assert (got[k] == want[k]).all(), k
    # the null matrix let go of: the identity (level 0's inputs)
    dev.set_task_qp(0)
    for k in want:
        dev.bind_task_qp(k, t[k])
    dev.bind_task_qp_input("null", None)
    tp.copy_(torch.tensor(s["levels"][0]["torque_prev"], dtype=torch.float64))
    torch.cuda.synchronize()
    dev.calc_single_task_torque_qp()
    want0 = _level(host, 0, s["levels"][0]["torque_prev"], None)
    got0 = dev.task_qp()
    for k in want0:
        assert (got0[k] == want0[k]).all(), k
    host.close()
    dev.close()


def test_a_new_task_space_request_leaves_the_bound_tensors_held():
    """Null_task of this launch comes from calc_task_space(): a task-space request set after the task-QP tensors were bound must not let go
    of them (the library keeps their device pointers); a change of the task levels, which drops the request in the library, does"""
    import gc
    import weakref

    import torch

    import libdwbc_amd as D

    s = qc.set_P(12, True)
    lv = s["levels"][1]
    host = _batch(s)
    _pose(host, s)
    want = _level(host, 1, lv["torque_prev"], lv["null"])
    host.close()
    dev = _batch(s)
    _pose(dev, s)
    dev.set_task_qp(1)
    bound = {"in_torque_prev": torch.tensor(lv["torque_prev"], dtype=torch.float64, device="cuda:0"),
             "in_null": torch.tensor(lv["null"], dtype=torch.float64, device="cuda:0"),
             "torque_null_h": torch.full((12, 33), -1.0, dtype=torch.float64, device="cuda:0"),
             "status": torch.full((12,), -1, dtype=torch.int32, device="cuda:0")}
    dev.bind_task_qp_input("torque_prev", bound["in_torque_prev"])
    dev.bind_task_qp_input("null", bound["in_null"])
    dev.bind_task_qp("torque_null_h", bound["torque_null_h"])
    dev.bind_task_qp("status", bound["status"])
    refs = {k: weakref.ref(t) for k, t in bound.items()}
    out = bound["torque_null_h"]
    del bound
    for names in (["Null_task"], ["J_task"], []):
        dev.set_task_space_outputs(names)
        gc.collect()
        for k, r in refs.items():
            assert r() is not None and dev._keep[f"task_qp_{k}"] is r(), (names, k)
    dev.set_task_space_outputs(["Null_task"])
    dev.calc_task_space()
    dev.calc_single_task_torque_qp()
    dev.sync()
    assert (out.cpu().numpy() == want["torque_null_h"]).all() and (refs["status"]().cpu().numpy() == want["status"]).all()
    # a new task-QP request lets go of the outputs (the library released them) and keeps the inputs
    dev.set_task_qp(1, ["torque_h"])
    assert sorted(k for k in dev._keep if k.startswith("task_qp_")) == ["task_qp_in_null", "task_qp_in_torque_prev"]
    # the levels change: the library drops the request and the inputs, and so does the Batch
    dev.close()
    two = _batch(dict(s, tasks=s["tasks"][:2]))
    two.set_task_qp(1)
    tp = torch.tensor(lv["torque_prev"], dtype=torch.float64, device="cuda:0")
    two.bind_task_qp_input("torque_prev", tp)
    two.add_task(2, D.TASK_LINK_6D, 23)
    assert not [k for k in two._keep if k.startswith("task_qp_")]
    with pytest.raises(D.DwbcError, match="no single-level task-QP request"):
        two.calc_single_task_torque_qp()
    two.close()


def test_builtin_generic_row(monkeypatch):
    """a TOCABI batch created under DWBC_DENSE_SWEEP (any 34-body tree) takes the built-in TopoGeneric row"""
    s = qc.set_P(12, True)
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    wbc = _batch(s)
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    assert wbc.task_qp_kernel_name() == KERNEL_ANY
    _, _, left = _chain(wbc, s, "P B=12, TopoGeneric", _bars())
    assert left == [0, 0, 0, 0]
    wbc.close()


def test_per_instance_torque_limits():
    st = qc.check_premises_inst_lim()
    s = qc.set_inst_lim()
    wbc = _batch(s)
    wbc.set_instance_params(tau_lim=s["inst_lim"])
    _, _, left = _chain(wbc, s, "per-instance limits", _bars())
    assert left == [int((row == 0).sum()) for row in st]
    wbc.close()


def test_device_bound_flags_and_three_flags():
    """an instance with three flags set on the device (which the host call refuses) fails alone, with zero outputs"""
    import torch

    s = qc.set_P(12, True)
    sub = dict(s, q=s["q"][:3], fstar=s["fstar"][:3])
    flags = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    ref = qc.chain_reference(cases.tocabi_model(), cases.CONTACTS_4, s["tasks"], sub["q"], flags, sub["fstar"], s["tau_lim"])["levels"][0]
    wbc = _batch(sub, contacts=cases.CONTACTS_4)
    fl = torch.tensor(flags, dtype=torch.uint8, device="cuda:0")
    wbc.bind_tensor("in_contact", fl)
    wbc.set_state(sub["q"])
    wbc.set_fstar_all(sub["fstar"])
    got = _level(wbc, 0, ref["torque_prev"], None)
    assert got["status"].tolist() == [1, 0, 1]
    assert qc.compare(got, ref["ref"], _bars(), "device-bound flags, three flags in instance 1")[1] == 1
    for k in ALL:
        assert not got[k][1].any(), k
    wbc.close()


def test_refusals():
    import libdwbc_amd as D

    s = qc.set_P(12, True)
    lv = s["levels"][0]
    f = _batch(s, dtype="f32")
    with pytest.raises(D.DwbcError, match="single-level task QP: fp64 batches only"):
        f.set_task_qp(0)
    with pytest.raises(D.DwbcError, match="single-level task QP: fp64 batches only"):
        f.calc_single_task_torque_qp()
    f.close()
    w = _batch(s)
    _pose(w, s)
    with pytest.raises(D.DwbcError, match="no single-level task-QP request"):
        w.calc_single_task_torque_qp()
    with pytest.raises(D.DwbcError, match="unknown output bit"):
        D.batch._check(w._L.dwbc_batch_set_task_qp(w._h, 0, 1 << 6))
    for level in (-1, 4):
        with pytest.raises(D.DwbcError, match="single-level task QP: no such task level"):
            w.set_task_qp(level)
    w.set_task_qp(0, ["f_star_qp", "torque_h"])
    with pytest.raises(D.DwbcError, match="single-level task QP: no torque_prev"):
        w.calc_single_task_torque_qp()
    with pytest.raises(D.DwbcError, match="torque_prev is NULL"):
        D.batch._check(w._L.dwbc_batch_set_task_qp_inputs(w._h, None, None))
    w.set_task_qp_inputs(lv["torque_prev"])
    with pytest.raises(D.DwbcError, match="no single-level task-QP output yet"):
        w.task_qp()
    w.calc_single_task_torque_qp()
    before = w.task_qp()
    assert sorted(before) == ["f_star_qp", "status", "torque_h"]
    buf = np.zeros((12, 33))
    get = w._L.dwbc_batch_get_task_qp
    with pytest.raises(D.DwbcError, match="this output was not asked for"):
        D.batch._check(get(w._h, D.TASK_QP_OUTPUTS["torque_contact"], buf.ctypes.data, buf.nbytes))
    with pytest.raises(D.DwbcError, match="single-level task QP: the host buffer has"):
        D.batch._check(get(w._h, D.TASK_QP_OUTPUTS["torque_h"], buf.ctypes.data, buf.nbytes - 8))
    with pytest.raises(D.DwbcError, match="single-level task QP: unknown output"):
        D.batch._check(get(w._h, 6, buf.ctypes.data, buf.nbytes))
    # a bound buffer of the wrong size; set while bound
    import torch

    small = torch.zeros(12 * 33 - 1, dtype=torch.float64, device="cuda:0")
    with pytest.raises(D.DwbcError, match="single-level task QP: the device buffer has"):
        w.bind_task_qp("torque_h", small)
    with pytest.raises(D.DwbcError, match="single-level task QP: the device buffer has"):
        w.bind_task_qp_input("torque_prev", small)
    with pytest.raises(D.DwbcError, match="single-level task QP: the device buffer has"):
        w.bind_task_qp_input("null", small)
    with pytest.raises(D.DwbcError, match="single-level task QP: unknown input"):
        D.batch._check(w._L.dwbc_batch_bind_task_qp_input(w._h, 2, small.data_ptr(), 8))
    tp = torch.tensor(lv["torque_prev"], dtype=torch.float64, device="cuda:0")
    w.bind_task_qp_input("torque_prev", tp)
    with pytest.raises(D.DwbcError, match="torque_prev is bound to a device buffer"):
        w.set_task_qp_inputs(lv["torque_prev"])
    w.bind_task_qp_input("torque_prev", None)
    with pytest.raises(D.DwbcError, match="single-level task QP: no torque_prev"):
        w.calc_single_task_torque_qp()
    w.set_task_qp_inputs(lv["torque_prev"])
    # a level that carries a trajectory
    w.set_trajectory(1, 0, np.zeros((12, 34)))
    with pytest.raises(D.DwbcError, match="single-level task QP: the level carries a trajectory"):
        w.set_task_qp(1)
    w.set_trajectory(1, 0, None)
    w.set_max_active_contacts(3)
    with pytest.raises(D.DwbcError, match="single-level task QP: two simultaneously active contacts at most"):
        w.calc_single_task_torque_qp()
    with pytest.raises(D.DwbcError, match="single-level task QP: two simultaneously active contacts at most"):
        w.task_qp_kernel_name()
    after = w.task_qp()  # nothing was launched
    assert all((after[k] == before[k]).all() for k in before)
    w.set_max_active_contacts(2)
    w.close()
    # a change of the task levels drops the request and the inputs
    g = _batch(dict(s, tasks=s["tasks"][:2]))
    g.set_task_qp(1)
    g.set_task_qp_inputs(lv["torque_prev"])
    g.add_task(2, D.TASK_LINK_6D, 23)
    assert [g._L.dwbc_batch_task_qp_bytes(g._h, i) for i in range(6)] == [0] * 6
    with pytest.raises(D.DwbcError, match="no single-level task-QP request"):
        g.calc_single_task_torque_qp()
    g.add_task(2, D.TASK_LINK_6D, 33)  # a second 6D link: the level is 12 dof wide
    with pytest.raises(D.DwbcError, match="single-level task QP: task levels of at most 6 dof"):
        g.set_task_qp(0)
    g.close()
    c = _batch(dict(s, tasks=s["tasks"][:1]))
    c.add_custom_task(1, 3)
    with pytest.raises(D.DwbcError, match="single-level task QP: TASK_CUSTOM levels are not built"):
        c.set_task_qp(0)
    c.close()
    bare = _batch(dict(s, tasks=[]))
    with pytest.raises(D.DwbcError, match="single-level task QP: no task level"):
        bare.set_task_qp(0)
    bare.close()


def test_solve_before_and_after_the_launch_is_bitwise_what_it_was():
    s = qc.set_P(12, True)
    lv = s["levels"][1]
    alone = _batch(s)
    _pose(alone, s)
    alone.solve()
    want = {k: alone.get(k) for k in ("tau", "wrench", "status")}
    alone.close()
    wbc = _batch(s)
    _pose(wbc, s)
    wbc.solve()
    first = {k: wbc.get(k) for k in want}
    got = _level(wbc, 1, lv["torque_prev"], lv["null"])
    assert (got["status"] == 1).all()
    between = {k: wbc.get(k) for k in want}  # the launch names no output of the cycle
    wbc.solve()
    second = {k: wbc.get(k) for k in want}
    for k in want:
        assert (first[k] == want[k]).all() and (between[k] == want[k]).all() and (second[k] == want[k]).all(), k
    wbc.close()
