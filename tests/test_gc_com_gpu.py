"""COM task levels in the general-contact kernel through the C-ABI (libdwbc_amd.Batch), B = 256, against the C restatement: the
reference's whole-body harness hierarchies as written (COM on level 0, both hands on one 12-dof level) and feet + a hand in contact
with a COM level.  Set-ups: tests/com_cases.py; tolerances: those of tests/test_wide_tasks.py for this kernel.  What the kernel
still lacks (trajectories, TASK_CUSTOM levels, the dump record, fp32, the reduced path) is refused at the solve, before any launch."""
import numpy as np
import pytest

from oracle import orc
from tests import cases
from tests import com_cases as cc

TOL_TAU, TOL_WR = 1e-6, 1e-5
B = 256
pytestmark = pytest.mark.gpu


def _batch(contacts, tasks, lim, n_active, B=B, dtype="f64"):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0, dtype=dtype)
    assert wbc.model.link_id("COM") == cc.COM
    for c in contacts:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(tasks):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    if lim is not None:
        wbc.set_torque_limit(np.array(lim))
    if n_active > 2:
        wbc.set_max_active_contacts(n_active)
    return wbc


def _solve_and_check(wbc, contacts, tasks, lim, q, fl, fs, tg, ncols):
    wbc.set_state(q)
    wbc.set_contact(fl)
    wbc.set_fstar_all(fs)
    wbc.solve()
    assert f"kernel_gc<39, 34, 64, {tg}>" in wbc.kernel_name()
    tau, wr, st = wbc.get("tau"), wbc.get("wrench"), wbc.get("status")
    M = orc.make_model(cases.tocabi_model())
    tau_r, wr_r, st_r, _ = orc.cycle_batch(M, orc.make_setup(contacts, tasks, lim), q, fl, fs, 0)
    dt, dw = np.abs(tau - tau_r).max(), np.abs(wr - wr_r[:, :ncols]).max() if wr.shape == (len(q), ncols) else np.inf
    print(f"status ok {int(st.sum())}/{len(st)} oracle {int(st_r.sum())} max|dtau| {dt:.3e} max|dwrench| {dw:.3e} {wbc.kernel_name()}")
    assert st_r.all()  # (the recipes were chosen so: com_cases.py)
    assert (st == st_r).all()
    assert wr.shape == (len(q), ncols)
    assert dt < TOL_TAU and dw < TOL_WR
    return tau


@pytest.mark.parametrize("limit", [False, True])
def test_gpu_regulation_harness_hierarchy_as_written(limit):
    q, fl, fs = cc.reg_batch(B, 43)
    lim = cases.TAU_LIM if limit else None
    wbc = _batch(cc.CONTACTS_REG, cc.TASKS_REG, lim, 2)
    tau = _solve_and_check(wbc, cc.CONTACTS_REG, cc.TASKS_REG, lim, q, fl, fs, 12, 12)
    assert np.abs(tau[:, 1]).max() > 1.0


def test_gpu_data_confirmation_harness_hierarchy_as_written():
    q, fl, fs = cc.dc_batch(B, 44)
    wbc = _batch(cc.CONTACTS_DC, cc.TASKS_DC, None, 2)
    _solve_and_check(wbc, cc.CONTACTS_DC, cc.TASKS_DC, None, q, fl, fs, 12, 12)


@pytest.mark.parametrize("name", list(cc.TASKS_3C))
def test_gpu_three_contacts_with_a_com_level(name):
    tasks, _, tg = cc.TASKS_3C[name]
    q, fl, fs = cc.three_contact_batch(name, B, 55)
    wbc = _batch(cases.CONTACTS_4, tasks, cases.TAU_LIM, 3)
    _solve_and_check(wbc, cases.CONTACTS_4, tasks, cases.TAU_LIM, q, fl, fs, tg, 18)


def test_gpu_com_level_keeps_two_workgroups_per_cu():
    """the TG = 6 map with or without a COM level: 81 696 bytes of LDS, under the 81 920 that let two workgroups share a CU's 160 KiB"""
    tasks = cc.TASKS_3C["a"][0]
    com = _batch(cases.CONTACTS_4, tasks, cases.TAU_LIM, 3, B=4)
    pel = _batch(cases.CONTACTS_4, cc.with_pelvis(tasks), cases.TAU_LIM, 3, B=4)
    assert com.launch_info()[1] <= 81920
    assert pel.launch_info()[1] == 81696 and com.launch_info()[1] == pel.launch_info()[1]
    assert com.kernel_name() == pel.kernel_name()


def test_gpu_com_level_scope_is_refused_cleanly():
    """a trajectory level, a TASK_CUSTOM level and the dump record on a three-contact batch with a COM level: the solve returns 0 with the
    reworded message and launches nothing (the outputs of the solve before stay as they were)"""
    import libdwbc_amd as D

    Bs = 32
    tasks = cc.TASKS_3C["a"][0]
    q, fl, fs = cc.three_contact_batch("a", Bs, 57)
    wbc = _batch(cases.CONTACTS_4, tasks, cases.TAU_LIM, 3, B=Bs)
    wbc.set_state(q, np.zeros((Bs, 39)))
    wbc.set_contact(fl)
    wbc.set_fstar_all(fs)
    wbc.solve()
    tau0 = wbc.get("tau")
    assert wbc.get("status").all() and np.abs(tau0).max() > 1.0
    wbc.set_fstar_all(2.0 * fs)  # a launch would give other torques
    msg = "no trajectories, no TASK_CUSTOM levels, no dump record"
    wbc.enable_dump(True)
    with pytest.raises(D.batch.DwbcError, match=msg):
        wbc.solve()
    wbc.enable_dump(False)
    tr = np.zeros((Bs, 34))
    tr[:, 1] = 1.0
    wbc.set_task_gain(1, 0, 100.0, 10.0, 0.0, 100.0, 10.0)
    wbc.set_trajectory(1, 0, tr)
    wbc.set_control_time(0.5)
    with pytest.raises(D.batch.DwbcError, match=msg):
        wbc.solve()
    wbc.set_trajectory(1, 0, None)
    wbc.add_custom_task(2, 3)
    with pytest.raises(D.batch.DwbcError, match=msg):
        wbc.solve()
    wbc.sync()
    assert (wbc.get("tau") == tau0).all()


def test_gpu_com_level_fp32_and_reduced_are_refused():
    import libdwbc_amd as D

    Bs = 8
    q, fl, fs = cc.reg_batch(Bs, 45)
    f32 = _batch(cc.CONTACTS_REG, cc.TASKS_REG, None, 2, B=Bs, dtype="f32")
    f32.set_state(q)
    f32.set_contact(fl)
    f32.set_fstar_all(fs)
    with pytest.raises(D.batch.DwbcError, match="fp64 batches only"):
        f32.solve()
    with pytest.raises(D.batch.DwbcError, match="fp64 batches only"):
        f32.set_max_active_contacts(3)
    red = _batch(cc.CONTACTS_REG, cc.TASKS_REG, None, 2, B=Bs)
    red.set_state(q)
    red.set_contact(fl)
    red.set_fstar_all(fs)
    with pytest.raises(D.batch.DwbcError, match="not built on the reduced dynamics path"):
        red.solve(reduced=True)
    red.solve()  # the same batch on the full model
    assert red.get("status").all()
