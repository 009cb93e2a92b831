"""COM task levels in the general-contact kernel (dwbc_cycle_gc.h), host emulation of the kernel source against the C restatement.

The reference's whole-body harnesses put the synthetic "COM" link on level 0 next to a 12-dof level of both hands
(tests/sp_test/regulation_test.cpp:27,82-94, data_confirmation.cpp:27,60-73); a 12-dof level, like a third contact, is served by the
general-contact kernel only.  Before this path existed the kernel's task stage indexed its link tables with link == nb, one past the
last body, and returned status 1 with torques 5 - 6 Nm off (the launcher's refusal hid it; the emulation below calls the kernel
function directly).  Set-ups and their recipes: tests/com_cases.py.  Tolerances: those of tests/test_wide_tasks.py for this kernel."""
import os

import numpy as np
import pytest

from oracle import orc
from tests import cases
from tests import com_cases as cc
from tests.emu.emu import Emu

TOL_TAU, TOL_WR = 1e-6, 1e-5


def _check(contacts, tasks, lim, q, fl, fs, model=None, urdf=cases.URDF):
    M = orc.make_model(cases.tocabi_model() if model is None else model)
    S = orc.make_setup(contacts, tasks, lim)
    tau_r, wr_r, st_r, _ = orc.cycle_batch(M, S, q, fl, fs, 0)
    r = Emu(urdf, contacts, tasks, lim).run_gc(q, fl, fs)
    dt, dw = np.abs(r["tau"] - tau_r).max(), np.abs(r["wrench"] - wr_r[:, :18]).max()
    print(f"status {r['status'].tolist()} oracle {st_r.tolist()} max|dtau| {dt:.3e} max|dwrench| {dw:.3e}")
    assert st_r.all()  # (the recipes were chosen so: com_cases.py)
    assert (r["status"] == st_r).all()
    assert np.isfinite(r["tau"]).all() and np.isfinite(r["wrench"]).all()
    assert dt < TOL_TAU and dw < TOL_WR
    return r, tau_r


@pytest.mark.parametrize("limit", [False, True])
def test_emulated_regulation_harness_hierarchy_as_written(limit):
    """COM 6D | pelvis rotation | upper-body rotation | both hands: TG = 12, two contacts of four registered"""
    q, fl, fs = cc.reg_batch(8, 41)
    assert fs.shape[1] == 24
    r, tau_r = _check(cc.CONTACTS_REG, cc.TASKS_REG, cases.TAU_LIM if limit else None, q, fl, fs)
    assert np.abs(tau_r[:, 1]).max() > 1.0  # the task torques are not trivially zero


def test_emulated_data_confirmation_harness_hierarchy_as_written():
    """COM POSITION on level 0 (the linear rows of jac_com_ alone); instance 0 is the harness's own state and f*"""
    q, fl, fs = cc.dc_batch(8, 42)
    q2 = cc.Q_DC.copy()
    q2[[3, 4, 5, 39]] /= np.linalg.norm(q2[[3, 4, 5, 39]])  # (four-digit quaternion of the harness)
    assert fs.shape[1] == 21 and (q[0] == q2).all() and (fs[0] == cc.F_DC).all()
    _check(cc.CONTACTS_DC, cc.TASKS_DC, None, q, fl, fs)


@pytest.mark.parametrize("name", list(cc.TASKS_3C))
def test_emulated_three_contacts_with_a_com_level(name):
    """feet + a hand in contact: (a) TG = 6, (b) / (e) TG = 12 with 24-variable QPs, (c) COM below level 0, (d) four levels, (f) mixed flags"""
    tasks, _, _ = cc.TASKS_3C[name]
    B = 12 if name == "f" else 6
    q, fl, fs = cc.three_contact_batch(name, B, 51)
    if name == "f":
        assert len({tuple(f) for f in fl.tolist()}) >= 4
    _check(cases.CONTACTS_4, tasks, cases.TAU_LIM, q, fl, fs)


def test_emulated_com_frame_mode_on_the_com_link_reads_no_body():
    """a *_COM_FRAME mode on the COM link: jac_ = jac_com_ all the same (no body row nb exists to take a local COM from), next to an
    ordinary link on the same level"""
    tasks = [[(1, cc.COM, cc.Z)], [(cc.TP, 33, cc.Z), (cc.TR, 15, cc.Z)]]  # TASK_LINK_6D_COM_FRAME = 1
    q, fs, _ = cc.posture_batch(4, 53, 12)
    fl = np.tile(np.array([1, 1, 1, 0], np.uint8), (4, 1))
    _check(cases.CONTACTS_4, tasks, cases.TAU_LIM, q, fl, fs)


def test_emulated_a_level_mixing_the_com_with_a_link():
    """COM POSITION and the upper body's rotation on ONE level (the reference allows any two links, src/dwbc.cpp:592-600)"""
    tasks = [[(cc.TP, cc.COM, cc.Z), (cc.TR, 15, cc.Z)], [(cc.T6, 33, cc.Z)]]
    q, fs, _ = cc.posture_batch(4, 54, 12)
    fl = np.tile(np.array([1, 1, 1, 0], np.uint8), (4, 1))
    _check(cases.CONTACTS_4, tasks, cases.TAU_LIM, q, fl, fs)


def test_emulated_com_level_on_a_37_dof_model(tmp_path):
    """the pack-size instantiation (37, 32) of tests/test_model_packs.py (TOCABI with the head fixed), COM link id 32: set-up (a) --
    feet + left hand in contact, COM 6D, upper-body rotation"""
    from tests.test_model_packs import variant_states
    from tests.test_three_contacts import _variant37

    path, mo, links = _variant37(tmp_path)
    assert mo["nb"] == 32
    B = 6
    q, fs = variant_states(mo, B, seed=19)
    fl = np.tile(np.array([1, 1, 1], np.uint8), (B, 1))
    contacts = [dict(c, link=l) for c, l in zip(cases.CONTACTS_4[:3], links[:3])]
    tasks = [[(cc.T6, 32, cc.Z)], [(cc.TR, links[3], cc.Z)]]
    _check(contacts, tasks, np.full(31, 300.0), q, fl, fs, model=mo, urdf=path)


def test_emulated_batch_without_a_com_level_is_unchanged():
    """TASKS_WIDE_3C of tests/test_wide_tasks.py against the arrays the emulation gave before the COM path existed (recorded once,
    tests/golden/gc_com): same status, tau and wrench within 1e-12 (the path is the same; the slack is for another host compiler)"""
    from tests.test_wide_tasks import TASKS_WIDE_3C, regulation_batch

    B = 6
    q, fs = regulation_batch(B, 32, tasks=TASKS_WIDE_3C)
    fl = np.tile(np.array([1, 1, 1, 0], np.uint8), (B, 1))
    r = Emu(cases.URDF, cases.CONTACTS_4, TASKS_WIDE_3C, cases.TAU_LIM).run_gc(q, fl, fs)
    g = np.load(os.path.join(cases.ROOT, "tests", "golden", "gc_com", "parent_wide_3c.npz"))
    assert (r["status"] == g["status"]).all()
    assert np.abs(r["tau"] - g["tau"]).max() < 1e-12 and np.abs(r["wrench"] - g["wrench"]).max() < 1e-12
