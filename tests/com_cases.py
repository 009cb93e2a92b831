"""Set-ups with the synthetic COM link (link id = number of links: 34 for TOCABI) on a task level of the general-contact kernel, shared
by tests/test_gc_com_emu.py, tests/test_gc_com_gpu.py and the tools.

REG  the hierarchy of the reference's tests/sp_test/regulation_test.cpp:27,82-94 as written: COM 6D, pelvis rotation, upper-body
     rotation, both hands 6D + 6D on one level; four registered contacts, the feet raised.
DC   tests/sp_test/data_confirmation.cpp:27,41-73: the same with COM POSITION on level 0; instance 0 is the harness's own q2 / f*.
3C   feet + a hand in contact with a COM level: (a) .. (f) below.

Every recipe gives status 1 on every instance in the C restatement (oracle/dwbc_oracle.c) at B = 256 (B = 512 for the mixed flags of
(f)), so the tests assert `st_r.all()`.  No recipe has a hand both in contact and as a task link: the oracle itself returns status 0
or torques of 1e5 Nm there."""
import numpy as np

from tests import cases
from tests.test_wide_tasks import Q_REG, regulation_batch

COM = 34  # dwbc_model_link_id("COM") for TOCABI
T6, TP, TR = cases.TASK_LINK_6D, 3, cases.TASK_LINK_ROTATION  # TASK_LINK_POSITION = 3 (include/dwbc_task.h:23-33)
Z = (0, 0, 0)

TASKS_REG = [[(T6, COM, Z)], [(TR, 0, Z)], [(TR, 15, Z)], [(T6, 23, Z), (T6, 33, Z)]]
TASKS_DC = [[(TP, COM, Z)], [(TR, 0, Z)], [(TR, 15, Z)], [(T6, 23, Z), (T6, 33, Z)]]
FEET = [1, 1, 0, 0]


def contacts(lx, ly):
    """the four registered contacts with the feet's half-sizes of the harness (regulation_test.cpp:77-78: 0.13 x 0.06,
    data_confirmation.cpp:61-62: 0.12 x 0.06); hands 0.04 x 0.04"""
    c = [dict(d) for d in cases.CONTACTS_4]
    for d in c[:2]:
        d["lx"], d["ly"] = lx, ly
    return c


CONTACTS_REG = contacts(0.13, 0.06)
CONTACTS_DC = contacts(0.12, 0.06)

# data_confirmation.cpp:41-57
Q_DC = np.array([-0.0325, -0.0579, 0.7273, 0.0194, -0.0118, -0.0008, -0.0006, 0.0698, -0.7835, 1.6487, -0.8420, -0.0911,
                 -0.0007, 0.0767, -0.7963, 1.6742, -0.8549, -0.1150, -0.0001, -0.0003, 0.0204,
                 0.2998, 0.3001, 1.5000, -1.2701, -1.0507, 0.0000, -1.0000, 0.0000, -0.0000, 0.0003,
                 -0.2998, -0.3060, -1.5001, 1.2700, 1.0848, 0.0000, 1.0000, 0.0000, 0.9997])
F_DC = np.array([0.3142, -1.8202, -1.7750, -17.8677, 8.4977, 1.0850, -8.5340, 8.5992, 1.2655,
                 4.0251, 3.9975, 7.5672, -8.2841, 30.3652, 0.8954, 2.7585, 3.7898, 9.3234, -9.5724, 43.8036, 2.5202])


def reg_batch(B, seed):
    """states and the 24 f* columns of tests/test_wide_tasks.regulation_batch"""
    q, fs = regulation_batch(B, seed)
    return q, np.tile(np.array(FEET, np.uint8), (B, 1)), fs


def dc_batch(B, seed):
    """instance 0: q2 and fstar_0..3 of the harness; the others q2 + 0.01 U(-1, 1) with the quaternion re-normalised and
    f* (1 + 0.1 U(-1, 1))"""
    rng = np.random.Generator(np.random.Philox(seed))
    q = Q_DC[None, :] + 0.01 * rng.uniform(-1, 1, size=(B, 40))
    q[0] = Q_DC
    q[:, [3, 4, 5, 39]] /= np.linalg.norm(q[:, [3, 4, 5, 39]], axis=1, keepdims=True)
    fs = F_DC[None, :] * (1 + 0.1 * rng.uniform(-1, 1, size=(B, 21)))
    fs[0] = F_DC
    return q, np.tile(np.array(FEET, np.uint8), (B, 1)), fs


# name -> (tasks, flags of every instance or None for the mixed batch, TG of the instantiation that serves it)
TASKS_3C = {
    "a": ([[(T6, COM, Z)], [(TR, 15, Z)]], [1, 1, 1, 0], 6),
    "b": ([[(T6, COM, Z)], [(T6, 33, Z), (T6, 25, Z)]], [1, 1, 1, 0], 12),
    "c": ([[(TR, 0, Z)], [(TP, COM, Z)], [(T6, 33, Z)]], [1, 1, 1, 0], 6),  # the COM is not on level 0
    "d": ([[(TP, COM, Z)], [(TR, 0, Z)], [(TR, 15, Z)], [(T6, 33, Z)]], [1, 1, 1, 0], 6),  # four levels
    "e": ([[(T6, COM, Z)], [(T6, 23, Z), (T6, 25, Z)]], [1, 1, 0, 1], 12),
    "f": ([[(T6, COM, Z)], [(TR, 15, Z)]], None, 6),
}
FLAGS_MIXED = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 1, 0]], np.uint8)


def task_dof(tasks):
    return sum(6 if m <= 2 else 3 for lv in tasks for (m, _, _) in lv)


def posture_batch(B, seed, ndof_f):
    """Q_REG + 0.01 U with a random yaw and +-0.05 of tilt; f* = 0.3 U(-1, 1)"""
    rng = np.random.Generator(np.random.Philox(seed))
    q = Q_REG[None, :] + 0.01 * rng.uniform(-1, 1, size=(B, 40))
    q[:, 3:6] = 0.0
    q[:, 39] = 1.0
    for b in range(B):
        qu = cases.yaw_quat(rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05))
        q[b, 3:6] = qu[:3]
        q[b, 39] = qu[3]
    fs = 0.3 * rng.uniform(-1, 1, size=(B, ndof_f))
    return q, fs, rng


def three_contact_batch(name, B, seed, tasks=None):
    tasks_, flags, _ = TASKS_3C[name]
    tasks = tasks_ if tasks is None else tasks
    q, fs, rng = posture_batch(B, seed, task_dof(tasks))
    fl = np.tile(np.array(flags, np.uint8), (B, 1)) if flags is not None else FLAGS_MIXED[rng.integers(0, len(FLAGS_MIXED), size=B)]
    return q, fl, fs


def with_pelvis(tasks):
    """the same hierarchy with the pelvis (link 0) where the COM link stands"""
    return [[(m, 0 if l == COM else l, p) for (m, l, p) in lv] for lv in tasks]
