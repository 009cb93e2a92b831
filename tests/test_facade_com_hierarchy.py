"""The reference's whole-body harness hierarchy through the drop-in class include/dwbc_amd.hpp (tests/cpp/facade_com_hierarchy.cpp:
tests/sp_test/regulation_test.cpp:81-129 as written -- "COM" 6D on level 0, both hands on level 3, SetContact(1, 1, 0, 0)).
not-gpu: it compiles and links.   gpu: the three torque vectors and the contact force against the C restatement."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import com_cases as cc

ROOT = cases.ROOT
EXE = os.path.join(ROOT, "tests", "cpp", "facade_com_hierarchy")
TOL_TAU, TOL_WR = 1e-6, 1e-5


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "facade_com_hierarchy.cpp")
    libdir = os.path.join(ROOT, "libdwbc_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE, "-L" + libdir, "-l:libdwbc_hip.so",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])


def test_facade_com_hierarchy_compiles():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_facade_regulation_harness_with_the_com_on_level_0():
    from oracle import orc
    from tests.test_wide_tasks import Q_REG

    _build()
    out = subprocess.check_output([EXE, cases.URDF], text=True)
    r = json.loads(out[out.index("{"):])
    e = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b).reshape(-1)).max())
    q = Q_REG[None, :].copy()
    q[0, 2] = 0.0  # the harness leaves the pelvis at the origin (regulation_test.cpp:64)
    f1 = np.array([0.5, 0.3, 0.2, 0.12, -0.11, 0.05])  # rot_z = 0: link_[0].rotm is the identity
    fs = np.concatenate([[-2, -2.2, 0.2, 0.5, 0.4, -0.6], f1[3:], -f1[3:], 0.5 * f1, 0.2 * f1])[None, :]
    M = orc.make_model(cases.tocabi_model())
    S = orc.make_setup(cc.CONTACTS_REG, cc.TASKS_REG, None)
    tau, wr, st, _ = orc.cycle_batch(M, S, q, np.array([cc.FEET], np.uint8), fs, 0)
    assert st[0] == 1
    assert r["com_id"] == cc.COM and r["dims"] == [4, 6, 12, 12] and r["ok"] == [1, 1, 1]
    assert e(r["pelvis_rotm"], np.eye(3)) == 0.0
    d = [e(r["torque_grav_"], tau[0, 0]), e(r["torque_task_"], tau[0, 1]), e(r["torque_contact_"], tau[0, 2]), e(r["contact_force"], wr[0, :12])]
    print("max|d| grav task contact wrench:", d)
    assert max(d[:3]) < TOL_TAU and d[3] < TOL_WR
    assert np.abs(tau[0, 1]).max() > 1.0
