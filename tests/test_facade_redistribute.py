"""RobotData::CalcContactRedistribute(torque_input, hqp, init) of the header-only facade include/dwbc_amd.hpp.
not-gpu: tests/cpp/facade_redistribute.cpp compiles and links.   gpu: on the CASE 1 state the overload, handed the cycle's own torque,
leaves the torque_contact_ of the no-argument overload; a torque pushed along the contact null space is redistributed as the numpy
restatement does it (this driver computes that torque and the expected answers and passes the torque in)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import redist_cases as rc

ROOT = cases.ROOT
EXE = os.path.join(ROOT, "tests", "cpp", "facade_redistribute")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "facade_redistribute.cpp")
    libdir = os.path.join(ROOT, "libdwbc_amd")
    cmd = ["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
           "-L" + libdir, "-l:libdwbc_hip.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)


def test_facade_redistribute_compiles_and_links():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_facade_redistributes_a_supplied_torque():
    q = np.array(cases.Q_CASE[1])
    cyc = rc._cycle()
    tau = cyc.run(q, [True, True], [np.array(cases.FSTAR_CASE[1][0]), np.array(cases.FSTAR_CASE[1][1])])
    assert cyc.status == 1
    tau_in = tau + cyc.NwJw @ (10.0 * np.random.default_rng(11).standard_normal(6))
    st, dt, c, w, _ = rc.redistribute_ref(cyc, q, [1, 1], tau_in)
    assert st == 1 and np.linalg.norm(c) > 1e-3 and np.abs(dt).max() > 1.0  # the QP has work to do
    _build()
    out = subprocess.check_output([EXE, cases.URDF] + [repr(float(v)) for v in tau_in], text=True)
    r = json.loads(out[out.index("{"):])
    e = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b).reshape(-1)).max())
    # contact constraint, task torque, no-argument overload, the overload on the same torque, the perturbed torque, an Eigen-like vector;
    # hqp = false and a vector of the wrong size return 0
    assert r["ok"] == [1, 1, 1, 1, 1, 1, 0, 0], r["ok"]
    assert e(r["torque_contact_arg"], r["torque_contact_noarg"]) <= 1e-6
    assert e(r["delta"], dt) <= rc.TOL_TAU and r["delta_eigen_like"] == r["delta"]
    assert e(cyc.NwJw @ np.asarray(r["cf_redis_qp_"]), dt) <= rc.TOL_TAU
    assert e(r["wrench_in"], w[0]) <= rc.TOL_WRENCH and e(r["wrench_out"], w[1]) <= rc.TOL_WRENCH
    assert "libdwbc_amd : CalcContactRedistribute(torque_input, hqp = false)" in out
    assert "Contact Redistribution : torque input size is not matched with model size" in out
