"""ctypes loader of the CPU emulation of the single-level task-QP kernel (tests/emu/emu_task_qp.cpp).  TEST HARNESS ONLY.  The library is
built on first use, aside and then renamed, as the other single-kernel emulations are."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")
_SO = os.path.join(_HERE, "libdwbc_emu_task_qp.so")

# enum dwbc_task_qp_output without the status
OUTPUTS = {"f_star_qp": 0, "contact_qp": 1, "torque_h": 2, "torque_null_h": 3, "torque_contact": 4}
SENTINEL_STATUS = -1


@functools.lru_cache(maxsize=None)
def lib():
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.libdwbc_emu_task_qp.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp,
                           os.path.join(_HERE, "emu_task_qp.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.emu_task_qp_lds_bytes.restype = C.c_int
    L.emu_task_qp_lds_bytes.argtypes = [C.c_int]
    L.emu_task_qp_run.restype = C.c_int
    L.emu_task_qp_run.argtypes = ([C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int] +
                                  [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int])
    return L


def lds_bytes(n):
    """LdsTq<n, n - 5>::total_bytes"""
    b = lib().emu_task_qp_lds_bytes(n)
    assert b > 0, n
    return b


def shapes(B, n):
    m = n - 6
    return {"f_star_qp": (B, 6), "contact_qp": (B, 6), "torque_h": (B, m), "torque_null_h": (B, m), "torque_contact": (B, m)}


def _ptr(a):
    return None if a is None else a.ctypes.data


def run(model, contacts, tasks, q, flags, fstar, level, torque_prev, null=None, tau_lim=None, inst_par=None, outputs=tuple(OUTPUTS), tree=False):
    """model: dict of arrays (nb, parent, R_T, p_T, axis, mass, com, inertia); contacts: dicts (link, point, lx, ly, mu, muz); tasks: levels
    of (mode, link, point); flags (B, len(contacts)); fstar (B, sum of the levels' dof); torque_prev (B, m); null (B, m, m) or None.
    Returns the five outputs and ``status``; every buffer is handed to the kernel pre-filled with NaN (status: -1), whether it is asked
    for or not, so an entry the kernel never writes shows up -- as does a write to an output that was not asked for."""
    nb = int(model["nb"])
    n = nb + 5
    m = n - 6
    arrs = [np.ascontiguousarray(model["parent"], np.int32)] + [np.ascontiguousarray(model[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")]
    q = np.ascontiguousarray(q, np.float64)
    B = q.shape[0]
    flags = np.ascontiguousarray(flags, np.uint8)
    nc = len(contacts)
    c_link = np.array([c["link"] for c in contacts], np.int32)
    c_point = np.array([c["point"] for c in contacts], np.float64).reshape(nc, 3)
    c_par = np.array([[c["lx"], c["ly"], c["mu"], c["muz"]] for c in contacts], np.float64).reshape(nc, 4)
    flat = [(l, mode, link, pt) for l, lv in enumerate(tasks) for mode, link, pt in lv]
    t_level, t_mode, t_link = (np.array([f[i] for f in flat], np.int32) for i in range(3))
    t_point = np.array([f[3] for f in flat], np.float64).reshape(len(flat), 3)
    ftot = sum(6 if mode <= 2 else 3 for lv in tasks for mode, _, _ in lv)
    fstar = np.ascontiguousarray(fstar, np.float64)
    torque_prev = np.ascontiguousarray(torque_prev, np.float64)
    assert q.shape == (B, n + 1) and flags.shape == (B, nc) and fstar.shape == (B, ftot) and torque_prev.shape == (B, m)
    if null is not None:
        null = np.ascontiguousarray(null, np.float64)
        assert null.shape == (B, m, m)
    if tau_lim is not None:
        tau_lim = np.ascontiguousarray(tau_lim, np.float64)
        assert tau_lim.shape == (m,)
    if inst_par is not None:
        inst_par = np.ascontiguousarray(inst_par, np.float64)
        assert inst_par.shape == (B, m + 4 * nc)
    mask = 0
    for k in outputs:
        mask |= 1 << OUTPUTS[k]
    out = {k: np.full(s, np.nan) for k, s in shapes(B, n).items()}
    out["status"] = np.full(B, SENTINEL_STATUS, np.int32)
    ptrs = (C.c_void_p * len(OUTPUTS))()
    for k, w in OUTPUTS.items():
        ptrs[w] = out[k].ctypes.data
    err = C.create_string_buffer(256)
    ok = lib().emu_task_qp_run(nb, *[a.ctypes.data for a in arrs], nc, c_link.ctypes.data, c_point.ctypes.data, c_par.ctypes.data, len(flat),
                               t_level.ctypes.data, t_mode.ctypes.data, t_link.ctypes.data, t_point.ctypes.data, _ptr(tau_lim), _ptr(inst_par), B,
                               q.ctypes.data, flags.ctypes.data, fstar.ctypes.data, int(level), torque_prev.ctypes.data, _ptr(null), mask,
                               1 if tree else 0, C.cast(ptrs, C.c_void_p), out["status"].ctypes.data, err, 256)
    assert ok == 1, err.value.decode()
    return out
