"""ctypes loader of the CPU emulation of the task-space kernel (tests/emu/emu_task_space.cpp).  TEST HARNESS ONLY.  The library is built on
first use, aside and then renamed, as the other single-kernel emulations are."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")
_SO = os.path.join(_HERE, "libdwbc_emu_task_space.so")

# enum dwbc_task_space_output without the status
OUTPUTS = {"J_task": 0, "Lambda_task": 1, "J_kt": 2, "Null_task": 3}
MAX_LEVELS = 4
SENTINEL_STATUS = -1


@functools.lru_cache(maxsize=None)
def lib():
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.libdwbc_emu_task_space.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp,
                           os.path.join(_HERE, "emu_task_space.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.emu_task_space_lds_bytes.restype = C.c_int
    L.emu_task_space_lds_bytes.argtypes = [C.c_int]
    L.emu_task_space_run.restype = C.c_int
    L.emu_task_space_run.argtypes = ([C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] + [C.c_void_p] * 4 +
                                     [C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int])
    return L


def lds_bytes(n):
    """LdsTs<n, n - 5>::total_bytes"""
    b = lib().emu_task_space_lds_bytes(n)
    assert b > 0, n
    return b


def shapes(B, n, ts):
    """per output a list of shapes, one per level (Null_task: every level but the last)"""
    m = n - 6
    return {"J_task": [(B, t, n) for t in ts], "Lambda_task": [(B, t, t) for t in ts], "J_kt": [(B, m, t) for t in ts], "Null_task": [(B, m, m) for _ in ts[:-1]]}


def run(model, contacts, tasks, q, flags, outputs=tuple(OUTPUTS), tree=False):
    """model: dict of arrays (nb, parent, R_T, p_T, axis, mass, com, inertia); contacts: dicts (link, point); tasks: levels of (mode, link,
    point); flags (B, len(contacts)).  Returns per output a list of arrays, one per level, and ``status``; every buffer is handed to the
    kernel pre-filled with NaN (status: -1), whether it is asked for or not, so an entry the kernel never writes shows up -- as does a
    write to an output that was not asked for."""
    nb = int(model["nb"])
    n = nb + 5
    arrs = [np.ascontiguousarray(model["parent"], np.int32)] + [np.ascontiguousarray(model[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")]
    q = np.ascontiguousarray(q, np.float64)
    B = q.shape[0]
    flags = np.ascontiguousarray(flags, np.uint8)
    nc = len(contacts)
    assert q.shape == (B, n + 1) and flags.shape == (B, nc)
    c_link = np.array([c["link"] for c in contacts], np.int32)
    c_point = np.array([c["point"] for c in contacts], np.float64).reshape(nc, 3)
    flat = [(l, mode, link, pt) for l, lv in enumerate(tasks) for mode, link, pt in lv]
    t_level, t_mode, t_link = (np.array([f[i] for f in flat], np.int32) for i in range(3))
    t_point = np.array([f[3] for f in flat], np.float64).reshape(len(flat), 3)
    ts = [sum(6 if mode <= 2 else 3 for mode, _, _ in lv) for lv in tasks]
    mask = 0
    for k in outputs:
        mask |= 1 << OUTPUTS[k]
    out = {k: [np.full(s, np.nan) for s in ss] for k, ss in shapes(B, n, ts).items()}
    out["status"] = np.full(B, SENTINEL_STATUS, np.int32)
    ptrs = (C.c_void_p * (4 * MAX_LEVELS))()
    for k, w in OUTPUTS.items():
        for l, a in enumerate(out[k]):
            ptrs[w * MAX_LEVELS + l] = a.ctypes.data
    err = C.create_string_buffer(256)
    ok = lib().emu_task_space_run(nb, *[a.ctypes.data for a in arrs], nc, c_link.ctypes.data, c_point.ctypes.data, len(flat), t_level.ctypes.data,
                                  t_mode.ctypes.data, t_link.ctypes.data, t_point.ctypes.data, B, q.ctypes.data, flags.ctypes.data, mask,
                                  1 if tree else 0, C.cast(ptrs, C.c_void_p), out["status"].ctypes.data, err, 256)
    assert ok == 1, err.value.decode()
    return out
