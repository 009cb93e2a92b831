"""ctypes loader of the CPU emulation of the dynamics kernel (tests/emu/emu_dynamics.cpp).  TEST HARNESS ONLY.  The library is built on
first use, aside and then renamed, as the other single-kernel emulations are."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")
_SO = os.path.join(_HERE, "libdwbc_emu_dynamics.so")

OUTPUTS = {"A": 0, "A_inv": 1, "B": 2, "G": 3, "CMM": 4, "com": 5}  # enum dwbc_dynamics_output without the status
SENTINEL_STATUS = -1


@functools.lru_cache(maxsize=None)
def lib():
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.libdwbc_emu_dynamics.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp,
                           os.path.join(_HERE, "emu_dynamics.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.emu_dynamics_lds_bytes.restype = C.c_int
    L.emu_dynamics_lds_bytes.argtypes = [C.c_int]
    L.emu_dynamics_run.restype = C.c_int
    L.emu_dynamics_run.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 7 + [C.c_char_p, C.c_int]
    return L


def lds_bytes(n):
    """LdsDyn<n, n - 5>::total_bytes"""
    b = lib().emu_dynamics_lds_bytes(n)
    assert b > 0, n
    return b


def run(model, q, qd=None, outputs=tuple(OUTPUTS), tree=False):
    """model: dict of arrays (nb, parent, R_T, p_T, axis, mass, com, inertia).  qd None: the state has no velocity.  Returns a dict of
    all six outputs and ``status``; every buffer is handed to the kernel pre-filled with NaN (status: -1), whether it is asked for or not, so
    an entry the kernel never writes shows up -- as does a write to an output that was not asked for."""
    nb = int(model["nb"])
    n = nb + 5
    arrs = [np.ascontiguousarray(model["parent"], np.int32)] + [np.ascontiguousarray(model[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")]
    q = np.ascontiguousarray(q, np.float64)
    B = q.shape[0]
    v = None if qd is None else np.ascontiguousarray(qd, np.float64)
    assert q.shape == (B, n + 1) and (v is None or v.shape == (B, n))
    mask = 0
    for k in outputs:
        mask |= 1 << OUTPUTS[k]
    out = dict(A=np.full((B, n, n), np.nan), A_inv=np.full((B, n, n), np.nan), B=np.full((B, n), np.nan), G=np.full((B, n), np.nan),
               CMM=np.full((B, 6, n), np.nan), com=np.full((B, 3), np.nan), status=np.full(B, SENTINEL_STATUS, np.int32))
    err = C.create_string_buffer(256)
    ok = lib().emu_dynamics_run(nb, *[a.ctypes.data for a in arrs], B, q.ctypes.data, None if v is None else v.ctypes.data, mask, 1 if tree else 0,
                                *[out[k].ctypes.data for k in ("A", "A_inv", "B", "G", "CMM", "com", "status")], err, 256)
    assert ok == 1, err.value.decode()
    return out
