"""ctypes loader of the CPU emulation of the contact-space kernel (tests/emu/emu_contact_space.cpp).  TEST HARNESS ONLY.  The library is
built on first use, aside and then renamed, as the other single-kernel emulations are."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")
_SO = os.path.join(_HERE, "libdwbc_emu_contact_space.so")

# enum dwbc_contact_space_output without the status
OUTPUTS = {"J_C": 0, "Lambda_c": 1, "J_C_INV_T": 2, "N_C": 3, "A_inv_N_C": 4, "W": 5, "W_inv": 6, "NwJw": 7, "contact_pos": 8, "contact_rot": 9}
SENTINEL_STATUS = -1


@functools.lru_cache(maxsize=None)
def lib():
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.libdwbc_emu_contact_space.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp,
                           os.path.join(_HERE, "emu_contact_space.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.emu_contact_space_lds_bytes.restype = C.c_int
    L.emu_contact_space_lds_bytes.argtypes = [C.c_int]
    L.emu_contact_space_run.restype = C.c_int
    L.emu_contact_space_run.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return L


def lds_bytes(n):
    """LdsCs<n, n - 5>::total_bytes"""
    b = lib().emu_contact_space_lds_bytes(n)
    assert b > 0, n
    return b


def shapes(B, n):
    m = n - 6
    return {"J_C": (B, 12, n), "Lambda_c": (B, 12, 12), "J_C_INV_T": (B, 12, n), "N_C": (B, n, n), "A_inv_N_C": (B, n, n), "W": (B, m, m), "W_inv": (B, m, m),
            "NwJw": (B, m, 6), "contact_pos": (B, 2, 3), "contact_rot": (B, 2, 3, 3)}


def run(model, contacts, q, flags, outputs=tuple(OUTPUTS), tree=False):
    """model: dict of arrays (nb, parent, R_T, p_T, axis, mass, com, inertia); contacts: dicts (link, point); flags (B, len(contacts)).
    Returns a dict of all ten outputs and ``status``; every buffer is handed to the kernel pre-filled with NaN (status: -1), whether it is
    asked for or not, so an entry the kernel never writes shows up -- as does a write to an output that was not asked for."""
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
    mask = 0
    for k in outputs:
        mask |= 1 << OUTPUTS[k]
    out = {k: np.full(s, np.nan) for k, s in shapes(B, n).items()}
    out["status"] = np.full(B, SENTINEL_STATUS, np.int32)
    ptrs = (C.c_void_p * 10)(*[out[k].ctypes.data for k in OUTPUTS])
    err = C.create_string_buffer(256)
    ok = lib().emu_contact_space_run(nb, *[a.ctypes.data for a in arrs], nc, c_link.ctypes.data, c_point.ctypes.data, B, q.ctypes.data, flags.ctypes.data,
                                     mask, 1 if tree else 0, C.cast(ptrs, C.c_void_p), out["status"].ctypes.data, err, 256)
    assert ok == 1, err.value.decode()
    return out
