"""ctypes loader of the CPU emulation of the gravity-compensation kernel (tests/emu/emu_gravcomp.cpp).  TEST HARNESS ONLY.  The library is
built on first use, aside and then renamed, as the redistribution's emulation at the pack sizes is."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")
_SO = os.path.join(_HERE, "libdwbc_emu_gravcomp.so")


@functools.lru_cache(maxsize=None)
def lib():
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.libdwbc_emu_gravcomp.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp,
                           os.path.join(_HERE, "emu_gravcomp.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.emu_gravcomp_lds_bytes.restype = C.c_int
    L.emu_gravcomp_lds_bytes.argtypes = [C.c_int]
    L.emu_gravcomp_run.restype = C.c_int
    L.emu_gravcomp_run.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 7 + [C.c_char_p, C.c_int]
    return L


def lds_bytes(n):
    """LdsGc<n, n - 5>::total_bytes"""
    b = lib().emu_gravcomp_lds_bytes(n)
    assert b > 0, n
    return b


def run(model, contacts, tau_lim, q, flags, tau_in=None, inst_par=None, tree=False):
    """model: dict of arrays (nb, parent, R_T, p_T, axis, mass, com, inertia); contacts: dicts (link, point, lx, ly, mu, muz).
    tau_in None: the gravity-only form.  Returns (redistribution, gravity): dict(tau (B, m), cf (B, 6), wrench (B, 2, 12), status (B,)) and
    dict(tau (B, m), wrench (B, 12), status (B,)); every output is pre-filled with NaN (status: -1), so an entry the kernel never writes shows
    up -- as do, in the gravity-only form, the redistribution outputs it must not write"""
    nb = int(model["nb"])
    m = nb - 1
    arrs = [np.ascontiguousarray(model["parent"], np.int32)] + [np.ascontiguousarray(model[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")]
    q = np.ascontiguousarray(q, np.float64)
    B = q.shape[0]
    flags = np.ascontiguousarray(flags, np.uint8)
    tin = None if tau_in is None else np.ascontiguousarray(tau_in, np.float64)
    nc = len(contacts)
    assert q.shape == (B, nb + 6) and flags.shape == (B, nc) and (tin is None or tin.shape == (B, m))
    c_link = np.array([c["link"] for c in contacts], np.int32)
    c_point = np.array([c["point"] for c in contacts], np.float64).reshape(nc, 3)
    c_par = np.array([[c["lx"], c["ly"], c["mu"], c["muz"]] for c in contacts], np.float64)
    lim = None if tau_lim is None else np.ascontiguousarray(tau_lim, np.float64)
    rec = None if inst_par is None else np.ascontiguousarray(inst_par, np.float64)
    assert lim is None or lim.shape == (m,)
    assert rec is None or rec.shape == (B, m + 4 * nc)
    rd = dict(tau=np.full((B, m), np.nan), cf=np.full((B, 6), np.nan), wrench=np.full((B, 2, 12), np.nan), status=np.full(B, -1, np.int32))
    gr = dict(tau=np.full((B, m), np.nan), wrench=np.full((B, 12), np.nan), status=np.full(B, -1, np.int32))
    err = C.create_string_buffer(256)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    ok = lib().emu_gravcomp_run(nb, *[a.ctypes.data for a in arrs], nc, c_link.ctypes.data, c_point.ctypes.data, c_par.ctypes.data, ptr(lim), B,
                                q.ctypes.data, flags.ctypes.data, ptr(tin), ptr(rec), 1 if tree else 0, rd["tau"].ctypes.data, rd["cf"].ctypes.data,
                                rd["wrench"].ctypes.data, rd["status"].ctypes.data, gr["tau"].ctypes.data, gr["wrench"].ctypes.data, gr["status"].ctypes.data,
                                err, 256)
    assert ok == 1, err.value.decode()
    return rd, gr
