"""ctypes loader of the CPU emulation of the link-query kernel (tests/emu/emu_link_query.cpp).  TEST HARNESS ONLY.  The library is built on
first use, aside and then renamed, as the cycle's emulation is."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")
_SO = os.path.join(_HERE, "libdwbc_emu_link_query.so")


@functools.lru_cache(maxsize=None)
def lib():
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.libdwbc_emu_link_query.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp,
                           os.path.join(_HERE, "emu_link_query.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.emu_link_query_run.restype = C.c_int
    L.emu_link_query_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_char_p, C.c_int]
    return L


def lds_bytes():
    return lib().emu_link_query_lds_bytes()


def run(urdf, q, qdot, links, points, jacobians):
    """dict(pos (B, L, 3), rot (B, L, 3, 3), vel (B, L, 6)[, jac (B, L, 6, 39)]); every output is pre-filled with NaN, so an entry the kernel
    never writes shows up"""
    q = np.ascontiguousarray(q, np.float64)
    B, n = q.shape[0], len(links)
    qd = None if qdot is None else np.ascontiguousarray(qdot, np.float64)
    assert q.shape == (B, 40) and (qd is None or qd.shape == (B, 39))
    links = np.ascontiguousarray(links, np.int32)
    points = np.ascontiguousarray(points, np.float64)
    assert points.shape == (n, 3)
    out = dict(pos=np.full((B, n, 3), np.nan), rot=np.full((B, n, 3, 3), np.nan), vel=np.full((B, n, 6), np.nan))
    if jacobians:
        out["jac"] = np.full((B, n, 6, 39), np.nan)
    err = C.create_string_buffer(256)
    ok = lib().emu_link_query_run(urdf.encode(), B, q.ctypes.data, None if qd is None else qd.ctypes.data, n, links.ctypes.data, points.ctypes.data,
                                  out["pos"].ctypes.data, out["rot"].ctypes.data, out["vel"].ctypes.data, out["jac"].ctypes.data if jacobians else None, err, 256)
    assert ok == 1, err.value.decode()
    return out
