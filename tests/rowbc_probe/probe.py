"""ctypes loader of the row-broadcast probe (rowbc_probe.hip).  TEST HARNESS ONLY.

Two builds of the same source: ``"emu"`` (host emulation, built here on demand like tests/emu) and ``"gpu"`` (libdwbc_rowbc_probe.so, made by
``__graft_entry__.build()``; one wavefront per problem, 64 or 128 threads per block).  Nothing touches the GPU at import.
The kinds and their records are described at the top of rowbc_probe.hip.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_FILES = {"emu": "libdwbc_rowbc_probe_emu.so", "gpu": "libdwbc_rowbc_probe.so"}
_libs = {}
REPLICATE, FMA, DZ6, DZ9, DZ12, SWEEP = range(6)
NIN = (64, 192, 832, 832, 832, 144)
NOUT = (64, 1024, 128, 128, 128, 290)
SENTINEL = -4242.0


def lib(build):
    if build not in _libs:
        path = os.path.join(_HERE, _FILES[build])
        if build == "emu":
            subprocess.check_call(["make", "-C", _HERE, "-s"])
        elif not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: __graft_entry__.build() makes it (make -C tests/rowbc_probe gpu)")
        L = C.CDLL(path)
        L.rowbc_probe_error.restype = C.c_char_p
        L.rowbc_probe_run.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
        _libs[build] = L
    return _libs[build]


def run(build, kind, din, threads=64):
    """runs the batch ``din`` (B, NIN[kind]) through ``kind``; (B, NOUT[kind]) doubles.  RuntimeError with the probe's message"""
    L = lib(build)
    din = np.ascontiguousarray(din, dtype=np.float64)
    B = din.shape[0]
    assert din.shape == (B, NIN[kind]), (kind, din.shape)
    out = np.full((B, NOUT[kind]), SENTINEL)
    if L.rowbc_probe_run(kind, threads, B, din.ctypes.data, din.size, out.ctypes.data, out.size) != 1:
        raise RuntimeError(L.rowbc_probe_error().decode())
    return out
