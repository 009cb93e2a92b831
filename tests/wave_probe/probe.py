"""ctypes loader of the wave-routine probe (wave_probe_body.h).  TEST HARNESS ONLY.

The probe runs the shipped text of the device-only wave routines (dwbc_wave.h, dwbc_cycle2.h, dwbc_cycle2p.h, dwbc_cycle_gc.h) alone, in two builds of
the same source: ``"emu"`` (host emulation, built here on demand like tests/emu) and ``"gpu"`` (libdwbc_wave_probe.so, made by
``__graft_entry__.build()``; one wavefront per problem, 64 or 128 threads per block).  Nothing touches the GPU at import.

One C entry per routine family; an instantiation is looked up by its name in the table of wave_probe.hip.  ``run`` takes the flat
records of a batch, (B, NIN) doubles and (B, NIP) ints, and returns (B, NOUT) doubles; what a problem does not write holds SENTINEL.
The record layouts are described next to each family in wave_probe_body.h and unpacked in tests/wave_cases.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_FILES = {"emu": "libdwbc_wave_probe_emu.so", "gpu": "libdwbc_wave_probe.so"}
_ENTRY = {1: "wave_probe_lanes", 2: "wave_probe_math", 3: "wave_probe_gemm", 4: "wave_probe_inverse", 5: "wave_probe_rows"}
_libs = {}
_tables = {}
SENTINEL = -4242.0  # of the caller's output record (the blocks the probe frames in LDS carry kWpSentinel = -7777)
FRAME_SENTINEL = -7777.0
MAX_B = 512


def lib(build):
    if build not in _libs:
        path = os.path.join(_HERE, _FILES[build])
        if build == "emu":
            subprocess.check_call(["make", "-C", _HERE, "-s"])
        elif not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: __graft_entry__.build() makes it (make -C tests/wave_probe gpu)")
        L = C.CDLL(path)
        L.wave_probe_error.restype = C.c_char_p
        L.wave_probe_inst_name.restype = C.c_char_p
        L.wave_probe_inst_info.argtypes = [C.c_int, C.c_void_p]
        for name in _ENTRY.values():
            getattr(L, name).argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
        _libs[build] = L
    return _libs[build]


def table(build):
    """name -> (index, family, NIN, NIP, NOUT) of the loaded library"""
    if build not in _tables:
        L = lib(build)
        t = {}
        for i in range(L.wave_probe_inst_count()):
            info = np.zeros(4, np.int32)
            assert L.wave_probe_inst_info(i, info.ctypes.data) == 1
            t[L.wave_probe_inst_name(i).decode()] = (i,) + tuple(int(v) for v in info)
        _tables[build] = t
    return _tables[build]


def sizes(build, name):
    return table(build)[name][2:]


def run_raw(build, family, index, threads, B, din, ip, out):
    """the entry as it is (the refusal tests hand it records of the wrong size); RuntimeError with the probe's message"""
    L = lib(build)
    before = out.copy()
    ok = getattr(L, _ENTRY[family])(index, threads, B, din.ctypes.data, din.size, ip.ctypes.data, ip.size, out.ctypes.data, out.size)
    if ok != 1:
        assert np.array_equal(before, out), "a refused batch must leave the outputs alone"
        raise RuntimeError(L.wave_probe_error().decode())
    return out


def run(build, name, din, ip=None, threads=64):
    """runs the batch ``din`` (B, NIN) [+ ``ip`` (B, NIP)] through instantiation ``name``; (B, NOUT) doubles"""
    index, family, nin, nip, nout = table(build)[name]
    din = np.ascontiguousarray(din, dtype=np.float64)
    B = din.shape[0]
    assert din.shape == (B, nin), (name, din.shape, nin)
    ip = np.zeros((B, nip), np.int32) if ip is None else np.ascontiguousarray(ip, dtype=np.int32).reshape(B, nip)
    out = np.full((B, nout), SENTINEL)
    return run_raw(build, family, index, threads, B, din, ip, out)
