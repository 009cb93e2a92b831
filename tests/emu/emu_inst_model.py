"""ctypes loader of the CPU emulation of the per-instance-model build (tests/emu/emu_inst_model.cpp, compiled with DWBC_INST_MODEL).
TEST HARNESS ONLY.  The library is built on first use, aside and then renamed, as the other single-kernel emulations are.  `mutant` names a
wrong DWBC_BODY the source is built with instead of the one of dwbc_types.h: the mutations tests/test_instance_model_emu.py must catch."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc")

EXTRAS, COMPACT, TWO_WAVE = range(3)
MUTANTS = {
    "short_stride": "((io).body + (size_t)(inst) * ((nb) - 1) * kBodyStride)",  # a stride of (nb - 1) * kBodyStride
    "ignores_inst": "((io).body + (size_t)0 * (inst) * (nb) * kBodyStride)",    # an offset that ignores inst
}


@functools.lru_cache(maxsize=None)
def lib(mutant=None):
    name = "libdwbc_emu_inst_model" + (f"_{mutant}" if mutant else "") + ".so"
    tmp = os.path.join(_HERE, f"tmp.{os.getpid()}.{name}")
    defs = ["-DDWBC_INST_MODEL"] + ([f"-DDWBC_BODY(io,inst,nb)={MUTANTS[mutant]}", "-DEMU_IM_DYNAMICS_ONLY"] if mutant else [])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__="] + defs +
                          ["-o", tmp, os.path.join(_HERE, "emu_inst_model.cpp"), os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
    so = os.path.join(_HERE, name)
    os.replace(tmp, so)
    L = C.CDLL(so)
    P, I = C.c_void_p, C.c_int
    if not mutant:  # (a mutant is the dynamics kernel alone)
        L.emu_im_cycle.restype = I
        L.emu_im_cycle.argtypes = [I] + [P] * 7 + [I, P, I, P, P, P, I, I, I] + [P] * 7 + [C.c_char_p, I]
    L.emu_im_dynamics.restype = I
    L.emu_im_dynamics.argtypes = [I] + [P] * 7 + [I] + [P] * 10 + [C.c_char_p, I]
    return L


def _model(model):
    return [np.ascontiguousarray(model["parent"], np.int32)] + [np.ascontiguousarray(model[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")]


def cycle(model, contacts, tasks, tau_lim, tables, q, flags, fstar, build=EXTRAS, hqp=True):
    """model: dict of arrays (the tree; its own inertial data is not read); tables: (B, nb, 25).  Returns dict(tau, wrench, status), every
    buffer pre-filled with NaN (status: -1)"""
    nb = int(model["nb"])
    arrs = _model(model)
    B = len(q)
    tables = np.ascontiguousarray(tables, np.float64)
    assert tables.shape == (B, nb, 25), tables.shape
    con = np.array([[c["link"], *c["point"], c["lx"], c["ly"], c.get("mu", 0.2), c.get("muz", 0.2)] for c in contacts], np.float64)
    nl = np.array([len(lv) for lv in tasks], np.int32)
    tk = np.zeros((len(tasks), 2, 5))
    for l, lv in enumerate(tasks):
        for j, (mode, link, pt) in enumerate(lv):
            tk[l, j] = [mode, link, *pt]
    lim = None if tau_lim is None else np.ascontiguousarray(tau_lim, np.float64)
    q = np.ascontiguousarray(q, np.float64)
    flags = np.ascontiguousarray(flags, np.uint8)
    fstar = np.ascontiguousarray(fstar, np.float64)
    out = dict(tau=np.full((B, 3, nb - 1), np.nan), wrench=np.full((B, 12), np.nan), status=np.full(B, -1, np.int32))
    err = C.create_string_buffer(256)
    ok = lib().emu_im_cycle(nb, *[a.ctypes.data for a in arrs], len(contacts), con.ctypes.data, len(tasks), nl.ctypes.data, tk.ctypes.data,
                                  None if lim is None else lim.ctypes.data, build, 1 if hqp else 0, B, tables.ctypes.data, q.ctypes.data, flags.ctypes.data,
                                  fstar.ctypes.data, out["tau"].ctypes.data, out["wrench"].ctypes.data, out["status"].ctypes.data, err, 256)
    assert ok == 1, err.value.decode()
    return out


def dynamics(model, tables, q, qd=None, mutant=None):
    nb = int(model["nb"])
    n = nb + 5
    arrs = _model(model)
    B = len(q)
    tables = np.ascontiguousarray(tables, np.float64)
    assert tables.shape == (B, nb, 25), tables.shape
    q = np.ascontiguousarray(q, np.float64)
    v = None if qd is None else np.ascontiguousarray(qd, np.float64)
    out = dict(A=np.full((B, n, n), np.nan), A_inv=np.full((B, n, n), np.nan), B=np.full((B, n), np.nan), G=np.full((B, n), np.nan),
               CMM=np.full((B, 6, n), np.nan), com=np.full((B, 3), np.nan), status=np.full(B, -1, np.int32))
    err = C.create_string_buffer(256)
    ok = lib(mutant).emu_im_dynamics(nb, *[a.ctypes.data for a in arrs], B, tables.ctypes.data, q.ctypes.data, None if v is None else v.ctypes.data,
                                     *[out[k].ctypes.data for k in ("A", "A_inv", "B", "G", "CMM", "com", "status")], err, 256)
    assert ok == 1, err.value.decode()
    return out
