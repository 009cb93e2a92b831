"""ctypes loader of the wave-QP probe (qp_probe_body.h).  TEST HARNESS ONLY.

The probe runs the shipped text of ``qp_solve_wave`` (libdwbc_amd/csrc/dwbc_qp_wave.h) on rows of the caller's choosing, in two builds
of the same source: ``"emu"`` (host emulation, built here on demand like tests/emu) and ``"gpu"`` (libdwbc_qp_probe.so, made by
``__graft_entry__.build()``; one wavefront per problem, 64 or 128 threads per block).  Nothing touches the GPU at import.

A problem is a dict:
    G       (64, nv)  row coefficients as given (the probe scales the contact columns j >= t by kQpScaleGI, as qp_rows_and_solve does)
    hi, lo  (64,)     g.x <= hi, -g.x <= lo; +inf = side absent (an inert lane: G = 0, hi = lo = inf)
    id_hi, id_lo (64,) int   reference row index of each side, -1 = none
    nv, t   variables and task variables (k = nv - t contact-null variables follow them)
    max_iter, vtol, warm (None or a list of ids, -1 = empty; WS = 1 only)

Layout contract of ``WS = 0``.  The solver picks the lexicographic solve by ``if (!WS || (t == NV - KCV && k == KCV)) lex_point(std::true_type{})``:
a build without the working-set report ALWAYS reads the contact block at its compile-time positions.  So ``WS = 0`` is valid only for the
standard layout ``t = NV - KCV, k = KCV`` or for ``t = 0`` / ``k = 0`` (no lexicographic solve at all).  The probe refuses any other
``(t, k)`` for a ``WS = 0`` instantiation and runs nothing.  In every build the lexicographic solve holds KCV contact-null variables at the
most: ``k > KCV`` with ``t > 0`` is refused too (the solver would silently leave the excess out).  Range limits of the entry: 1 <= nv <= NV, 0 <= t <= nv,
1 <= max_iter <= 2000, B <= 1024.
"""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_FILES = {"emu": "libdwbc_qp_probe_emu.so", "gpu": "libdwbc_qp_probe.so"}
_libs = {}

Inst = namedtuple("Inst", "index ws nv qn kcv f32")
Inst.name = property(lambda s: f"ws{s.ws}_nv{s.nv}_qn{s.qn}_k{s.kcv}" + ("_f32" if s.f32 else ""))
# the fp64 canon and what the fp32 build uses instead (dwbc_cycle.h)
Inst.zero_row = property(lambda s: 1.0e-5 if s.f32 else 1.0e-9)
Inst.inf = property(lambda s: float(np.float32(1.0e30)) if s.f32 else 1.0e300)  # DWBC_QP_INF: sfin of an inert lane


# (WS, NV, QN, KCV, fp32) of the library's table (qp_probe.hip: kInst), spelt out here so that tests can be collected without building anything
INSTANTIATIONS = tuple(Inst(i, *v) for i, v in enumerate([
    (0, 6, 12, 6, 0), (1, 6, 12, 6, 0), (0, 9, 12, 6, 0), (1, 9, 12, 6, 0), (0, 12, 12, 6, 0), (1, 12, 12, 6, 0),
    (1, 18, 18, 12, 0), (1, 24, 24, 12, 0), (1, 12, 12, 6, 1)]))


def lib(build):
    if build not in _libs:
        path = os.path.join(_HERE, _FILES[build])
        if build == "emu":
            subprocess.check_call(["make", "-C", _HERE, "-s"])
        elif not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: __graft_entry__.build() makes it (make -C tests/qp_probe gpu)")
        L = C.CDLL(path)
        L.qp_probe_error.restype = C.c_char_p
        L.qp_probe_inst_info.argtypes = [C.c_int, C.c_void_p]
        L.qp_probe_inst_scale.restype = C.c_double
        L.qp_probe_solve.argtypes = [C.c_int] * 3 + [C.c_void_p] * 7
        _libs[build] = L
    return _libs[build]


def instantiations(build="emu"):
    """the table of the loaded library (the tests assert that it equals INSTANTIATIONS)"""
    L = lib(build)
    out = []
    for i in range(L.qp_probe_inst_count()):
        info = np.zeros(5, np.int32)
        assert L.qp_probe_inst_info(i, info.ctypes.data) == 1
        out.append(Inst(i, *[int(v) for v in info]))
    return out


def scale(build, inst):
    """kQpScaleGI of the instantiation's arithmetic type, as the loaded library was built"""
    return float(lib(build).qp_probe_inst_scale(inst.index))


def pack(inst, problems):
    """the flat records of a batch (rows, ids, par, vtol, warm or None)"""
    B, qn = len(problems), inst.qn
    rows = np.zeros((B, 64, qn + 2))
    ids = np.full((B, 64, 2), -1, np.int32)
    par = np.zeros((B, 4), np.int32)
    vtol = np.zeros(B)
    warm = np.full((B, qn), -1, np.int32)
    for b, p in enumerate(problems):
        nv = p["nv"]
        rows[b, :, :nv] = p["G"]
        rows[b, :, qn] = p["hi"]
        rows[b, :, qn + 1] = p["lo"]
        ids[b, :, 0] = p["id_hi"]
        ids[b, :, 1] = p["id_lo"]
        w = p.get("warm")
        par[b] = (nv, p["t"], p["max_iter"], 0 if w is None else 1)
        vtol[b] = p["vtol"]
        if w is not None:
            assert len(w) <= qn
            warm[b, : len(w)] = w
    return rows, ids, par, vtol, (warm if par[:, 3].any() else None)


def solve_packed(build, inst, threads, rows, ids, par, vtol, warm):
    """the entry on flat records; the outputs, or RuntimeError with the probe's message"""
    L = lib(build)
    B, qn = len(par), inst.qn
    oi = np.full((B, 4 + qn), -7, np.int32)
    od = np.full((B, 1 + qn + 64), np.nan)
    ok = L.qp_probe_solve(inst.index, threads, B, rows.ctypes.data, ids.ctypes.data, par.ctypes.data, vtol.ctypes.data,
                          None if warm is None else warm.ctypes.data, oi.ctypes.data, od.ctypes.data)
    if ok != 1:
        assert (oi == -7).all() and np.isnan(od).all(), "a refused batch must leave the outputs alone"
        raise RuntimeError(L.qp_probe_error().decode())
    return dict(status=oi[:, 0].copy(), iters=oi[:, 1].copy(), nact=oi[:, 2].copy(), act=oi[:, 4:].copy(), viol=od[:, 0].copy(),
                x=od[:, 1 : 1 + qn].copy(), sfin=od[:, 1 + qn :].copy())


def solve(build, inst, problems, threads=64):
    """runs the batch through instantiation ``inst`` (an Inst or its index) of ``build``; dict of arrays status, iters, nact (B,), act (B, QN),
    viol (B,), x (B, QN), sfin (B, 64).  Raises RuntimeError with the probe's message when it refuses the batch or the run fails."""
    if not isinstance(inst, Inst):
        inst = INSTANTIATIONS[inst]
    return solve_packed(build, inst, threads, *pack(inst, problems))
