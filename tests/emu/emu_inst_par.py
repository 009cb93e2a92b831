"""ctypes loader of the CPU emulation of the cycle and redistribution kernels run with a per-instance parameter record
(tests/emu/emu_inst_par.cpp).  TEST HARNESS ONLY.  Builds libdwbc_emu_inst_par.so with the flags of tests/emu/Makefile whenever a source
it is made of is newer than the library."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.normpath(os.path.join(_HERE, "..", "..", "libdwbc_amd", "csrc"))
_SO = os.path.join(_HERE, "libdwbc_emu_inst_par.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "emu_inst_par.cpp")
        deps = [src] + glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(_CSRC, "*.inc")) + [os.path.join(_CSRC, "dwbc_model.cpp")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            tmp = _SO + ".%d.tmp" % os.getpid()  # (built aside and renamed: test processes running side by side never load half a file)
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-D__host__=", "-D__device__=", "-o", tmp, src,
                                   os.path.join(_CSRC, "dwbc_model.cpp"), "-lm"])
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        L.ip_create.restype = C.c_void_p
        L.ip_create.argtypes = [C.c_char_p]
        L.ip_error.restype = C.c_char_p
        L.ip_error.argtypes = [C.c_void_p]
        for f in ("ip_destroy", "ip_ndof", "ip_fstar_total", "ip_stride"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.ip_add_contact.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
        L.ip_add_task.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ip_set_tau_lim.argtypes = [C.c_void_p, C.c_void_p]
        L.ip_run_cycle.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4
        L.ip_run_redist.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
        _lib = L
    return _lib


class EmuInstPar:
    def __init__(self, urdf, contacts, tau_lim=None, tasks=()):
        L = lib()
        self.L = L
        self.h = L.ip_create(urdf.encode())
        err = L.ip_error(self.h).decode()
        if err:
            raise RuntimeError(err)
        self.n = L.ip_ndof(self.h)
        self.m = self.n - 6
        for c in contacts:
            pt = np.asarray(c["point"], dtype=np.float64)
            assert L.ip_add_contact(self.h, c["link"], pt.ctypes.data, c["lx"], c["ly"], c.get("mu", 0.2), c.get("muz", 0.2)) >= 0
        for lv, links in enumerate(tasks):
            for mode, link, pt in links:
                p = np.asarray(pt, dtype=np.float64)
                assert L.ip_add_task(self.h, lv, mode, link, p.ctypes.data) == 1, L.ip_error(self.h)
        if tau_lim is not None:
            t = np.asarray(tau_lim, dtype=np.float64)
            L.ip_set_tau_lim(self.h, t.ctypes.data)
        self.ncon = len(contacts)
        self.F = L.ip_fstar_total(self.h)
        self.stride = L.ip_stride(self.h)
        assert self.stride == self.m + 4 * self.ncon

    def _record(self, B, record):
        if record is None:
            return None
        r = np.ascontiguousarray(record, np.float64)
        assert r.shape == (B, self.stride), r.shape
        return r

    def run_cycle(self, q, flags, fstar, record=None, compact=False):
        B = q.shape[0]
        q = np.ascontiguousarray(q, np.float64)
        flags = np.ascontiguousarray(flags, np.uint8)
        fstar = np.ascontiguousarray(fstar, np.float64)
        assert flags.shape == (B, self.ncon) and fstar.shape == (B, self.F)
        rec = self._record(B, record)
        tau = np.full((B, 3, self.m), np.nan)
        wr = np.full((B, 12), np.nan)
        st = np.full(B, -1, np.int32)
        diag = np.zeros((B, 90), np.int32)  # DG_COUNT
        ok = self.L.ip_run_cycle(self.h, B, q.ctypes.data, flags.ctypes.data, fstar.ctypes.data, None if rec is None else rec.ctypes.data, int(compact),
                                 tau.ctypes.data, wr.ctypes.data, st.ctypes.data, diag.ctypes.data)
        assert ok == 1, self.L.ip_error(self.h)
        return dict(tau=tau, wrench=wr, status=st)

    def run_redist(self, q, flags, tau_in, record=None):
        B = q.shape[0]
        q = np.ascontiguousarray(q, np.float64)
        flags = np.ascontiguousarray(flags, np.uint8)
        tau_in = np.ascontiguousarray(tau_in, np.float64)
        assert flags.shape == (B, self.ncon) and tau_in.shape == (B, self.m)
        rec = self._record(B, record)
        fstar = np.zeros((B, max(self.F, 1)))
        tau = np.full((B, self.m), np.nan)
        cf = np.full((B, 6), np.nan)
        wr = np.full((B, 2, 12), np.nan)
        st = np.full(B, -1, np.int32)
        ok = self.L.ip_run_redist(self.h, B, q.ctypes.data, flags.ctypes.data, fstar.ctypes.data, tau_in.ctypes.data, None if rec is None else rec.ctypes.data,
                                  tau.ctypes.data, cf.ctypes.data, wr.ctypes.data, st.ctypes.data)
        assert ok == 1, self.L.ip_error(self.h)
        return dict(tau=tau, cf=cf, wrench=wr, status=st)

    def __del__(self):
        try:
            self.L.ip_destroy(self.h)
        except Exception:
            pass
