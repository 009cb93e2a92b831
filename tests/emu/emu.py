"""ctypes loader of the CPU emulation of the kernel source (tests/emu/emu_cycle.cpp).  TEST HARNESS ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}


class EmuRun(C.Structure):
    """everything a run reads beyond the context (struct EmuRun of emu_cycle.cpp)"""
    _fields_ = [("build", C.c_int), ("hqp", C.c_int), ("warm", C.c_int)] + [(k, C.c_void_p) for k in ("qdot", "traj", "ctime", "custom_J", "inst_par")]


EXTRAS, EXTRAS_GENERIC, COMPACT, TWO_WAVE, REDUCED, GC = range(6)  # enum EmuBuild

_P, _I, _D = C.c_void_p, C.c_int, C.c_double
# name: (restype, argtypes) of every entry point (emu_run_redist and emu_redist_lds_bytes: the fp64 library only)
_SIGNATURES = {
    "emu_create": (_P, [C.c_char_p]),
    "emu_create_from_arrays": (_P, [_I] + [_P] * 7),
    "emu_error": (C.c_char_p, [_P]),
    "emu_destroy": (None, [_P]),
    "emu_nb": (_I, [_P]),
    "emu_ndof": (_I, [_P]),
    "emu_link_id": (_I, [_P, C.c_char_p]),
    "emu_get_model": (None, [_P] * 8),
    "emu_add_contact": (_I, [_P, _I, _P, _D, _D, _D, _D]),
    "emu_add_task": (_I, [_P, _I, _I, _I, _P]),
    "emu_add_custom_task": (_I, [_P, _I, _I]),
    "emu_set_tau_lim": (None, [_P, _P]),
    "emu_set_traj": (None, [_P, _I, _I, _I, _P]),
    "emu_fstar_total": (_I, [_P]),
    "emu_dump_total": (_I, [_P]),
    "emu_dump_offset": (_I, [_P, C.c_char_p]),
    "emu_diag_count": (_I, []),
    "emu_lds_bytes": (_I, []),
    "emu_lds_bytes_reduced": (_I, [_I]),
    "emu_lds_bytes_v2": (_I, [_I]),
    "emu_lds_bytes_compact": (_I, [_I]),
    "emu_lds_bytes_pair": (_I, [_I]),
    "emu_run": (_I, [_P, C.POINTER(EmuRun), _I] + [_P] * 8),
    "emu_redist_lds_bytes": (_I, []),
    "emu_run_redist": (_I, [_P, _I] + [_P] * 9),
    "emu_hqp_create": (_P, [_I, _I, _I, _P, _P, _P, _I, _I]),
    "emu_hqp_destroy": (None, [_P]),
    "emu_hqp_rec": (_I, [_P]),
    "emu_hqp_offset": (_I, [_P, _I, _I]),
    "emu_hqp_data": (C.POINTER(_D), [_P]),
    "emu_hqp_stat": (C.POINTER(_I), [_P]),
    "emu_hqp_lds_bytes": (_I, [_P]),
    "emu_hqp_solve": (None, [_P]),
    "emu_hqp_set_exact": (None, [_P, _I, _I]),
    "emu_hqp_solve_levels": (None, [_P, _I, _I]),
    "emu_rrec_total": (_I, [_I]),
    "emu_rrec_offset": (_I, [_I, C.c_char_p]),
    "emu_reduced_record": (None, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "emu_jacc_rec": (_I, [_P]),
    "emu_jacc_rec_r": (_I, [_I]),
    "emu_jacc_nc_rec": (_I, [_I]),
    "emu_jacc_solve": (None, [_P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "emu_jacc_solve_r": (None, [_P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "emu_jacc_nc_solve": (None, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P]),
    "emu_lqp_configure": (None, [_P, _P, _I, _P, _I, _P, _P]),
    "emu_lqp_torque": (None, [_P, _P, _I, _I, _P, _P]),
    "emu_lqp_configure_r": (None, [_P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "emu_lqp_torque_r": (None, [_P, _P, _I, _P, _I, _P, _P]),
    "emu_lqp_nc_configure": (None, [_P, _P, _I, _I, _P, _P, _P, _I, _I]),
}


def lib(f32=False):
    if f32 not in _libs:
        subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = C.CDLL(os.path.join(_HERE, "libdwbc_emu_f32.so" if f32 else "libdwbc_emu.so"))
        for name, (res, args) in _SIGNATURES.items():
            if f32 and "redist" in name:
                continue
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        _libs[f32] = L
    return _libs[f32]


def _in(a, dtype=np.float64):
    """(array kept alive by the caller, its address) of an optional input"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype)
    return a, a.ctypes.data


class Emu:
    def __init__(self, urdf, contacts, tasks, tau_lim=None, f32=False):
        L = lib(f32)
        self.L = L
        if isinstance(urdf, dict):  # a model given as arrays (the result of model surgery)
            arrs = [np.ascontiguousarray(urdf["parent"], np.int32)] + [np.ascontiguousarray(urdf[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")]
            self.h = L.emu_create_from_arrays(int(urdf["nb"]), *[a.ctypes.data for a in arrs])
        else:
            self.h = L.emu_create(urdf.encode())
        err = L.emu_error(self.h).decode()
        if err:
            raise RuntimeError(err)
        self.n = L.emu_ndof(self.h)
        self.nb = L.emu_nb(self.h)
        self.m = self.n - 6
        for c in contacts:
            pt = np.asarray(c["point"], dtype=np.float64)
            assert L.emu_add_contact(self.h, c["link"], pt.ctypes.data, c["lx"], c["ly"], c.get("mu", 0.2), c.get("muz", 0.2)) >= 0
        for lv, links in enumerate(tasks):
            if isinstance(links, int):  # TASK_CUSTOM level of that many dof
                assert L.emu_add_custom_task(self.h, lv, links) == 1, L.emu_error(self.h)
                continue
            for mode, link, pt in links:
                p = np.asarray(pt, dtype=np.float64)
                assert L.emu_add_task(self.h, lv, mode, link, p.ctypes.data) == 1, L.emu_error(self.h)
        if tau_lim is not None:
            t = np.asarray(tau_lim, dtype=np.float64)
            L.emu_set_tau_lim(self.h, t.ctypes.data)
        self.ncon = len(contacts)
        self.stride = self.m + 4 * self.ncon  # of a per-instance record: [tau_lim[m] | lx ly mu muz of every contact]
        self.F = L.emu_fstar_total(self.h)
        self.D = L.emu_dump_total(self.h)
        self.DG = L.emu_diag_count()

    def model_arrays(self):
        nb = self.nb
        out = dict(parent=np.zeros(nb, np.int32), R_T=np.zeros((nb, 3, 3)), p_T=np.zeros((nb, 3)), axis=np.zeros((nb, 3)),
                   mass=np.zeros(nb), com=np.zeros((nb, 3)), inertia=np.zeros((nb, 3, 3)))
        self.L.emu_get_model(self.h, *[out[k].ctypes.data for k in ("parent", "R_T", "p_T", "axis", "mass", "com", "inertia")])
        return out

    def set_traj(self, level, link_index, slot, gains15):
        g = np.ascontiguousarray(gains15, np.float64)
        self.L.emu_set_traj(self.h, level, link_index, slot, g.ctypes.data)

    def _record(self, B, inst_par):
        rec, ptr = _in(inst_par)
        assert rec is None or rec.shape == (B, self.stride), rec.shape
        return rec, ptr

    def _run(self, build, q, flags, fstar, wrench_ld=12, dump=False, qdot=None, traj=None, ctime=None, custom_J=None, hqp=True, warm_diag=None, inst_par=None):
        """one emu_run; every output is pre-filled with NaN (status: -1), so an entry the kernel never writes shows up"""
        B = q.shape[0]
        q = np.ascontiguousarray(q, np.float64)
        flags = np.ascontiguousarray(flags, np.uint8)
        fstar = np.ascontiguousarray(fstar, np.float64)
        assert flags.shape == (B, self.ncon) and fstar.shape == (B, self.F)
        tau = np.full((B, 3, self.m), np.nan)
        wr = np.full((B, wrench_ld), np.nan)
        st = np.full(B, -1, np.int32)
        diag = np.full((B, self.DG), -1, np.int32)
        if warm_diag is not None:  # init = false: the working sets of a previous run (its "diag") seed the QPs
            diag[:] = warm_diag
        dmp = np.full((B, self.D), np.nan) if dump else None
        keep = [_in(a) for a in (qdot, traj, ctime, custom_J)] + [self._record(B, inst_par)]  # custom_J: (B, n_custom, 6, n)
        run = EmuRun(build, 1 if hqp else 0, 1 if warm_diag is not None else 0, *[ptr for _, ptr in keep])
        ok = self.L.emu_run(self.h, C.byref(run), B, q.ctypes.data, flags.ctypes.data, fstar.ctypes.data, tau.ctypes.data, wr.ctypes.data,
                            st.ctypes.data, diag.ctypes.data, dmp.ctypes.data if dump else None)
        assert ok == 1, self.L.emu_error(self.h)
        return dict(tau=tau, wrench=wr, status=st, diag=diag, dump=dmp)

    def run(self, q, flags, fstar, dump=False, reduced=False, qdot=None, traj=None, ctime=None, custom_J=None, hqp=True, dense=False, warm_diag=None, compact=False,
            inst_par=None):
        """compact: True = lean build on the compact LDS map (Lds3); "pair" = the two-wave kernel of dwbc_cycle2p.h, roles run in turn.
        dense: the extras build on TopoGeneric (dense A^-1 sweep).  inst_par: (B, stride) per-instance record"""
        build = REDUCED if reduced else TWO_WAVE if compact == "pair" else COMPACT if compact else EXTRAS_GENERIC if dense else EXTRAS
        return self._run(build, q, flags, fstar, dump=dump, qdot=qdot, traj=traj, ctime=ctime, custom_J=custom_J, hqp=hqp, warm_diag=warm_diag, inst_par=inst_par)

    def run_gc(self, q, flags, fstar):
        """the general-contact kernel (dwbc_cycle_gc.h, up to three simultaneously active contacts); wrench is (B, 18)"""
        r = self._run(GC, q, flags, fstar, wrench_ld=18)
        del r["dump"]
        return r

    def run_redist(self, q, flags, tau_in, inst_par=None):
        """the redistribution kernel for a caller-supplied torque (dwbc_redistribute.h); wrench is (B, 2, 12): of tau_in, of the answer"""
        B = q.shape[0]
        q = np.ascontiguousarray(q, np.float64)
        flags = np.ascontiguousarray(flags, np.uint8)
        tau_in = np.ascontiguousarray(tau_in, np.float64)
        assert flags.shape == (B, self.ncon) and tau_in.shape == (B, self.m)
        rec, rec_ptr = self._record(B, inst_par)
        fstar = np.zeros((B, max(self.F, 1)))
        tau = np.full((B, self.m), np.nan)
        cf = np.full((B, 6), np.nan)
        wr = np.full((B, 2, 12), np.nan)
        st = np.full(B, -1, np.int32)
        ok = self.L.emu_run_redist(self.h, B, q.ctypes.data, flags.ctypes.data, fstar.ctypes.data, tau_in.ctypes.data, rec_ptr, tau.ctypes.data, cf.ctypes.data,
                                   wr.ctypes.data, st.ctypes.data)
        assert ok == 1, self.L.emu_error(self.h)
        return dict(tau=tau, cf=cf, wrench=wr, status=st)

    def redist_lds_bytes(self):
        return self.L.emu_redist_lds_bytes()

    def dump_field(self, dmp, name, shape):
        off = self.L.emu_dump_offset(self.h, name.encode())
        assert off >= 0
        n = int(np.prod(shape))
        return dmp[:, off : off + n].reshape((dmp.shape[0],) + tuple(shape))

    def __del__(self):
        try:
            self.L.emu_destroy(self.h)
        except Exception:
            pass


class EmuHQP:
    """host emulation of the batched hierarchical-QP kernels (libdwbc_amd/csrc/dwbc_hqp.h), same entry points as the C-ABI"""

    def __init__(self, B, nv, m, e, has_cost, share_cost=False, solve_first=False):
        L = lib(False)
        self.L = L
        self.B, self.nv = B, nv
        self.m = np.asarray(m, np.int32)
        self.e = np.asarray(e, np.int32)
        self.hc = np.asarray(has_cost, np.int32)
        self.h = L.emu_hqp_create(B, nv, len(self.m), self.m.ctypes.data, self.e.ctypes.data, self.hc.ctypes.data, 1 if share_cost else 0, 1 if solve_first else 0)
        self.rec = np.ctypeslib.as_array(L.emu_hqp_data(self.h), shape=(B, L.emu_hqp_rec(self.h)))
        self.stat = np.ctypeslib.as_array(L.emu_hqp_stat(self.h), shape=(B, 24))

    def block(self, level, what, shape):
        """view of a per-instance block: what = 0 A 1 a 2 B 3 b 4 H 5 y 6 v 7 w"""
        off = self.L.emu_hqp_offset(self.h, level, what)
        n = int(np.prod(shape))
        return self.rec[:, off : off + n].reshape((self.B,) + tuple(shape))

    def solve(self):
        self.L.emu_hqp_solve(self.h)

    def configure_lqp(self, emu, act, dump, fstar, use_B=False):
        act = np.asarray(act, np.int32)
        dump = np.ascontiguousarray(dump, np.float64)
        fstar = np.ascontiguousarray(fstar, np.float64)
        self.L.emu_lqp_configure(self.h, emu.h, len(act), act.ctypes.data, 1 if use_B else 0, dump.ctypes.data, fstar.ctypes.data)

    def lqp_torque(self, emu, nc, dump, use_B=False):
        dump = np.ascontiguousarray(dump, np.float64)
        tau = np.zeros((self.B, emu.m))
        self.L.emu_lqp_torque(self.h, emu.h, nc, 1 if use_B else 0, dump.ctypes.data, tau.ctypes.data)
        return tau

    def set_exact(self, level, on=True):
        self.L.emu_hqp_set_exact(self.h, level, 1 if on else 0)

    def jacc_solve(self, emu, act, level, dump, fstar, prev):
        """CalcSingleTaskTorqueWithJACC_QP for one level; prev = list of (B, rec) arrays of the earlier levels"""
        L = self.L
        rs = L.emu_jacc_rec(emu.h)
        act = np.asarray(act, np.int32)
        dump = np.ascontiguousarray(dump, np.float64)
        fstar = np.ascontiguousarray(fstar, np.float64)
        prev = [np.ascontiguousarray(p, np.float64) for p in prev]
        ptrs = (C.c_void_p * max(1, len(prev)))(*[p.ctypes.data for p in prev])
        out = np.zeros((self.B, rs))
        st = np.zeros(self.B, np.int32)
        L.emu_jacc_solve(self.h, emu.h, len(act), act.ctypes.data, level, dump.ctypes.data, fstar.ctypes.data, ptrs, out.ctypes.data, st.ctypes.data)
        return out, st

    # ---- reduced variants (ConfigureLQP_R, JACC_QP_R and the _NC halves): same device functions on the reduced record
    @staticmethod
    def reduced_record(emu, B, vcd, cd, src, dump):
        L = lib(False)
        src = np.asarray(src, np.int32)
        dump = np.ascontiguousarray(dump, np.float64)
        rrec = np.zeros((B, L.emu_rrec_total(vcd + 6)))
        L.emu_reduced_record(emu.h, B, vcd, cd, len(src), src.ctypes.data, dump.ctypes.data, rrec.ctypes.data)
        return rrec

    @staticmethod
    def rrec_field(rrec, RS, name, shape):
        L = lib(False)
        off = L.emu_rrec_offset(RS, name.encode())
        n = int(np.prod(shape))
        return rrec[:, off : off + n].reshape((rrec.shape[0],) + tuple(shape))

    def configure_lqp_r(self, emu, act, RS, src, rrec, fstar):
        act = np.asarray(act, np.int32)
        src = np.asarray(src, np.int32)
        fstar = np.ascontiguousarray(fstar, np.float64)
        self.L.emu_lqp_configure_r(self.h, emu.h, len(act), act.ctypes.data, RS, len(src), src.ctypes.data, rrec.ctypes.data, fstar.ctypes.data)

    def lqp_torque_r(self, emu, act, RS, rrec):
        act = np.asarray(act, np.int32)
        tau = np.zeros((self.B, RS - 6))
        self.L.emu_lqp_torque_r(self.h, emu.h, len(act), act.ctypes.data, RS, rrec.ctypes.data, tau.ctypes.data)
        return tau

    def jacc_solve_r(self, emu, act, RS, src, level, rrec, fstar, prev):
        L = self.L
        act = np.asarray(act, np.int32)
        src = np.asarray(src, np.int32)
        fstar = np.ascontiguousarray(fstar, np.float64)
        prev = [np.ascontiguousarray(p, np.float64) for p in prev]
        ptrs = (C.c_void_p * max(1, len(prev)))(*[p.ctypes.data for p in prev])
        out = np.zeros((self.B, L.emu_jacc_rec_r(RS)))
        st = np.zeros(self.B, np.int32)
        L.emu_jacc_solve_r(self.h, emu.h, len(act), act.ctypes.data, RS, len(src), src.ctypes.data, level, rrec.ctypes.data, fstar.ctypes.data, ptrs, out.ctypes.data, st.ctypes.data)
        return out, st

    def configure_lqp_nc(self, emu, vcd, level, dump, fstar, prev, prev_off=0):
        """prev: (B, stride) array whose columns prev_off.. hold the reduced answer [base 6 | chain | centroidal 6]"""
        dump = np.ascontiguousarray(dump, np.float64)
        fstar = np.ascontiguousarray(fstar, np.float64)
        prev = np.ascontiguousarray(prev, np.float64)
        self.L.emu_lqp_nc_configure(self.h, emu.h, vcd, level, dump.ctypes.data, fstar.ctypes.data, prev.ctypes.data, prev.shape[1], prev_off)

    def solve_levels(self, n_levels, solve_first):
        self.L.emu_hqp_solve_levels(self.h, n_levels, 1 if solve_first else 0)

    def jacc_solve_nc(self, emu, vcd, level, dump, fstar, prev):
        L = self.L
        dump = np.ascontiguousarray(dump, np.float64)
        fstar = np.ascontiguousarray(fstar, np.float64)
        prev = np.ascontiguousarray(prev, np.float64)
        out = np.zeros((self.B, L.emu_jacc_nc_rec(emu.n - vcd)))
        st = np.zeros(self.B, np.int32)
        L.emu_jacc_nc_solve(self.h, emu.h, vcd, level, dump.ctypes.data, fstar.ctypes.data, prev.ctypes.data, prev.shape[1], out.ctypes.data, st.ctypes.data)
        return out, st

    def status(self, level):
        return self.stat[:, level]

    def iters(self, level):
        return self.stat[:, 8 + level]

    def null_size(self, level):
        return self.stat[:, 16 + level]

    def __del__(self):
        try:
            self.L.emu_hqp_destroy(self.h)
        except Exception:
            pass
