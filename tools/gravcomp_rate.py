#!/usr/bin/env python3
"""Time per launch of the gravity-compensation kernel, alone and ahead of the redistribution, against the plain redistribution and
against the PARENT commit's ways to the same results.

    python tools/gravcomp_rate.py --parent-lib /path/to/parent/libdwbc_amd/libdwbc_hip.so [--steps 200] [--out profiles/gravcomp_rate.txt]

Routes, every run in a process of its own under a time limit of its own (two builds of one library do not share a process), the routes
alternating, three runs of --steps launches each after a warm one, HIP-event time per launch:
  (a) gravity only                           dwbc_batch_time_grav
  (b) redistribution with the option         dwbc_batch_time_redistribute, DWBC_REDIST_ADD_GRAVITY
  (c) plain redistribution                   dwbc_batch_time_redistribute
  (d) the parent's lean cycle                dwbc_batch_time_solves of the parent library -- its only way to torque_grav_
  (e) the parent's lean cycle, then its plain redistribution -- its only way to what (b) returns; the two timed back to back, summed
TOCABI on the states of BASELINE configs[1] (synth_batch seed 20251226 + 2, double support, pelvis 6D + upper-body rotation, torque limit
300) and the head-fixed 37-dof / 32-body model through its kernel pack (tests/test_model_packs.py states, seed 7), B = 1024 and 8192.
The torque that is redistributed is the same in (b), (c) and (e): the cycle's own total torque pushed along the contact null space by
NwJw d, d = 10 N(0, I6) (every QP at work); (b) is handed that torque minus the cycle's torque_grav_.
Conditions (structural): (a) below (d) by more than the spread of (d)'s three runs, (b) below (e) by more than (e)'s spread; (b) - (c),
the price of the gravity torque, and (a) against (c) are reported as measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HQP_INIT = 1 | 2
ADD_GRAVITY = 8
F_TAU, F_STATUS, F_REDIST_STATUS, F_NWJW = 10, 12, 17, 37
ROUTES = (("a", "gravity only", False), ("b", "redistribution with the option", False), ("c", "plain redistribution", False),
          ("d", "parent: lean cycle", True), ("e", "parent: lean cycle + plain redistribution", True))


def child(lib_path, route, model, urdf, B, steps):
    import numpy as np

    from libdwbc_amd import workloads as W

    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.dwbc_model_create_from_urdf.restype = vp
    L.dwbc_batch_create.restype = vp
    L.dwbc_last_error.restype = C.c_char_p

    def ok(r):
        if not r:
            raise RuntimeError(L.dwbc_last_error().decode())

    dbl = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    md = vp(L.dwbc_model_create_from_urdf(urdf.encode(), 1))
    ok(md.value)
    if model == "tocabi":
        links = (W.CONTACTS_2[0]["link"], W.CONTACTS_2[1]["link"], 15)
        q, _, fstar = W.synth_batch(B, seed=20251226 + 2)
    else:
        from oracle import urdf_model
        from tests.test_model_packs import variant_states

        mo = urdf_model.load_urdf(urdf)
        names = list(mo["names"])
        links = tuple(names.index(n) for n in ("L_AnkleRoll_Link", "R_AnkleRoll_Link", "Upperbody_Link"))
        q, fstar = variant_states(mo, B, seed=7)
    m = q.shape[1] - 7
    b = vp(L.dwbc_batch_create(md, B, 0, 0))
    ok(b.value)
    for c, l in zip(W.CONTACTS_2, links):
        p = dbl(c["point"])
        assert L.dwbc_batch_add_contact(b, l, 0, vp(p.ctypes.data), C.c_double(c["lx"]), C.c_double(c["ly"]), C.c_double(c["mu"]), C.c_double(c["muz"])) >= 0
    z = dbl([0, 0, 0])
    ok(L.dwbc_batch_add_task(b, 0, 0, 0, vp(z.ctypes.data)))         # pelvis 6D
    ok(L.dwbc_batch_add_task(b, 1, 6, links[2], vp(z.ctypes.data)))  # upper-body rotation
    lim = dbl(np.full(m, 300.0))
    ok(L.dwbc_batch_set_torque_limit(b, vp(lim.ctypes.data)))
    q, flags = dbl(q), np.ones((B, 2), np.uint8)
    ok(L.dwbc_batch_set_state(b, vp(q.ctypes.data), None, None))
    ok(L.dwbc_batch_set_contact(b, vp(flags.ctypes.data)))
    f0, f1 = dbl(fstar[:, :6]), dbl(fstar[:, 6:9])
    ok(L.dwbc_batch_set_fstar(b, 0, vp(f0.ctypes.data)))
    ok(L.dwbc_batch_set_fstar(b, 1, vp(f1.ctypes.data)))
    # the cycle once with the dump record: its torques and NwJw make the torque input
    ok(L.dwbc_batch_enable_dump(b, 1))
    ok(L.dwbc_batch_solve(b, HQP_INIT))
    tau3, nwjw = np.zeros((B, 3, m)), np.zeros((B, m, 6))
    ok(L.dwbc_batch_get(b, F_TAU, vp(tau3.ctypes.data), C.c_size_t(tau3.nbytes)))
    ok(L.dwbc_batch_get(b, F_NWJW, vp(nwjw.ctypes.data), C.c_size_t(nwjw.nbytes)))
    ok(L.dwbc_batch_enable_dump(b, 0))
    tin = tau3.sum(axis=1) + np.einsum("bij,bj->bi", nwjw, 10.0 * np.random.default_rng(11).standard_normal((B, 6)))
    if route == "b":
        tin = tin - tau3[:, 0]
    tin = dbl(tin)
    ok(L.dwbc_batch_set_torque_input(b, vp(tin.ctypes.data)))
    ms, ms2 = C.c_float(0), C.c_float(0)
    st = np.zeros(B, np.int32)
    name = C.c_char_p
    for f in ("dwbc_batch_kernel_name", "dwbc_batch_redistribute_kernel_name"):
        getattr(L, f).restype = name
    if route == "a":
        L.dwbc_batch_grav_kernel_name.restype = name
        ok(L.dwbc_batch_time_grav(b, steps, C.byref(ms)))
        ok(L.dwbc_batch_get_grav(b, 2, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        kernel = L.dwbc_batch_grav_kernel_name(b).decode()
    elif route in ("b", "c"):
        fl = HQP_INIT | (ADD_GRAVITY if route == "b" else 0)
        ok(L.dwbc_batch_time_redistribute(b, fl, steps, C.byref(ms)))
        ok(L.dwbc_batch_get(b, F_REDIST_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        if route == "b":
            L.dwbc_batch_grav_kernel_name.restype = name
        kernel = (L.dwbc_batch_grav_kernel_name if route == "b" else L.dwbc_batch_redistribute_kernel_name)(b).decode()
    else:
        ok(L.dwbc_batch_solve(b, HQP_INIT))  # (the dump is off again: the lean cycle)
        ok(L.dwbc_batch_sync(b))
        ok(L.dwbc_batch_time_solves(b, HQP_INIT, steps, C.byref(ms)))
        ok(L.dwbc_batch_get(b, F_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        kernel = L.dwbc_batch_kernel_name(b).decode()
        if route == "e":
            ok(L.dwbc_batch_time_redistribute(b, HQP_INIT, steps, C.byref(ms2)))
            kernel += " + " + L.dwbc_batch_redistribute_kernel_name(b).decode()
    L.dwbc_batch_destroy(b)
    print(json.dumps(dict(route=route, B=B, ms=(ms.value + ms2.value) / steps, kernel=kernel, status_ok=float(st.mean()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libdwbc_hip.so built from the parent commit, with its kernel packs beside it")
    ap.add_argument("--lib", default=os.path.join(ROOT, "libdwbc_amd", "libdwbc_hip.so"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=5, metavar=("LIB", "ROUTE", "MODEL", "URDF", "B"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.child[2], args.child[3], int(args.child[4]), args.steps)
        return
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    from libdwbc_amd import workloads as W
    from tests import cases
    from tests.test_model_packs import VARIANTS

    lines = ["Gravity compensation alone (a) and ahead of the redistribution (b) against the plain redistribution (c), the parent commit's lean cycle (d)",
             "and the parent's lean cycle followed by its plain redistribution (e) (tools/gravcomp_rate.py): one MI355X, every run in a process of its own,",
             f"routes alternating, three runs each of {args.steps} launches after a warm one; HIP-event ms per launch, median, spread = max - min of the three.", ""]
    verdict = []
    with tempfile.TemporaryDirectory() as tmp:
        models = (("tocabi", W.TOCABI_URDF), ("fixed_head", cases.variant_urdf(os.path.join(tmp, "fixed_head.urdf"), VARIANTS["fixed_head"][0])))
        for model, urdf in models:
            for B in (1024, 8192):
                runs = {r[0]: [] for r in ROUTES}
                info = {}
                for _ in range(3):
                    for route, _, parent in ROUTES:
                        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--child", args.parent_lib if parent else args.lib, route,
                                              model, urdf, str(B)], capture_output=True, text=True, timeout=300)
                        if out.returncode != 0:  # nothing more is started on the device after a failed run
                            sys.stderr.write(out.stdout + out.stderr)
                            sys.exit(f"route ({route}) on {model} at B = {B} ended with status {out.returncode}")
                        r = json.loads(out.stdout.strip().splitlines()[-1])
                        runs[route].append(r["ms"])
                        info[route] = r
                med = {k: statistics.median(v) for k, v in runs.items()}
                spread = {k: max(v) - min(v) for k, v in runs.items()}
                for route, label, _ in ROUTES:
                    r = info[route]
                    lines.append(f"{model:10s} B = {B:5d}  ({route}) {label:44s} {' '.join(f'{x:7.4f}' for x in runs[route])}   median {med[route]:7.4f} spread {spread[route]:6.4f} ms"
                                 f"   status ok {r['status_ok']:.3f}   {r['kernel']}")
                lines.append("")
                verdict.append(f"{model} B = {B}: (a) {med['a']:.4f} against (d) {med['d']:.4f} ms, (d)'s spread {spread['d']:.4f}: {'below' if med['d'] - med['a'] > spread['d'] else 'NOT below'};  "
                               f"(b) {med['b']:.4f} against (e) {med['e']:.4f} ms, (e)'s spread {spread['e']:.4f}: {'below' if med['e'] - med['b'] > spread['e'] else 'NOT below'};  "
                               f"(b) - (c) = {med['b'] - med['c']:+.4f} ms, (a) / (c) = {med['a'] / med['c']:.3f}")
    lines += verdict
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
