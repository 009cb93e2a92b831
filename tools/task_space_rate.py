#!/usr/bin/env python3
"""Time per launch of the task-space kernel (SetTaskSpace + CalcTaskSpace: J_task, Lambda_task, J_kt, Null_task per level) against the
PARENT commit's only way to the first three, a full solve with the dump record on.

    python tools/task_space_rate.py --parent-lib /path/to/parent/libdwbc_amd/libdwbc_hip.so [--steps 200] [--out profiles/task_space_rate.txt]

Routes, every run in a process of its own under a time limit of its own (two builds of one library do not share a process), the routes
alternating, three runs of --steps launches each after a warm one, HIP-event time per launch:
  (a) {J_task}                         dwbc_batch_time_task_space: nothing behind the kinematics
  (b) {J_task, Lambda_task, J_kt}      dwbc_batch_time_task_space: what the parent's dump record holds; no projector
  (c) all outputs                      dwbc_batch_time_task_space: with Null_task of the first three levels (3 m^2 doubles per instance more)
  (d) the parent's way                 dwbc_batch_time_solves of the parent library with the dump record on, torque limit 300 (a caller then
                                       pulls the three fields out of the record with dwbc_batch_get, which is not in this figure)
Hierarchy H4 on every route: pelvis 6D, upper-body rotation, left hand 6D, right hand 6D.  Both feet down.  TOCABI on the states of BASELINE
configs[1] (synth_batch seed 20251226 + 2), the hands' f* a seeded uniform; B = 1024 and 8192.
Condition (structural): (b) below (d) by more than the spread of (d)'s three runs.  (a) and (c) are reported as measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HQP_INIT = 1 | 2
F_STATUS = 12
TS_STATUS = 4
MASKS = {"a": 1, "b": 1 | 2 | 4, "c": 1 | 2 | 4 | 8}
ROUTES = (("a", "{J_task}", False), ("b", "{J_task, Lambda_task, J_kt}", False), ("c", "all outputs", False), ("d", "parent: dump-on solve", True))
H4 = ((0, 0, 0), (1, 6, 15), (2, 0, 23), (3, 0, 33))  # (level, mode, link)


def child(lib_path, route, B, steps):
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

    def dbl(a):
        return np.ascontiguousarray(a, np.float64)

    md = vp(L.dwbc_model_create_from_urdf(W.TOCABI_URDF.encode(), 1))
    ok(md.value)
    q, _, fstar = W.synth_batch(B, seed=20251226 + 2)
    hands = 0.5 * np.random.default_rng(20251226 + 3).uniform(-1, 1, size=(B, 12))
    n = q.shape[1] - 1
    b = vp(L.dwbc_batch_create(md, B, 0, 0))
    ok(b.value)
    q = dbl(q)
    ok(L.dwbc_batch_set_state(b, vp(q.ctypes.data), None, None))
    ms = C.c_float(0)
    st = np.zeros(B, np.int32)
    for c in W.CONTACTS_2:
        p = dbl(c["point"])
        assert L.dwbc_batch_add_contact(b, c["link"], 0, vp(p.ctypes.data), C.c_double(c["lx"]), C.c_double(c["ly"]), C.c_double(c["mu"]), C.c_double(c["muz"])) >= 0
    flags = np.ones((B, 2), np.uint8)
    ok(L.dwbc_batch_set_contact(b, vp(flags.ctypes.data)))
    z = dbl([0, 0, 0])
    for level, mode, link in H4:
        ok(L.dwbc_batch_add_task(b, level, mode, link, vp(z.ctypes.data)))
    if route == "d":
        lim = dbl(np.full(n - 6, 300.0))
        ok(L.dwbc_batch_set_torque_limit(b, vp(lim.ctypes.data)))
        for level, f in enumerate((fstar[:, :6], fstar[:, 6:9], hands[:, :6], hands[:, 6:])):
            f = dbl(f)
            ok(L.dwbc_batch_set_fstar(b, level, vp(f.ctypes.data)))
        ok(L.dwbc_batch_enable_dump(b, 1))
        ok(L.dwbc_batch_time_solves(b, HQP_INIT, steps, C.byref(ms)))
        ok(L.dwbc_batch_get(b, F_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        L.dwbc_batch_kernel_name.restype = C.c_char_p
        kernel = L.dwbc_batch_kernel_name(b).decode()
    else:
        ok(L.dwbc_batch_set_task_space_outputs(b, C.c_uint(MASKS[route])))
        ok(L.dwbc_batch_time_task_space(b, steps, C.byref(ms)))
        ok(L.dwbc_batch_get_task_space(b, 0, TS_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        L.dwbc_batch_task_space_kernel_name.restype = C.c_char_p
        kernel = L.dwbc_batch_task_space_kernel_name(b).decode()
    L.dwbc_batch_destroy(b)
    print(json.dumps(dict(route=route, B=B, ms=ms.value / steps, kernel=kernel, status_ok=float(st.mean()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libdwbc_hip.so built from the parent commit")
    ap.add_argument("--lib", default=os.path.join(ROOT, "libdwbc_amd", "libdwbc_hip.so"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, metavar=("LIB", "ROUTE", "B"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], int(args.child[2]), args.steps)
        return
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    lines = ["The task-space launch with {J_task} (a), {J_task, Lambda_task, J_kt} (b) and all outputs (c) against the parent commit's only way to these",
             "matrices, a solve with the dump record on (d) (tools/task_space_rate.py): hierarchy H4, both feet down, TOCABI, one MI355X, every run in a process of",
             f"its own, routes alternating, three runs each of {args.steps} launches after a warm one; HIP-event ms per launch, median, spread = max - min of the three.", ""]
    verdict = []
    for B in (1024, 8192):
        runs = {r[0]: [] for r in ROUTES}
        info = {}
        for _ in range(3):
            for route, _, parent in ROUTES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--child", args.parent_lib if parent else args.lib, route, str(B)],
                                     capture_output=True, text=True, timeout=300)
                if out.returncode != 0:  # nothing more is started on the device after a failed run
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(f"route ({route}) at B = {B} ended with status {out.returncode}")
                r = json.loads(out.stdout.strip().splitlines()[-1])
                runs[route].append(r["ms"])
                info[route] = r
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = {k: max(v) - min(v) for k, v in runs.items()}
        for route, label, _ in ROUTES:
            r = info[route]
            lines.append(f"B = {B:5d}  ({route}) {label:28s} {' '.join(f'{x:7.4f}' for x in runs[route])}   median {med[route]:7.4f} spread {spread[route]:6.4f} ms"
                         f"   status ok {r['status_ok']:.3f}   {r['kernel']}")
            print(lines[-1], flush=True)
        lines.append("")
        verdict.append(f"B = {B}: (b) {med['b']:.4f} against (d) {med['d']:.4f} ms, (d)'s spread {spread['d']:.4f}: {'below' if med['d'] - med['b'] > spread['d'] else 'NOT below'};  "
                       f"(b) / (d) = {med['b'] / med['d']:.3f};  (a) {med['a']:.4f} ms, (c) {med['c']:.4f} ms as measured")
    lines += verdict
    text = "\n".join(lines) + "\n"
    print("\n".join(verdict))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
