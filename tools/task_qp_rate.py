#!/usr/bin/env python3
"""Time per launch of the single-level task-QP kernel (CalcSingleTaskTorqueWithQP of one level) beside the PARENT commit's task-space launch
of a one-level set-up with all its outputs and its one-level lean cycle.

    python tools/task_qp_rate.py --parent-lib /path/to/parent/libdwbc_amd/libdwbc_hip.so [--steps 200] [--out profiles/task_qp_rates.txt]

Routes, every run in a process of its own under a time limit of its own (two builds of one library do not share a process), the routes
alternating, three runs of --steps launches each after a warm one, HIP-event time per launch:
  (a) task QP, level 0, identity       dwbc_batch_time_task_qp on a one-level set-up (pelvis 6D), all outputs, torque_prev = torque_grav_
  (b) task QP, level 1, null matrix    dwbc_batch_time_task_qp on the two-level set-up (upper-body rotation beneath the pelvis), all outputs,
                                       with Null_task of level 0 (m x m per instance, from dwbc_batch_calc_task_space on the same batch) read
                                       from device memory; torque_prev = torque_grav_ (what level 0 adds is left out: a figure of the rate)
  (c) parent: task space, one level    dwbc_batch_time_task_space of the parent library, one-level set-up, J_task, Lambda_task and J_kt
  (d) parent: one-level lean cycle     dwbc_batch_time_solves of the parent library, one-level set-up, hqp, cold, no dump record
Both feet down, torque limit cases.TAU_LIM.  TOCABI on the states of BASELINE configs[1] (synth_batch seed 20251226 + 2); B = 1024 and 8192.
No condition: the figures are reported as measured."""
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
ROUTES = (("a", "task QP, level 0, identity", False), ("b", "task QP, level 1, null matrix", False), ("c", "parent: task space, one level", True),
          ("d", "parent: one-level lean cycle", True))
LEVELS = ((0, 0, 0), (1, 6, 15))  # (level, mode, link)


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
    n = q.shape[1] - 1
    m = n - 6
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
    for level, mode, link in LEVELS[: 2 if route == "b" else 1]:
        ok(L.dwbc_batch_add_task(b, level, mode, link, vp(z.ctypes.data)))
    lim = dbl(W.TAU_LIM)
    ok(L.dwbc_batch_set_torque_limit(b, vp(lim.ctypes.data)))
    for level, f in enumerate((fstar[:, :6], fstar[:, 6:9])[: 2 if route == "b" else 1]):
        f = dbl(f)
        ok(L.dwbc_batch_set_fstar(b, level, vp(f.ctypes.data)))
    name = {"a": "task_qp", "b": "task_qp", "c": "task_space", "d": ""}[route]
    if route in "ab":
        ok(L.dwbc_batch_grav_compensation(b))
        tg = np.zeros((B, m))
        ok(L.dwbc_batch_get_grav(b, 0, vp(tg.ctypes.data), C.c_size_t(tg.nbytes)))
        null = None
        if route == "b":  # Null_task of level 0 from the task-space launch on the same batch: the projector the reference hands to level 1
            null = np.zeros((B, m, m))
            ok(L.dwbc_batch_set_task_space_outputs(b, C.c_uint(1 << 3)))
            ok(L.dwbc_batch_calc_task_space(b))
            ok(L.dwbc_batch_get_task_space(b, 0, 3, vp(null.ctypes.data), C.c_size_t(null.nbytes)))
            assert np.abs(null - np.eye(m)).max() > 0.1 and np.abs(null @ null - null).max() < 1e-9  # a projector, not the identity
        ok(L.dwbc_batch_set_task_qp(b, 1 if route == "b" else 0, C.c_uint(63)))
        ok(L.dwbc_batch_set_task_qp_inputs(b, vp(tg.ctypes.data), vp(null.ctypes.data) if null is not None else None))
        ok(L.dwbc_batch_time_task_qp(b, steps, C.byref(ms)))
        ok(L.dwbc_batch_get_task_qp(b, 5, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
    elif route == "c":
        ok(L.dwbc_batch_set_task_space_outputs(b, C.c_uint(1 | 2 | 4)))
        ok(L.dwbc_batch_time_task_space(b, steps, C.byref(ms)))
        ok(L.dwbc_batch_get_task_space(b, 0, 4, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
    else:
        ok(L.dwbc_batch_time_solves(b, HQP_INIT, steps, C.byref(ms)))
        ok(L.dwbc_batch_get(b, F_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
    fn = getattr(L, f"dwbc_batch_{name}_kernel_name" if name else "dwbc_batch_kernel_name")
    fn.restype = C.c_char_p
    kernel = fn(b).decode()
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
    lines = ["The single-level task-QP launch at level 0 without a null matrix (a) and at level 1 with one (b), all outputs, beside the parent commit's task-space",
             "launch of a one-level set-up with all its outputs (c) and its one-level lean cycle (d) (tools/task_qp_rate.py): both feet down, torque limit, TOCABI,",
             f"one MI355X, every run in a process of its own, routes alternating, three runs each of {args.steps} launches after a warm one; HIP-event ms per launch,",
             "median, spread = max - min of the three.", ""]
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
        for route, label, _ in ROUTES:
            r = info[route]
            lines.append(f"B = {B:5d}  ({route}) {label:30s} {' '.join(f'{x:7.4f}' for x in runs[route])}   median {statistics.median(runs[route]):7.4f} "
                         f"spread {max(runs[route]) - min(runs[route]):6.4f} ms   {B / statistics.median(runs[route]) / 1e3:6.2f} M instances/s   status ok {r['status_ok']:.3f}   {r['kernel']}")
            print(lines[-1], flush=True)
        lines.append("")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
