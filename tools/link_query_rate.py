#!/usr/bin/env python3
"""Time per launch of the link-query kernel (dwbc_batch_update_kinematics) against the PARENT commit's two routes to the same data.

    python tools/link_query_rate.py --parent-lib /path/to/parent/libdwbc_amd/libdwbc_hip.so [--steps 200] [--out profiles/link_query_rate.txt]

States: BASELINE configs[1] (synth_batch seed 20251226 + 2, double support, pelvis 6D + upper-body rotation, torque limit 300) with joint
rates U(-1, 1) of default_rng(5), at B = 1024 and B = 8192.  Query: the pelvis, both feet at their contact points, the upper body, both
hands and the COM link, with and without Jacobians.  The parent's routes: (a) its lean cycle, which gives none of the data and is the
yardstick -- the query does a strict subset of its work, so it has to be below it -- and (b) its cycle with the dump record enabled
followed by dwbc_batch_get of link_R / link_p / link_v / link_w, which is how a caller got at link poses before.  The four run
alternately, three times each, every run in a process of its own (two builds of one library do not share a process), each after a warm
launch; medians are reported.  `device` is HIP-event time over `steps` back-to-back launches; `with get` is a host clock around one launch
plus the read-back of its outputs to host memory, the mean of 20."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HQP_INIT = 1 | 2
F_STATUS, F_LINK_R, F_LINK_P, F_LINK_V, F_LINK_W = 12, 40, 41, 55, 56
LINKS = (0, 6, 12, 15, 23, 33, 34)
N_GET = 20


def child(lib_path, what, B, steps):
    """one measurement through the C-ABI of the library at lib_path (the parent's has no link-query entry points)"""
    import numpy as np

    from libdwbc_amd import workloads as W

    L = C.CDLL(lib_path)
    # the HIP runtime the library has loaded: events on the batch's (null) stream
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    vp = C.c_void_p
    L.dwbc_model_create_from_urdf.restype = vp
    L.dwbc_batch_create.restype = vp
    L.dwbc_last_error.restype = C.c_char_p
    L.dwbc_batch_kernel_name.restype = C.c_char_p

    def ok(r):
        if not r:
            raise RuntimeError(L.dwbc_last_error().decode())

    def hip_ok(e):
        if e != 0:
            raise RuntimeError(f"HIP error {e}")

    model = vp(L.dwbc_model_create_from_urdf(W.TOCABI_URDF.encode(), 1))
    b = vp(L.dwbc_batch_create(model, B, 0, 0))
    ok(b.value)
    dbl = lambda a: np.ascontiguousarray(a, np.float64)
    for c in W.CONTACTS_2:
        p = dbl(c["point"])
        assert L.dwbc_batch_add_contact(b, c["link"], 0, vp(p.ctypes.data), C.c_double(c["lx"]), C.c_double(c["ly"]), C.c_double(c["mu"]), C.c_double(c["muz"])) >= 0
    z = dbl([0, 0, 0])
    for lv, links in enumerate(W.TASKS_2LEVEL):
        for mode, link, _ in links:
            ok(L.dwbc_batch_add_task(b, lv, mode, link, vp(z.ctypes.data)))
    lim = dbl(W.TAU_LIM)
    ok(L.dwbc_batch_set_torque_limit(b, vp(lim.ctypes.data)))
    q, flags, fstar = W.synth_batch(B, seed=20251226 + 2)
    q, flags = dbl(q), np.ascontiguousarray(flags, np.uint8)
    qd = dbl(np.random.default_rng(5).uniform(-1, 1, (B, 39)))
    ok(L.dwbc_batch_set_state(b, vp(q.ctypes.data), vp(qd.ctypes.data), None))
    ok(L.dwbc_batch_set_contact(b, vp(flags.ctypes.data)))
    f0, f1 = dbl(fstar[:, :6]), dbl(fstar[:, 6:9])
    ok(L.dwbc_batch_set_fstar(b, 0, vp(f0.ctypes.data)))
    ok(L.dwbc_batch_set_fstar(b, 1, vp(f1.ctypes.data)))
    res = dict(what=what, B=B)
    if what.startswith("cycle"):
        dump = what == "cycle_dump"
        ok(L.dwbc_batch_enable_dump(b, 1 if dump else 0))
        launch = lambda: ok(L.dwbc_batch_solve(b, HQP_INIT))
        outs = [(f, np.zeros((B, 48, w))) for f, w in ((F_LINK_R, 9), (F_LINK_P, 3), (F_LINK_V, 3), (F_LINK_W, 3))] if dump else []
        get = lambda: [ok(L.dwbc_batch_get(b, f, vp(a.ctypes.data), C.c_size_t(a.nbytes))) for f, a in outs]
    else:
        jac = what == "query_jac"
        links = np.ascontiguousarray(LINKS, np.int32)
        pts = dbl([(0, 0, 0), W.CONTACTS_2[0]["point"], W.CONTACTS_2[1]["point"], (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)])
        ok(L.dwbc_batch_set_link_query(b, len(LINKS), vp(links.ctypes.data), vp(pts.ctypes.data), 1 if jac else 0))
        launch = lambda: ok(L.dwbc_batch_update_kinematics(b))
        n = len(LINKS)
        outs = [(w, np.zeros((B, n, k))) for w, k in ((0, 3), (1, 9), (2, 6))] + ([(3, np.zeros((B, n, 6 * 39)))] if jac else [])
        get = lambda: [ok(L.dwbc_batch_get_link_query(b, w, vp(a.ctypes.data), C.c_size_t(a.nbytes))) for w, a in outs]
    launch()  # uploads + warm launch
    ok(L.dwbc_batch_sync(b))
    e0, e1, ms = vp(), vp(), C.c_float(0)
    hip_ok(hip.hipEventCreate(C.byref(e0)))
    hip_ok(hip.hipEventCreate(C.byref(e1)))
    hip_ok(hip.hipEventRecord(e0, None))
    for _ in range(steps):
        launch()
    hip_ok(hip.hipEventRecord(e1, None))
    hip_ok(hip.hipEventSynchronize(e1))
    hip_ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    res["ms"] = ms.value / steps
    if outs:
        get()
        t0 = time.perf_counter()
        for _ in range(N_GET):
            launch()
            get()
        res["ms_get"] = (time.perf_counter() - t0) * 1e3 / N_GET
        res["get_bytes"] = int(sum(a.nbytes for _, a in outs))
    if what.startswith("cycle"):
        st = np.zeros(B, np.int32)
        ok(L.dwbc_batch_get(b, F_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        res.update(kernel=L.dwbc_batch_kernel_name(b).decode(), status_ok=float(st.mean()))
    else:
        L.dwbc_batch_link_query_kernel_name.restype = C.c_char_p
        res.update(kernel=L.dwbc_batch_link_query_kernel_name(b).decode(), finite=bool(all(np.isfinite(a).all() for _, a in outs)))
    L.dwbc_batch_destroy(b)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libdwbc_hip.so built from the parent commit")
    ap.add_argument("--lib", default=os.path.join(ROOT, "libdwbc_amd", "libdwbc_hip.so"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, metavar=("LIB", "WHAT", "B"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], int(args.child[2]), args.steps)
        return
    env = dict(os.environ, DWBC_NO_TORCH="1")
    routes = (("query", args.lib, "link query, Q7"), ("query_jac", args.lib, "link query, Q7 with Jacobians"), ("cycle_lean", args.parent_lib, "(a) parent lean cycle"),
              ("cycle_dump", args.parent_lib, "(b) parent cycle + dump"))
    lines = ["Link query against the parent commit's routes to link poses and velocities (tools/link_query_rate.py): states of BASELINE configs[1] with joint",
             f"rates, one MI355X, the routes alternating, three runs each of {args.steps} launches after a warm one, every run in its own process; ms per launch",
             f"(device: HIP events; with get: host clock around launch + read-back, mean of {N_GET}).", ""]
    verdict = []
    for B in (1024, 8192):
        runs = {w: [] for w, _, _ in routes}
        info = {}
        for _ in range(3):
            for what, lib, _ in routes:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-lib", args.parent_lib, "--steps", str(args.steps), "--child", lib, what, str(B)],
                                     capture_output=True, text=True, timeout=300, env=env)
                if out.returncode != 0:  # nothing more is started on the device after a failed run
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(f"{what} at B = {B} ended with status {out.returncode}")
                r = json.loads(out.stdout.strip().splitlines()[-1])
                runs[what].append(r)
                info[what] = r
        med = {w: statistics.median(r["ms"] for r in v) for w, v in runs.items()}
        for what, _, label in routes:
            r = info[what]
            got = f"   with get {statistics.median(x['ms_get'] for x in runs[what]):8.4f} ms ({r['get_bytes'] / 1e6:.1f} MB)" if "ms_get" in r else "   with get        -"
            state = f"status ok {r['status_ok']:.3f}" if "status_ok" in r else f"finite {r['finite']}"
            each = " ".join(f"{x['ms']:7.4f}" for x in runs[what])
            lines.append(f"B = {B:5d}  {label:32s} device {each}   median {med[what]:7.4f} ms{got}   {state}   {r['kernel']}")
        lean = [r["ms"] for r in runs["cycle_lean"]]
        spread = max(lean) - min(lean)
        worst = max(med["query"], med["query_jac"])
        below = worst + spread < med["cycle_lean"]
        verdict.append(f"B = {B}: link query {med['query']:.4f} / {med['query_jac']:.4f} ms (without / with Jacobians) against the parent lean cycle's {med['cycle_lean']:.4f} ms "
                       f"(spread of its three runs {spread:.4f} ms): {'below' if below else 'NOT below'}, {worst / med['cycle_lean']:.3f} of it; "
                       f"{med['query'] / med['cycle_dump']:.4f} / {med['query_jac'] / med['cycle_dump']:.4f} of route (b)'s device time")
        lines.append("")
    lines += verdict
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
