#!/usr/bin/env python3
"""Time per launch of the contact-space kernel (SetContact + CalcContactConstraint: J_C, Lambda_contact, J_C_INV_T, N_C, A_inv_N_C, W,
W_inv, NwJw, contact frames) against the PARENT commit's only way to the same matrices, a full solve with the dump record on.

    python tools/contact_space_rate.py --parent-lib /path/to/parent/libdwbc_amd/libdwbc_hip.so [--steps 100] [--out profiles/contact_space_rate.txt]

Routes, every run in a process of its own under a time limit of its own (two builds of one library do not share a process), the routes
alternating, three runs of --steps launches each after a warm one, HIP-event time per launch:
  (a) {J_C, contact frames}            dwbc_batch_time_contact_space: no A^-1 sweep
  (b) {Lambda_c, J_C_INV_T, NwJw}      dwbc_batch_time_contact_space: the sweep and the contact stage; no A^-1 N_c, no W^+ sweep, no N_C
  (c) all outputs                      dwbc_batch_time_contact_space
  (d) the parent's way                 dwbc_batch_time_solves of the parent library with the dump record on: pelvis 6D over upper-body
                                       rotation (the task set of BASELINE configs[1]), torque limit 300
Both feet down on every route.  TOCABI on the states of BASELINE configs[1] (synth_batch seed 20251226 + 2) and the head-fixed 37-dof /
32-body model through the kernel pack of its own tree (tests/test_model_packs.py states, seed 7), B = 1024 and 8192.  Routes (a) to (c)
run on a batch with the two contacts and no task.
Conditions (structural): (c) below (d) by more than the spread of (d)'s three runs; (a) below (b) below (c)."""
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
F_STATUS = 12
CS_STATUS = 10
MASKS = {"a": (1 << 0) | (1 << 8) | (1 << 9), "b": (1 << 1) | (1 << 2) | (1 << 7), "c": 0x3FF}
ROUTES = (("a", "{J_C, frames}", False), ("b", "{Lambda_c, J_C_INV_T, NwJw}", False), ("c", "all outputs", False), ("d", "parent: dump-on solve", True))


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
    n = q.shape[1] - 1
    b = vp(L.dwbc_batch_create(md, B, 0, 0))
    ok(b.value)
    q = dbl(q)
    ok(L.dwbc_batch_set_state(b, vp(q.ctypes.data), None, None))
    ms = C.c_float(0)
    st = np.zeros(B, np.int32)
    for c, l in zip(W.CONTACTS_2, links):
        p = dbl(c["point"])
        assert L.dwbc_batch_add_contact(b, l, 0, vp(p.ctypes.data), C.c_double(c["lx"]), C.c_double(c["ly"]), C.c_double(c["mu"]), C.c_double(c["muz"])) >= 0
    flags = np.ones((B, 2), np.uint8)
    ok(L.dwbc_batch_set_contact(b, vp(flags.ctypes.data)))
    if route == "d":
        z = dbl([0, 0, 0])
        ok(L.dwbc_batch_add_task(b, 0, 0, 0, vp(z.ctypes.data)))         # pelvis 6D
        ok(L.dwbc_batch_add_task(b, 1, 6, links[2], vp(z.ctypes.data)))  # upper-body rotation
        lim = dbl(np.full(n - 6, 300.0))
        ok(L.dwbc_batch_set_torque_limit(b, vp(lim.ctypes.data)))
        f0, f1 = dbl(fstar[:, :6]), dbl(fstar[:, 6:9])
        ok(L.dwbc_batch_set_fstar(b, 0, vp(f0.ctypes.data)))
        ok(L.dwbc_batch_set_fstar(b, 1, vp(f1.ctypes.data)))
        ok(L.dwbc_batch_enable_dump(b, 1))
        ok(L.dwbc_batch_time_solves(b, HQP_INIT, steps, C.byref(ms)))
        ok(L.dwbc_batch_get(b, F_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        L.dwbc_batch_kernel_name.restype = C.c_char_p
        kernel = L.dwbc_batch_kernel_name(b).decode()
    else:
        ok(L.dwbc_batch_set_contact_space_outputs(b, C.c_uint(MASKS[route])))
        ok(L.dwbc_batch_time_contact_space(b, steps, C.byref(ms)))
        ok(L.dwbc_batch_get_contact_space(b, CS_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        L.dwbc_batch_contact_space_kernel_name.restype = C.c_char_p
        kernel = L.dwbc_batch_contact_space_kernel_name(b).decode()
    L.dwbc_batch_destroy(b)
    print(json.dumps(dict(route=route, B=B, ms=ms.value / steps, kernel=kernel, status_ok=float(st.mean()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libdwbc_hip.so built from the parent commit, with its kernel packs beside it")
    ap.add_argument("--lib", default=os.path.join(ROOT, "libdwbc_amd", "libdwbc_hip.so"))
    ap.add_argument("--steps", type=int, default=100)
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

    lines = ["The contact-space launch with {J_C, contact frames} (a), {Lambda_c, J_C_INV_T, NwJw} (b) and all outputs (c) against the parent commit's only way to",
             "these matrices, a solve with the dump record on (d) (tools/contact_space_rate.py): both feet down, one MI355X, every run in a process of its own, routes alternating,",
             f"three runs each of {args.steps} launches after a warm one; HIP-event ms per launch, median, spread = max - min of the three.", ""]
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
                    lines.append(f"{model:10s} B = {B:5d}  ({route}) {label:28s} {' '.join(f'{x:7.4f}' for x in runs[route])}   median {med[route]:7.4f} spread {spread[route]:6.4f} ms"
                                 f"   status ok {r['status_ok']:.3f}   {r['kernel']}")
                    print(lines[-1], flush=True)
                lines.append("")
                verdict.append(f"{model} B = {B}: (c) {med['c']:.4f} against (d) {med['d']:.4f} ms, (d)'s spread {spread['d']:.4f}: {'below' if med['d'] - med['c'] > spread['d'] else 'NOT below'};  "
                               f"(a) {med['a']:.4f} < (b) {med['b']:.4f} < (c) {med['c']:.4f} ms: {'holds' if med['a'] < med['b'] < med['c'] else 'DOES NOT hold'};  (c) / (d) = {med['c'] / med['d']:.3f}")
    lines += verdict
    text = "\n".join(lines) + "\n"
    print("\n".join(verdict))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
