#!/usr/bin/env python3
"""Time per launch of the redistribution kernel for a caller-supplied torque against the PARENT commit's full cycle on the same states.

    python tools/redistribute_rate.py --parent-lib /path/to/parent/libdwbc_amd/libdwbc_hip.so [--steps 50] [--out profiles/redistribute_rate.txt]

States: BASELINE configs[1] (synth_batch seed 20251226 + 2, double support, pelvis 6D + upper-body rotation, torque limit 300) at
B = 1024 and B = 8192.  This build's dwbc_batch_time_redistribute and the parent library's dwbc_batch_time_solves run alternately,
three times each, every run in a process of its own (two builds of one library do not share a process), each after a warm launch;
medians are reported, as profiles/gc_com_gc_rate.txt does.  The torque handed to the redistribution is the cycle's own total torque
(nothing to redistribute: the QP accepts c = 0), that torque pushed along the contact null space by NwJw d, d = 10 N(0, I6) (the input
of the parity tests: every QP works and ends feasible) and that torque with 10 Nm of seeded noise on every joint (every QP works, about
half of them end infeasible: status 0); the requirement -- below the parent cycle at both sizes -- is judged on the slowest of the three."""
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
F_TAU_TOTAL, F_STATUS, F_REDIST_CF, F_REDIST_STATUS, F_NWJW = 23, 12, 15, 17, 37


def child(lib_path, what, B, steps):
    """one measurement through the C-ABI of the library at lib_path (the parent's has no redistribution entry points)"""
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
    ok(L.dwbc_batch_set_state(b, vp(q.ctypes.data), None, None))
    ok(L.dwbc_batch_set_contact(b, vp(flags.ctypes.data)))
    f0, f1 = dbl(fstar[:, :6]), dbl(fstar[:, 6:9])
    ok(L.dwbc_batch_set_fstar(b, 0, vp(f0.ctypes.data)))
    ok(L.dwbc_batch_set_fstar(b, 1, vp(f1.ctypes.data)))
    ms = C.c_float(0)
    res = dict(what=what, B=B)
    L.dwbc_batch_kernel_name.restype = C.c_char_p
    if what == "cycle":
        ok(L.dwbc_batch_solve(b, HQP_INIT))
        ok(L.dwbc_batch_sync(b))
        ok(L.dwbc_batch_time_solves(b, HQP_INIT, steps, C.byref(ms)))
        st = np.zeros(B, np.int32)
        ok(L.dwbc_batch_get(b, F_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        res.update(ms=ms.value / steps, kernel=L.dwbc_batch_kernel_name(b).decode(), status_ok=float(st.mean()))
    else:
        ok(L.dwbc_batch_enable_dump(b, 1 if what == "redistribute_null" else 0))
        ok(L.dwbc_batch_solve(b, HQP_INIT))
        tau = np.zeros((B, 33))
        ok(L.dwbc_batch_get(b, F_TAU_TOTAL, vp(tau.ctypes.data), C.c_size_t(tau.nbytes)))
        if what == "redistribute_noise":
            tau = tau + 10.0 * np.random.default_rng(11).standard_normal(tau.shape)
        if what == "redistribute_null":
            nwjw = np.zeros((B, 33, 6))
            ok(L.dwbc_batch_get(b, F_NWJW, vp(nwjw.ctypes.data), C.c_size_t(nwjw.nbytes)))
            ok(L.dwbc_batch_enable_dump(b, 0))
            tau = tau + np.einsum("bij,bj->bi", nwjw, 10.0 * np.random.default_rng(11).standard_normal((B, 6)))
        ok(L.dwbc_batch_set_torque_input(b, vp(tau.ctypes.data)))
        ok(L.dwbc_batch_redistribute(b, HQP_INIT))
        ok(L.dwbc_batch_sync(b))
        ok(L.dwbc_batch_time_redistribute(b, HQP_INIT, steps, C.byref(ms)))
        st, cf = np.zeros(B, np.int32), np.zeros((B, 6))
        ok(L.dwbc_batch_get(b, F_REDIST_STATUS, vp(st.ctypes.data), C.c_size_t(st.nbytes)))
        ok(L.dwbc_batch_get(b, F_REDIST_CF, vp(cf.ctypes.data), C.c_size_t(cf.nbytes)))
        L.dwbc_batch_redistribute_kernel_name.restype = C.c_char_p
        res.update(ms=ms.value / steps, kernel=L.dwbc_batch_redistribute_kernel_name(b).decode(), status_ok=float(st.mean()),
                   qp_busy=float((np.linalg.norm(cf, axis=1) > 1e-3).mean()))
    L.dwbc_batch_destroy(b)
    print(json.dumps(res), flush=True)


PACK_MODELS = ("fixed_head", "fixed_arms", "surgery_43")  # tests/redist_pack_cases.py: 37 / 32, 23 / 18 and 43 / 38


def pack_model(name, steps, out):
    """A model that runs through a kernel pack: before the packs carried a redistribution kernel such a model's redistribution was refused,
    so there is no earlier time; the yardstick is the same model's lean full cycle (solve(), dump off) in the same process at the same B --
    the only launch a caller had, and the redistribution is a strict subset of its work.  Cycle and redistribution alternate, five windows
    of `steps` launches each after a warm launch of both; medians.  Torque input: the cycle's own total torque pushed along the contact
    null space by NwJw d, d = 10 N(0, I6) (every QP at work)."""
    import tempfile

    import numpy as np

    import libdwbc_amd as D
    from tests import cases
    from tests.test_model_packs import VARIANTS, model_43, states_43, variant_states

    from oracle import urdf_model

    with tempfile.TemporaryDirectory() as tmp:
        if name == "surgery_43":
            md, _ = model_43()
            links = [6, 12, 15]
            states = lambda B: states_43(B, 7)
        else:
            path = cases.variant_urdf(os.path.join(tmp, name + ".urdf"), VARIANTS[name][0])
            md, mo = D.Model.from_urdf(path), urdf_model.load_urdf(path)
            links = [md.link_id(n) for n in ("L_AnkleRoll_Link", "R_AnkleRoll_Link", "Upperbody_Link")]
            states = lambda B: variant_states(mo, B, seed=7)
    cases.ensure_pack(md)
    lines = [f"Redistribution of a caller-supplied torque against the lean full cycle of the same model ({name}: {md.ndof} dof / {md.nb} bodies;",
             f"tools/redistribute_rate.py --model {name}): one MI355X, one process, cycle and redistribution alternating, five windows of {steps} launches each",
             "after a warm launch of both; ms per launch.", ""]
    for B in (1024, 8192):
        wbc = D.Batch(md, B, device=0)
        for cc, l in zip(cases.CONTACTS_2, links[:2]):
            wbc.add_contact(l, cc["point"], cc["lx"], cc["ly"], cc["mu"], cc["muz"])
        wbc.add_task(0, D.TASK_LINK_6D, 0)
        wbc.add_task(1, D.TASK_LINK_ROTATION, links[2])
        wbc.set_torque_limit(np.full(md.ndof - 6, 300.0))
        q, fs = states(B)
        wbc.set_state(q); wbc.set_contact(np.ones((B, 2), np.uint8)); wbc.set_fstar_all(fs)
        wbc.enable_dump(True)
        wbc.solve()
        tau = wbc.get("tau").sum(axis=1) + np.einsum("bij,bj->bi", wbc.get("NwJw")[:, : md.ndof - 6, :6], 10.0 * np.random.default_rng(11).standard_normal((B, 6)))
        wbc.enable_dump(False)
        wbc.set_torque_input(tau)
        wbc.solve(); wbc.redistribute(); wbc.sync()  # warm launches of the two kernels that are timed
        runs = {"cycle": [], "redistribute": []}
        for _ in range(5):
            runs["cycle"].append(wbc.time_solves(steps) / steps)
            runs["redistribute"].append(wbc.time_redistributes(steps) / steps)
        st_c, st_r, cf = wbc.get("status"), wbc.get("redist_status"), wbc.get("redist_cf")
        med = {k: statistics.median(v) for k, v in runs.items()}
        for what, kernel, okf in (("cycle", wbc.kernel_name(), float(st_c.mean())), ("redistribute", wbc.redistribute_kernel_name(), float(st_r.mean()))):
            extra = f", QP at work on {float((np.linalg.norm(cf, axis=1) > 1e-3).mean()):.3f}" if what == "redistribute" else ""
            lines.append(f"B = {B:5d}  {what:13s} {' '.join(f'{x:7.4f}' for x in runs[what])}   median {med[what]:7.4f} ms -> {B / med[what] / 1e3:7.3f} M instances/s"
                         f"   status ok {okf:.3f}{extra}   {kernel}")
        r = med["redistribute"] / med["cycle"]
        lines.append(f"B = {B}: redistribution {med['redistribute']:.4f} ms against the lean cycle's {med['cycle']:.4f} ms ({r:.3f} of it): {'not slower' if r <= 1.0 else 'SLOWER'}")
        lines.append("")
        wbc.close()
    text = "\n".join(lines)
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=PACK_MODELS, help="a kernel-pack model instead of TOCABI: against its own lean full cycle (no parent library needed)")
    ap.add_argument("--parent-lib", help="libdwbc_hip.so built from the parent commit (TOCABI)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "libdwbc_amd", "libdwbc_hip.so"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, metavar=("LIB", "WHAT", "B"))
    args = ap.parse_args()
    if args.model:
        pack_model(args.model, args.steps, args.out)
        return
    if not args.parent_lib:
        ap.error("--parent-lib is required without --model")
    if args.child:
        child(args.child[0], args.child[1], int(args.child[2]), args.steps)
        return
    lines = ["Redistribution of a caller-supplied torque against the parent commit's full cycle (tools/redistribute_rate.py): states of BASELINE",
             f"configs[1], one MI355X, the builds alternating, three runs each of {args.steps} launches after a warm one, every run in its own process; ms per launch.",
             ""]
    verdict = []
    for B in (1024, 8192):
        runs = {"redistribute_own": [], "redistribute_null": [], "redistribute_noise": [], "cycle": []}
        info = {}
        for _ in range(3):
            for what, lib in (("redistribute_own", args.lib), ("redistribute_null", args.lib), ("redistribute_noise", args.lib), ("cycle", args.parent_lib)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-lib", args.parent_lib, "--steps", str(args.steps), "--child", lib, what, str(B)],
                                     capture_output=True, text=True, timeout=300)
                if out.returncode != 0:  # nothing more is started on the device after a failed run
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(f"{what} at B = {B} ended with status {out.returncode}")
                r = json.loads(out.stdout.strip().splitlines()[-1])
                runs[what].append(r["ms"])
                info[what] = r
        med = {k: statistics.median(v) for k, v in runs.items()}
        for what, label in (("cycle", "parent cycle"), ("redistribute_own", "redistribution, the cycle's own torque"), ("redistribute_null", "redistribution, + NwJw d"),
                            ("redistribute_noise", "redistribution, + 10 Nm noise")):
            r = info[what]
            extra = f", QP at work on {r['qp_busy']:.3f}" if "qp_busy" in r else ""
            lines.append(f"B = {B:5d}  {label:40s} {' '.join(f'{x:7.4f}' for x in runs[what])}   median {med[what]:7.4f} ms -> {B / med[what] / 1e3:7.3f} M instances/s"
                         f"   status ok {r['status_ok']:.3f}{extra}   {r['kernel']}")
        worst = max(med["redistribute_own"], med["redistribute_null"], med["redistribute_noise"])
        verdict.append(f"B = {B}: redistribution {worst:.4f} ms against the parent cycle's {med['cycle']:.4f} ms ({worst / med['cycle']:.3f} of it): {'below' if worst < med['cycle'] else 'NOT below'}")
        lines.append("")
    lines += verdict
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
