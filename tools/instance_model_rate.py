#!/usr/bin/env python3
"""Cost of the per-instance model record (dwbc_batch_set_instance_model) on the full-model cycle, against the library of the parent commit.

    python tools/instance_model_rate.py --parent-tree DIR [--runs 3] [--steps 200] [--out FILE]

DIR is a checkout of the parent commit with its library built (libdwbc_amd/libdwbc_hip.so): the yardstick is that library on the same
states, not this build's own path without a record.  States: the bench's (synth_batch seed 20251226 + 2, double support; pelvis 6D +
upper-body rotation, torque limit 300) at B = 1024 and B = 8192.  The record: every link's mass and inertia times U(0.8, 1.2), COM +
U(-0.01, 0.01) m, joint offsets times U(0.97, 1.03), from default_rng(31).  Each figure is dwbc_batch_time_solves (HIP events around `steps`
back-to-back launches on the batch's stream, after a warm launch), one process per figure; (a) this build with a record and (b) the parent's
library alternate, `--runs` times each, and the medians are reported with their spread (max - min of the runs)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 8192)


def child(tree, B, steps, record):
    """one figure: ms per solve, from the package of `tree`"""
    sys.path.insert(0, tree)
    import numpy as np

    import libdwbc_amd as D
    from libdwbc_amd import workloads as W

    assert os.path.dirname(os.path.dirname(os.path.abspath(D.__file__))) == os.path.abspath(tree), D.__file__
    model = D.Model.from_urdf(W.TOCABI_URDF)
    q, flags, fstar = W.synth_batch(B, seed=20251226 + 2, contact_mode="LR")
    wbc = D.Batch(model, B, device=0)
    for c in W.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(W.TASKS_2LEVEL):
        for m_, link, pt in links:
            wbc.add_task(lv, m_, link, pt)
    wbc.set_torque_limit(np.array(W.TAU_LIM))
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    if record:
        rng = np.random.default_rng(31)
        a = model.arrays()
        nb = model.nb
        f = rng.uniform(0.8, 1.2, (B, nb))
        p_T = np.broadcast_to(a["p_T"], (B, nb, 3)).copy()
        p_T[:, 1:] *= rng.uniform(0.97, 1.03, (B, nb - 1, 1))
        wbc.set_instance_model(model.instance_model(B, mass=a["mass"] * f, inertia=a["inertia"] * f[:, :, None, None],
                                                    com=a["com"] + rng.uniform(-0.01, 0.01, (B, nb, 3)), p_T=p_T))
    wbc.time_solves(steps)  # ramp
    ms = wbc.time_solves(steps) / steps
    print(json.dumps(dict(ms=ms, kernel=wbc.kernel_name(), ok=float((wbc.get("status") == 1).mean()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, metavar=("TREE", "B", "RECORD"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.steps, args.child[2] == "1")
    if not args.parent_tree:
        ap.error("--parent-tree DIR: a checkout of the parent commit with its library built")

    def figure(tree, B, record):
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--child", os.path.abspath(tree), str(B), "1" if record else "0"],
                                      text=True, timeout=600)
        return json.loads(out.strip().splitlines()[-1])

    lines = []
    for B in SIZES:
        runs = {"a": [], "b": []}
        for _ in range(args.runs):
            runs["a"].append(figure(ROOT, B, True))
            runs["b"].append(figure(args.parent_tree, B, False))
        med = {k: statistics.median(r["ms"] for r in v) for k, v in runs.items()}
        spread = {k: max(r["ms"] for r in v) - min(r["ms"] for r in v) for k, v in runs.items()}
        for k, what in (("a", "(a) this build, with a record "), ("b", "(b) parent's library, no record")):
            lines.append(f"B = {B:5d} {what}: median {med[k]:.4f} ms per solve, spread {spread[k]:.4f} ms, runs " + " ".join(f"{r['ms']:.4f}" for r in runs[k]) +
                         f", status 1 on {100 * runs[k][0]['ok']:.1f} %, {runs[k][0]['kernel']}")
        d = med["a"] - med["b"]
        lines.append(f"B = {B:5d} (a) - (b) = {d:+.4f} ms ({100 * d / med['b']:+.1f} %); (b)'s spread {spread['b']:.4f} ms: " +
                     ("within it" if d <= spread["b"] else f"exceeds it by {d - spread['b']:.4f} ms"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
