#!/usr/bin/env python3
"""Cost of the per-instance parameter record (dwbc_batch_set_instance_params) on the full-model cycle: time per launch without and
with a record on the three shapes of the bench table this feature is judged on.

    python tools/instance_params_rate.py [--runs 3] [--out FILE]

States: the bench's (synth_batch seed 20251226 + 2; pelvis 6D + upper-body rotation, torque limit 300): B = 1024 and B = 8192 in double
support, B = 8192 with mixed support.  The record holds TAU_LIM * U(0.15, 0.5) and the contact constants times U(0.4, 1.0), as the tests
do.  Each figure is dwbc_batch_time_solves (HIP events around back-to-back launches on the batch's stream, after a warm launch); the
two variants alternate, `--runs` times each, and the median is reported with the spread."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("ds2_1024", 1024, "LR", 1000), ("ds2_8192", 8192, "LR", 200), ("mixed_8192", 8192, "mixed", 200))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import libdwbc_amd as D
    from libdwbc_amd import workloads as W

    lines = []
    model = D.Model.from_urdf(W.TOCABI_URDF)
    for name, B, mode, steps in SHAPES:
        q, flags, fstar = W.synth_batch(B, seed=20251226 + 2, contact_mode=mode)
        lim = np.array(W.TAU_LIM) * np.random.default_rng(29).uniform(0.15, 0.5, size=(B, 33))
        base = np.array([[c["lx"], c["ly"], c["mu"], c["muz"]] for c in W.CONTACTS_2])
        con = base * np.random.default_rng(23).uniform(0.4, 1.0, size=(B, 2, 4))
        batches = {}
        for variant in ("none", "record"):
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
            if variant == "record":
                wbc.set_instance_params(lim, con)
            wbc.time_solves(steps)  # ramp
            batches[variant] = wbc
        ms = {v: [] for v in batches}
        for _ in range(args.runs):
            for v, wbc in batches.items():
                ms[v].append(wbc.time_solves(steps) / steps)
        ok = {v: float((w.get("status") == 1).mean()) for v, w in batches.items()}
        kern = batches["record"].kernel_name()
        assert kern == batches["none"].kernel_name()
        for v in ("none", "record"):
            med = statistics.median(ms[v])
            lines.append(f"{name:11s} {v:7s} median {1e3 * med:8.2f} us per launch  {B / med / 1e3:8.3f} M cycles/s  runs " +
                         " ".join(f"{1e3 * x:.2f}" for x in ms[v]) + f"  status 1 on {100 * ok[v]:.1f} %")
        r = statistics.median(ms["record"]) / statistics.median(ms["none"])
        lines.append(f"{name:11s} record / none = {r:.4f}   ({kern})")
        for w in batches.values():
            w.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
