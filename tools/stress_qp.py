"""Sweep of the wave QP solver on its own (tests/qp_probe) against oracle/dwbc_oracle.c: the dense and the product-shaped family of
tests/qp_cases.py at many seeds, through either build of the probe.  Development only; the suite runs the same families at one seed.
python tools/stress_qp.py [--build emu|gpu] [--n 100000] [--threads 64|128] [--inst NAME]
Prints, per instantiation and family: problems, status / step-count / working-set disagreements with the oracle (first five: seed, index,
both outputs) and the worst |x - x_oracle|inf / max(1, |x_oracle|inf) (the oracle's own error is part of that figure)."""
import argparse, sys, numpy as np
import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import qp_cases as qc, qp_reference as ref
from tests.qp_probe import probe
ap = argparse.ArgumentParser()
ap.add_argument("--build", default="emu", choices=("emu", "gpu"))
ap.add_argument("--n", type=int, default=100000, help="problems per family, over all instantiations")
ap.add_argument("--threads", type=int, default=64)
ap.add_argument("--inst", default=None)
a = ap.parse_args()
insts = [i for i in probe.INSTANTIATIONS if a.inst in (None, i.name)]
per = max(1, a.n // len(insts))
for inst in insts:
    for fam, gen, chunk in (("dense", qc.fam_dense, 256), ("product", qc.fam_product, 256)):
        done, bad, worst, n_bad = 0, [], 0.0, 0
        seed = 100000
        while done < per:
            seed += 1000
            ps = gen(inst, min(chunk, per - done) * (2 if inst.nv > 12 else 1), seed)  # (the generators halve their count on the large builds)
            out = probe.solve(a.build, inst, ps, a.threads)
            for b, p in enumerate(ps):
                st, x, act, it = ref.oracle(p)
                mine = (int(out["status"][b]), int(out["iters"][b]), sorted(int(v) for v in out["act"][b] if v >= 0) if inst.ws else act)
                if mine != (st, it, act) and not inst.f32:
                    n_bad += 1
                    if len(bad) < 5:
                        bad.append((seed, b, mine, (st, it, act)))
                if st == 1 and mine[0] == 1:
                    worst = max(worst, qc.relerr(out["x"][b][: p["nv"]], x))
            done += len(ps)
        print(inst.name, fam, "problems", done, "disagreements", n_bad, "worst x vs oracle %.3e" % worst, "first", bad, flush=True)
