"""Launch rate of the general-contact kernel on three shapes (B = 1024 with three and with two active contacts, B = 8192 with three):
pelvis 6D + upper-body rotation.  python tools/gc_rate.py [--com]
--com: the same three shapes once more with the synthetic COM link on level 0 in place of the pelvis (another level 0 is another QP:
the median QP iteration counts of the diagnostics are printed next to both)."""
import os, sys, numpy as np
sys.path.insert(0, os.getcwd())
import libdwbc_amd as D
from tests import cases
com = "--com" in sys.argv[1:]
model = D.Model.from_urdf(cases.URDF)
for level0 in ([0, model.link_id("COM")] if com else [0]):
    for B, flags in ((1024, [1, 1, 1, 0]), (1024, [1, 1, 0, 0]), (8192, [1, 1, 1, 0])):
        wbc = D.Batch(model, B, device=0)
        for c in cases.CONTACTS_4:
            wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
        wbc.add_task(0, D.TASK_LINK_6D, level0)
        wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
        wbc.set_torque_limit(np.array(cases.TAU_LIM))
        wbc.set_max_active_contacts(3)
        q, _, fs = cases.synth_batch(B, seed=5, yaw=True)
        wbc.set_state(q); wbc.set_contact(np.tile(np.array(flags, np.uint8), (B, 1))); wbc.set_fstar_all(fs)
        wbc.solve(); wbc.sync()
        ms = wbc.time_solves(20) / 20
        it = np.median(wbc.get("diag")[:, 4:9], axis=0).astype(int).tolist() if com else None  # DG_QP_ITER (dwbc_types.h)
        print(f"general-contact kernel, B = {B}, flags {flags}{', COM on level 0' if level0 else ''} ({wbc.kernel_name()}): {ms:8.3f} ms per launch -> {B / ms * 1e3 / 1e6:6.3f} M cycles/s, status ok {wbc.get('status').mean():.3f}"
              + (f", median QP iterations (levels 0..3, redistribution) {it}" if com else ""), flush=True)
