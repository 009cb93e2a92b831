"""Is the path of the QP search the same in two builds of the library?  Records, for the bench's 1024 states and the tilted-feet and
mixed-contact sets of tools/stress_parity.py, what every QP of every instance did -- steps (DG_QP_ITER), size of the final working set
(DG_QP_NACT), on the full build the working set itself (DG_QP_ACT) -- and the outputs, through the two-wave kernel, the compact kernel
and the full one-wave build, and the outputs of the general-contact kernel and the link query on the first 256 states of each set; a
second call compares two records bit for bit.
    python tools/qp_path_record.py record OUT.npz          (DWBC_LIB_VARIANT selects the build, as everywhere)
    python tools/qp_path_record.py compare A.npz B.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = {"bench": dict(seed=20251226 + 2), "tilted": dict(seed=9000, yaw=True), "mixed": dict(seed=9000, contact_mode="mixed")}
BUILDS = {"two_wave": {}, "compact": {"DWBC_NO_WIDE": "1"}, "full": {"DWBC_NO_LEAN": "1"}}


def record(path):
    import libdwbc_amd as D
    from libdwbc_amd import workloads as W

    out = {}
    B = 1024
    for sname, kw in SETS.items():
        q, fl, fs = W.synth_batch(B, **kw)
        for bname, env in BUILDS.items():
            os.environ.update(env)
            try:
                wbc = D.Batch(D.Model.from_urdf(W.URDF), B)
                for c in W.CONTACTS_2:
                    wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
                wbc.add_task(0, D.TASK_LINK_6D, 0)
                wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
                wbc.set_torque_limit(np.array(W.TAU_LIM))
                wbc.set_state(q); wbc.set_contact(fl); wbc.set_fstar_all(fs)
                wbc.solve()
                d = wbc.get("diag")
                name = wbc.kernel_name()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            key = f"{sname}/{bname}"
            print(f"{key:16s} {name[:70]:70s} steps/instance {d[:, 4:9].sum(axis=1).mean():.2f}  ok {int(wbc.get('status').sum())}/{B}", flush=True)
            out[key + "/iter"], out[key + "/nact"] = d[:, 4:9], d[:, 9:14]
            if bname == "full":
                out[key + "/act"] = d[:, 14:74]
            for f in ("tau", "wrench", "status"):
                out[f"{key}/{f}"] = wbc.get(f)
        record_others(D, W, sname, q, fs, out)
    np.savez(path, **out)


def record_others(D, W, sname, q, fs, out, B=256):
    """the kernels beside the cycle builds that share the front end (dwbc_front.h), at B = 256: the general-contact kernel with three flags
    up and the link query (Jacobians, the COM link among the entries)"""
    model = D.Model.from_urdf(W.URDF)
    q, fs = q[:B], fs[:B]
    wbc = D.Batch(model, B)
    for c in W.CONTACTS_4:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    wbc.add_task(0, D.TASK_LINK_6D, 0)
    wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(W.TAU_LIM))
    wbc.set_max_active_contacts(3)
    wbc.set_state(q); wbc.set_contact(np.tile(np.array([1, 1, 1, 0], np.uint8), (B, 1))); wbc.set_fstar_all(fs)
    wbc.solve()
    print(f"{sname + '/general_contact':24s} {wbc.kernel_name()[:70]:70s} ok {int(wbc.get('status').sum())}/{B}", flush=True)
    for f in ("tau", "wrench", "status"):
        out[f"{sname}/general_contact/{f}"] = wbc.get(f)
    wbc = D.Batch(model, B)
    wbc.set_state(q, np.random.default_rng(5).uniform(-1, 1, (B, 39)))
    wbc.set_link_query([0, 6, 12, 15, 23, 33, model.link_id("COM")], None, jacobians=True)
    wbc.update_kinematics()
    print(f"{sname + '/link_query':24s} {wbc.link_query_kernel_name()[:70]}", flush=True)
    for k, v in wbc.link_states().items():
        out[f"{sname}/link_query/{k}"] = v


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files)
    bad = 0
    for k in sorted(a.files):
        same = np.array_equal(a[k], b[k], equal_nan=True)
        extra = ""
        if not same:
            bad += 1
            extra = f"   differs on {int((a[k] != b[k]).reshape(len(a[k]), -1).any(axis=1).sum())} instances"
            if a[k].dtype.kind == "f":
                extra += f", max |difference| {np.nanmax(np.abs(a[k] - b[k])):.3e}"
        print(f"{k:24s} {'identical' if same else 'DIFFERENT'}{extra}")
    print(f"{len(a.files) - bad} of {len(a.files)} arrays bit-identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(record(sys.argv[2]) if sys.argv[1] == "record" else compare(sys.argv[2], sys.argv[3]))
