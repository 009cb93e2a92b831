"""gpu: the dynamics half of UpdateKinematics as a lean launch (dwbc_batch_update_dynamics -> dwbc_dynamics_kernel,
libdwbc_amd/csrc/dwbc_dynamics.h): rd_.A_, A_inv_, B_, G_, CMM_ and com_pos against the numpy restatement and the reference's goldens,
bound to torch tensors, beside the cycle and its dump record, its refusals, and on the kernel packs.

Inputs, references, premises and bars: tests/dynamics_cases.py.  On the parent of the change that added the launch every test here fails
for lack of the entry points.  One refusal of the C-ABI cannot be reached on a device: a model without the kernel -- every pack the loader
accepts carries the row -- so its message is pinned by tests/test_dynamics_plan.py alone."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import dynamics_cases as dc
from tests import redist_pack_cases as pc

pytestmark = pytest.mark.gpu

B = 8
KERNEL = "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoTocabi>"
KERNEL_ANY = "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoGeneric>"
ALL = list(dc.NAMES)


def _bare(n, dtype="f64"):
    """no contact, no task"""
    import libdwbc_amd as D

    return D.Batch(D.Model.from_urdf(cases.URDF), n, device=0, dtype=dtype)


def _full(n):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), n, device=0)
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    wbc.add_task(0, D.TASK_LINK_6D, 0)
    wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _check_tocabi(wbc, what):
    s = dc.tocabi_set(B)
    dc.check_residual_premise(s["ref"], ("tocabi", B))
    wbc.set_dynamics_outputs(ALL)
    wbc.set_state(s["q"], s["qd"])
    wbc.update_dynamics()
    got = wbc.dynamics()
    assert sorted(got) == sorted(ALL + ["status"]) and (got["status"] == 1).all()
    dc.compare(got, s["ref"], ("tocabi", B), what)
    # the goldens at the CASE 1 state, in instance 0 of the same batch; the other instances keep their states
    g = dc.golden_set()
    q = np.array(s["q"])
    q[0] = g["q"][0]
    wbc.set_state(q, s["qd"])
    wbc.update_dynamics()
    again = wbc.dynamics()
    e_a, e_i = float(np.abs(again["A"][0] - g["A"][0]).max()), float(np.abs(again["A_inv"][0] - g["A_inv"][0]).max())
    print(f"{what}: CASE 1 |A - Acontact_mat| = {e_a:.2e}, |A_inv - A_inv_| = {e_i:.2e}")
    assert e_a <= dc.BARS["A"] and e_i <= dc.BARS["A_inv"]
    for k in ALL:
        assert (again[k][1:] == got[k][1:]).all(), k


def test_tocabi_matches_restatement_and_goldens():
    wbc = _bare(B)
    assert wbc.dynamics_kernel_name() == KERNEL
    _check_tocabi(wbc, "TOCABI tree")
    wbc.close()


def test_builtin_generic_row(monkeypatch):
    """a TOCABI batch created under DWBC_DENSE_SWEEP (any 34-body tree) takes the built-in TopoGeneric row"""
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    wbc = _bare(B)
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    assert wbc.dynamics_kernel_name() == KERNEL_ANY
    _check_tocabi(wbc, "TOCABI generic")
    wbc.close()


def test_without_qdot_and_single_outputs():
    """a state without a qdot: B_ is G_ to the bit; one output alone equals the same output of the all-outputs run"""
    s = dc.tocabi_set(B)
    nov = _bare(B)
    nov.set_dynamics_outputs(["B", "G"])
    nov.set_state(s["q"])
    nov.update_dynamics()
    got = nov.dynamics()
    assert sorted(got) == ["B", "G", "status"] and (got["B"] == got["G"]).all()
    assert np.abs(got["G"] - s["ref"]["G"]).max() <= dc.BARS["G"]
    nov.close()
    wbc = _bare(B)
    wbc.set_state(s["q"], s["qd"])
    wbc.set_dynamics_outputs(ALL)
    wbc.update_dynamics()
    full = wbc.dynamics()
    for name in ("G", "A_inv", "B", "CMM"):
        wbc.set_dynamics_outputs([name])
        wbc.update_dynamics()
        one = wbc.dynamics()
        assert sorted(one) == sorted([name, "status"]) and (one[name] == full[name]).all(), name
    wbc.close()


def test_bound_tensors_match_the_host_path():
    import torch

    s = dc.tocabi_set(B)
    host = _bare(B)
    host.set_dynamics_outputs(["A_inv", "B", "G"])
    host.set_state(s["q"], s["qd"])
    host.update_dynamics()
    want = host.dynamics()
    dev = _bare(B)
    st = torch.cuda.Stream()
    dev.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        t = dict(A_inv=torch.full((B, 39, 39), float("nan"), dtype=torch.float64, device="cuda:0"),
                 B=torch.full((B, 39), float("nan"), dtype=torch.float64, device="cuda:0"))
        dev.set_dynamics_outputs(["A_inv", "B", "G"])
        for k, v in t.items():
            dev.bind_dynamics(k, v)
        dev.set_state(s["q"], s["qd"])
        dev.update_dynamics()
        st.synchronize()
        got = dev.dynamics()  # reads the bound buffers back through get
        for k, v in t.items():
            assert (v.cpu().numpy() == want[k]).all() and (got[k] == want[k]).all(), k
        assert (got["G"] == want["G"]).all()
        dev.bind_dynamics("B", None)  # back to the batch's own buffer
        t["B"].fill_(-1.0)
        dev.update_dynamics()
        assert (dev.dynamics()["B"] == want["B"]).all() and (t["B"].cpu().numpy() == -1.0).all()
    host.close()
    dev.close()


def _posed_full(n, q, qd, flags, fstar):
    wbc = _full(n)
    wbc.set_state(q, qd)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    return wbc


def test_solve_is_untouched_by_the_launch():
    """solve() -> update_dynamics() -> solve() gives bit-equal tau, wrench, status (and diag); a warm solve() behind the launch is the
    one of a twin batch that never ran it; the launch gives the same bits on a batch with nothing registered"""
    n = 16
    q, flags, fstar = cases.synth_batch(n, seed=dc.SEED, yaw=True, contact_mode="mixed")
    qd = dc.velocities(n, 39)
    wbc, twin = _posed_full(n, q, qd, flags, fstar), _posed_full(n, q, qd, flags, fstar)
    wbc.solve()
    first = {k: wbc.get(k) for k in ("tau", "wrench", "status", "diag")}
    assert first["status"].sum() >= 0.9 * n
    wbc.set_dynamics_outputs(ALL)
    wbc.update_dynamics()
    d1 = wbc.dynamics()
    for k, v in first.items():
        assert (wbc.get(k) == v).all(), k  # nothing of the cycle was written
    wbc.solve()
    for k, v in first.items():
        assert (wbc.get(k) == v).all(), k
    # the cycle's warm-start state: the same sequence of solves on the twin, without the launch in between
    twin.solve()
    twin.solve()
    for _ in range(2):
        wbc.update_dynamics()
        wbc.solve(init=False)
        twin.solve(init=False)
        for k in first:
            assert (wbc.get(k) == twin.get(k)).all(), k
    d2 = wbc.dynamics()
    for k in ALL:
        assert (d1[k] == d2[k]).all(), k
    # and the launch does not depend on what the batch is set up for: a bare batch gives the same bits
    bare = _bare(n)
    bare.set_max_active_contacts(3)
    bare.set_dynamics_outputs(ALL)
    bare.set_state(q, qd)
    bare.update_dynamics()
    d3 = bare.dynamics()
    for k in ALL:
        assert (d1[k] == d3[k]).all(), k
    bare.close()
    twin.close()
    wbc.close()


def test_agrees_with_the_dump_record():
    n = B
    s = dc.tocabi_set(n)
    _, flags, fstar = cases.synth_batch(n, seed=dc.SEED, yaw=True)
    wbc = _full(n)
    wbc.enable_dump(True)
    wbc.set_state(s["q"], s["qd"])
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    wbc.solve()
    dump = {k: wbc.get(k) for k in ALL}
    wbc.set_dynamics_outputs(ALL)
    wbc.update_dynamics()
    got = wbc.dynamics()
    for k in ALL:
        assert (wbc.get(k) == dump[k]).all(), k  # the dump record stays as the solve left it
    errs = {k: float(np.abs(got[k] - dump[k]).max()) for k in ALL}
    print("launch against the dump record: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in ALL:
        assert errs[k] <= dc.BARS[k], (k, errs[k])
    wbc.close()


def test_refusals():
    import libdwbc_amd as D
    from libdwbc_amd import _lib

    s = dc.tocabi_set(B)
    w = _bare(B)
    w.set_state(s["q"], s["qd"])
    with pytest.raises(D.DwbcError, match="no dynamics request"):
        w.update_dynamics()
    w.set_dynamics_outputs(["A", "G"])
    with pytest.raises(D.DwbcError, match="no dynamics output yet"):
        w.dynamics()
    w.update_dynamics()
    before = w.dynamics()
    assert sorted(before) == ["A", "G", "status"]
    nbytes = [w._L.dwbc_batch_dynamics_bytes(w._h, i) for i in range(8)]
    assert nbytes == [B * 39 * 39 * 8, 0, 0, B * 39 * 8, 0, 0, B * 4, 0]
    # an unknown bit: the request and its outputs stay as they were
    assert w._L.dwbc_batch_set_dynamics_outputs(w._h, (1 << 7) | 1) == 0
    assert _lib.last_error().startswith("dynamics: unknown output bit")
    assert [w._L.dwbc_batch_dynamics_bytes(w._h, i) for i in range(8)] == nbytes
    after = w.dynamics()
    assert all((after[k] == before[k]).all() for k in before)
    # get / bind of an output that was not asked for
    out = np.zeros((B, 39, 39))
    assert w._L.dwbc_batch_get_dynamics(w._h, D.batch.DYNAMICS_OUTPUTS["A_inv"], out.ctypes.data, C.c_size_t(out.nbytes)) == 0
    assert _lib.last_error() == "dynamics: this output was not asked for (dwbc_batch_set_dynamics_outputs)"
    assert w._L.dwbc_batch_bind_dynamics(w._h, D.batch.DYNAMICS_OUTPUTS["B"], None) == 0
    assert _lib.last_error() == "dynamics: this output was not asked for (dwbc_batch_set_dynamics_outputs)"
    assert w._L.dwbc_batch_get_dynamics(w._h, 9, out.ctypes.data, C.c_size_t(out.nbytes)) == 0
    assert _lib.last_error() == "dynamics: unknown output"
    small = np.zeros(4)
    assert w._L.dwbc_batch_get_dynamics(w._h, 0, small.ctypes.data, C.c_size_t(small.nbytes)) == 0
    assert _lib.last_error() == "output buffer too small"
    w.update_dynamics()
    after = w.dynamics()
    assert sorted(after) == ["A", "G", "status"] and all((after[k] == before[k]).all() for k in before)
    w.set_dynamics_outputs([])  # dropped, with its buffers
    assert [w._L.dwbc_batch_dynamics_bytes(w._h, i) for i in range(8)] == [0] * 8
    with pytest.raises(D.DwbcError, match="no dynamics request"):
        w.update_dynamics()
    with pytest.raises(D.DwbcError, match="no dynamics request"):
        w.dynamics()
    w.close()

    f = _bare(B, dtype="f32")
    with pytest.raises(D.DwbcError, match="dynamics: fp64 batches only"):
        f.set_dynamics_outputs(["A"])
    with pytest.raises(D.DwbcError, match="dynamics: fp64 batches only"):
        f.dynamics_kernel_name()
    with pytest.raises(D.DwbcError, match="no dynamics request"):
        f.update_dynamics()  # the refused call left no request behind
    f.close()


def _pack_model(name, tmp_path):
    import libdwbc_amd as D
    from tests.test_model_packs import VARIANTS, model_43

    if name == "surgery_43":
        return model_43()[0]
    return D.Model.from_urdf(cases.variant_urdf(tmp_path / f"{name}.urdf", VARIANTS[name][0]))


@pytest.mark.parametrize("name", ["fixed_head", "fixed_arms", "surgery_43", "fixed_head_own_tree"])
def test_packs_match_restatement(tmp_path, name):
    import libdwbc_amd as D

    own = name.endswith("_own_tree")
    name = name.replace("_own_tree", "")
    md = _pack_model(name, tmp_path)
    assert (md.ndof, md.nb) == pc.SIZES[name]
    cases.ensure_pack(md)
    if own:
        cases.ensure_pack(md, tree=True)
    s = dc.pack_set(name, B)
    dc.check_residual_premise(s["ref"], (name, B))
    wbc = D.Batch(md, B, device=0)
    kn = wbc.dynamics_kernel_name()
    assert f"dwbc_dynamics_kernel<{md.ndof}, {md.nb}," in kn
    if own:
        assert "TopoPack" in kn, kn
    elif name != "fixed_head":  # (no pack of their own tree is ever built for these two)
        assert "TopoGeneric" in kn, kn
    wbc.set_dynamics_outputs(ALL)
    wbc.set_state(s["q"], s["qd"])
    wbc.update_dynamics()
    got = wbc.dynamics()
    assert (got["status"] == 1).all()
    dc.compare(got, s["ref"], (name, B), "own tree" if own else "")
    wbc.close()
