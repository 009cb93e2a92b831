"""gpu: CalcContactRedistribute(torque_input) / getContactForce(torque) on models other than TOCABI -- the redistribution kernel of the
kernel packs (libdwbc_amd/csrc/dwbc_pack.hip: generic packs of 37 / 32, 23 / 18 and 43 / 38, the own-tree pack of the head-fixed model) and the
built-in (39, 34, TopoGeneric) row -- against the numpy restatement.

Inputs, flag mix and premises: tests/redist_pack_cases.py; bars: tests/redist_cases.py (1e-6 Nm, 1e-5 N).  On the parent of the change
that added these rows every test here ends in "no redistribution kernel for this model (built in for TOCABI's size and tree; kernel packs
do not carry one)"."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import redist_cases as rc
from tests import redist_pack_cases as pc

pytestmark = pytest.mark.gpu


def _model(name, tmp_path):
    """the library's model of a case of redist_pack_cases"""
    import libdwbc_amd as D
    from tests.test_model_packs import VARIANTS, model_43

    if name == "surgery_43":
        return model_43()[0]
    return D.Model.from_urdf(cases.variant_urdf(tmp_path / f"{name}.urdf", VARIANTS[name][0]))


def _batch(md, links, B, tasks=True, contacts=None):
    import libdwbc_amd as D

    wbc = D.Batch(md, B, device=0)
    for c in contacts or pc.contacts_of(links):
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    if tasks:
        wbc.add_task(0, D.TASK_LINK_6D, 0)
        wbc.add_task(1, D.TASK_LINK_ROTATION, links[2])
    wbc.set_torque_limit(np.full(md.ndof - 6, pc.TAU_LIM))
    return wbc


def _outputs(wbc):
    return dict(tau=wbc.get("redist_tau"), cf=wbc.get("redist_cf"), wrench=wbc.get("redist_wrench"), status=wbc.get("redist_status"))


def _redistribute(wbc, ref, tau_in=None):
    wbc.set_state(ref["q"])
    wbc.set_contact(ref["flags"])
    wbc.set_torque_input(ref["tau_in"] if tau_in is None else tau_in)
    wbc.redistribute()
    return _outputs(wbc)


@pytest.mark.parametrize("name", sorted(pc.SIZES))
def test_gpu_packs_match_restatement(tmp_path, name):
    """the generic pack of 37 / 32 (or its own-tree pack: the loader prefers it), the pack of 23 / 18 (32 bodies fewer than a wave, the
    smallest M) and the pack of 43 / 38 (the TopoDense sweep): against the restatement, a feasible input left alone, and independent of the
    cycle as tests/test_redistribute_gpu.py::test_independent_of_the_cycle has it on TOCABI"""
    n, nb = pc.SIZES[name]
    B = pc.BATCH[name]
    md = _model(name, tmp_path)
    assert (md.ndof, md.nb) == (n, nb)
    cases.ensure_pack(md)
    ref = pc.state_set(name, B)
    rc.check_premises(ref)
    _, links = pc.model(name)
    alone = _batch(md, links, B, tasks=False)  # no task space is needed
    assert f"dwbc_redistribute_kernel<{n}, {nb}," in alone.redistribute_kernel_name()
    got = _redistribute(alone, ref)
    rc.compare(got, ref)
    pc.check_flag_mix_outputs(got, ref)
    assert alone.get("in_torque").shape == (B, n - 6) and (alone.get("in_torque") == ref["tau_in"]).all()

    # a feasible input -- the restatement's own torque -- is left alone
    fea = _redistribute(alone, ref, ref["tau_feasible"])
    assert (fea["status"] == 1).all()
    assert np.abs(fea["tau"]).max() <= 1e-6
    assert (fea["wrench"][:, 0] == fea["wrench"][:, 1]).all()
    double = ref["flags"].sum(axis=1) == 2
    assert np.abs(fea["wrench"][double][:, 0]).max(axis=1).min() > 100.0

    # a full solve() before or after changes neither launch's outputs
    only, after, before = _batch(md, links, B), _batch(md, links, B), _batch(md, links, B)
    for w in (only, after, before):
        w.set_state(ref["q"])
        w.set_contact(ref["flags"])
        w.set_torque_input(ref["tau_in"])
        w.set_fstar_all(ref["fstar"])
    only.solve()
    after.solve()
    after.redistribute()
    before.redistribute()
    before.solve()
    cyc = {k: only.get(k) for k in ("tau", "wrench", "status", "diag")}
    assert cyc["status"].sum() >= 0.9 * double.sum()
    for w in (after, before):
        assert w.kernel_name() == only.kernel_name()
        for k, v in cyc.items():
            assert (w.get(k) == v).all(), k
        for k, v in _outputs(w).items():
            assert (v == got[k]).all(), k
    for w in (alone, only, after, before):
        w.close()


def _renumbered(mo, perm):
    """the same robot with its bodies in the order perm (new index -> old index; still depth first)"""
    inv = {int(o): i for i, o in enumerate(perm)}
    out = {k: np.asarray(mo[k])[perm] for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")}
    out["parent"] = np.array([inv[max(int(mo["parent"][o]), 0)] if i > 0 else int(mo["parent"][0]) for i, o in enumerate(perm)], np.int32)
    out["nb"], out["ndof"] = len(perm), len(perm) + 5
    return out


def test_gpu_own_tree_pack_matches_restatement_and_the_generic_pack(tmp_path):
    """The head-fixed model runs the redistribution of its own-tree pack (TopoPack: the tree-sparse LDS-fed sweep, on a tree other than
    TOCABI's for the first time).  The loader prefers that pack for this parent table whenever it exists, so the generic 37 / 32 pack is
    reached the way tests/test_model_packs.py reaches it -- through another parent table: the SAME robot with the waist / arm subtree
    numbered before the legs, the same 48 states and torques in that joint order."""
    import libdwbc_amd as D

    B = 48
    md = _model("fixed_head", tmp_path)
    cases.ensure_pack(md)
    cases.ensure_pack(md, tree=True)
    ref = pc.state_set("fixed_head", B)
    rc.check_premises(ref)
    mo, links = pc.model("fixed_head")
    own = _batch(md, links, B, tasks=False)
    name = own.redistribute_kernel_name()
    assert "dwbc_redistribute_kernel<37, 32," in name and "TopoPack" in name
    got = _redistribute(own, ref)
    rc.compare(got, ref)
    pc.check_flag_mix_outputs(got, ref)

    names = list(mo["names"])
    waist = names.index("Waist1_Link")
    assert list(mo["parent"][1:waist]).count(0) == 2 and mo["parent"][waist] <= 0  # two legs below the pelvis, then the waist chain
    perm = np.array([0] + list(range(waist, 32)) + list(range(1, waist)))
    other = D.Model.from_arrays(_renumbered(md.arrays(), perm))
    assert (other.ndof, other.nb) == (37, 32) and list(other.arrays()["parent"]) != list(md.arrays()["parent"])
    jp = perm[1:] - 1  # joint order: new joint i is old joint jp[i]
    inv = {int(o): i for i, o in enumerate(perm)}
    q2 = ref["q"].copy()
    q2[:, 6:37] = ref["q"][:, 6 + jp]
    gen = _batch(other, [inv[l] for l in links], B, tasks=False)
    assert "TopoGeneric" in gen.redistribute_kernel_name() and "dwbc_redistribute_kernel<37, 32," in gen.redistribute_kernel_name()
    gen.set_state(q2)
    gen.set_contact(ref["flags"])
    gen.set_torque_input(ref["tau_in"][:, jp])
    gen.redistribute()
    g2 = _outputs(gen)
    tau2 = np.zeros_like(g2["tau"])
    tau2[:, jp] = g2["tau"]
    assert (g2["status"] == got["status"]).all()
    e_tau, e_wr = float(np.abs(tau2 - got["tau"]).max()), float(np.abs(g2["wrench"] - got["wrench"]).max())
    print(f"own-tree pack against the generic pack: worst |d tau| = {e_tau:.3e} Nm, worst |d wrench| = {e_wr:.3e} N")
    assert e_tau <= 1e-9 and e_wr <= 1e-8
    own.close()
    gen.close()


def _tocabi_pair(monkeypatch, B):
    """(TOCABI batch on its constant tree, TOCABI batch created under DWBC_DENSE_SWEEP: any 34-body tree)"""
    import libdwbc_amd as D

    def make():
        wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0)
        for c in cases.CONTACTS_2:
            wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
        wbc.set_torque_limit(np.array(cases.TAU_LIM))
        return wbc

    tree = make()
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    dense = make()
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    return tree, dense


def test_gpu_builtin_generic_row(monkeypatch):
    """a TOCABI batch created under DWBC_DENSE_SWEEP (any 34-body tree: DeleteLink / AddLink results, other robots of the size) takes
    the built-in TopoGeneric row and meets the restatement's bars"""
    B = 250
    ref = rc.state_set(B, True, "mixed")
    rc.check_premises(ref)
    tree, dense = _tocabi_pair(monkeypatch, B)
    assert tree.redistribute_kernel_name() == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"
    assert dense.redistribute_kernel_name() == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoGeneric>"
    rc.compare(_redistribute(dense, ref), ref)
    tree.close()
    dense.close()


def test_gpu_builtin_generic_row_agrees_with_the_tree_kernel(monkeypatch):
    """the TopoGeneric row against the TOCABI-tree kernel on rc.state_set(250, True, "mixed"): 1e-9 Nm.

    The two kernels differ in the A^-1 sweep alone, and three of these 250 instances amplify a rounding of 1e-16 there to 1e-9 Nm and
    more (on instance 111 either kernel is 2.5e-7 Nm from the restatement): with the ascending runtime pivots of the cycle's generic
    kernels (sweep_inverse_rl) the two were 5.4e-9 Nm apart on the device and 2.75e-9 in host emulation.  The generic build of the
    redistribution kernel therefore pivots leaves first through LDS like the constant-tree build (dwbc_cycle2_stage0.inc): entries
    outside the tree's pattern stay exact zeros, and the two sweeps are the same arithmetic."""
    B = 250
    ref = rc.state_set(B, True, "mixed")
    tree, dense = _tocabi_pair(monkeypatch, B)
    got, want = _redistribute(dense, ref), _redistribute(tree, ref)
    assert (got["status"] == want["status"]).all()
    d = np.abs(got["tau"] - want["tau"]).max(axis=1)
    print(f"worst |tau generic - tau tree| = {d.max():.3e} Nm (instance {int(d.argmax())}), median {np.median(d):.3e}, above 1e-9 on {int((d > 1e-9).sum())} of {B}")
    tree.close()
    dense.close()
    assert d.max() <= 1e-9


def test_gpu_instance_params_on_a_pack(tmp_path):
    """Batch.set_instance_params through the pack row: tau_lim halved on the odd instances, mu and lx of both contacts scaled by 1.5 on
    every third; every instance against the restatement set up with its own constants.  (With the restatement alone: 16 of 16 solve under
    these constants and the four double-support instances with wider cones move by 0.4 - 0.9 Nm; cones NARROWED to 0.8 or 0.9 leave the
    restatement itself without a solution on two to four of them, as tests/inst_par_cases.py found on TOCABI.)"""
    B = 16
    md = _model("fixed_head", tmp_path)
    cases.ensure_pack(md)
    base = pc.state_set("fixed_head", B)
    mo, links = pc.model("fixed_head")
    m = md.ndof - 6
    lim = np.full((B, m), pc.TAU_LIM)
    lim[1::2] *= 0.5
    con = np.broadcast_to(np.array([[c["lx"], c["ly"], c["mu"], c["muz"]] for c in cases.CONTACTS_2]), (B, 2, 4)).copy()
    con[::3, :, 0] *= 1.5
    con[::3, :, 2] *= 1.5
    ref = {k: np.array(v) for k, v in base.items()}
    for b in range(B):
        cyc = pc.cycle_of(mo, links, tau_lim=lim[b], consts=con[b])
        st, dt, c, w, nw = rc.redistribute_ref(cyc, base["q"][b], base["flags"][b], base["tau_in"][b])
        ref["status"][b], ref["tau"][b], ref["cf"][b], ref["wrench"][b] = st, dt, c, w
        ref["nwjw"][b] = 0.0
        ref["nwjw"][b, :, : nw.shape[1]] = nw
    rc.check_premises(ref)
    double = base["flags"].sum(axis=1) == 2
    moved = np.abs(ref["tau"] - base["tau"]).max(axis=1) > 1e-3
    assert moved[double].sum() >= 3, moved  # the record changes answers (asserted on the restatement alone)
    wbc = _batch(md, links, B, tasks=False)
    wbc.set_instance_params(tau_lim=lim, contact=con)
    got = _redistribute(wbc, base)
    rc.compare(got, ref)
    pc.check_flag_mix_outputs(got, ref)
    wbc.close()


ROOT = cases.ROOT
EXE = os.path.join(ROOT, "tests", "cpp", "facade_redistribute_pack")


def test_gpu_facade_on_a_pack_model(tmp_path):
    """include/dwbc_amd.hpp's CalcContactRedistribute(torque_input) on the head-fixed URDF (tests/cpp/facade_redistribute_pack.cpp): returns
    1, and torque_contact_ grows by the restatement's torque_contact_"""
    md = _model("fixed_head", tmp_path)
    cases.ensure_pack(md)
    ref = pc.state_set("fixed_head", 48)
    b = 0
    assert ref["flags"][b].all() and ref["status"][b] == 1 and np.linalg.norm(ref["cf"][b]) > 1e-3 and np.abs(ref["tau"][b]).max() > 1.0
    src = os.path.join(ROOT, "tests", "cpp", "facade_redistribute_pack.cpp")
    libdir = os.path.join(ROOT, "libdwbc_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE, "-L" + libdir, "-l:libdwbc_hip.so",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    args = [repr(float(v)) for v in ref["q"][b]] + [repr(float(v)) for v in ref["tau_in"][b]]
    out = subprocess.check_output([EXE, str(tmp_path / "fixed_head.urdf"), "37"] + args, text=True)
    r = json.loads(out[out.index("{"):])
    assert r["ok"] == [1, 1, 1] and r["model_dof"] == 31, r
    e = float(np.abs(np.asarray(r["torque_contact_increment"]) - ref["tau"][b]).max())
    print(f"facade: worst |d torque_contact_| = {e:.3e} Nm")
    assert e <= 1e-6
    assert float(np.abs(ref["nwjw"][b] @ np.asarray(r["cf_redis_qp_"]) - ref["tau"][b]).max()) <= 1e-6
