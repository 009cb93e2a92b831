"""gpu: SetContact + CalcContactConstraint as a lean launch (dwbc_batch_calc_contact_constraint -> dwbc_contact_space_kernel,
libdwbc_amd/csrc/dwbc_contact_space.h): J_C, Lambda_contact, J_C_INV_T, N_C, A_inv_N_C, W, W_inv, NwJw and the contact frames against the
numpy restatement and the reference's goldens, their identities, against the dump record of a solve, bound to torch tensors, with flags
bound on the device, beside the cycle and the other lean launches, its refusals, and on the kernel packs.

Inputs, references, premises and bars: tests/contact_space_cases.py.  On the parent of the change that added the launch every test here
fails for lack of the entry points.  One refusal cannot be reached on a device: a model without the kernel -- every pack the loader accepts
carries the row -- so its message is pinned by tests/test_contact_space_plan.py alone."""
import numpy as np
import pytest

from tests import cases
from tests import contact_space_cases as cc
from tests import redist_pack_cases as pc

pytestmark = pytest.mark.gpu

B = 8
KERNEL = "dwbc::dwbc_contact_space_kernel<39, 34, dwbc::TopoTocabi>"
KERNEL_ANY = "dwbc::dwbc_contact_space_kernel<39, 34, dwbc::TopoGeneric>"
ALL = list(cc.NAMES)
SHARED = ("J_C", "Lambda_c", "J_C_INV_T", "A_inv_N_C", "W_inv", "NwJw", "contact_pos", "contact_rot")  # what the dump record holds too


def _contacts(n, contacts=cases.CONTACTS_2, dtype="f64"):
    """contacts registered, no task"""
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), n, device=0, dtype=dtype)
    for c in contacts:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    return wbc


def _full(n, contacts=cases.CONTACTS_2):
    import libdwbc_amd as D

    wbc = _contacts(n, contacts)
    wbc.add_task(0, D.TASK_LINK_6D, 0)
    wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _launch(wbc, q, flags, names=ALL):
    wbc.set_contact_space_outputs(names)
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.calc_contact_constraint()
    return wbc.contact_space()


def _dump_outputs(wbc, ref):
    """the dump record of the last solve in the launch's shapes, on the active cd of every instance (Lambda_c re-strided)"""
    n = wbc.n
    nB = len(ref["cd"])
    out = {k: np.zeros(s) for k, s in cc.shapes(nB, n).items()}
    raw = {k: wbc.get(k) for k in SHARED}
    for b in range(nB):
        cd = int(ref["cd"][b])
        out["J_C"][b, :cd] = raw["J_C"][b][:cd]
        out["J_C_INV_T"][b, :cd] = raw["J_C_INV_T"][b][:cd]
        out["Lambda_c"][b, :cd, :cd] = raw["Lambda_c"][b].ravel()[: cd * cd].reshape(cd, cd)
        out["A_inv_N_C"][b] = raw["A_inv_N_C"][b]
        out["W"][b] = raw["A_inv_N_C"][b][6:, 6:]
        out["W_inv"][b] = raw["W_inv"][b]
        if cd > 6:
            out["NwJw"][b] = raw["NwJw"][b].reshape(n - 6, 6)
        out["contact_pos"][b, : cd // 6] = raw["contact_pos"][b][: cd // 6]
        out["contact_rot"][b, : cd // 6] = raw["contact_rot"][b].reshape(2, 3, 3)[: cd // 6]
    return out


def _check_dump_premise(s, contacts, what):
    """premise: on the same states the dump record of a solve() -- code the launch does not touch -- meets every bar against the
    restatement.  Returns the posed batch (solved once) and its dump outputs."""
    nB = len(s["q"])
    _, _, fstar = cases.synth_batch(nB, seed=cc.SEED, yaw=True)
    wbc = _full(nB, contacts)
    wbc.enable_dump(True)
    wbc.set_state(s["q"])
    wbc.set_contact(s["flags"])
    wbc.set_fstar_all(fstar)
    wbc.solve()
    dump = _dump_outputs(wbc, s["ref"])
    names = [k for k in SHARED] + ["W"]
    errs = {k: float(np.abs(dump[k] - s["ref"][k]).max()) for k in names}
    print(f"{what}: dump record against the restatement: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in names:
        assert errs[k] <= cc.BARS[k], ("premise", k, errs[k])
    return wbc, dump


def _check_tocabi(wbc, what):
    s = cc.tocabi_set(B)
    cc.check_residual_premise(s["ref"], ("tocabi", B))
    pre, _ = _check_dump_premise(s, cases.CONTACTS_2, what)
    pre.close()
    got = _launch(wbc, s["q"], s["flags"])
    assert sorted(got) == sorted(ALL + ["status"])
    cc.compare(got, s["ref"], what)
    cc.check_identities(got, s["ref"], ("tocabi", B), what)
    return got


def _check_goldens(wbc, what):
    """the CASE states with four registered contacts, two enabled, in instances 0 and 1; the other instances stand on the left foot"""
    g = cc.golden_set()
    cc.check_residual_premise(g["ref"], ("golden", 2))
    q = np.repeat(g["q"][:1], B, axis=0)
    q[1] = g["q"][1]
    fl = np.zeros((B, 4), np.uint8)
    fl[:, 0] = 1
    fl[:2, 1] = 1
    got = _launch(wbc, q, fl)
    assert (got["status"] == 1).all()
    two = {k: got[k][:2] for k in got}
    cc.compare(two, g["ref"], what + ", CASE states")
    cc.compare_goldens(two, g, what)
    cc.check_identities(two, g["ref"], ("golden", 2), what + ", CASE states")


def test_tocabi_matches_restatement_goldens_and_identities():
    wbc = _contacts(B)
    assert wbc.contact_space_kernel_name() == KERNEL
    _check_tocabi(wbc, "TOCABI tree")
    wbc.close()
    w4 = _contacts(B, cases.CONTACTS_4)
    _check_goldens(w4, "TOCABI tree")
    w4.close()


def test_builtin_generic_row(monkeypatch):
    """a TOCABI batch created under DWBC_DENSE_SWEEP (any 34-body tree) takes the built-in TopoGeneric row"""
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    wbc, w4 = _contacts(B), _contacts(B, cases.CONTACTS_4)
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    assert wbc.contact_space_kernel_name() == KERNEL_ANY and w4.contact_space_kernel_name() == KERNEL_ANY
    _check_tocabi(wbc, "TOCABI generic")
    _check_goldens(w4, "TOCABI generic")
    wbc.close()
    w4.close()


def test_single_outputs_equal_the_full_run():
    s = cc.tocabi_set(B)
    wbc = _contacts(B)
    full = _launch(wbc, s["q"], s["flags"])
    for names in (("J_C",), ("Lambda_c", "J_C_INV_T"), ("NwJw",), ("W_inv",), ("N_C",), ("contact_pos", "contact_rot"), ("A_inv_N_C", "W")):
        wbc.set_contact_space_outputs(list(names))
        wbc.calc_contact_constraint()
        one = wbc.contact_space()
        assert sorted(one) == sorted(list(names) + ["status"]) and (one["status"] == full["status"]).all()
        for k in names:
            assert (one[k] == full[k]).all(), (names, k)
    wbc.close()


def test_agrees_with_the_dump_record():
    s = cc.tocabi_set(B)
    wbc, dump = _check_dump_premise(s, cases.CONTACTS_2, "TOCABI")
    raw = {k: wbc.get(k) for k in SHARED}
    wbc.set_contact_space_outputs(ALL)
    wbc.calc_contact_constraint()
    got = wbc.contact_space()
    for k in SHARED:
        assert (wbc.get(k) == raw[k]).all(), k  # the dump record stays as the solve left it
    names = list(SHARED) + ["W"]
    errs = {k: float(np.abs(got[k] - dump[k]).max()) for k in names}
    print("launch against the dump record: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print("bit-equal to the dump record: " + (", ".join(k for k in names if (got[k] == dump[k]).all()) or "none"))
    for k in names:
        assert errs[k] <= cc.BARS[k], (k, errs[k])
    wbc.close()


def _posed_full(n, q, flags, fstar):
    wbc = _full(n)
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    return wbc


def test_the_other_launches_are_untouched():
    """solve() -> calc_contact_constraint() -> solve() gives bit-equal tau, wrench, status, diag; warm solves behind the launch are those of
    a twin batch that never ran it; the same around redistribute(), grav_compensation() and update_dynamics()"""
    n = 16
    q, flags, fstar = cases.synth_batch(n, seed=cc.SEED, yaw=True, contact_mode="mixed")
    wbc, twin = _posed_full(n, q, flags, fstar), _posed_full(n, q, flags, fstar)
    wbc.solve()
    first = {k: wbc.get(k) for k in ("tau", "wrench", "status", "diag")}
    assert first["status"].sum() >= 0.9 * n
    wbc.set_contact_space_outputs(ALL)
    wbc.calc_contact_constraint()
    c1 = wbc.contact_space()
    for k, v in first.items():
        assert (wbc.get(k) == v).all(), k  # nothing of the cycle was written
    wbc.solve()
    for k, v in first.items():
        assert (wbc.get(k) == v).all(), k
    twin.solve()
    twin.solve()
    for _ in range(2):
        wbc.calc_contact_constraint()
        wbc.solve(init=False)
        twin.solve(init=False)
        for k in first:
            assert (wbc.get(k) == twin.get(k)).all(), k
    # the other lean launches, with and without this one between them
    tau_in = np.array(first["tau"]).sum(axis=1)
    for w in (wbc, twin):
        w.set_torque_input(tau_in)
        w.set_dynamics_outputs(["A", "A_inv", "G"])
    wbc.calc_contact_constraint()
    for w in (wbc, twin):
        w.redistribute()
    wbc.calc_contact_constraint()
    for w in (wbc, twin):
        w.grav_compensation()
    wbc.calc_contact_constraint()
    for w in (wbc, twin):
        w.update_dynamics()
    wbc.calc_contact_constraint()
    for k in ("redist_tau", "redist_cf", "redist_wrench", "redist_status"):
        assert (wbc.get(k) == twin.get(k)).all(), k
    ga, gb = wbc.grav_outputs(), twin.grav_outputs()
    da, db = wbc.dynamics(), twin.dynamics()
    assert all((ga[k] == gb[k]).all() for k in ga) and all((da[k] == db[k]).all() for k in da)
    c2 = wbc.contact_space()
    for k in ALL:
        assert (c1[k] == c2[k]).all(), k
    twin.close()
    wbc.close()


def test_bound_tensors_are_written_in_place():
    import torch

    s = cc.tocabi_set(B)
    names = ["N_C", "A_inv_N_C", "J_C", "W_inv"]
    host = _contacts(B)
    want = _launch(host, s["q"], s["flags"], names)
    dev = _contacts(B)
    st = torch.cuda.Stream()
    dev.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        t = dict(N_C=torch.full((B, 39, 39), float("nan"), dtype=torch.float64, device="cuda:0"),
                 J_C=torch.full((B, 12, 39), float("nan"), dtype=torch.float64, device="cuda:0"),
                 status=torch.full((B,), -1, dtype=torch.int32, device="cuda:0"))
        dev.set_contact_space_outputs(names)
        for k, v in t.items():
            dev.bind_contact_space(k, v)
        dev.set_state(s["q"])
        dev.set_contact(s["flags"])
        dev.calc_contact_constraint()
        st.synchronize()
        got = dev.contact_space()  # reads the bound buffers back through get
        for k, v in t.items():
            assert (v.cpu().numpy() == want[k]).all() and (got[k] == want[k]).all(), k
        assert (got["A_inv_N_C"] == want["A_inv_N_C"]).all() and (got["W_inv"] == want["W_inv"]).all()
        dev.bind_contact_space("N_C", None)  # back to the batch's own buffer
        t["N_C"].fill_(-1.0)
        dev.calc_contact_constraint()
        assert (dev.contact_space()["N_C"] == want["N_C"]).all() and (t["N_C"].cpu().numpy() == -1.0).all()
    host.close()
    dev.close()


def test_device_bound_flags_and_three_flags():
    """flags bound on the device are read where they are: no host round trip; an instance with three flags set (which the host call
    refuses) fails alone, with zero outputs"""
    import torch

    s = cc.too_many_set()
    nB = len(s["q"])
    wbc = _contacts(nB, cases.CONTACTS_4)
    fl = torch.tensor(np.array(s["flags"]), dtype=torch.uint8, device="cuda:0")
    wbc.bind_tensor("in_contact", fl)
    wbc.set_contact_space_outputs(ALL)
    wbc.set_state(s["q"])
    wbc.calc_contact_constraint()
    got = wbc.contact_space()
    assert got["status"].tolist() == [1, 0, 1]
    cc.compare(got, s["ref"], "device-bound flags, three flags in instance 1")
    # the flags change on the device, nothing is uploaded: the next launch sees them
    fl[1, 2] = 0
    torch.cuda.synchronize()
    wbc.calc_contact_constraint()
    again = wbc.contact_space()
    assert again["status"].tolist() == [1, 1, 1] and again["NwJw"][1].any()
    for k in ALL:
        assert (again[k][[0, 2]] == got[k][[0, 2]]).all(), k
    wbc.close()


def test_refusals():
    import libdwbc_amd as D

    s = cc.tocabi_set(B)
    f = _contacts(B, dtype="f32")
    with pytest.raises(D.DwbcError, match="contact space: fp64 batches only"):
        f.set_contact_space_outputs(["J_C"])
    with pytest.raises(D.DwbcError, match="contact space: fp64 batches only"):
        f.calc_contact_constraint()
    f.close()
    w = _contacts(B)
    w.set_state(s["q"])
    w.set_contact(s["flags"])
    with pytest.raises(D.DwbcError, match="no contact-space request"):
        w.calc_contact_constraint()
    w.set_contact_space_outputs(["J_C", "W"])
    with pytest.raises(D.DwbcError, match="no contact-space output yet"):
        w.contact_space()
    w.calc_contact_constraint()
    before = w.contact_space()
    assert sorted(before) == ["J_C", "W", "status"]
    nbytes = [w._L.dwbc_batch_contact_space_bytes(w._h, i) for i in range(12)]
    assert nbytes == [B * 12 * 39 * 8, 0, 0, 0, 0, B * 33 * 33 * 8, 0, 0, 0, 0, B * 4, 0]
    w.set_max_active_contacts(3)
    with pytest.raises(D.DwbcError, match="contact space: two simultaneously active contacts at most"):
        w.calc_contact_constraint()
    with pytest.raises(D.DwbcError, match="contact space: two simultaneously active contacts at most"):
        w.contact_space_kernel_name()
    after = w.contact_space()  # nothing was launched
    assert all((after[k] == before[k]).all() for k in before)
    w.set_max_active_contacts(2)
    with pytest.raises(D.DwbcError, match="this output was not asked for"):
        w.bind_contact_space("N_C", None)
    w.set_contact_space_outputs([])
    assert [w._L.dwbc_batch_contact_space_bytes(w._h, i) for i in range(12)] == [0] * 12
    w.close()
    bare = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0)
    with pytest.raises(D.DwbcError, match="contact space: no contact constraint"):
        bare.set_contact_space_outputs(["J_C"])
    bare.close()


def _pack_model(name, tmp_path):
    import libdwbc_amd as D
    from tests.test_model_packs import VARIANTS, model_43

    if name == "surgery_43":
        return model_43()[0]
    return D.Model.from_urdf(cases.variant_urdf(tmp_path / f"{name}.urdf", VARIANTS[name][0]))


def _pack_batch(md, links, nB):
    import libdwbc_amd as D

    wbc = D.Batch(md, nB, device=0)
    for c in pc.contacts_of(links):
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    return wbc


@pytest.mark.parametrize("name", ["fixed_head", "fixed_arms", "surgery_43"])
def test_packs_match_restatement(tmp_path, name):
    md = _pack_model(name, tmp_path)
    assert (md.ndof, md.nb) == pc.SIZES[name]
    cases.ensure_pack(md)
    _, links = pc.model(name)
    s = cc.pack_set(name, B)
    cc.check_residual_premise(s["ref"], (name, B))
    wbc = _pack_batch(md, links, B)
    assert f"dwbc_contact_space_kernel<{md.ndof}, {md.nb}," in wbc.contact_space_kernel_name()
    got = _launch(wbc, s["q"], s["flags"])
    cc.compare(got, s["ref"], name)
    cc.check_identities(got, s["ref"], (name, B), name)
    wbc.close()


def _renumbered(mo, perm):
    """the same robot with its bodies in the order perm (new index -> old index; still depth first)"""
    inv = {int(o): i for i, o in enumerate(perm)}
    out = {k: np.asarray(mo[k])[perm] for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")}
    out["parent"] = np.array([inv[max(int(mo["parent"][o]), 0)] if i > 0 else int(mo["parent"][0]) for i, o in enumerate(perm)], np.int32)
    out["nb"], out["ndof"] = len(perm), len(perm) + 5
    return out


def test_own_tree_pack_matches_restatement_and_the_generic_pack(tmp_path):
    """The head-fixed model runs the kernel of its own-tree pack (TopoPack).  The loader prefers that pack for this parent table, so the
    generic 37 / 32 pack is reached as tests/test_redistribute_packs_gpu.py reaches it: the SAME robot with the waist / arm subtree numbered
    before the legs, the same states in that joint order; its outputs are permuted back before the comparison."""
    import libdwbc_amd as D

    md = _pack_model("fixed_head", tmp_path)
    cases.ensure_pack(md)
    cases.ensure_pack(md, tree=True)
    mo, links = pc.model("fixed_head")
    s = cc.pack_set("fixed_head", B)
    own = _pack_batch(md, links, B)
    kn = own.contact_space_kernel_name()
    assert "dwbc_contact_space_kernel<37, 32," in kn and "TopoPack" in kn
    got = _launch(own, s["q"], s["flags"])
    cc.compare(got, s["ref"], "fixed_head, own tree")
    cc.check_identities(got, s["ref"], ("fixed_head", B), "fixed_head, own tree")

    names = list(mo["names"])
    waist = names.index("Waist1_Link")
    perm = np.array([0] + list(range(waist, 32)) + list(range(1, waist)))
    other = D.Model.from_arrays(_renumbered(md.arrays(), perm))
    assert list(other.arrays()["parent"]) != list(md.arrays()["parent"])
    jp = perm[1:] - 1  # joint order: new joint i is old joint jp[i]
    inv = {int(o): i for i, o in enumerate(perm)}
    q2 = s["q"].copy()
    q2[:, 6:37] = s["q"][:, 6 + jp]
    gen = _pack_batch(other, [inv[l] for l in links], B)
    assert "TopoGeneric" in gen.contact_space_kernel_name() and "dwbc_contact_space_kernel<37, 32," in gen.contact_space_kernel_name()
    g2 = _launch(gen, q2, s["flags"])
    P = np.concatenate([np.arange(6), 6 + jp])  # new dof i is old dof P[i]

    def back(x, axes, joints=False):
        p = jp if joints else P
        y = x
        for ax in axes:
            z = np.zeros_like(y)
            idx = [slice(None)] * y.ndim
            idx[ax] = p
            z[tuple(idx)] = y
            y = z
        return y

    same = dict(J_C=back(g2["J_C"], [2]), Lambda_c=g2["Lambda_c"], J_C_INV_T=back(g2["J_C_INV_T"], [2]), N_C=back(g2["N_C"], [1, 2]),
                A_inv_N_C=back(g2["A_inv_N_C"], [1, 2]), W=back(g2["W"], [1, 2], True), W_inv=back(g2["W_inv"], [1, 2], True),
                NwJw=back(g2["NwJw"], [1], True), contact_pos=g2["contact_pos"], contact_rot=g2["contact_rot"], status=g2["status"])
    errs = {k: float(np.abs(same[k] - got[k]).max()) for k in ALL}
    print("own-tree pack against the generic pack: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert (same["status"] == got["status"]).all()
    for k in ALL:
        assert errs[k] <= 2 * cc.BARS[k], (k, errs[k])  # (each is within its bar of the restatement)
    own.close()
    gen.close()
