"""gpu: SetTaskSpace + CalcTaskSpace as a lean launch (dwbc_batch_calc_task_space -> dwbc_task_space_kernel,
libdwbc_amd/csrc/dwbc_task_space.h): J_task, Lambda_task, J_kt and Null_task of every level against the numpy restatement, their
identities, the mask tiers, against the dump record of a solve, the hierarchy law formed from them against tau_task of solve(hqp=False),
beside the cycle and the other lean launches, bound to torch tensors, with three flags on the device, its refusals, and on a kernel pack.

Inputs, references, premises and bars: tests/task_space_cases.py.  On the parent of the change that added the launch every test here fails
for lack of the entry points.  One refusal cannot be reached on a device: a model without the kernel -- every pack the loader accepts
carries the row -- so its message is pinned by tests/test_task_space_plan.py alone."""
import numpy as np
import pytest

from tests import cases
from tests import redist_pack_cases as pc
from tests import task_space_cases as tc

pytestmark = pytest.mark.gpu

KERNEL = "dwbc::dwbc_task_space_kernel<39, 34, dwbc::TopoTocabi>"
KERNEL_ANY = "dwbc::dwbc_task_space_kernel<39, 34, dwbc::TopoGeneric>"
ALL = list(tc.NAMES)


def _batch(n, tasks, contacts=cases.CONTACTS_2, dtype="f64", model=None):
    import libdwbc_amd as D

    wbc = D.Batch(model or D.Model.from_urdf(cases.URDF), n, device=0, dtype=dtype)
    for c in contacts:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for l, lv in enumerate(tasks):
        for mode, link, pt in lv:
            wbc.add_task(l, mode, link, pt)
    return wbc


def _outputs(wbc):
    """task_space() as per-output lists over the levels, the layout of tests/task_space_cases.py"""
    levels, status = wbc.task_space()
    out = {k: [lv[k] for lv in levels if k in lv] for k in ALL}
    out["status"] = status
    return out


def _launch(wbc, q, flags, names=ALL):
    wbc.set_task_space_outputs(names)
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.calc_task_space()
    return _outputs(wbc)


def _a_inv_n_c(wbc):
    """A_inv_N_C of the contact-space launch on the same batch: the front end the levels were formed from"""
    wbc.set_contact_space_outputs(["A_inv_N_C"])
    wbc.calc_contact_constraint()
    return wbc.contact_space()["A_inv_N_C"]


def _check(wbc, hier, B, what):
    s = tc.tocabi_set(hier, B)
    tc.check_residual_premise(s["ref"], (hier, B))
    got = _launch(wbc, s["q"], s["flags"])
    assert len(got["Null_task"]) == len(s["tasks"]) - 1
    tc.compare(got, s["ref"], s["tasks"], s["nb"], f"{what}, {hier}, B = {B}")
    tc.check_identities(got, _a_inv_n_c(wbc), s["ref"], (hier, B), what)
    return got


@pytest.mark.parametrize("hier,B", [("H4", 7), ("H4", 130), ("HCOM", 7)])
def test_tocabi_matches_restatement_and_identities(hier, B):
    wbc = _batch(B, tc.HIERARCHIES[hier])
    assert wbc.task_space_kernel_name() == KERNEL
    _check(wbc, hier, B, "TOCABI tree")
    wbc.close()


def test_builtin_generic_row(monkeypatch):
    """a TOCABI batch created under DWBC_DENSE_SWEEP (any 34-body tree) takes the built-in TopoGeneric row"""
    monkeypatch.setenv("DWBC_DENSE_SWEEP", "1")
    wbc = _batch(7, tc.H4)
    monkeypatch.delenv("DWBC_DENSE_SWEEP")
    assert wbc.task_space_kernel_name() == KERNEL_ANY
    _check(wbc, "H4", 7, "TOCABI generic")
    wbc.close()


def test_mask_tiers_equal_the_full_run():
    s = tc.tocabi_set("H4", 7)
    wbc = _batch(7, tc.H4)
    full = _launch(wbc, s["q"], s["flags"])
    for names in (("J_task",), ("J_task", "Lambda_task", "J_kt"), ("Lambda_task",)):
        wbc.set_task_space_outputs(list(names))
        wbc.calc_task_space()
        one = _outputs(wbc)
        assert (one["status"] == full["status"]).all()
        for k in ALL:
            assert len(one[k]) == (len(full[k]) if k in names else 0), (names, k)
            for a, b in zip(one[k], full[k]):
                assert (a == b).all(), (names, k)
    # the status alone (no output bit in the kernel's mask): nothing but the status is written or can be read
    wbc.set_task_space_outputs(["status"])
    assert [wbc._L.dwbc_batch_task_space_bytes(wbc._h, 0, i) for i in range(5)] == [0, 0, 0, 0, 7 * 4]
    wbc.calc_task_space()
    wbc.sync()
    levels, status = wbc.task_space()
    assert (status == full["status"]).all() and levels == [{}, {}, {}, {}]
    assert wbc.task_space_kernel_name() == KERNEL
    wbc.close()


def _posed(n, q, flags, fstar, tasks=tc.H4):
    wbc = _batch(n, tasks)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_fstar_all(fstar)
    return wbc


def test_agrees_with_the_dump_record():
    """J_TASK / LAMBDA_TASK / J_KT against DWBC_J_TASK / DWBC_LAMBDA_TASK / DWBC_J_KT of a dump-on solve, to the bars against the
    restatement (the two paths sum in different orders)"""
    B = 7
    s = tc.tocabi_set("H4", B)
    _, _, _, fstar = cases.hierarchy_batch(B, 4, tc.SEED, yaw=True)
    wbc = _posed(B, s["q"], s["flags"], fstar)
    wbc.enable_dump(True)
    wbc.solve()
    raw = {k: wbc.get(k) for k in ("J_task", "Lambda_task", "J_kt")}
    ok = wbc.get("status") == 1
    assert ok.all(), ok  # every instance of the set solves, whatever its support: every record is complete and is compared
    got = _launch(wbc, s["q"], s["flags"], ["J_task", "Lambda_task", "J_kt"])
    n, m = wbc.n, wbc.m
    worst = dict.fromkeys(raw, 0.0)
    for l, t in enumerate(tc.task_dofs(tc.H4)):
        dump = {"J_task": raw["J_task"][:, l].reshape(B, -1)[:, : t * n].reshape(B, t, n),
                "Lambda_task": raw["Lambda_task"][:, l].reshape(B, -1)[:, : t * t].reshape(B, t, t),
                "J_kt": raw["J_kt"][:, l].reshape(B, -1)[:, : m * t].reshape(B, m, t)}
        for k, bar in (("J_task", tc.BAR_J_LINK), ("Lambda_task", tc.BAR_LAMBDA), ("J_kt", tc.BAR_W_DEVICE)):
            e = float(np.abs(got[k][l][ok] - dump[k][ok]).max())
            worst[k] = max(worst[k], e)
            assert e <= bar, (k, l, e, bar)
    for k in raw:
        assert (wbc.get(k) == raw[k]).all(), k  # the dump record stays as the solve left it
    print("launch against the dump record: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    wbc.close()


def test_hierarchy_law_from_the_outputs_gives_tau_task():
    """sum over the levels of Null_{l-1} J_kt Lambda f*, formed in numpy from the launch's outputs, is tau_task of solve(hqp=False) on the
    same batch, to the bar of J_kt times |Lambda f*|_inf summed over the levels"""
    B = 16
    _, q, flags, fstar = cases.hierarchy_batch(B, 4, tc.SEED, yaw=True)
    wbc = _posed(B, q, flags, fstar)
    wbc.solve(hqp=False)
    solved = wbc.get("status") == 1
    assert solved.all(), solved  # both feet down on every instance: all of them solve and all are compared
    tau_task = wbc.get("tau_task")
    got = _launch(wbc, q, flags)
    assert got["status"].all()
    ts = tc.task_dofs(tc.H4)
    off = np.concatenate([[0], np.cumsum(ts)])
    worst, worst_bar = 0.0, 0.0
    for b in np.nonzero(solved)[0]:
        tau, scale = np.zeros(wbc.m), 0.0
        for l in range(len(ts)):
            lf = got["Lambda_task"][l][b] @ fstar[b, off[l]:off[l + 1]]
            h = got["J_kt"][l][b] @ lf
            tau += h if l == 0 else got["Null_task"][l - 1][b] @ h
            scale += float(np.abs(lf).max())
        e, bar = float(np.abs(tau - tau_task[b]).max()), tc.BAR_W_DEVICE * scale
        if e / bar > worst / max(worst_bar, 1e-300):
            worst, worst_bar = e, bar
        assert e <= bar, (b, e, bar)
    print(f"hierarchy law from the launch's outputs against tau_task of solve(hqp=False): worst {worst:.2e} Nm at a bar of {worst_bar:.2e}")
    wbc.close()


def test_the_other_launches_are_untouched():
    """tau, wrench, status, diag and the outputs of the redistribution, gravity, dynamics, contact-space and link-query launches are
    bit-identical with and without a calc_task_space() between two solves"""
    n = 16
    _, q, flags, fstar = cases.hierarchy_batch(n, 4, tc.SEED, yaw=True, mixed=True)
    wbc, twin = _posed(n, q, flags, fstar), _posed(n, q, flags, fstar)
    wbc.solve()
    first = {k: wbc.get(k) for k in ("tau", "wrench", "status", "diag")}
    assert first["status"].sum() >= 0.9 * n
    wbc.set_task_space_outputs(ALL)
    wbc.calc_task_space()
    t1 = _outputs(wbc)
    for k, v in first.items():
        assert (wbc.get(k) == v).all(), k  # nothing of the cycle was written
    wbc.solve()
    for k, v in first.items():
        assert (wbc.get(k) == v).all(), k
    twin.solve()
    twin.solve()
    wbc.calc_task_space()
    wbc.solve(init=False)
    twin.solve(init=False)
    for k in first:
        assert (wbc.get(k) == twin.get(k)).all(), k
    tau_in = np.array(first["tau"]).sum(axis=1)
    for w in (wbc, twin):
        w.set_torque_input(tau_in)
        w.set_dynamics_outputs(["A", "A_inv", "G"])
        w.set_contact_space_outputs(["J_C", "W_inv", "N_C"])
        w.set_link_query([0, 23], jacobians=True)
    for step in ("redistribute", "grav_compensation", "update_dynamics", "calc_contact_constraint", "update_kinematics"):
        wbc.calc_task_space()
        for w in (wbc, twin):
            getattr(w, step)()
    wbc.calc_task_space()
    for k in ("redist_tau", "redist_cf", "redist_wrench", "redist_status"):
        assert (wbc.get(k) == twin.get(k)).all(), k
    for fn in ("grav_outputs", "dynamics", "contact_space", "link_states"):
        a, b = getattr(wbc, fn)(), getattr(twin, fn)()
        assert sorted(a) == sorted(b) and all((a[k] == b[k]).all() for k in a), fn
    t2 = _outputs(wbc)
    for k in ALL:
        for a, b in zip(t1[k], t2[k]):
            assert (a == b).all(), k
    twin.close()
    wbc.close()


def test_bound_tensors_are_written_in_place():
    import torch

    B = 5
    s = tc.tocabi_set("H4", B)
    host = _batch(B, tc.H4)
    want = _launch(host, s["q"], s["flags"])
    dev = _batch(B, tc.H4)
    st = torch.cuda.Stream()
    dev.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        nan = float("nan")
        t = {(0, "J_task"): torch.full((B, 6, 39), nan, dtype=torch.float64, device="cuda:0"),
             (1, "Lambda_task"): torch.full((B, 3, 3), nan, dtype=torch.float64, device="cuda:0"),
             (3, "J_kt"): torch.full((B, 33, 6), nan, dtype=torch.float64, device="cuda:0"),
             (2, "Null_task"): torch.full((B, 33, 33), nan, dtype=torch.float64, device="cuda:0"),
             (0, "status"): torch.full((B,), -1, dtype=torch.int32, device="cuda:0")}
        dev.set_task_space_outputs(ALL)
        for (l, k), v in t.items():
            dev.bind_task_space(l, k, v)
        dev.set_state(s["q"])
        dev.set_contact(s["flags"])
        dev.calc_task_space()
        st.synchronize()
        got = _outputs(dev)  # reads the bound buffers back through get
        for (l, k), v in t.items():
            w = want[k] if k == "status" else want[k][l]
            assert (v.cpu().numpy() == w).all(), (l, k)
        for k in ALL:
            for a, b in zip(got[k], want[k]):
                assert (a == b).all(), k
        dev.bind_task_space(2, "Null_task", None)  # back to the batch's own buffer
        t[(2, "Null_task")].fill_(-1.0)
        dev.calc_task_space()
        assert (dev.task_space(2)["Null_task"] == want["Null_task"][2]).all() and (t[(2, "Null_task")].cpu().numpy() == -1.0).all()
    host.close()
    dev.close()


def test_device_bound_flags_and_three_flags():
    """an instance with three flags set on the device (which the host call refuses) fails alone, with zero outputs"""
    import torch

    q, _, _ = cases.synth_batch(3, seed=tc.SEED, yaw=True)
    flags = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 0, 0]], np.uint8)
    ref = tc.reference(cases.tocabi_model(), cases.CONTACTS_4, tc.H4, q, flags)
    wbc = _batch(3, tc.H4, cases.CONTACTS_4)
    fl = torch.tensor(flags, dtype=torch.uint8, device="cuda:0")
    wbc.bind_tensor("in_contact", fl)
    wbc.set_task_space_outputs(ALL)
    wbc.set_state(q)
    wbc.calc_task_space()
    got = _outputs(wbc)
    assert got["status"].tolist() == [1, 0, 1]
    tc.compare(got, ref, tc.H4, tc.NB_TOCABI, "device-bound flags, three flags in instance 1")
    for k in ALL:
        assert not any(a[1].any() for a in got[k]), k
    fl[1, 2] = 0
    torch.cuda.synchronize()
    wbc.calc_task_space()
    again = _outputs(wbc)
    assert again["status"].tolist() == [1, 1, 1] and again["J_kt"][0][1].any()
    for k in ALL:
        for a, b in zip(again[k], got[k]):
            assert (a[[0, 2]] == b[[0, 2]]).all(), k
    wbc.close()


def test_refusal_ladder():
    import libdwbc_amd as D

    B = 4
    s = tc.tocabi_set("H4_2", B)
    f = _batch(B, tc.H4[:2], dtype="f32")
    with pytest.raises(D.DwbcError, match="task space: fp64 batches only"):
        f.set_task_space_outputs(["J_task"])
    with pytest.raises(D.DwbcError, match="task space: fp64 batches only"):
        f.calc_task_space()
    f.close()
    w = _batch(B, tc.H4[:2])
    w.set_state(s["q"])
    w.set_contact(s["flags"])
    with pytest.raises(D.DwbcError, match="no task-space request"):
        w.calc_task_space()
    with pytest.raises(D.DwbcError, match="unknown output bit"):
        D.batch._check(w._L.dwbc_batch_set_task_space_outputs(w._h, 1 << 5))
    w.set_task_space_outputs(["J_task", "Null_task"])
    with pytest.raises(D.DwbcError, match="no task-space output yet"):
        w.task_space(0)
    w.calc_task_space()
    before = w.task_space(0)
    assert sorted(before) == ["J_task", "Null_task"] and sorted(w.task_space(1)) == ["J_task"]
    nbytes = [[w._L.dwbc_batch_task_space_bytes(w._h, l, i) for i in range(6)] for l in range(3)]
    assert nbytes == [[B * 6 * 39 * 8, 0, 0, B * 33 * 33 * 8, B * 4, 0], [B * 3 * 39 * 8, 0, 0, 0, B * 4, 0], [0, 0, 0, 0, B * 4, 0]]
    buf = np.zeros((B, 33, 33))
    get = w._L.dwbc_batch_get_task_space
    with pytest.raises(D.DwbcError, match="the last level has no Null_task"):
        D.batch._check(get(w._h, 1, D.TASK_SPACE_OUTPUTS["Null_task"], buf.ctypes.data, buf.nbytes))
    with pytest.raises(D.DwbcError, match="this output was not asked for"):
        D.batch._check(get(w._h, 0, D.TASK_SPACE_OUTPUTS["J_kt"], buf.ctypes.data, buf.nbytes))
    with pytest.raises(D.DwbcError, match="no such task level"):
        D.batch._check(get(w._h, 2, D.TASK_SPACE_OUTPUTS["J_task"], buf.ctypes.data, buf.nbytes))
    with pytest.raises(D.DwbcError, match="task space: the host buffer has"):
        D.batch._check(get(w._h, 0, D.TASK_SPACE_OUTPUTS["Null_task"], buf.ctypes.data, buf.nbytes - 8))
    with pytest.raises(D.DwbcError, match="task space: unknown output"):
        D.batch._check(get(w._h, 0, 5, buf.ctypes.data, buf.nbytes))
    w.set_max_active_contacts(3)
    with pytest.raises(D.DwbcError, match="task space: two simultaneously active contacts at most"):
        w.calc_task_space()
    with pytest.raises(D.DwbcError, match="task space: two simultaneously active contacts at most"):
        w.task_space_kernel_name()
    after = w.task_space(0)  # nothing was launched
    assert all((after[k] == before[k]).all() for k in before)
    w.set_max_active_contacts(2)
    # a change of the task levels drops the request
    w.add_task(2, D.TASK_LINK_6D, 23)
    assert [w._L.dwbc_batch_task_space_bytes(w._h, 0, i) for i in range(5)] == [0] * 5
    with pytest.raises(D.DwbcError, match="no task-space request"):
        w.calc_task_space()
    w.add_task(2, D.TASK_LINK_6D, 33)  # a second 6D link: the level is 12 dof wide
    with pytest.raises(D.DwbcError, match="task space: task levels of at most 6 dof"):
        w.set_task_space_outputs(["J_task"])
    w.close()
    c = _batch(B, tc.H4[:1])
    c.add_custom_task(1, 3)
    with pytest.raises(D.DwbcError, match="task space: TASK_CUSTOM levels are not built"):
        c.set_task_space_outputs(["J_task"])
    c.close()
    bare = _batch(B, [])
    with pytest.raises(D.DwbcError, match="task space: no task level"):
        bare.set_task_space_outputs(["J_task"])
    bare.close()


def _renumbered(mo, perm):
    """the same robot with its bodies in the order perm (new index -> old index; still depth first)"""
    inv = {int(o): i for i, o in enumerate(perm)}
    out = {k: np.asarray(mo[k])[perm] for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")}
    out["parent"] = np.array([inv[max(int(mo["parent"][o]), 0)] if i > 0 else int(mo["parent"][0]) for i, o in enumerate(perm)], np.int32)
    out["nb"], out["ndof"] = len(perm), len(perm) + 5
    return out


def test_one_pack_on_its_own_tree_and_on_the_generic_pack(tmp_path):
    """The (37, 32) head-fixed model, the first three levels of H4, B = 8: through the pack of its own tree (TopoPack), and -- the loader
    prefers that one for this parent table -- through the generic pack as the SAME robot with the waist / arm subtree numbered before the
    legs, against the restatement on that renumbered model."""
    import libdwbc_amd as D
    from tests.test_model_packs import VARIANTS

    B = 8
    md = D.Model.from_urdf(cases.variant_urdf(tmp_path / "fixed_head.urdf", VARIANTS["fixed_head"][0]))
    assert (md.ndof, md.nb) == (37, 32)
    cases.ensure_pack(md)
    cases.ensure_pack(md, tree=True)
    mo, links = pc.model("fixed_head")
    s = tc.pack_set("fixed_head", B)
    tc.check_residual_premise(s["ref"], ("fixed_head", B))
    own = _batch(B, s["tasks"], s["contacts"], model=md)
    kn = own.task_space_kernel_name()
    assert "dwbc_task_space_kernel<37, 32," in kn and "TopoPack" in kn
    got = _launch(own, s["q"], s["flags"])
    tc.compare(got, s["ref"], s["tasks"], s["nb"], "fixed_head, own tree")
    tc.check_identities(got, _a_inv_n_c(own), s["ref"], ("fixed_head", B), "fixed_head, own tree")
    own.close()

    names = list(mo["names"])
    waist = names.index("Waist1_Link")
    perm = np.array([0] + list(range(waist, 32)) + list(range(1, waist)))
    mo2 = _renumbered(md.arrays(), perm)
    other = D.Model.from_arrays(mo2)
    assert list(other.arrays()["parent"]) != list(md.arrays()["parent"])
    inv = {int(o): i for i, o in enumerate(perm)}
    q2 = s["q"].copy()
    q2[:, 6:37] = s["q"][:, 6 + (perm[1:] - 1)]
    con2 = [dict(c, link=inv[c["link"]]) for c in s["contacts"]]
    tasks2 = [[(mode, inv[link], pt) for mode, link, pt in lv] for lv in s["tasks"]]
    ref2 = tc.reference(mo2, con2, tasks2, q2, s["flags"])
    gen = _batch(B, tasks2, con2, model=other)
    assert "TopoGeneric" in gen.task_space_kernel_name() and "dwbc_task_space_kernel<37, 32," in gen.task_space_kernel_name()
    g2 = _launch(gen, q2, s["flags"])
    tc.compare(g2, ref2, tasks2, 32, "fixed_head renumbered, generic pack")
    tc.check_identities(g2, _a_inv_n_c(gen), ref2, ("fixed_head", B), "fixed_head renumbered, generic pack")
    gen.close()
