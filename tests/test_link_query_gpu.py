"""gpu: UpdateKinematics as a launch of its own (dwbc_batch_update_kinematics -> dwbc_link_query_kernel, libdwbc_amd/csrc/dwbc_link_query.h):
poses, velocities and Jacobians of queried links against the numpy restatement, through bound torch tensors, beside the cycle and the
redistribution without touching them, and in the two uses it exists for -- a pelvis-frame f* rotated to the world on the device before
the solve, and a TASK_CUSTOM level built from a queried Jacobian.

The query Q7, the references and the bars (pos / rot 1e-12, vel 1e-11, link Jacobians 1e-12, COM Jacobian 1e-10): tests/link_query_cases.py."""
import numpy as np
import pytest

from tests import cases
from tests import link_query_cases as lqc

pytestmark = pytest.mark.gpu

KERNEL = "dwbc::dwbc_link_query_kernel<39, 34>"
TOL_TAU = 1e-6  # Nm: the project's bar of the cycle kernels against the restatement


def _batch(n, tasks=cases.TASKS_2LEVEL, dtype="f64"):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), n, device=0, dtype=dtype)
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(tasks):
        if isinstance(links, int):
            wbc.add_custom_task(lv, links)
            continue
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("B", [7, 130])
def test_gpu_matches_restatement(B):
    """130: more than two wavefronts' worth of instances"""
    q, qd, ref = lqc.state_set(B)
    wbc = _batch(B, tasks=[])  # neither a task space nor a contact flag is needed
    assert wbc.model.link_id("COM") == lqc.COM
    wbc.set_state(q, qd)
    wbc.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS, jacobians=True)
    assert wbc.link_query_kernel_name() == KERNEL
    wbc.update_kinematics()
    got = wbc.link_states()
    assert sorted(got) == ["jac", "pos", "rot", "vel"] and got["jac"].shape == (B, 7, 6, 39)
    lqc.compare(got, ref, lqc.Q7_LINKS)
    assert np.abs(ref["vel"]).max() > 0.1  # the rates move the links
    # without Jacobians and without rates: the same poses bit for bit, zero velocities
    wbc.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS)
    wbc.update_kinematics()
    lean = wbc.link_states()
    assert sorted(lean) == ["pos", "rot", "vel"] and all(_same_bits(lean[k], got[k]) for k in lean)
    still = _batch(B, tasks=[])
    still.set_state(q)
    still.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS)
    still.update_kinematics()
    s = still.link_states()
    assert (s["vel"] == 0.0).all() and _same_bits(s["pos"], got["pos"]) and _same_bits(s["rot"], got["rot"])
    wbc.close()
    still.close()


def test_bound_tensors_match_the_host_path():
    import torch

    B = 7
    q, qd, _ = lqc.state_set(B)
    host = _batch(B, tasks=[])
    host.set_state(q, qd)
    host.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS, jacobians=True)
    host.update_kinematics()
    want = host.link_states()
    dev = _batch(B, tasks=[])
    dev.set_stream(torch.cuda.current_stream().cuda_stream)
    dev.set_state(q, qd)
    dev.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS, jacobians=True)
    t = {k: torch.full(v.shape, float("nan"), dtype=torch.float64, device="cuda:0") for k, v in want.items()}
    for k, v in t.items():
        dev.bind_link_query(k, v)
    dev.update_kinematics()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert _same_bits(t[k].cpu().numpy(), v), k
    got = dev.link_states()  # the getter reads the bound buffers
    assert all(_same_bits(got[k], v) for k, v in want.items())
    # unbinding: the batch's own buffer is written from now on, the tensor is left alone
    t["pos"].fill_(7.0)
    dev.bind_link_query("pos", None)
    dev.update_kinematics()
    assert _same_bits(dev.link_states()["pos"], want["pos"]) and (t["pos"].cpu().numpy() == 7.0).all()
    host.close()
    dev.close()


def test_independent_of_the_cycle_and_the_redistribution():
    """DWBC_TAU / DWBC_WRENCH / DWBC_STATUS / DWBC_DIAG, the dump record and the redistribution's outputs of a batch with the dump enabled
    are bit-identical with and without update_kinematics() between the solves, in either order; the query's outputs do not depend on
    whether a cycle ran"""
    B = 64
    q, flags, fstar = cases.synth_batch(B, seed=7, yaw=True, contact_mode="mixed")
    qd = np.random.default_rng(5).uniform(-1, 1, (B, 39))
    pre = _batch(B)  # a torque near the cycle's own, so that the redistribution has a little work to do
    pre.set_state(q)
    pre.set_contact(flags)
    pre.set_fstar_all(fstar)
    pre.solve()
    tau_in = pre.get("tau_total") + np.random.default_rng(11).normal(0.0, 2.0, (B, 33))
    pre.close()
    CYCLE = ("tau", "wrench", "status", "diag", "dump_raw", "redist_tau", "redist_cf", "redist_wrench", "redist_status")

    only, between, around, alone = _batch(B), _batch(B), _batch(B), _batch(B, tasks=[])
    for w in (only, between, around, alone):
        w.set_state(q, qd)
        w.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS, jacobians=True)
        if w is not alone:
            w.enable_dump(True)
            w.set_contact(flags)
            w.set_fstar_all(fstar)
            w.set_torque_input(tau_in)
    alone.update_kinematics()
    want = alone.link_states()

    only.solve()
    only.redistribute()
    name, info = only.kernel_name(), only.launch_info()
    first = {k: only.get(k) for k in CYCLE}
    print(f"cycle status 1 on {first['status'].sum()} of {B}, redistribution status 1 on {first['redist_status'].sum()}")
    assert first["status"].sum() >= 0.9 * B
    only.solve(init=False)
    second = {k: only.get(k) for k in CYCLE}

    between.solve()
    between.update_kinematics()
    between.redistribute()
    around.update_kinematics()
    around.solve()
    around.redistribute()
    around.update_kinematics()
    for w in (between, around):
        assert w.kernel_name() == name and w.launch_info() == info
        for k, v in first.items():
            assert _same_bits(w.get(k), v), k
        assert all(_same_bits(v, want[k]) for k, v in w.link_states().items())
    # the cycle still starts warm from its own working sets after a query ran in between
    between.update_kinematics()
    between.solve(init=False)
    around.solve(init=False)
    around.update_kinematics()
    for w in (between, around):
        for k, v in second.items():
            assert _same_bits(w.get(k), v), k
        assert all(_same_bits(v, want[k]) for k, v in w.link_states().items())
    for w in (only, between, around, alone):
        w.close()


def _restatement():
    from tests import redist_cases as rc

    return rc._cycle()  # the restatement set up with CONTACTS_2, TASKS_2LEVEL and TAU_LIM


def test_pelvis_frame_fstar_rotated_on_the_device():
    """what the launch exists for (reference tests/sp_test/regulation_test.cpp:97-98): update_kinematics(), both halves of a pelvis-frame
    f* of level 0 rotated by the queried pelvis rotation into a tensor bound as in_fstar, solve() -- against the restatement's Cycle.run
    given f* rotated by its own R[0]"""
    import torch

    from oracle.dwbc_np import forward_kinematics

    B = 32
    q, flags, fstar = cases.synth_batch(B, seed=5, yaw=True)
    assert flags.all()  # feet down
    model = cases.tocabi_model()
    R0 = np.stack([forward_kinematics(model, q[b])[0][0] for b in range(B)])
    world = fstar.copy()
    world[:, 0:3] = np.einsum("bij,bj->bi", R0, fstar[:, 0:3])
    world[:, 3:6] = np.einsum("bij,bj->bi", R0, fstar[:, 3:6])
    moved = np.abs(world - fstar).max(axis=1)
    print(f"least |rotated f* - f*| over the batch = {moved.min():.3e}")
    assert (moved > 1e-3).all()  # the yaw makes the test mean something

    cyc = _restatement()
    tau_ref, st_ref = np.zeros((B, 33)), np.zeros(B, np.int32)
    for b in range(B):
        tau_ref[b] = cyc.run(q[b], [True, True], [world[b, :6], world[b, 6:9]])
        st_ref[b] = cyc.status

    wbc = _batch(B)
    wbc.set_stream(torch.cuda.current_stream().cuda_stream)  # the query, torch's rotation and the solve are ordered on one stream
    wbc.set_state(q)
    wbc.set_contact(flags)
    wbc.set_link_query([0])
    rot = torch.zeros((B, 1, 3, 3), dtype=torch.float64, device="cuda:0")
    f_in = torch.zeros((B, 9), dtype=torch.float64, device="cuda:0")
    wbc.bind_link_query("rot", rot)
    wbc.bind_tensor("in_fstar", f_in)
    f_pelvis = torch.from_numpy(fstar).to("cuda:0")
    wbc.update_kinematics()
    f_in[:, 0:3] = torch.einsum("bij,bj->bi", rot[:, 0], f_pelvis[:, 0:3])
    f_in[:, 3:6] = torch.einsum("bij,bj->bi", rot[:, 0], f_pelvis[:, 3:6])
    f_in[:, 6:9] = f_pelvis[:, 6:9]
    wbc.solve()
    torch.cuda.synchronize()
    assert np.abs(f_in.cpu().numpy() - world).max() <= 1e-12
    tau, status = wbc.get("tau_total"), wbc.get("status")
    e = np.abs(tau - tau_ref)[st_ref == 1].max()
    print(f"worst |tau - restatement| = {e:.3e} Nm over {int((st_ref == 1).sum())} instances")
    assert (status == st_ref).all() and st_ref.sum() >= 0.9 * B
    assert e <= TOL_TAU, e
    wbc.close()


def test_custom_level_from_a_queried_jacobian():
    """a 6-dof TASK_CUSTOM level whose Jacobian is the queried left-hand Jacobian reproduces a TASK_LINK_6D level on that link"""
    import libdwbc_amd as D

    B, HAND = 16, 23
    q, flags, fstar = cases.synth_batch(B, seed=5, yaw=True)
    f_hand = 0.5 * np.random.default_rng(6).uniform(-1, 1, (B, 6))
    link = _batch(B, tasks=[cases.TASKS_2LEVEL[0], [(D.TASK_LINK_6D, HAND, (0, 0, 0))]])
    custom = _batch(B, tasks=[cases.TASKS_2LEVEL[0], 6])
    for w in (link, custom):
        w.set_state(q)
        w.set_contact(flags)
        w.set_fstar(0, fstar[:, :6])
    link.set_fstar(1, f_hand)
    custom.set_link_query([HAND], jacobians=True)
    custom.update_kinematics()
    custom.set_custom_task(1, f_hand, custom.link_states()["jac"][:, 0])
    link.solve()
    custom.solve()
    assert (link.get("status") == 1).all() and (custom.get("status") == 1).all()
    e = np.abs(link.get("tau") - custom.get("tau")).max()
    print(f"worst |tau(TASK_LINK_6D) - tau(TASK_CUSTOM from the queried Jacobian)| = {e:.3e} Nm")
    assert np.abs(link.get("tau")[:, 1]).max() > 1.0  # the hand level asks for torque
    assert e <= TOL_TAU, e
    link.close()
    custom.close()


def test_refusals(tmp_path):
    import ctypes as C

    import libdwbc_amd as D
    from libdwbc_amd import _lib

    n = 4
    q, qd, _ = lqc.state_set(7)
    w = _batch(n, tasks=[])
    w.set_state(q[:n], qd[:n])
    with pytest.raises(D.DwbcError, match="no link query: call dwbc_batch_set_link_query first"):
        w.update_kinematics()
    with pytest.raises(D.DwbcError, match="no link query"):
        w.link_states()
    w.set_link_query(lqc.Q7_LINKS, lqc.Q7_POINTS)
    with pytest.raises(D.DwbcError, match="no link-query output yet: call dwbc_batch_update_kinematics first"):
        w.link_states()
    w.update_kinematics()
    before = w.link_states()
    # each refused query leaves the query and its outputs as they were
    for links, points, msg in (([0, 35], None, r"link 35 is outside \[0, 34\]"), ([-1], None, r"link -1 is outside \[0, 34\]"),
                               ([0, lqc.COM], [(0, 0, 0), (0, 0, 0.1)], "the COM link takes no point"), ([0] * 17, None, "at most 16 entries")):
        with pytest.raises(D.DwbcError, match=msg):
            w.set_link_query(links, points, jacobians=True)
        assert all(_same_bits(v, before[k]) for k, v in w.link_states().items()) and sorted(w.link_states()) == ["pos", "rot", "vel"]
    out = np.zeros((n, 7, 6, 39))
    assert w._L.dwbc_batch_link_query_bytes(w._h, 3) == 0
    assert w._L.dwbc_batch_get_link_query(w._h, 3, out.ctypes.data, C.c_size_t(out.nbytes)) == 0
    assert _lib.last_error() == "link query: set without Jacobians (dwbc_batch_set_link_query with want_jacobians = 1)"
    w.update_kinematics()
    assert all(_same_bits(v, before[k]) for k, v in w.link_states().items())
    w.set_link_query([])  # dropped
    with pytest.raises(D.DwbcError, match="no link query"):
        w.update_kinematics()
    w.close()

    f = _batch(n, tasks=[], dtype="f32")
    with pytest.raises(D.DwbcError, match="link query: fp64 batches only"):
        f.set_link_query([0])
    with pytest.raises(D.DwbcError, match="link query: fp64 batches only"):
        f.link_query_kernel_name()
    f.close()

    model = D.Model.from_urdf(cases.variant_urdf(tmp_path / "fixed_head.urdf", cases.HEAD_JOINTS))
    assert (model.ndof, model.nb) == (37, 32)
    cases.ensure_pack(model)
    p = D.Batch(model, n, device=0)
    with pytest.raises(D.DwbcError, match="no link-query kernel for this model"):
        p.set_link_query([0])
    p.close()
