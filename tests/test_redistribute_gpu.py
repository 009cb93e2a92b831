"""gpu: CalcContactRedistribute(torque_input) / getContactForce(torque) for a caller-supplied torque, batched
(dwbc_batch_redistribute -> dwbc_redistribute_kernel, libdwbc_amd/csrc/dwbc_redistribute.h) against the numpy restatement.

Inputs, the two premises every comparison asserts first, and the bars (1e-6 Nm, 1e-5 N): tests/redist_cases.py."""
import numpy as np
import pytest

from tests import cases
from tests import redist_cases as rc

pytestmark = pytest.mark.gpu

B = 250
KERNEL = "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"


def _batch(n, tasks=True, dtype="f64", contacts=cases.CONTACTS_2):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), n, device=0, dtype=dtype)
    for c in contacts:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    if tasks:
        wbc.add_task(0, D.TASK_LINK_6D, 0)
        wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _outputs(wbc):
    return dict(tau=wbc.get("redist_tau"), cf=wbc.get("redist_cf"), wrench=wbc.get("redist_wrench"), status=wbc.get("redist_status"))


def _with_free_instances(ref):
    """the state set with every third instance in the air: zeros and status 1 there, the restatement's answers elsewhere"""
    out = {k: v.copy() for k, v in ref.items()}
    out["flags"][::3] = 0
    out["status"][::3] = 1
    for k in ("tau", "cf", "wrench", "nwjw"):
        out[k][::3] = 0.0
    return out


@pytest.mark.parametrize("case", ["flat_LR", "yaw_mixed", "third_free"])
def test_gpu_matches_restatement(case):
    ref = rc.state_set(B, True, "mixed") if case == "yaw_mixed" else rc.state_set(B, False, "LR")
    if case == "third_free":
        ref = _with_free_instances(ref)
    rc.check_premises(ref)
    wbc = _batch(B, tasks=False)  # no task space is needed
    assert wbc.redistribute_kernel_name() == KERNEL
    wbc.set_state(ref["q"])
    wbc.set_contact(ref["flags"])
    wbc.set_torque_input(ref["tau_in"])
    wbc.redistribute()
    got = _outputs(wbc)
    rc.compare(got, ref)
    free = ref["flags"].sum(axis=1) == 0
    single = ref["flags"].sum(axis=1) == 1
    for k in ("tau", "cf", "wrench"):
        assert np.abs(got[k][free]).max(initial=0.0) == 0.0, k
    assert np.abs(got["tau"][single]).max(initial=0.0) == 0.0 and (got["status"][single] == 1).all()
    assert (got["wrench"][single][:, 0] == got["wrench"][single][:, 1]).all()
    assert (wbc.get("in_torque") == ref["tau_in"]).all()
    wbc.close()


def test_feasible_input_is_left_alone():
    ref = rc.state_set(B, False, "LR")
    wbc = _batch(B)
    wbc.set_state(ref["q"])
    wbc.set_contact(ref["flags"])
    view = wbc.host_view("in_torque")  # the page-locked mirror, filled in place
    view[:] = ref["tau_feasible"]
    wbc.set_torque_input(view)
    wbc.redistribute(init=False)  # accepted: runs cold
    got = _outputs(wbc)
    assert (got["status"] == 1).all()
    assert np.abs(got["tau"]).max() <= 1e-6
    assert (got["wrench"][:, 0] == got["wrench"][:, 1]).all() and np.abs(got["wrench"][:, 0]).max(axis=1).min() > 100.0
    wbc.close()


def test_independent_of_the_cycle():
    """solve() then redistribute() (and the other order) leaves DWBC_TAU / DWBC_WRENCH / DWBC_STATUS / DWBC_DIAG bit-identical to a batch
    that only solved, and the redistribution's outputs do not depend on whether a cycle ran"""
    ref = rc.state_set(B, True, "mixed")
    _, _, fstar = cases.synth_batch(B, seed=7, yaw=True, contact_mode="mixed")

    only, after, before, alone = _batch(B), _batch(B), _batch(B), _batch(B, tasks=False)
    for w in (only, after, before, alone):
        w.set_state(ref["q"])
        w.set_contact(ref["flags"])
        w.set_torque_input(ref["tau_in"])
        if w is not alone:
            w.set_fstar_all(fstar)
    only.solve()
    name = only.kernel_name()
    after.solve()
    assert after.kernel_name() == name
    after.redistribute()
    assert after.kernel_name() == name and after.launch_info() == only.launch_info()
    before.redistribute()
    before.solve()
    alone.redistribute()
    cyc = {k: only.get(k) for k in ("tau", "wrench", "status", "diag")}
    assert cyc["status"].sum() >= 0.9 * B
    for w in (after, before):
        for k, v in cyc.items():
            assert (w.get(k) == v).all(), k
        assert w.kernel_name() == name
    red = _outputs(alone)
    for w in (after, before):
        for k, v in _outputs(w).items():
            assert (v == red[k]).all(), k
    # the cycle still starts warm from its own working sets after a redistribution ran in between
    after.solve(init=False)
    only.solve(init=False)
    assert (after.get("tau") == only.get("tau")).all() and (after.get("diag") == only.get("diag")).all()
    for w in (only, after, before, alone):
        w.close()


def test_bound_tensors_match_the_host_path():
    import torch

    ref = rc.state_set(B, False, "LR")
    host = _batch(B, tasks=False)
    host.set_state(ref["q"])
    host.set_contact(ref["flags"])
    host.set_torque_input(ref["tau_in"])
    host.redistribute()
    want = _outputs(host)
    dev = _batch(B, tasks=False)
    dev.set_state(ref["q"])
    dev.set_contact(ref["flags"])
    tin = torch.from_numpy(ref["tau_in"].copy()).to("cuda:0")  # e.g. a policy's output
    tout = torch.full((B, dev.m), float("nan"), dtype=torch.float64, device="cuda:0")
    dev.bind_tensor("in_torque", tin)
    dev.bind_tensor("redist_tau", tout)
    with pytest.raises(Exception, match="bound to a device buffer"):
        dev.set_torque_input(ref["tau_in"])
    torch.cuda.synchronize()
    dev.redistribute()
    dev.sync()
    assert (tout.cpu().numpy() == want["tau"]).all()
    assert (dev.get("redist_tau") == want["tau"]).all() and (dev.get("redist_wrench") == want["wrench"]).all()
    tin += tout  # redistributed in place on the device
    torch.cuda.synchronize()  # (torch's stream and the batch's are not ordered against each other)
    dev.redistribute()
    dev.sync()
    assert np.abs(tout.cpu().numpy()).max() <= 1e-6  # already inside its rows
    host.close()
    dev.close()


def test_refusals():
    import libdwbc_amd as D

    ref = rc.state_set(B, False, "LR")
    n = 8

    def posed(**kw):
        w = _batch(n, **kw)
        w.set_state(ref["q"][:n])
        return w

    w = posed()
    w.set_contact(ref["flags"][:n])
    with pytest.raises(D.DwbcError, match="no torque input"):
        w.redistribute()
    w.set_torque_input(ref["tau_in"][:n])
    with pytest.raises(D.DwbcError, match=r"hqp = true only \(the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque\)"):
        w.redistribute(hqp=False)
    w.redistribute()
    assert (w.get("redist_status") == 1).all()
    w.set_max_active_contacts(3)
    with pytest.raises(D.DwbcError, match="two simultaneously active contacts at most"):
        w.redistribute()
    with pytest.raises(D.DwbcError, match="two simultaneously active contacts at most"):
        w.redistribute_kernel_name()
    w.close()
    f = posed(dtype="f32")
    f.set_contact(ref["flags"][:n])
    f.set_torque_input(ref["tau_in"][:n])
    with pytest.raises(D.DwbcError, match="fp64 batches only"):
        f.redistribute()
    f.close()
