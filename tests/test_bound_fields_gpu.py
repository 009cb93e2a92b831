"""gpu: every bindable field of the C-ABI bound to a caller-owned device buffer at once (dwbc_batch_bind_device over the buffer slots of
dwbc_capi.hip) against a batch that runs on its own buffers: same inputs, one solve and one redistribution each, outputs bit for bit.
B = 5: odd and more than one instance, so a per-instance stride that is off shows."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

B = 5
INPUTS = ("in_q", "in_contact", "in_fstar", "in_torque")
OUTPUTS = ("tau", "wrench", "status", "redist_tau", "redist_cf", "redist_wrench", "redist_status")


def _batch():
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0)
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    wbc.add_task(0, D.TASK_LINK_6D, 0)
    wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_all_bindable_fields_bound_at_once():
    import torch

    import libdwbc_amd as D
    from libdwbc_amd.batch import FIELDS

    q, flags, fstar = cases.synth_batch(B, seed=23)
    tau_in = np.random.default_rng(23).normal(0.0, 20.0, (B, 33))
    own = _batch()
    own.set_state(q)
    own.set_contact(flags)
    own.set_fstar_all(fstar)
    own.set_torque_input(tau_in)
    own.solve()
    own.redistribute()
    want = {k: own.get(k) for k in OUTPUTS}

    dev = _batch()
    given = dict(in_q=q, in_contact=flags, in_fstar=fstar, in_torque=tau_in)
    like = {**given, **want}
    torch_type = {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}
    t = {}
    for name in INPUTS + OUTPUTS:
        dt = torch_type[like[name].dtype]
        nbytes = dev._L.dwbc_batch_field_bytes(dev._h, FIELDS[name])
        t[name] = torch.zeros(nbytes // like[name].dtype.itemsize, dtype=dt, device="cuda:0")
        assert t[name].numel() == like[name].size, name  # sized by the library, and that is the documented shape
        if name in given:
            t[name].copy_(torch.from_numpy(np.ascontiguousarray(given[name]).reshape(-1)))
        elif dt == torch.float64:
            t[name].fill_(float("nan"))
        dev.bind_tensor(name, t[name])
    torch.cuda.synchronize()
    # what a bound field refuses, word for word
    for call, msg in ((lambda: dev.set_fstar(0, fstar[:, :6]), "f* is bound to a device buffer"),
                      (lambda: dev.set_torque_input(tau_in), "the torque input is bound to a device buffer"),
                      (lambda: dev.set_max_active_contacts(3), "wrench is bound to a device buffer: set the contact capacity before binding")):
        with pytest.raises(D.DwbcError) as e:
            call()
        assert str(e.value) == msg
    dev.solve()
    dev.redistribute()
    dev.sync()
    for name in OUTPUTS:
        got = t[name].cpu().numpy().reshape(want[name].shape)
        assert _same_bits(got, want[name]), name
        assert _same_bits(dev.get(name), want[name]), name  # get() reads the bound buffer
    for name in INPUTS:
        assert _same_bits(dev.get(name), np.ascontiguousarray(given[name])), name

    # rebinding: the second tensor is written from now on, the first is left alone
    first, second = t["tau"], torch.full_like(t["tau"], float("nan"))
    first.fill_(7.0)
    torch.cuda.synchronize()
    dev.bind_tensor("tau", second)
    dev.solve()
    dev.sync()
    assert _same_bits(second.cpu().numpy().reshape(want["tau"].shape), want["tau"])
    assert (first.cpu().numpy() == 7.0).all()

    own.close()
    dev.close()
    torch.cuda.synchronize()
    assert (first.cpu().numpy() == 7.0).all() and _same_bits(t["in_q"].cpu().numpy().reshape(q.shape), q)  # the caller's memory is still the caller's
