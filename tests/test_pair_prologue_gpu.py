"""-m gpu: the two-wave kernel's request phase on the device (dwbc_cycle2p.h): the cases of tests/pair_prologue_cases.py at B = 1, 3 and
5 -- odd per-instance strides, first and last instance -- with in_contact, in_q and in_fstar bound as contiguous views into the
middle of larger device buffers: the flags view starts at an odd byte offset between bytes set to 1, the q and f* views sit between
NaNs.  A flag, a q entry or an f* entry taken from outside an instance's own range changes an answer: a neighbouring flag raises a
contact (or refuses the instance), a NaN reaches the torques.  Every flag pattern visits every instance of the batch, the last one
included."""
import numpy as np
import pytest

from tests import cases
from tests import pair_prologue_cases as pc

pytestmark = pytest.mark.gpu

SWITCHES = ("DWBC_NO_WIDE", "DWBC_NO_PAIR", "DWBC_NO_LEAN", "DWBC_DENSE_SWEEP", "DWBC_PAIR_ALWAYS")
TWO_WAVE = "dwbc::dwbc_cycle_kernel_v2p<39, 34, 2, dwbc::TopoTocabi>"
PAD_FLAGS, PAD_Q, PAD_FSTAR = 7, 5, 3  # elements in front of the views: an odd byte offset, 8-byte but not 16-byte aligned rows


def _view(torch, n, pad, dtype, fill):
    big = torch.full((pad + n + pad,), fill, dtype=dtype, device="cuda:0")
    return big, big[pad : pad + n]


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n", pc.DECLARED)
def test_two_wave_cycle_on_views_between_poisoned_neighbours(n, B, monkeypatch):
    import torch

    import libdwbc_amd as D

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    q, fstar = pc.states()
    pat = pc.patterns(n)
    P = len(pat)
    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0)
    for c in cases.CONTACTS_4[:n]:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(cases.TASKS_2LEVEL):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    big_f, v_f = _view(torch, B * n, PAD_FLAGS, torch.uint8, 1)
    big_q, v_q = _view(torch, B * q.shape[1], PAD_Q, torch.float64, float("nan"))
    big_s, v_s = _view(torch, B * fstar.shape[1], PAD_FSTAR, torch.float64, float("nan"))
    assert v_f.data_ptr() % 2 == 1 and v_q.data_ptr() % 16 == 8
    si = np.arange(B) % pc.NSTATES
    v_q.copy_(torch.from_numpy(np.ascontiguousarray(q[si]).reshape(-1)))
    v_s.copy_(torch.from_numpy(np.ascontiguousarray(fstar[si]).reshape(-1)))
    for name, v in (("in_contact", v_f), ("in_q", v_q), ("in_fstar", v_s)):
        wbc.bind_tensor(name, v)
    for shift in range(P):  # every pattern on every instance of the batch
        pi = (np.arange(B) + shift) % P
        v_f.copy_(torch.from_numpy(np.ascontiguousarray(pat[pi]).reshape(-1)))
        torch.cuda.synchronize()
        wbc.solve()
        assert wbc.kernel_name() == TWO_WAVE, wbc.kernel_name()
        pc.check(f"gpu[{n} declared, B = {B}, shift {shift}]", n, pi, si, wbc.get("tau"), wbc.get("wrench"), wbc.get("status"))
    # the neighbours are what they were
    assert (big_f[:PAD_FLAGS] == 1).all() and (big_f[PAD_FLAGS + B * n :] == 1).all()
    assert torch.isnan(big_q[:PAD_Q]).all() and torch.isnan(big_q[PAD_Q + B * q.shape[1] :]).all()
    assert torch.isnan(big_s[:PAD_FSTAR]).all() and torch.isnan(big_s[PAD_FSTAR + B * fstar.shape[1] :]).all()
    wbc.close()
