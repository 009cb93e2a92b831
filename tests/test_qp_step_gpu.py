"""-m gpu: the batches of tests/qp_step_cases.py through the HIP kernels (the C-ABI): the two-wave kernel that runs the bench line, the
compact kernel (DWBC_NO_WIDE) and the general-contact kernel, against the oracle -- torques, wrench, status and the steps of every QP.
The host-emulation twin is tests/test_qp_step_emu.py."""
import numpy as np
import pytest

from tests import cases
from tests import qp_step_cases as qs

pytestmark = pytest.mark.gpu


def _solve(q, fl, fs, contacts=cases.CONTACTS_2, max_active=2):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), len(q), device=0)
    for c in contacts:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    for lv, links in enumerate(cases.TASKS_2LEVEL):
        for mode, link, pt in links:
            wbc.add_task(lv, mode, link, pt)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    if max_active > 2:
        wbc.set_max_active_contacts(max_active)
    wbc.set_state(q)
    wbc.set_contact(fl)
    wbc.set_fstar_all(fs)
    wbc.solve()
    return dict(tau=wbc.get("tau"), wrench=wbc.get("wrench"), status=wbc.get("status"), diag=wbc.get("diag")), wbc.kernel_name()


@pytest.mark.parametrize("kernel", ["two_wave", "compact"])
@pytest.mark.parametrize("batch", ["paths", "tilted"])
def test_gpu_step_paths_vs_oracle(batch, kernel, monkeypatch):
    if kernel == "compact":
        monkeypatch.setenv("DWBC_NO_WIDE", "1")
    if batch == "paths":
        (q, fl, fs), ref, _ = qs.paths_batch()
    else:
        (q, fl, fs), ref = qs.tilted_batch()
        assert (ref["status"] == 1).mean() > 0.9
    r, name = _solve(q, fl, fs)
    assert ("dwbc_cycle_kernel_v2p<" if kernel == "two_wave" else "dwbc_cycle_kernel_v2<") in name, name
    qs.check(f"{batch}[{kernel}]", r, ref)


def test_gpu_step_general_contact_kernel_vs_oracle():
    (q, fl, fs), ref = qs.gc_batch(64)
    r, name = _solve(q, fl, fs, contacts=cases.CONTACTS_4, max_active=3)
    assert "dwbc_cycle_kernel_gc<39, 34, 64, 6>" in name, name
    assert (ref["status"] == 1).mean() > 0.9 and ref["steps"][:, 0].max() > 0
    qs.check("gc", r, ref, ncols=18)
