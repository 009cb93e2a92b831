"""not-gpu: the redistribution kernel (libdwbc_amd/csrc/dwbc_redistribute.h) on TopoGeneric at the sizes the kernel packs and the built-in
generic row are built for -- (23, 18), (37, 32), (43, 38), (39, 34) -- in host emulation (tests/emu/emu_redist_sizes.cpp: one "thread" per
workgroup, LDS of exactly LdsRd<N, NB>::total doubles NaN-poisoned before every instance, a guard behind it) against the numpy restatement.

Inputs, flag mix and premises: tests/redist_pack_cases.py; bars: tests/redist_cases.py (1e-6 Nm, 1e-5 N)."""
import numpy as np
import pytest

from tests import cases
from tests import redist_cases as rc
from tests import redist_pack_cases as pc
from tests.emu import emu_redist_sizes as ers

# LdsRd<N, NB>::total_bytes as DESIGN.md section 5 lists them ("Redistribution of a caller-supplied torque")
LDS_BYTES = {23: 12880, 37: 19488, 39: 20432, 43: 22320, 50: 26792}
CASES = [("fixed_arms", 16), ("fixed_head", 16), ("surgery_43", 8), ("tocabi", 16)]


@pytest.mark.parametrize("name,B", CASES, ids=[c[0] for c in CASES])
def test_emulation_matches_restatement_at_pack_sizes(name, B):
    ref = pc.state_set(name, B)
    rc.check_premises(ref)
    mo, links = pc.model(name)
    got = ers.run(mo, pc.contacts_of(links), np.full(mo["ndof"] - 6, pc.TAU_LIM), ref["q"], ref["flags"], ref["tau_in"])
    for k in ("tau", "cf", "wrench"):
        assert np.isfinite(got[k]).all(), k
    rc.compare(got, ref)
    pc.check_flag_mix_outputs(got, ref)


def test_generic_tree_agrees_with_the_constant_tree_on_tocabi():
    """(39, 34, TopoGeneric) -- the dense runtime-pivot sweep, tree and body count read at run time -- against the existing emulation of the
    TOCABI-tree kernel on the same states"""
    from tests.emu.emu import Emu

    ref = rc.state_set(32, True, "mixed")
    tree = Emu(cases.URDF, cases.CONTACTS_2, (), cases.TAU_LIM).run_redist(ref["q"], ref["flags"], ref["tau_in"])
    mo = cases.tocabi_model()
    gen = ers.run(mo, cases.CONTACTS_2, cases.TAU_LIM, ref["q"], ref["flags"], ref["tau_in"])
    assert (gen["status"] == tree["status"]).all() and tree["status"].sum() >= 0.9 * 32
    e = float(np.abs(gen["tau"] - tree["tau"]).max())
    print(f"worst |tau generic - tau tree| = {e:.3e} Nm")
    assert e <= 1e-9
    rc.compare(gen, ref)


@pytest.mark.parametrize("n", sorted(LDS_BYTES))
def test_lds_bytes_are_the_documented_ones(n):
    assert ers.lds_bytes(n) == LDS_BYTES[n]
