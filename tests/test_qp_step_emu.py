"""The active-set step of the wave QP solver (libdwbc_amd/csrc/dwbc_qp_wave.h) through the host build of the same header: the batches of
tests/qp_step_cases.py -- every step count the bench's states produce, adds and drops, the second projection on tilted feet, the
18-variable instantiation -- against the oracle: torques, wrench, status, and the number of steps of every QP (the search must take the
oracle's path: most violated row first, the same ratio test, the same working set)."""
import pytest

from tests import cases
from tests import qp_step_cases as qs
from tests.emu.emu import Emu


def test_paths_batch_holds_every_step_count_of_the_bench_states():
    _, ref, hist = qs.paths_batch()
    print("steps over the 1024 bench states:", hist)
    for col, counts in ((0, qs.L0_STEPS), (1, qs.L1_STEPS)):
        for c in counts:
            assert (ref["steps"][:, col] == c).sum() >= min(qs.PER_CLASS, hist[f"level{col}"][c])
    assert ref["status"].all() and (ref["steps"][:, 2] == 0).all()  # (the redistribution has nothing to do on these states)


@pytest.mark.parametrize("build", ["pair", True, False])
def test_emulated_step_paths_vs_oracle(build):
    """build: the two-wave kernel (the bench line), the compact kernel, the full one-wave build (which reports its working sets)"""
    (q, fl, fs), ref, _ = qs.paths_batch()
    r = Emu(cases.URDF, cases.CONTACTS_2, cases.TASKS_2LEVEL, cases.TAU_LIM).run(q, fl, fs, compact=build)
    qs.check(f"paths[{build}]", r, ref)


@pytest.mark.parametrize("build", ["pair", True])
def test_emulated_step_tilted_feet_vs_oracle(build):
    (q, fl, fs), ref = qs.tilted_batch()
    r = Emu(cases.URDF, cases.CONTACTS_2, cases.TASKS_2LEVEL, cases.TAU_LIM).run(q, fl, fs, compact=build)
    assert (ref["status"] == 1).mean() > 0.9
    qs.check(f"tilted[{build}]", r, ref)


def test_emulated_step_general_contact_kernel_vs_oracle():
    (q, fl, fs), ref = qs.gc_batch(16)
    r = Emu(cases.URDF, cases.CONTACTS_4, cases.TASKS_2LEVEL, cases.TAU_LIM).run_gc(q, fl, fs)
    assert (ref["status"] == 1).mean() > 0.9 and ref["steps"][:, 0].max() > 0
    qs.check("gc", r, ref, ncols=18)
