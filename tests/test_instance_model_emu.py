"""not-gpu: the per-instance-model build of the kernels on the host (tests/emu/emu_inst_model.cpp, compiled with DWBC_INST_MODEL as the
dwbc_im:: translation units of the library are): the cycle -- extras, compact lean and two-wave build -- and the dynamics kernel at B = 6
against the restatement with instance i's own model, and the premises of every comparison of the GPU tests on the restatement alone.

Two mutations of DWBC_BODY (dwbc_types.h) are built here as well and must miss the dynamics comparison: a stride of (nb - 1) * kBodyStride
and an offset that ignores `inst`.  Recipe, references and bars: tests/instance_model_cases.py, tests/dynamics_cases.py."""
import numpy as np
import pytest

from tests import cases
from tests import dynamics_cases as dc
from tests import instance_model_cases as im
from tests.emu import emu_inst_model as emu

N = 6  # the first six instances of the recipe's 24


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_premises_hold_on_the_restatement(levels):
    """what every comparison of the GPU tests asserts first, here once on the CPU: the restatement solves the instances and the record
    moves them"""
    for state in im.SETS:
        if im.exists(levels, state):
            im.check_premises(im.reference(levels, state), im.shared_reference(levels, state), f"L = {levels}, {state}")


def _first(ref):
    return tuple(a[:N] for a in ref)


@pytest.mark.parametrize("build,levels", [(emu.EXTRAS, 2), (emu.COMPACT, 2), (emu.TWO_WAVE, 2), (emu.COMPACT, 4), (emu.EXTRAS, 3)])
def test_cycle_reads_the_instances_own_table(build, levels):
    state = "yaw" if levels == 3 else "mixed"
    tasks, q, flags, fstar = im.states(levels, state)
    ref, base = _first(im.reference(levels, state)), _first(im.shared_reference(levels, state))
    moved = np.abs(ref[0].sum(axis=1) - base[0].sum(axis=1)).max(axis=1)
    assert (moved > im.MOVED).sum() >= N // 2, moved
    got = emu.cycle(im.base_arrays(), cases.CONTACTS_2, tasks, cases.TAU_LIM, im.tables()[:N], q[:N], flags[:N], fstar[:N], build=build)
    im.compare(got["tau"], got["wrench"], got["status"], ref, f"emulation, build {build}, L = {levels}")


def _dyn_reference():
    _, q, _, _ = im.states(2, "yaw")
    qd = dc.velocities(N, 39)
    outs = [dc.reference(im.arrays(i), q[i : i + 1], qd[i : i + 1]) for i in range(N)]
    return q[:N], qd, {k: np.concatenate([o[k] for o in outs]) for k in dc.NAMES}


def _dyn_errors(got, ref):
    return {k: float(np.abs(got[k] - ref[k]).max()) for k in dc.NAMES}


def test_dynamics_reads_the_instances_own_table():
    q, qd, ref = _dyn_reference()
    got = emu.dynamics(im.base_arrays(), im.tables()[:N], q, qd)
    assert (got["status"] == 1).all()
    errs = _dyn_errors(got, ref)
    print("dynamics, per-instance tables: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in dc.NAMES:
        assert errs[k] <= dc.BARS[k], (k, errs[k])
    # the record moves the answer: against the shared model's mass matrix every instance differs by far more than the bar
    shared = dc.reference(im.base_arrays(), q, qd)
    assert (np.abs(shared["A"] - ref["A"]).max(axis=(1, 2)) > 1e3 * dc.BARS["A"]).all()


@pytest.mark.parametrize("mutant", sorted(emu.MUTANTS))
def test_a_wrong_offset_misses_the_dynamics_comparison(mutant):
    """the comparison above on a build whose DWBC_BODY is wrong: instance 0 (offset 0 either way) still passes, the others miss the bar of
    A by orders of magnitude"""
    q, qd, ref = _dyn_reference()
    got = emu.dynamics(im.base_arrays(), im.tables()[:N], q, qd, mutant=mutant)
    e = np.abs(got["A"] - ref["A"]).reshape(N, -1)
    e = np.where(np.isfinite(e), e, np.inf).max(axis=1)
    print(f"{mutant}: |d A| per instance = " + ", ".join(f"{v:.2e}" for v in e))
    assert e[0] <= dc.BARS["A"]
    assert (e[1:] > 1e3 * dc.BARS["A"]).all(), e
