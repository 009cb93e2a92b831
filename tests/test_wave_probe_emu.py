"""The wave-routine probe (tests/wave_probe) in its HOST build: every case of tests/wave_cases.py through the host side of the
DWBC_HOST_EMU forks and the 50-digit references.  This validates the cases and the references, pins the host forms the whole
-m "not gpu" suite trusts (the tie rules of the arg-min among them), and is where the committed bars of the inverses come from
(profiles/wave_probe_tolerances.txt).  The device twin is tests/test_wave_probe_gpu.py."""
import os

import pytest

from tests import wave_cases as wc
from tests.wave_probe import probe

BUILD = "emu"


def test_instantiation_table_holds_every_family():
    t = probe.table(BUILD)
    names = ["lanes", "lanes_f32", "math", "math_f32"] + [g[0] for g in wc.GEMM_INSTS] + list(wc.DOT_INSTS) + list(wc.AXPY_INSTS)
    names += list(wc.SWEEP_INSTS) + list(wc.SMALL_INSTS) + list(wc.GC_INVERSE_INSTS) + list(wc.MMG_INSTS) + list(wc.TILE_INSTS)
    assert sorted(t) == sorted(names)


def test_entry_refuses_out_of_range_sizes():
    wc.check_lanes_refusals(BUILD)


def test_general_contact_routines_refuse_out_of_range_sizes():
    wc.check_gc_refusals(BUILD)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_cross_lane_primitives(f32):
    wc.check_lanes(BUILD, f32)


@pytest.mark.parametrize("op", [0, 1], ids=["fast_rcp", "fast_rsqrt"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_rcp_rsqrt(f32, op):
    wc.check_rcp_rsqrt(BUILD, f32, op)


def test_sincos():
    wc.check_sincos(BUILD)


@pytest.mark.parametrize("inst", wc.GEMM_INSTS, ids=[g[0] for g in wc.GEMM_INSTS])
def test_wave_gemm(inst):
    wc.check_gemm(BUILD, *inst)


def test_wave_gemm_unit_matrices():
    wc.check_gemm_units(BUILD)


@pytest.mark.parametrize("name", list(wc.DOT_INSTS))
def test_lds_rows_dot(name):
    wc.check_rows_dot(BUILD, name)


@pytest.mark.parametrize("name", list(wc.AXPY_INSTS))
def test_lds_rows_axpy(name):
    wc.check_rows_axpy(BUILD, name)


@pytest.mark.parametrize("name", list(wc.SWEEP_INSTS) + list(wc.SMALL_INSTS))
def test_inverse(name):
    wc.check_inverse(BUILD, name)


@pytest.mark.parametrize("t", wc.PINV_TS)
def test_pinv_cod(t):
    """pinv_cod_small / qr_small at every (t, rank).  With the second permutation list at vec + 6 (before it moved to vec + t) the
    cases of t >= 7 failed here -- |M P M - M| up to 1e4 -- and those of t <= 6 passed: the test fails where that bug was and only there"""
    wc.check_pinv_cod(BUILD, (t,))


@pytest.mark.parametrize("name", list(wc.GJ_INSTS))
def test_gj_inverse_rows(name):
    wc.check_gj_rows(BUILD, name)


@pytest.mark.parametrize("name", list(wc.SPD_REG_INSTS))
def test_spd_inverse_reg(name):
    wc.check_spd_reg(BUILD, name)


def test_spd_inverse_scaled():
    wc.check_spd_scaled(BUILD)


@pytest.mark.parametrize("name", list(wc.MMG_INSTS))
def test_mmg(name):
    wc.check_mmg(BUILD, name)


@pytest.mark.parametrize("name", list(wc.GRAM_INSTS))
def test_contact_gram(name):
    """contact_gram (dwbc_cycle2.h: J A^-1 J^T = Y J_C^T of stage 1, of the redistribution and of the gravity compensation) alone: K
    padding with 0 to 3 masked lane groups, cd = 6 and 12, the unit sweep over every (i, j) and one reduction index per K step"""
    wc.check_gram(BUILD, name)


@pytest.mark.parametrize("name", list(wc.WRENCH_INSTS))
def test_wrench_maps(name):
    """wrench_maps (dwbc_cycle2.h) alone over every hierarchy of wave_cases.WRENCH_HIER: col_src against a restatement written from the
    comment above the function, K padding, partial tiles, one contact with NaN in the stale operands"""
    wc.check_wrench(BUILD, name)


def test_wrench_maps_layout():
    wc.check_wrench_layout(BUILD)


def test_committed_tolerances_are_the_host_figures(tmp_path):
    """the committed bars are what --write-tolerances gives today (a change of the cases or of the host forms must renew the file).
    Within a factor of two: the condition number in g comes from LAPACK and the host forms from libm, whose last bits differ between
    machines, and a bar is 10 x its figure"""
    path = os.path.join(tmp_path, "tol.txt")
    wc.write_tolerances(path)

    def table(p):
        with open(p) as f:
            return {w[0]: (float(w[1]), int(w[3])) for w in (line.split() for line in f if not line.startswith("#"))}

    new, old = table(path), table(wc.TOL_FILE)
    assert sorted(new) == sorted(old)
    for name in new:
        assert new[name][1] == old[name][1], (name, "number of cases")
        assert 0.5 * old[name][0] <= new[name][0] <= 2.0 * old[name][0], (name, new[name], old[name])
