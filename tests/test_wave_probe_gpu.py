"""-m gpu: the wave-routine probe (tests/wave_probe) in its DEVICE build -- the bodies that ship behind the DWBC_HOST_EMU forks (DPP
reductions and scans, v_readlane broadcasts, fast_rcp / fast_rsqrt / sincos_r, wave_gemm on the matrix cores, the LDS-fed sweeps,
spd_inverse12_lds, the three-group Cholesky inverse, the hand-batched row products, and the general-contact kernel's pinv_cod_small,
gj_inverse_rows, spd_inverse_reg, spd_inverse_scaled and mmg, and the two in-place matrix-core tiles of the cycle, contact_gram and
wrench_maps), each alone on the cases and against the 50-digit
references of tests/wave_cases.py, with 64 and with 128 threads per block (the two-wave kernel runs them in wave 1).  One launch per
instantiation.  The host twin, which validates the same cases and references, is tests/test_wave_probe_emu.py."""
import pytest

from tests import wave_cases as wc
from tests.wave_probe import probe

pytestmark = pytest.mark.gpu
BUILD = "gpu"
THREADS = pytest.mark.parametrize("threads", [64, 128])


def test_instantiation_table_holds_every_family():
    names = ["lanes", "lanes_f32", "math", "math_f32"] + [g[0] for g in wc.GEMM_INSTS] + list(wc.DOT_INSTS) + list(wc.AXPY_INSTS)
    names += list(wc.SWEEP_INSTS) + list(wc.SMALL_INSTS) + list(wc.GC_INVERSE_INSTS) + list(wc.MMG_INSTS) + list(wc.TILE_INSTS)
    assert sorted(probe.table(BUILD)) == sorted(names)


def test_entry_refuses_out_of_range_sizes():
    wc.check_lanes_refusals(BUILD)


def test_general_contact_routines_refuse_out_of_range_sizes():
    wc.check_gc_refusals(BUILD)


@THREADS
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_cross_lane_primitives(f32, threads):
    wc.check_lanes(BUILD, f32, threads)


@THREADS
@pytest.mark.parametrize("op", [0, 1], ids=["fast_rcp", "fast_rsqrt"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_rcp_rsqrt(f32, op, threads):
    wc.check_rcp_rsqrt(BUILD, f32, op, threads)


@THREADS
def test_sincos(threads):
    wc.check_sincos(BUILD, threads)


@THREADS
@pytest.mark.parametrize("inst", wc.GEMM_INSTS, ids=[g[0] for g in wc.GEMM_INSTS])
def test_wave_gemm(inst, threads):
    wc.check_gemm(BUILD, *inst, threads)


@THREADS
def test_wave_gemm_unit_matrices(threads):
    wc.check_gemm_units(BUILD, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.DOT_INSTS))
def test_lds_rows_dot(name, threads):
    wc.check_rows_dot(BUILD, name, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.AXPY_INSTS))
def test_lds_rows_axpy(name, threads):
    wc.check_rows_axpy(BUILD, name, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.SWEEP_INSTS) + list(wc.SMALL_INSTS))
def test_inverse(name, threads):
    wc.check_inverse(BUILD, name, threads)


@THREADS
@pytest.mark.parametrize("t", wc.PINV_TS)
def test_pinv_cod(t, threads):
    """pinv_cod_small / qr_small at every (t, rank): t > 6 is the general-contact kernel's TG = 12 build"""
    wc.check_pinv_cod(BUILD, (t,), threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.GJ_INSTS))
def test_gj_inverse_rows(name, threads):
    wc.check_gj_rows(BUILD, name, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.SPD_REG_INSTS))
def test_spd_inverse_reg(name, threads):
    """spd_inverse_reg in place through both feeds.  spd_reg39_lds is the case that found the pivot-lane defect of the LDS-fed sweep
    (lds_pivot, dwbc_cycle2.h): with the pivot lane forming own - other (1 - 1/d) from the gathered column it scored g = 194.8
    against the bar of 12.25 on the synthetic matrix with pivots near 1e3 (errors in X[i][j], i > j, only: u |A_ij| undivided);
    spd_inverse_reg now has the pivot lane scale its own copy."""
    wc.check_spd_reg(BUILD, name, threads)


@THREADS
def test_spd_inverse_scaled(threads):
    wc.check_spd_scaled(BUILD, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.MMG_INSTS))
def test_mmg(name, threads):
    wc.check_mmg(BUILD, name, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.GRAM_INSTS))
def test_contact_gram(name, threads):
    """contact_gram (dwbc_cycle2.h: J A^-1 J^T = Y J_C^T of stage 1, of the redistribution and of the gravity compensation) alone: K
    padding with 0 to 3 masked lane groups, cd = 6 and 12, the unit sweep over every (i, j) and one reduction index per K step"""
    wc.check_gram(BUILD, name, threads)


@THREADS
@pytest.mark.parametrize("name", list(wc.WRENCH_INSTS))
def test_wrench_maps(name, threads):
    """wrench_maps (dwbc_cycle2.h) alone over every hierarchy of wave_cases.WRENCH_HIER: col_src against a restatement written from the
    comment above the function, K padding, partial tiles, one contact with NaN in the stale operands"""
    wc.check_wrench(BUILD, name, threads)


@THREADS
def test_wrench_maps_layout(threads):
    wc.check_wrench_layout(BUILD, threads)
