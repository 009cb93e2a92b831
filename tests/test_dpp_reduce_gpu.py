"""-m gpu: the cases of tests/dpp_reduce_cases.py through the DEVICE builds of the wave probe and the row-broadcast probe: the
one-instruction DPP minima behind WAVE_ARGMIN_F32 (v_min_f32 with row shifts and row broadcasts) and WAVE_ARGMIN_ROW1 (two stages of
v_min_u32 over the high and the low word of the key), and the single-statement ROW_REPLICATE in front of ROWBC_DOT, with 64 and with
128 threads per block.  One wavefront per case, one launch per test; expectations from numpy.  The host twin is
tests/test_dpp_reduce_emu.py."""
import pytest

from tests import dpp_reduce_cases as dc

pytestmark = pytest.mark.gpu
BUILD = "gpu"
THREADS = pytest.mark.parametrize("threads", [64, 128])


@THREADS
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_argmin_forms(f32, threads):
    assert dc.check_argmin(BUILD, f32, threads) <= 1024


@THREADS
def test_replicate(threads):
    assert dc.check_replicate(BUILD, threads) <= 1024


@THREADS
@pytest.mark.parametrize("nv", [6, 9, 12])
def test_replicate_then_dot(nv, threads):
    assert dc.check_replicate_dot(BUILD, nv, threads) <= 1024
