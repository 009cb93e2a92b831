"""-m gpu: the row-broadcast probe (tests/rowbc_probe) in its DEVICE build -- v_fmac_f64_dpp row_newbcast behind ROWBC_FMA / ROWBC_DOT /
ROWBC_AXPY and the two permlane swaps behind ROW_REPLICATE (dwbc_wave.h), each alone on the cases of tests/rowbc_cases.py with 64 and
128 threads per block and one to three blocks, and the 12-pivot sweep of spd_inverse12_lds (dwbc_cycle2p.h) bit for bit against the
LDS-fed sweep it replaces.  The host twin is tests/test_rowbc_emu.py."""
import pytest

from tests import rowbc_cases as rc

pytestmark = pytest.mark.gpu
BUILD = "gpu"
THREADS = pytest.mark.parametrize("threads", [64, 128])


@THREADS
def test_row_replicate(threads):
    rc.check_replicate(BUILD, threads)


@THREADS
def test_rowbc_fma_every_lane_every_row(threads):
    rc.check_fma(BUILD, threads)


@THREADS
@pytest.mark.parametrize("nv", [6, 9, 12])
def test_dz_product(nv, threads):
    rc.check_dz(BUILD, nv, threads)


@THREADS
def test_sweep12_matches_lds_fed_sweep(threads):
    rc.check_sweep(BUILD, threads)
