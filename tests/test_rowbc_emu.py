"""The row-broadcast probe (tests/rowbc_probe) in its HOST build: the DWBC_HOST_EMU forms of ROW_REPLICATE, ROWBC_FMA and ROWBC_DOT
(dwbc_wave.h) on the cases of tests/rowbc_cases.py -- the forms the host emulation of qp_solve_wave runs.  The 12-pivot sweep is device
text (the host emulation of spd_inverse12_lds is spd_inverse_small): the probe refuses it here.  The device twin is
tests/test_rowbc_gpu.py."""
import numpy as np
import pytest

from tests import rowbc_cases as rc
from tests.rowbc_probe import probe

BUILD = "emu"
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


def test_entry_refuses_what_it_cannot_run():
    x = np.zeros((1, 64))
    for kind, threads, din in ((6, 64, x), (-1, 64, x), (0, 32, x), (0, 256, x), (probe.SWEEP, 64, np.zeros((1, 144)))):
        out = np.full((1, 512), probe.SENTINEL)
        L = probe.lib(BUILD)
        assert L.rowbc_probe_run(kind, threads, 1, din.ctypes.data, din.size, out.ctypes.data, out.size) == 0
        assert L.rowbc_probe_error() and (out == probe.SENTINEL).all()
    with pytest.raises(AssertionError):
        probe.run(BUILD, probe.FMA, x)  # (record of the wrong size: caught by the loader)
    out = np.full((1, 63), probe.SENTINEL)
    assert probe.lib(BUILD).rowbc_probe_run(0, 64, 1, x.ctypes.data, x.size, out.ctypes.data, out.size) == 0
