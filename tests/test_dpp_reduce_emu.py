"""The cases of tests/dpp_reduce_cases.py through the HOST builds of the wave probe and the row-broadcast probe: validates the cases and
their numpy expectations on the emulation twins of WAVE_ARGMIN_F32, WAVE_ARGMIN_ROW1, ROW_REPLICATE and ROWBC_DOT.  The device twin is
tests/test_dpp_reduce_gpu.py."""
import pytest

from tests import dpp_reduce_cases as dc

BUILD = "emu"


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_argmin_forms(f32):
    assert dc.check_argmin(BUILD, f32) <= 1024


def test_replicate():
    assert dc.check_replicate(BUILD) <= 1024


@pytest.mark.parametrize("nv", [6, 9, 12])
def test_replicate_then_dot(nv):
    assert dc.check_replicate_dot(BUILD, nv) <= 1024
