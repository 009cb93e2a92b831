"""The wave QP solver on its own (libdwbc_amd/csrc/dwbc_qp_wave.h through tests/qp_probe), host build: every case family of tests/qp_cases.py on
every instantiation the product uses, against the canon oracle and the 50-digit reference (tests/qp_reference.py)."""
import numpy as np
import pytest

from tests import qp_cases as qc, qp_reference
from tests.qp_probe import probe

CASES = [pytest.param(inst, fam, id=f"{inst.name}-{fam}") for inst in probe.INSTANTIATIONS for fam in qc.families_of(inst)]


def test_instantiation_table():
    assert tuple(probe.instantiations("emu")) == probe.INSTANTIATIONS
    # the cases and both references scale the contact columns by qp_reference.QP_SCALE in either arithmetic type
    assert all(probe.scale("emu", inst) == qp_reference.QP_SCALE for inst in probe.INSTANTIATIONS)


@pytest.mark.parametrize("inst,family", CASES)
def test_family(inst, family):
    qc.check_family_conditions(family, inst)
    qc.run_family("emu", family, inst)


@pytest.mark.parametrize("ws", [0, 1])
def test_result_does_not_depend_on_nv_bound(ws):
    """the padded entries are exact zeros: one problem through the builds of 6, 9 and 12 variables agrees to the last bit"""
    ps = qc.fam_padding(ws)
    outs = [probe.solve("emu", inst, ps) for inst in probe.INSTANTIATIONS if inst.ws == ws and inst.qn == 12 and not inst.f32]
    assert len(outs) == 3
    for o in outs[1:]:
        for key in outs[0]:
            assert np.array_equal(outs[0][key], o[key]), key
    assert (outs[0]["status"] == 1).all() and (outs[0]["nact"] > 0).any()


def test_probe_refuses_what_it_is_not_built_for():
    qc.check_refusals("emu")
