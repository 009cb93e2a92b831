"""The wave QP solver on its own, GPU build of the probe (tests/qp_probe: one wavefront per problem): the cases and the check of
test_qp_wave_emu.py, with 64 and with 128 threads per block (the two-wave cycle runs the solver in a 128-thread block).  The bars come from
the host build and the references (profiles/qp_probe_tolerances.txt), never from GPU output.  One launch per family and instantiation;
the probe bounds max_iter, so no case can spin."""
import pytest

from tests import qp_cases as qc, qp_reference
from tests.qp_probe import probe

pytestmark = pytest.mark.gpu

CASES = [pytest.param(inst, fam, id=f"{inst.name}-{fam}") for inst in probe.INSTANTIATIONS for fam in qc.families_of(inst)]


def test_instantiation_table():
    assert tuple(probe.instantiations("gpu")) == probe.INSTANTIATIONS
    # the cases and both references scale the contact columns by qp_reference.QP_SCALE in either arithmetic type
    assert all(probe.scale("gpu", inst) == qp_reference.QP_SCALE for inst in probe.INSTANTIATIONS)


@pytest.mark.parametrize("threads", [64, 128])
@pytest.mark.parametrize("inst,family", CASES)
def test_family(inst, family, threads):
    qc.run_family("gpu", family, inst, threads, label=f"[{threads} threads] ")


def test_probe_refuses_what_it_is_not_built_for():
    qc.check_refusals("gpu")
