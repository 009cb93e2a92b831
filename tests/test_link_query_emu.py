"""not-gpu: the link-query kernel source (libdwbc_amd/csrc/dwbc_link_query.h) compiled for the host (tests/emu/emu_link_query.cpp: LDS
poisoned with NaN before every instance) against the numpy restatement: Q7 with and without Jacobians, no qdot, one entry, sixteen, the
identity Jacobian . qdot = velocity, and the foot Jacobians against the golden J_C of reference CASE 1."""
import numpy as np

from tests import cases
from tests import link_query_cases as lqc
from tests.emu import emu_link_query as emu

B = 6


def _q7(jacobians=True, qdot=True):
    q, qd, _ = lqc.state_set(B)
    return emu.run(cases.URDF, q, qd if qdot else None, lqc.Q7_LINKS, lqc.Q7_POINTS, jacobians)


def test_lds_map_is_small():
    assert emu.lds_bytes() == 13152  # far below the compact cycle map's 20 432 B: twelve workgroups per CU


def test_premise_jacobian_times_qdot_is_the_velocity():
    """asserted on the restatement first: point_jacobian(...) @ qd equals [v at the point; w] of link_velocities"""
    q, qd, ref = lqc.state_set(B)
    link = np.asarray(lqc.Q7_LINKS) != lqc.COM
    e = np.abs(np.einsum("beij,bj->bei", ref["jac"][:, link], qd) - ref["vel"][:, link]).max()
    print(f"restatement: worst |J qd - vel| = {e:.3e}")
    assert e <= lqc.TOL_VEL, e
    assert np.abs(ref["vel"]).max() > 0.1  # the rates move the links


def test_q7_with_jacobians():
    _, qd, ref = lqc.state_set(B)
    got = _q7()
    assert not any(np.isnan(v).any() for v in got.values())
    lqc.compare(got, ref, lqc.Q7_LINKS)
    # the same identity on the kernel's own outputs (every entry: the COM's velocity is jac_com_ qdot by definition)
    e = np.abs(np.einsum("beij,bj->bei", got["jac"], qd) - got["vel"]).max()
    print(f"kernel: worst |J qd - vel| = {e:.3e}")
    assert e <= lqc.TOL_VEL, e


def test_q7_without_jacobians_is_bit_equal():
    _, _, ref = lqc.state_set(B)
    with_j, without = _q7(), _q7(jacobians=False)
    assert "jac" not in without
    lqc.compare(without, ref, lqc.Q7_LINKS, jac=False)
    for k in ("pos", "rot", "vel"):
        assert (with_j[k] == without[k]).all(), k


def test_no_qdot_means_zero_velocity():
    with_qd, without = _q7(), _q7(qdot=False)
    assert (without["vel"] == 0.0).all()
    for k in ("pos", "rot", "jac"):
        assert (with_qd[k] == without[k]).all(), k


def test_one_entry_and_sixteen():
    q, qd, ref = lqc.state_set(B)
    for e, (l, pt) in enumerate(zip(lqc.Q7_LINKS, lqc.Q7_POINTS)):  # each entry of Q7 alone, the COM among them
        got = emu.run(cases.URDF, q, qd, [l], [pt], True)
        lqc.compare(got, {k: v[:, e : e + 1] for k, v in ref.items()}, [l])
    links, points = lqc.q16()
    assert len(links) == 16
    got = emu.run(cases.URDF, q, qd, links, points, True)
    assert not any(np.isnan(v).any() for v in got.values())
    lqc.compare(got, lqc.reference(q, qd, links, points), links)
    q7 = _q7()
    for k in q7:  # the first seven entries are Q7 itself: what else is asked changes nothing
        assert (got[k][:, :7] == q7[k]).all(), k


def test_foot_jacobians_are_the_golden_j_c():
    """the state of reference CASE 1 (tests/dwbc_test.cpp): the Jacobians of the two foot entries are the fixture's J_C rows"""
    q = np.array(cases.Q_CASE[1], dtype=np.float64)[None, :]
    got = emu.run(cases.URDF, q, None, lqc.Q7_LINKS, lqc.Q7_POINTS, True)
    J_C = cases.golden(1, "J_C")
    assert J_C.shape == (12, 39)
    e = max(np.abs(got["jac"][0, 1] - J_C[:6]).max(), np.abs(got["jac"][0, 2] - J_C[6:]).max())
    print(f"worst |J_foot - golden J_C| = {e:.3e}")
    assert e <= lqc.TOL_JAC, e
