"""Queries, bars and restatement references of the link-query tests (tests/test_link_query_*.py), computed once per state set.

Q7 is what the reference's harnesses read between UpdateKinematics and SetTaskSpace: the pelvis, both feet at their contact points, the
upper body, both hands at their origins and the synthetic COM link.  The reference of an entry is oracle/dwbc_np.py's own restatement:
forward_kinematics, point_jacobian, link_velocities and Cycle.update_kinematics (com, J_com)."""
import functools

import numpy as np

from tests import cases

COM = 34  # model.link_id("COM") of TOCABI: the body count
Q7_LINKS = (0, 6, 12, 15, 23, 33, COM)
Q7_POINTS = ((0, 0, 0), cases.CONTACTS_2[0]["point"], cases.CONTACTS_2[1]["point"], (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0))
# the project's own bars: com on the device (pos, rot), link_v / link_w (vel), golden J_C on the GPU (link Jacobians), J_com (COM Jacobian)
TOL_POS = TOL_ROT = 1e-12
TOL_VEL = 1e-11
TOL_JAC = 1e-12
TOL_JAC_COM = 1e-10


def q16():
    """16 entries: Q7 twice with other points on the links (the COM takes none), then the pelvis and the upper body once more"""
    rng = np.random.default_rng(16)
    links = list(Q7_LINKS) + list(Q7_LINKS) + [0, 15]
    points = [list(p) for p in Q7_POINTS] + [[0.0] * 3 if l == COM else list(rng.uniform(-0.2, 0.2, 3)) for l in Q7_LINKS] + [list(rng.uniform(-0.2, 0.2, 3)) for _ in range(2)]
    return tuple(links), tuple(tuple(p) for p in points)


def reference(q, qd, links, points):
    """dict(pos, rot, vel, jac) of the restatement for states q (B, 40), rates qd (B, 39) or None (zero velocity)"""
    from oracle.dwbc_np import Cycle, forward_kinematics, link_velocities, point_jacobian

    model = cases.tocabi_model()
    B, n = len(q), len(links)
    out = dict(pos=np.zeros((B, n, 3)), rot=np.zeros((B, n, 3, 3)), vel=np.zeros((B, n, 6)), jac=np.zeros((B, n, 6, 39)))
    cyc = Cycle(model) if COM in links else None
    for b in range(B):
        R, p = forward_kinematics(model, q[b])
        v0, w0, _ = link_velocities(model, R, p, qd[b]) if qd is not None else (np.zeros((34, 3)), np.zeros((34, 3)), None)
        if cyc:
            cyc.update_kinematics(q[b])
        for e, (l, pt) in enumerate(zip(links, points)):
            pt = np.asarray(pt, float)
            if l == COM:
                out["pos"][b, e], out["rot"][b, e], out["jac"][b, e] = cyc.com, R[0], cyc.J_com
                if qd is not None:
                    out["vel"][b, e] = cyc.J_com @ qd[b]
                continue
            out["pos"][b, e], out["rot"][b, e] = p[l] + R[l] @ pt, R[l]
            out["jac"][b, e] = point_jacobian(model, R, p, l, pt)
            out["vel"][b, e, :3] = v0[l] + np.cross(w0[l], R[l] @ pt)  # v at the point from link_[l].v / .w at the origin
            out["vel"][b, e, 3:] = w0[l]
    return out


@functools.lru_cache(maxsize=None)
def state_set(B, seed=5):
    """(q, qd, Q7 reference): cases.synth_batch(B, seed, yaw=True) with rates U(-1, 1) of default_rng(seed); read-only arrays"""
    q, _, _ = cases.synth_batch(B, seed=seed, yaw=True)
    qd = np.random.default_rng(seed).uniform(-1, 1, (B, 39))
    ref = reference(q, qd, Q7_LINKS, Q7_POINTS)
    for a in (q, qd) + tuple(ref.values()):
        a.setflags(write=False)
    return q, qd, ref


def compare(got, ref, links, jac=True):
    """every output against the restatement at the bars above; prints the worst figures first.  Returns them."""
    com = np.asarray(links) == COM
    worst = dict(pos=float(np.abs(got["pos"] - ref["pos"]).max()), rot=float(np.abs(got["rot"] - ref["rot"]).max()),
                 vel=float(np.abs(got["vel"] - ref["vel"]).max()))
    if jac:
        worst["jac"] = float(np.abs(got["jac"][:, ~com] - ref["jac"][:, ~com]).max()) if (~com).any() else 0.0
        worst["jac_com"] = float(np.abs(got["jac"][:, com] - ref["jac"][:, com]).max()) if com.any() else 0.0
    print("worst |difference| to the restatement: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["pos"] <= TOL_POS and worst["rot"] <= TOL_ROT and worst["vel"] <= TOL_VEL, worst
    assert not jac or (worst["jac"] <= TOL_JAC and worst["jac_com"] <= TOL_JAC_COM), worst
    return worst
