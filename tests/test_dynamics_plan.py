"""not-gpu: the launch planner's answer to a dynamics request (dwbc_plan::Request::dynamics, the dynamics half of UpdateKinematics) over
the hand-written table of tests/cpp/dynamics_plan.cpp: the request picks the kDynamics row of the model's size and tree whatever the batch
size, the task levels, the contact capacity or the cycle's options are, each of its two refusals returns its own message, the arithmetic
type before the model, and cycle, redistribution, gravity-compensation and link-query requests are planned as before."""
import functools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "dynamics_plan")
DYN = "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoTocabi>"
DYN_ANY = "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoGeneric>"
DYN_PACK = "dwbc::dwbc_dynamics_kernel<37, 32, dwbc::TopoGeneric>"
REFUSED = {
    "fp32": (dict(arith=1), "dynamics: fp64 batches only"),
    "no row": (dict(n=23, nb=18, topo=0), "no dynamics kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)"),
}


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "dynamics_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_request_picks_the_row():
    for extra in ({}, dict(B=1), dict(B=100000), dict(levels=0), dict(levels=1), dict(levels=4), dict(hqp=0), dict(warm=1), dict(dump_on=1), dict(max_active=3),
                  dict(inst_par=1), dict(B=1, levels=4, hqp=0, warm=1, dump_on=1, max_active=3)):
        (p,) = plans(dict(dynamics=1, **extra))
        assert p["err"] == "" and p["name"] == DYN and p["threads"] == 64 and p["lds"] == 15536 and not p["ws_valid_after"], (extra, p)


def test_tree_and_pack_rows():
    any_tree, pack = plans(dict(dynamics=1, topo=0), dict(dynamics=1, n=37, nb=32, topo=0, levels=0))
    assert any_tree["err"] == "" and any_tree["name"] == DYN_ANY
    assert pack["err"] == "" and pack["name"] == DYN_PACK and pack["lds"] == 14448


def test_each_refusal_has_its_message():
    for what, (q, msg) in REFUSED.items():
        (p,) = plans(dict(dynamics=1, **q))
        assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (what, p)
    # the arithmetic type before the model
    assert plans(dict(dynamics=1, arith=1, n=23, nb=18, topo=0))[0]["err"] == REFUSED["fp32"][1]
    # a contact capacity the other lean launches refuse does not matter here, on a pack either
    assert plans(dict(dynamics=1, max_active=3, n=37, nb=32, topo=0))[0]["name"] == DYN_PACK


def test_other_requests_plan_as_before():
    lean, extras, redist, grav, lq, pack_redist, pack_grav, pack_lq = plans(
        dict(B=5000), dict(B=5000, warm=1), dict(redistribute=1), dict(grav_comp=1), dict(link_query=1), dict(redistribute=1, n=37, nb=32, topo=0),
        dict(grav_comp=1, n=37, nb=32, topo=0), dict(link_query=1, n=37, nb=32, topo=0))
    assert lean["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, false, dwbc::TopoTocabi, true>"
    assert extras["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc::TopoTocabi>" and extras["ws_valid_after"]
    assert redist["name"] == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"
    assert grav["name"] == "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoTocabi>"
    assert lq["name"] == "dwbc::dwbc_link_query_kernel<39, 34>"
    assert pack_redist["name"] == "dwbc::dwbc_redistribute_kernel<37, 32, dwbc::TopoGeneric>"
    assert pack_grav["name"] == "dwbc::dwbc_gravcomp_kernel<37, 32, dwbc::TopoGeneric>"
    assert pack_lq["name"] == "" and pack_lq["err"].startswith("no link-query kernel for this model")
    # the earlier lean launches keep their precedence over one another when a caller sets more than one member
    both = plans(dict(grav_comp=1, redistribute=1))[0]
    assert both["name"] == "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoTocabi>"
