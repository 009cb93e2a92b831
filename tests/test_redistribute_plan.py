"""not-gpu: the launch planner's answer to a redistribution of a caller-supplied torque (dwbc_plan::Request::redistribute) over the
hand-written table of tests/cpp/redistribute_plan.cpp: the request picks the kRedist row whatever the batch size, the task levels or the
cycle's optional paths are, each refusal returns its own message, and a request without the member set is planned as before."""
import functools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "redistribute_plan")
REDIST = "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "redistribute_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_request_picks_the_row():
    for extra in ({}, dict(B=1), dict(B=100000), dict(levels=1), dict(levels=4), dict(warm=1), dict(dump_on=1), dict(levels=0)):
        (p,) = plans(dict(redistribute=1, **extra))
        assert p["err"] == "" and p["name"] == REDIST and p["threads"] == 64 and p["lds"] == 20432 and not p["ws_valid_after"], (extra, p)


def test_each_refusal_has_its_message():
    refused = {
        "fp32": (dict(arith=1), "redistribution of a supplied torque: fp64 batches only"),
        "three contacts": (dict(max_active=3), "redistribution of a supplied torque: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
        "size": (dict(n=37, nb=32, topo=0), "no redistribution kernel for this model (built in for TOCABI's size and tree; kernel packs do not carry one)"),
        "tree": (dict(topo=0), "no redistribution kernel for this model (built in for TOCABI's size and tree; kernel packs do not carry one)"),
        "hqp": (dict(hqp=0), "redistribution of a supplied torque: hqp = true only (the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque)"),
    }
    for what, (q, msg) in refused.items():
        (p,) = plans(dict(redistribute=1, **q))
        assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (what, p)
    # one cause at a time, in the order arithmetic type, contact capacity, model, hqp
    assert plans(dict(redistribute=1, arith=1, max_active=3, hqp=0))[0]["err"] == refused["fp32"][1]
    assert plans(dict(redistribute=1, max_active=3, n=37, nb=32, topo=0, hqp=0))[0]["err"] == refused["three contacts"][1]
    assert plans(dict(redistribute=1, n=37, nb=32, topo=0, hqp=0))[0]["err"] == refused["size"][1]


def test_cycle_requests_never_see_the_row():
    lean, extras, pack = plans(dict(B=5000), dict(B=5000, warm=1), dict(n=37, nb=32, topo=0))
    assert lean["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, false, dwbc::TopoTocabi, true>"
    assert extras["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc::TopoTocabi>" and extras["ws_valid_after"]
    assert pack["name"] == "dwbc::dwbc_cycle_kernel_v2<37, 32, 2, 64, true, dwbc::TopoGeneric>"
