"""not-gpu: the launch planner's answer to a link query (dwbc_plan::Request::link_query) over the hand-written table of
tests/cpp/link_query_plan.cpp: the request picks the kLinkQuery row whatever the batch size, the task levels, the model's tree or the
cycle's optional paths are, each refusal returns its own message, and cycle and redistribution requests are planned as before."""
import functools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "link_query_plan")
LINK_QUERY = "dwbc::dwbc_link_query_kernel<39, 34>"
NO_F32 = "link query: fp64 batches only"
NO_ROW = "no link-query kernel for this model (built in for TOCABI's size, any tree; kernel packs do not carry one)"


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "link_query_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_request_picks_the_row():
    for extra in (dict(B=1), dict(B=250), dict(B=100000), dict(warm=1), dict(dump_on=1), dict(levels=0), dict(levels=1), dict(levels=4), dict(n_custom=1),
                  dict(hqp=0), dict(max_active=3), dict(topo=0)):
        (p,) = plans(dict(link_query=1, **extra))
        assert p["err"] == "" and p["name"] == LINK_QUERY and p["threads"] == 64 and p["lds"] == 13152 and not p["ws_valid_after"], (extra, p)


def test_each_refusal_has_its_message():
    for what, q, msg in (("fp32", dict(arith=1), NO_F32), ("pack model", dict(n=37, nb=32, topo=0), NO_ROW)):
        (p,) = plans(dict(link_query=1, **q))
        assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (what, p)
    # one cause at a time, the arithmetic type before the model
    assert plans(dict(link_query=1, arith=1, n=37, nb=32, topo=0))[0]["err"] == NO_F32


def test_cycle_and_redistribution_requests_never_see_the_row():
    lean, extras, pack, redist, any_tree = plans(dict(B=5000), dict(B=5000, warm=1), dict(n=37, nb=32, topo=0), dict(redistribute=1), dict(topo=0))
    assert lean["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, false, dwbc::TopoTocabi, true>"
    assert extras["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc::TopoTocabi>" and extras["ws_valid_after"]
    assert pack["name"] == "dwbc::dwbc_cycle_kernel_v2<37, 32, 2, 64, true, dwbc::TopoGeneric>"
    assert redist["name"] == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>" and redist["lds"] == 20432
    # a 39-dof model with another tree has no cycle row in this table: the any-tree link-query row does not stand in for one
    assert any_tree["name"] == "" and any_tree["err"] == "no kernel for this model / number of task levels"
    assert plans(dict(redistribute=1, topo=0))[0]["err"].startswith("no redistribution kernel for this model")
