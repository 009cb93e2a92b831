"""not-gpu: the launch planner's answer to a contact-space request (dwbc_plan::Request::contact_space, SetContact + CalcContactConstraint
on their own) over the hand-written table of tests/cpp/contact_space_plan.cpp: the request picks the kContactSpace row of the model's size
and tree whatever the batch size, the task levels or the cycle's options are, each of its four refusals returns its own message in the order
arithmetic type, contact capacity, model, registered contacts, and every other request is planned as before."""
import functools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "contact_space_plan")
CS = "dwbc::dwbc_contact_space_kernel<39, 34, dwbc::TopoTocabi>"
CS_ANY = "dwbc::dwbc_contact_space_kernel<39, 34, dwbc::TopoGeneric>"
CS_PACK = "dwbc::dwbc_contact_space_kernel<37, 32, dwbc::TopoGeneric>"
REFUSED = {
    "fp32": (dict(arith=1), "contact space: fp64 batches only"),
    "three contacts": (dict(max_active=3), "contact space: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
    "no row": (dict(n=23, nb=18, topo=0), "no contact-space kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)"),
    "no contact": (dict(n_contacts=0), "contact space: no contact constraint (call dwbc_batch_add_contact first)"),
}


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "contact_space_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_request_picks_the_row():
    for extra in ({}, dict(B=1), dict(B=100000), dict(levels=0), dict(levels=1), dict(levels=4), dict(hqp=0), dict(warm=1), dict(dump_on=1), dict(inst_par=1),
                  dict(n_contacts=4), dict(B=1, levels=4, hqp=0, warm=1, dump_on=1)):
        (p,) = plans(dict(contact_space=1, **extra))
        assert p["err"] == "" and p["name"] == CS and p["threads"] == 64 and p["lds"] == 20432 and not p["ws_valid_after"], (extra, p)


def test_tree_and_pack_rows():
    any_tree, pack = plans(dict(contact_space=1, topo=0), dict(contact_space=1, n=37, nb=32, topo=0, levels=0))
    assert any_tree["err"] == "" and any_tree["name"] == CS_ANY
    assert pack["err"] == "" and pack["name"] == CS_PACK and pack["lds"] == 19488


def test_each_refusal_has_its_message():
    for what, (q, msg) in REFUSED.items():
        (p,) = plans(dict(contact_space=1, **q))
        assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (what, p)
    # one cause at a time, in the order arithmetic type, contact capacity, model, registered contacts
    assert plans(dict(contact_space=1, arith=1, max_active=3, n=23, nb=18, topo=0, n_contacts=0))[0]["err"] == REFUSED["fp32"][1]
    assert plans(dict(contact_space=1, max_active=3, n=23, nb=18, topo=0, n_contacts=0))[0]["err"] == REFUSED["three contacts"][1]
    assert plans(dict(contact_space=1, n=23, nb=18, topo=0, n_contacts=0))[0]["err"] == REFUSED["no row"][1]


def test_other_requests_plan_as_before():
    lean, extras, redist, grav, lq, dyn, pack_redist, pack_grav, pack_dyn, no_contact_dyn = plans(
        dict(B=5000), dict(B=5000, warm=1), dict(redistribute=1), dict(grav_comp=1), dict(link_query=1), dict(dynamics=1), dict(redistribute=1, n=37, nb=32, topo=0),
        dict(grav_comp=1, n=37, nb=32, topo=0), dict(dynamics=1, n=37, nb=32, topo=0), dict(dynamics=1, n_contacts=0))
    assert lean["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, false, dwbc::TopoTocabi, true>"
    assert extras["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc::TopoTocabi>" and extras["ws_valid_after"]
    assert redist["name"] == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"
    assert grav["name"] == "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoTocabi>"
    assert lq["name"] == "dwbc::dwbc_link_query_kernel<39, 34>"
    assert dyn["name"] == "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoTocabi>" and no_contact_dyn["name"] == dyn["name"]
    assert pack_redist["name"] == "dwbc::dwbc_redistribute_kernel<37, 32, dwbc::TopoGeneric>"
    assert pack_grav["name"] == "dwbc::dwbc_gravcomp_kernel<37, 32, dwbc::TopoGeneric>"
    assert pack_dyn["name"] == "dwbc::dwbc_dynamics_kernel<37, 32, dwbc::TopoGeneric>"
    # the earlier lean launches keep their precedence when a caller sets more than one member
    assert plans(dict(dynamics=1, contact_space=1))[0]["name"] == dyn["name"]
    assert plans(dict(contact_space=1, grav_comp=1))[0]["name"] == grav["name"] and plans(dict(contact_space=1, redistribute=1))[0]["name"] == redist["name"]
