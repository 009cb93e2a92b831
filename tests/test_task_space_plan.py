"""not-gpu: the launch planner's answer to a task-space request (dwbc_plan::Request::task_space, SetTaskSpace + CalcTaskSpace on their own)
over the hand-written table of tests/cpp/task_space_plan.cpp: the request picks the kTaskSpace row of the model's size and tree whatever
the batch size, hqp, warm and the dump record are, each of its six refusals returns its own message in the order arithmetic type, contact
capacity, level width, TASK_CUSTOM, model, task levels, and every other request is planned as before."""
import functools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "task_space_plan")
TS = "dwbc::dwbc_task_space_kernel<39, 34, dwbc::TopoTocabi>"
TS_ANY = "dwbc::dwbc_task_space_kernel<39, 34, dwbc::TopoGeneric>"
TS_PACK = "dwbc::dwbc_task_space_kernel<37, 32, dwbc::TopoGeneric>"
# in the order the planner checks them
REFUSED = [
    ("fp32", dict(arith=1), "task space: fp64 batches only"),
    ("three contacts", dict(max_active=3), "task space: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
    ("wide level", dict(wide_tasks=1), "task space: task levels of at most 6 dof"),
    ("custom level", dict(n_custom=1), "task space: TASK_CUSTOM levels are not built (their J_task is the caller's own)"),
    ("no row", dict(n=23, nb=18, topo=0), "no task-space kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)"),
    ("no level", dict(levels=0), "task space: no task level (call dwbc_batch_add_task first)"),
]


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "task_space_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_request_picks_the_row():
    for extra in ({}, dict(B=1), dict(B=100000), dict(levels=1), dict(levels=4), dict(hqp=0), dict(warm=1), dict(dump_on=1), dict(inst_par=1), dict(n_contacts=0),
                  dict(n_contacts=4), dict(B=1, levels=4, hqp=0, warm=1, dump_on=1)):
        (p,) = plans(dict(task_space=1, **extra))
        assert p["err"] == "" and p["name"] == TS and p["threads"] == 64 and p["lds"] == 38656 and not p["ws_valid_after"], (extra, p)


def test_tree_and_pack_rows():
    any_tree, pack = plans(dict(task_space=1, topo=0), dict(task_space=1, n=37, nb=32, topo=0))
    assert any_tree["err"] == "" and any_tree["name"] == TS_ANY
    assert pack["err"] == "" and pack["name"] == TS_PACK and pack["lds"] == 36944


def test_each_refusal_has_its_message_and_its_place():
    assert len({msg for _, _, msg in REFUSED}) == len(REFUSED)
    for what, q, msg in REFUSED:
        (p,) = plans(dict(task_space=1, **q))
        assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (what, p)
    # one cause at a time: with every later cause present as well, the earliest one answers
    for i, (what, _, msg) in enumerate(REFUSED):
        q = {}
        for _, later, _ in REFUSED[i:]:
            q.update(later)
        assert plans(dict(task_space=1, **q))[0]["err"] == msg, what


def test_other_requests_plan_as_before():
    lean, extras, redist, grav, lq, dyn, cs, gc, pack_cs, wide = plans(
        dict(B=5000), dict(B=5000, warm=1), dict(redistribute=1), dict(grav_comp=1), dict(link_query=1), dict(dynamics=1), dict(contact_space=1),
        dict(max_active=3), dict(contact_space=1, n=37, nb=32, topo=0), dict(wide_tasks=1, n_custom=1))
    assert lean["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, false, dwbc::TopoTocabi, true>"
    assert extras["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc::TopoTocabi>" and extras["ws_valid_after"]
    assert redist["name"] == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"
    assert grav["name"] == "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoTocabi>"
    assert lq["name"] == "dwbc::dwbc_link_query_kernel<39, 34>"
    assert dyn["name"] == "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoTocabi>"
    assert cs["name"] == "dwbc::dwbc_contact_space_kernel<39, 34, dwbc::TopoTocabi>"
    assert gc["name"] == "dwbc::dwbc_cycle_kernel_gc<39, 34, 64, 6>"
    assert pack_cs["name"] == "dwbc::dwbc_contact_space_kernel<37, 32, dwbc::TopoGeneric>"
    assert wide["err"] == "task levels of more than 6 dof: built in for TOCABI's size only"  # (the table above has no TG = 12 row)
    # the earlier lean launches keep their precedence when a caller sets more than one member
    assert plans(dict(dynamics=1, task_space=1))[0]["name"] == dyn["name"]
    assert plans(dict(task_space=1, contact_space=1))[0]["name"] == cs["name"] and plans(dict(task_space=1, redistribute=1))[0]["name"] == redist["name"]
