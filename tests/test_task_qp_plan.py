"""not-gpu: the launch planner's answer to a single-level task-QP request (dwbc_plan::Request::task_qp, CalcSingleTaskTorqueWithQP of one
level on its own) over the hand-written table of tests/cpp/task_qp_plan.cpp: the request picks the kTaskQp row of the model's tree whatever
the batch size, hqp, warm, the dump record and the per-instance parameters are, each of its six refusals returns its own message in the order
arithmetic type, contact capacity, level width, TASK_CUSTOM, model, task levels, a batch with a per-instance model gets the planner's one
text for that, and every request without task_qp is planned as before."""
import functools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "task_qp_plan")
TQ = "dwbc::dwbc_task_qp_kernel<39, 34, dwbc::TopoTocabi>"
TQ_ANY = "dwbc::dwbc_task_qp_kernel<39, 34, dwbc::TopoGeneric>"
LDS = 37872  # LdsTq<39, 34>::total_bytes
NO_ROW = "no single-level task-QP kernel for this model (built in for TOCABI's size, any tree; kernel packs do not carry one)"
# in the order the planner checks them
REFUSED = [
    ("fp32", dict(arith=1), "single-level task QP: fp64 batches only"),
    ("three contacts", dict(max_active=3), "single-level task QP: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
    ("wide level", dict(wide_tasks=1), "single-level task QP: task levels of at most 6 dof"),
    ("custom level", dict(n_custom=1), "single-level task QP: TASK_CUSTOM levels are not built (their J_task is the caller's own)"),
    ("no row", dict(n=37, nb=32, topo=0), NO_ROW),
    ("no level", dict(levels=0), "single-level task QP: no task level (call dwbc_batch_add_task first)"),
]
INST_MODEL_NONE = ("per-instance model: no kernel for this request (built for fp64 batches on TOCABI's constant tree: the full-model cycle of 1 to 4 task levels on every "
                   "launch route, and the redistribution, gravity-compensation, link-query, dynamics, contact-space and task-space launches)")


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "task_qp_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_request_picks_the_row():
    for extra in ({}, dict(B=1), dict(B=100000), dict(levels=1), dict(levels=4), dict(hqp=0), dict(warm=1), dict(dump_on=1), dict(inst_par=1), dict(n_contacts=0),
                  dict(n_contacts=4), dict(B=1, levels=4, hqp=0, warm=1, dump_on=1, inst_par=1)):
        (p,) = plans(dict(task_qp=1, **extra))
        assert p["err"] == "" and p["name"] == TQ and p["threads"] == 64 and p["lds"] == LDS and not p["ws_valid_after"], (extra, p)


def test_any_tree_takes_the_generic_row_and_no_pack_carries_one():
    any_tree, pack = plans(dict(task_qp=1, topo=0), dict(task_qp=1, n=37, nb=32, topo=0))
    assert any_tree["err"] == "" and any_tree["name"] == TQ_ANY and any_tree["lds"] == LDS
    assert pack["name"] == "" and pack["err"] == NO_ROW  # (the pack of the table carries the task-space row: that launch is served)
    assert plans(dict(task_space=1, n=37, nb=32, topo=0))[0]["name"] == "dwbc::dwbc_task_space_kernel<37, 32, dwbc::TopoGeneric>"


def test_each_refusal_has_its_message_and_its_place():
    assert len({msg for _, _, msg in REFUSED}) == len(REFUSED)
    for what, q, msg in REFUSED:
        (p,) = plans(dict(task_qp=1, **q))
        assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (what, p)
    # one cause at a time: with every later cause present as well, the earliest one answers
    for i, (what, _, msg) in enumerate(REFUSED):
        q = {}
        for _, later, _ in REFUSED[i:]:
            q.update(later)
        assert plans(dict(task_qp=1, **q))[0]["err"] == msg, what


def test_per_instance_model_gets_the_planners_own_text():
    """no dwbc_im:: build of the kernel: after every refusal the request meets without the record, the one unchanged message"""
    (p,) = plans(dict(task_qp=1, inst_model=1))
    assert p["name"] == "" and p["err"] == INST_MODEL_NONE
    for what, q, msg in REFUSED:
        if what != "no row":
            assert plans(dict(task_qp=1, inst_model=1, **q))[0]["err"] == msg, what
    # (the task-space launch of the same batch is served by its dwbc_im:: row)
    assert plans(dict(task_space=1, inst_model=1))[0]["name"] == "dwbc_im::dwbc_task_space_kernel<39, 34, dwbc_im::TopoTocabi>"


def test_requests_without_task_qp_plan_as_before():
    lean, extras, redist, grav, lq, dyn, cs, ts, gc, pack_cs, wide, f32 = plans(
        dict(B=5000), dict(B=5000, warm=1), dict(redistribute=1), dict(grav_comp=1), dict(link_query=1), dict(dynamics=1), dict(contact_space=1),
        dict(task_space=1), dict(max_active=3), dict(contact_space=1, n=37, nb=32, topo=0), dict(wide_tasks=1, n_custom=1), dict(arith=1))
    assert lean["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, false, dwbc::TopoTocabi, true>"
    assert extras["name"] == "dwbc::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc::TopoTocabi>" and extras["ws_valid_after"]
    assert redist["name"] == "dwbc::dwbc_redistribute_kernel<39, 34, dwbc::TopoTocabi>"
    assert grav["name"] == "dwbc::dwbc_gravcomp_kernel<39, 34, dwbc::TopoTocabi>"
    assert lq["name"] == "dwbc::dwbc_link_query_kernel<39, 34>"
    assert dyn["name"] == "dwbc::dwbc_dynamics_kernel<39, 34, dwbc::TopoTocabi>"
    assert cs["name"] == "dwbc::dwbc_contact_space_kernel<39, 34, dwbc::TopoTocabi>"
    assert ts["name"] == "dwbc::dwbc_task_space_kernel<39, 34, dwbc::TopoTocabi>" and ts["lds"] == 38656
    assert gc["name"] == "dwbc::dwbc_cycle_kernel_gc<39, 34, 64, 6>"
    assert pack_cs["name"] == "dwbc::dwbc_contact_space_kernel<37, 32, dwbc::TopoGeneric>"
    assert wide["err"] == "task levels of more than 6 dof: built in for TOCABI's size only"  # (the table above has no TG = 12 row)
    assert f32["name"] == "dwbc_f32::dwbc_cycle_kernel_v2<39, 34, 2, 64, true, dwbc_f32::TopoTocabi>"
    # the earlier launches keep their precedence when a caller sets more than one member
    for first, name in (("dynamics", dyn), ("contact_space", cs), ("redistribute", redist), ("task_space", ts), ("link_query", lq), ("grav_comp", grav)):
        assert plans({first: 1, "task_qp": 1})[0]["name"] == name["name"], first
