"""not-gpu: the launch planner's answer to a batch that carries one body table per instance (dwbc_plan::Request::inst_model) over the
hand-written table of tests/cpp/inst_model_plan.cpp.  With the record every route of the full-model cycle and every lean launch is served
by the dwbc_im:: twin of the kernel it picks without one -- same launch shape, working-set flag and swap bit; without the record nothing
changes whether the dwbc_im table is there or not; the three new refusals have one message each and come after every refusal the same
request meets without a record."""
import functools
import itertools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "inst_model_plan")
KINSTMODEL = 32
REDUCED = "per-instance model: not built on the reduced dynamics path (drop the record with dwbc_batch_set_instance_model(b, NULL))"
GC = "per-instance model: not built for three active contacts or task levels of more than 6 dof (the general-contact kernel has no such build)"
NONE = ("per-instance model: no kernel for this request (built for fp64 batches on TOCABI's constant tree: the full-model cycle of 1 to 4 task levels on every "
        "launch route, and the redistribution, gravity-compensation, link-query, dynamics, contact-space and task-space launches)")
GC_SCOPE = "three active contacts / task levels of more than 6 dof: "
ROUTES = {
    "two_wave": (dict(), "dwbc_cycle_kernel_v2p<39, 34, {L}, {ns}TopoTocabi>"),
    "wide_lean": (dict(no_pair=1), "dwbc_cycle_kernel_v2w<39, 34, {L}, 64, false, {ns}TopoTocabi>"),
    "compact_lean": (dict(no_wide=1), "dwbc_cycle_kernel_v2<39, 34, {L}, 64, false, {ns}TopoTocabi, true>"),
    "wide_extras": (dict(no_lean=1), "dwbc_cycle_kernel_v2w<39, 34, {L}, 64, true, {ns}TopoTocabi>"),
    "capped_extras": (dict(no_lean=1, no_wide=1), "dwbc_cycle_kernel_v2<39, 34, {L}, 64, true, {ns}TopoTocabi>"),
}
LEAN = {"redistribute": "dwbc_redistribute_kernel", "grav_comp": "dwbc_gravcomp_kernel", "link_query": "dwbc_link_query_kernel",
        "dynamics": "dwbc_dynamics_kernel", "contact_space": "dwbc_contact_space_kernel", "task_space": "dwbc_task_space_kernel"}


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "inst_model_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def _twin(plain):
    return dict(plain, name=plain["name"].replace("dwbc::", "dwbc_im::"), flavour=plain["flavour"] | KINSTMODEL)


def test_each_route_picks_its_twin():
    seen = set()
    for (route, (sw, name)), levels in itertools.product(ROUTES.items(), (1, 2, 3, 4)):
        if route == "two_wave" and levels > 2:
            continue
        for extra in (dict(), dict(pair_swap_bit=8) if route == "two_wave" else dict(B=4 * 256), dict(inst_par=1)):
            q = dict(sw, levels=levels, **extra)
            plain, rec = plans(q, dict(q, inst_model=1))
            assert plain["err"] == "" and plain["name"] == "dwbc::" + name.format(L=levels, ns="dwbc::"), (q, plain)
            assert rec["name"] == "dwbc_im::" + name.format(L=levels, ns="dwbc_im::"), (q, rec)
            assert rec == _twin(plain), (q, plain, rec)
            assert not plain["flavour"] & KINSTMODEL
            seen.add(rec["name"])
    assert len(seen) == 18, sorted(seen)  # every cycle kernel of the dwbc_im build is some route's answer
    # the natural boundary and the optional paths go the same way
    for q in (dict(B=1025), dict(B=100000, levels=4), dict(warm=1), dict(warm=1, B=5000), dict(n_traj=1), dict(has_com_task=1), dict(n_custom=1), dict(dump_on=1),
              dict(hqp=0), dict(hqp=0, B=5000), dict(pair_always=1, B=5000, pair_swap_bit=9)):
        plain, rec = plans(q, dict(q, inst_model=1))
        assert plain["err"] == "" and rec == _twin(plain), (q, plain, rec)


def test_each_lean_launch_picks_its_twin():
    for key, kernel in LEAN.items():
        for extra in (dict(), dict(B=1), dict(levels=4, warm=1, dump_on=1)):
            q = dict({key: 1}, **extra)
            plain, rec = plans(q, dict(q, inst_model=1))
            assert plain["err"] == "" and plain["name"].startswith("dwbc::" + kernel + "<"), (q, plain)
            assert rec == _twin(plain) and rec["name"].startswith("dwbc_im::" + kernel + "<"), (q, plain, rec)


def test_without_the_record_the_new_table_changes_nothing():
    sizes = [dict(), dict(B=1024), dict(B=1025), dict(levels=1), dict(levels=3), dict(levels=4, B=5000), dict(levels=5)]
    switches = [dict(), dict(no_wide=1), dict(no_pair=1), dict(no_lean=1), dict(no_wide=1, no_lean=1), dict(topo=0), dict(warm=1), dict(dump_on=1), dict(hqp=0),
                dict(reduced=1), dict(arith=1), dict(max_active=3), dict(wide_tasks=1), dict(inst_par=1), dict(n=37, nb=32, topo=0)] + [{k: 1} for k in LEAN]
    reqs = [dict(a, **b) for a, b in itertools.product(sizes, switches)]
    with_tab = plans(*reqs)
    without = plans(*[dict(q, im_table=0) for q in reqs])
    for q, a, b in zip(reqs, with_tab, without):
        assert a == b, (q, a, b)
        assert not a["flavour"] & KINSTMODEL and "dwbc_im::" not in a["name"], (q, a)


def _refused(p, msg, q):
    assert p["name"] == "" and p["threads"] == 0 and p["lds"] == 0 and p["pair_swap_bit"] == -1 and p["err"] == msg, (q, p)


def test_new_refusals_each_have_one_message():
    for extra in (dict(), dict(B=5000), dict(levels=1), dict(levels=4, warm=1)):
        for q, msg in ((dict(reduced=1), REDUCED), (dict(max_active=3), GC), (dict(wide_tasks=1), GC), (dict(max_active=3, wide_tasks=1), GC)):
            q = dict(q, inst_model=1, **extra)
            _refused(plans(q)[0], msg, q)
    # no row at all: another arithmetic type, another tree, another model size, a library without the build -- for the cycle and the lean launches
    for q in (dict(arith=1), dict(topo=0), dict(topo=0, no_lean=1), dict(n=37, nb=32, topo=0), dict(im_table=0), dict(im_table=0, dynamics=1), dict(dynamics=1, topo=0),
              dict(dynamics=1, n=37, nb=32, topo=0), dict(task_space=1, topo=0), dict(redistribute=1, im_table=0), dict(link_query=1, im_table=0)):
        q = dict(q, inst_model=1)
        _refused(plans(q)[0], NONE, q)


def test_existing_refusals_come_first():
    cases_ = [
        (dict(levels=5), "no kernel for this model / number of task levels"),
        (dict(n=23, nb=18, topo=0), "no kernel for this model / number of task levels"),
        (dict(n=37, nb=32, topo=0, reduced=1), "no kernel for this model / number of task levels"),
        (dict(arith=1, levels=5, reduced=1), "no fp32 kernel for this model / number of task levels"),
        (dict(arith=1, dump_on=1), "the dump record is not available on DWBC_F32 batches"),
        (dict(reduced=1, inst_par=1), "per-instance parameters: not built on the reduced dynamics path (drop them with dwbc_batch_set_instance_params(b, NULL))"),
        (dict(hqp=0, inst_par=1), "per-instance parameters: hqp = true only (the closed form of hqp = false reads neither torque limits nor contact cones)"),
        (dict(max_active=3, reduced=1), GC_SCOPE + "not built on the reduced dynamics path"),
        (dict(max_active=3, arith=1), GC_SCOPE + "fp64 batches only"),
        (dict(max_active=3, hqp=0), GC_SCOPE + "hqp = true only (the reference's closed-form redistribution is written for two contacts, src/dwbc.cpp:1570-1619)"),
        (dict(wide_tasks=1, dump_on=1), GC_SCOPE + "link and COM tasks with f* from SetTaskSpace only (no trajectories, no TASK_CUSTOM levels, no dump record)"),
        (dict(redistribute=1, arith=1), "redistribution of a supplied torque: fp64 batches only"),
        (dict(redistribute=1, max_active=3), "redistribution of a supplied torque: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
        (dict(redistribute=1, hqp=0), "redistribution of a supplied torque: hqp = true only (the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque)"),
        (dict(grav_comp=1, max_active=3), "gravity compensation: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
        (dict(link_query=1, arith=1), "link query: fp64 batches only"),
        (dict(dynamics=1, arith=1), "dynamics: fp64 batches only"),
        (dict(dynamics=1, n=23, nb=18, topo=0), "no dynamics kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)"),
        (dict(contact_space=1, n_contacts=0), "contact space: no contact constraint (call dwbc_batch_add_contact first)"),
        (dict(task_space=1, wide_tasks=1), "task space: task levels of at most 6 dof"),
        (dict(task_space=1, n_custom=1), "task space: TASK_CUSTOM levels are not built (their J_task is the caller's own)"),
        (dict(task_space=1, levels=0), "task space: no task level (call dwbc_batch_add_task first)"),
    ]
    without = plans(*[q for q, _ in cases_])
    with_rec = plans(*[dict(q, inst_model=1) for q, _ in cases_])
    for (q, msg), a, b in zip(cases_, without, with_rec):
        _refused(a, msg, q)
        assert b == a, (q, b)
    # the stated order among the new ones: the reduced path, then the general-contact scope, then "no row"
    q = dict(reduced=1, topo=0, inst_model=1)
    _refused(plans(q)[0], REDUCED, q)
    q = dict(max_active=3, im_table=0, inst_model=1)
    _refused(plans(q)[0], GC, q)
