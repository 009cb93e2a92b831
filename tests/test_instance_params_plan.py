"""not-gpu: the launch planner's answer to a batch that carries per-instance torque limits and contact cone constants
(dwbc_plan::Request::inst_par) over the hand-written table of tests/cpp/instance_params_plan.cpp.  Every kernel of the table reads the
record where it fills a QP row, so the member changes no route; what has no QP rows to put the record in -- the reduced path and
hqp = false -- is refused with its own message, in that order, and only after every refusal a batch without a record gets."""
import functools
import itertools
import json
import os
import subprocess

from tests import cases

EXE = os.path.join(cases.ROOT, "tests", "cpp", "instance_params_plan")
REDUCED = "per-instance parameters: not built on the reduced dynamics path (drop them with dwbc_batch_set_instance_params(b, NULL))"
NO_HQP = "per-instance parameters: hqp = true only (the closed form of hqp = false reads neither torque limits nor contact cones)"
GC_SCOPE = "three active contacts / task levels of more than 6 dof: "


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "instance_params_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def test_the_record_keeps_every_route():
    """each accepted request of the table is planned the same with and without a record: the name, the launch shape, the working-set
    flag and the swap bit"""
    sizes = [dict(), dict(B=1024), dict(B=1025), dict(B=100000), dict(levels=1), dict(levels=3), dict(levels=4, B=5000)]
    switches = [dict(), dict(no_wide=1), dict(no_pair=1), dict(no_lean=1), dict(no_wide=1, no_lean=1), dict(topo=0), dict(pair_always=1, pair_swap_bit=8),
                dict(warm=1), dict(n_traj=1), dict(has_com_task=1), dict(n_custom=1), dict(dump_on=1)]
    others = [dict(arith=1), dict(arith=1, B=1025, warm=1), dict(max_active=3), dict(wide_tasks=1), dict(max_active=3, has_com_task=1, warm=1),
              dict(n=37, nb=32, topo=0, tree_match=1), dict(n=37, nb=32, topo=0, tree_match=0, B=1025), dict(n=37, nb=32, topo=0, max_active=3),
              dict(redistribute=1), dict(redistribute=1, B=1), dict(redistribute=1, levels=0, warm=1)]
    reqs = [dict(a, **b) for a, b in itertools.product(sizes, switches)] + others
    without = plans(*reqs)
    with_rec = plans(*[dict(q, inst_par=1) for q in reqs])
    seen = set()
    for q, a, b in zip(reqs, without, with_rec):
        assert a["err"] == "" and a["name"], (q, a)
        assert a == b, (q, a, b)
        seen.add(a["name"].split("<")[0] + ("/lean" if "false" in a["name"] else ""))
    # the table's kinds were all reached: capped and wide, lean and extras, two-wave, general-contact, redistribution, fp32
    assert len(seen) >= 9, seen


def test_each_new_refusal_has_its_message_and_order():
    for extra in (dict(), dict(B=5000), dict(levels=1), dict(topo=0), dict(arith=1)):
        red, nohqp, both = plans(dict(inst_par=1, reduced=1, **extra), dict(inst_par=1, hqp=0, **extra), dict(inst_par=1, reduced=1, hqp=0, **extra))
        for p, msg in ((red, REDUCED), (nohqp, NO_HQP), (both, REDUCED)):  # the reduced path first
            assert p["name"] == "" and p["threads"] == 0 and p["lds"] == 0 and p["pair_swap_bit"] == -1 and p["err"] == msg, (extra, p)
        # without a record both are served
        red0, nohqp0 = plans(dict(reduced=1, **extra), dict(hqp=0, **extra))
        assert red0["err"] == "" and "reduced" in red0["name"] and nohqp0["err"] == "" and "true" in nohqp0["name"], (extra, red0, nohqp0)


def test_existing_refusals_win():
    cases_ = [
        (dict(levels=5), "no kernel for this model / number of task levels"),
        (dict(n=23, nb=18, topo=0), "no kernel for this model / number of task levels"),
        (dict(n=37, nb=32, topo=0, reduced=1), "no kernel for this model / number of task levels"),
        (dict(arith=1, levels=5, reduced=1), "no fp32 kernel for this model / number of task levels"),
        (dict(arith=1, dump_on=1, hqp=0), "the dump record is not available on DWBC_F32 batches"),
        (dict(max_active=3, reduced=1), GC_SCOPE + "not built on the reduced dynamics path"),
        (dict(wide_tasks=1, reduced=1, hqp=0), GC_SCOPE + "not built on the reduced dynamics path"),
        (dict(max_active=3, arith=1, hqp=0), GC_SCOPE + "fp64 batches only"),
        (dict(max_active=3, hqp=0), GC_SCOPE + "hqp = true only (the reference's closed-form redistribution is written for two contacts, src/dwbc.cpp:1570-1619)"),
        (dict(max_active=3, n_traj=1), GC_SCOPE + "link and COM tasks with f* from SetTaskSpace only (no trajectories, no TASK_CUSTOM levels, no dump record)"),
        (dict(n=37, nb=32, topo=0, wide_tasks=1, hqp=0), "task levels of more than 6 dof: built in for TOCABI's size only"),
        (dict(redistribute=1, arith=1, hqp=0), "redistribution of a supplied torque: fp64 batches only"),
        (dict(redistribute=1, max_active=3), "redistribution of a supplied torque: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))"),
        (dict(redistribute=1, n=37, nb=32, topo=0), "no redistribution kernel for this model (built in for TOCABI's size and tree; kernel packs do not carry one)"),
        (dict(redistribute=1, hqp=0), "redistribution of a supplied torque: hqp = true only (the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque)"),
    ]
    without = plans(*[q for q, _ in cases_])
    with_rec = plans(*[dict(q, inst_par=1) for q, _ in cases_])
    for (q, msg), a, b in zip(cases_, without, with_rec):
        assert a["name"] == "" and a["err"] == msg, (q, a)
        assert b == a, (q, b)
