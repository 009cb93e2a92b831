"""not-gpu: the launch planner (libdwbc_amd/csrc/dwbc_launch_plan.h) over a hand-written table.

dwbc_batch_solve launches, and kernel_name() / launch_info() report, what dwbc_plan::plan() returns, so the decision itself can be
checked without a device: tests/cpp/launch_plan.cpp holds TOCABI's rows (fp64 and fp32) and a 37-dof / 32-body pack in its generic and
its tree-specific build, and answers each request with the chosen row.  n_cu = 256 throughout (B = 1024 is 4 instances per CU)."""
import functools
import json
import os
import subprocess

import pytest

from tests import cases
from tests.test_launch_flavours import ROUTES

EXE = os.path.join(cases.ROOT, "tests", "cpp", "launch_plan")
KEY = {"DWBC_NO_WIDE": "no_wide", "DWBC_NO_PAIR": "no_pair", "DWBC_NO_LEAN": "no_lean", "DWBC_PAIR_ALWAYS": "pair_always"}

V2P = "dwbc::dwbc_cycle_kernel_v2p<39, 34, {L}, dwbc::TopoTocabi>"
WIDE_LEAN = "dwbc::dwbc_cycle_kernel_v2w<39, 34, {L}, 64, false, dwbc::TopoTocabi>"
WIDE_EXTRAS = "dwbc::dwbc_cycle_kernel_v2w<39, 34, {L}, 64, true, dwbc::TopoTocabi>"
COMPACT = "dwbc::dwbc_cycle_kernel_v2<39, 34, {L}, 64, false, dwbc::TopoTocabi, true>"
GC_SCOPE = "three active contacts / task levels of more than 6 dof: "


@functools.lru_cache(maxsize=None)
def _build():
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(cases.ROOT, "tests", "cpp", "launch_plan.cpp"), "-o", EXE])
    return EXE


def plans(*requests):
    """one plan per request (dicts of dwbc_plan::Request members over the defaults of launch_plan.cpp: fp64 TOCABI, two levels, B = 250)"""
    args = [",".join(f"{k}={int(v)}" for k, v in r.items()) for r in requests]
    out = subprocess.check_output([_build()] + args, text=True)
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(requests)
    return res


def plan(**request):
    return plans(request)[0]


def _route_request(env):
    q = {KEY[k]: 1 for k in env if k in KEY}
    if "DWBC_DENSE_SWEEP" in env:  # read at batch creation: the model is treated as any 34-body tree
        q["topo"] = 0
    return q


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_six_routes(levels):
    """the switches of tests/test_launch_flavours.py choose the builds that file pins, at its batch size"""
    for route, (env, name, threads) in ROUTES.items():
        if route == "two_wave" and levels > 2:  # no two-wave build beyond two levels: the wide lean one
            name = ROUTES["wide_lean"][1]
            threads = 64
        p = plan(levels=levels, B=250, **_route_request(env))
        assert p["err"] == "" and p["name"] == name.format(L=levels), (route, p)
        assert p["threads"] == threads and p["lds"] > 0, (route, p)
        assert p["ws_valid_after"] == ("extras" in route or route == "generic"), (route, p)  # only the extras builds keep working sets
        assert p["pair_swap_bit"] == -1


def test_compact_map_is_the_small_one():
    lean, extras = plans(dict(no_wide=1), dict(no_wide=1, no_lean=1))
    assert lean["lds"] < extras["lds"]


def test_natural_boundary_and_pair_always():
    lo, hi, always, swapped, never = plans(dict(B=1024), dict(B=1025), dict(B=1025, pair_always=1), dict(B=1025, pair_always=1, pair_swap_bit=8),
                                           dict(B=1025, pair_always=1, no_pair=1))
    assert lo["name"] == V2P.format(L=2) and lo["threads"] == 128
    assert hi["name"] == COMPACT.format(L=2) and hi["threads"] == 64
    assert always["name"] == V2P.format(L=2) and always["threads"] == 128 and always["lds"] == lo["lds"] and always["pair_swap_bit"] == -1
    assert swapped["name"] == always["name"] and swapped["pair_swap_bit"] == 8
    assert never["name"] == hi["name"]
    assert not any(p["ws_valid_after"] for p in (lo, hi, always, swapped, never))
    # the swap bit goes to the two-wave kernel only
    assert plan(B=250, no_pair=1, pair_swap_bit=8)["pair_swap_bit"] == -1


@pytest.mark.parametrize("fact", [dict(warm=1), dict(n_traj=1), dict(has_com_task=1), dict(n_custom=1), dict(dump_on=1), dict(hqp=0)])
def test_each_optional_path_takes_the_extras_build(fact):
    small, large = plans(dict(B=250, **fact), dict(B=1025, **fact))
    assert small["name"] == WIDE_EXTRAS.format(L=2) and small["ws_valid_after"]
    assert large["name"] == cases.CAPPED_EXTRAS.format(L=2) and large["ws_valid_after"]
    assert small["threads"] == large["threads"] == 64 and small["lds"] == large["lds"]


def test_reduced():
    for topo, tree in ((1, "TopoTocabi"), (0, "TopoGeneric")):
        for levels in (1, 2, 3, 4):
            for extra in ({}, dict(warm=1), dict(B=5000)):
                p = plan(reduced=1, topo=topo, levels=levels, **extra)
                assert p["name"] == f"dwbc::dwbc_cycle_kernel_reduced<39, 34, {levels}, 64, dwbc::{tree}>", p
                assert p["threads"] == 64 and not p["ws_valid_after"]


def test_fp32():
    f = "dwbc_f32::"
    names = {
        (250, 0): f"{f}dwbc_cycle_kernel_v2w<39, 34, 2, 64, false, {f}TopoTocabi>",
        (250, 1): f"{f}dwbc_cycle_kernel_v2w<39, 34, 2, 64, true, {f}TopoTocabi>",
        (1025, 0): f"{f}dwbc_cycle_kernel_v2<39, 34, 2, 64, false, {f}TopoTocabi, true>",
        (1025, 1): f"{f}dwbc_cycle_kernel_v2<39, 34, 2, 64, true, {f}TopoTocabi>",
    }
    for (B, warm), name in names.items():
        for always in (0, 1):  # never the two-wave kernel
            p = plan(arith=1, B=B, warm=warm, pair_always=always)
            assert p["name"] == name and p["threads"] == 64 and p["ws_valid_after"] == bool(warm), p
    assert plan(arith=1, topo=0)["name"] == f"{f}dwbc_cycle_kernel_v2<39, 34, 2, 64, true, {f}TopoGeneric>"
    assert plan(arith=1, reduced=1)["name"] == f"{f}dwbc_cycle_kernel_reduced<39, 34, 2, 64, {f}TopoTocabi>"
    for q in (dict(n=37, nb=32, topo=0), dict(n=37, nb=32, topo=0, tree_match=1), dict(levels=5)):
        p = plan(arith=1, **q)
        assert p["name"] == "" and p["err"] == "no fp32 kernel for this model / number of task levels", p
    assert plan(arith=1, dump_on=1)["err"] == "the dump record is not available on DWBC_F32 batches"


def test_general_contact():
    three, wide, both = plans(dict(max_active=3), dict(wide_tasks=1), dict(max_active=3, wide_tasks=1, levels=4, B=5000))
    assert three["name"] == "dwbc::dwbc_cycle_kernel_gc<39, 34, 64, 6>" and three["lds"] == 81696
    assert wide["name"] == both["name"] == "dwbc::dwbc_cycle_kernel_gc<39, 34, 64, 12>" and wide["lds"] > three["lds"]
    for p in (three, wide, both):
        assert p["threads"] == 64 and not p["ws_valid_after"] and p["err"] == ""
    # a COM level and a warm request stay in scope (cold-started all the same)
    assert plan(max_active=3, has_com_task=1, warm=1)["name"] == three["name"]
    refused = {
        "reduced": GC_SCOPE + "not built on the reduced dynamics path",
        "arith": GC_SCOPE + "fp64 batches only",
        "hqp": GC_SCOPE + "hqp = true only (the reference's closed-form redistribution is written for two contacts, src/dwbc.cpp:1570-1619)",
        "n_traj": GC_SCOPE + "link and COM tasks with f* from SetTaskSpace only (no trajectories, no TASK_CUSTOM levels, no dump record)",
        "dump_on": GC_SCOPE + "link and COM tasks with f* from SetTaskSpace only (no trajectories, no TASK_CUSTOM levels, no dump record)",
    }
    for key, msg in refused.items():
        for scope in (dict(max_active=3), dict(wide_tasks=1)):
            p = plan(**scope, **{key: 0 if key == "hqp" else 1})
            assert p["name"] == "" and p["threads"] == 0 and p["err"] == msg, (key, p)
    assert plan(n=23, nb=18, topo=0, max_active=3)["err"].startswith("no general-contact kernel for this model size")


def test_pack_rows():
    """a pack compiled for the model's own tree before the generic one of its size; packs hold the fp64 full cycle (and the six-dof
    general-contact kernel) only"""
    own = plan(n=37, nb=32, topo=0, tree_match=1)
    other = plan(n=37, nb=32, topo=0, tree_match=0)
    assert own["name"] == "dwbc::dwbc_cycle_kernel_v2w<37, 32, 2, 64, false, dwbc::TopoPack>"
    assert other["name"] == "dwbc::dwbc_cycle_kernel_v2w<37, 32, 2, 64, false, dwbc::TopoGeneric>"
    for tm, tree in ((1, "TopoPack"), (0, "TopoGeneric")):
        big, warm = plans(dict(n=37, nb=32, topo=0, tree_match=tm, B=1025), dict(n=37, nb=32, topo=0, tree_match=tm, B=1025, warm=1, levels=4))
        assert big["name"] == f"dwbc::dwbc_cycle_kernel_v2<37, 32, 2, 64, false, dwbc::{tree}>" and not big["ws_valid_after"]  # (Lds2: no compact map in a pack)
        assert warm["name"] == f"dwbc::dwbc_cycle_kernel_v2<37, 32, 4, 64, true, dwbc::{tree}>" and warm["ws_valid_after"]
        assert big["lds"] == warm["lds"] - 2  # the hand-written table sizes Lds2 as 29000 + levels
        assert plan(n=37, nb=32, topo=0, tree_match=tm, pair_always=1)["threads"] == 64
        assert plan(n=37, nb=32, topo=0, tree_match=tm, max_active=3)["name"] == "dwbc::dwbc_cycle_kernel_gc<37, 32, 64, 6>"
        assert plan(n=37, nb=32, topo=0, tree_match=tm, wide_tasks=1)["err"] == "task levels of more than 6 dof: built in for TOCABI's size only"
        assert plan(n=37, nb=32, topo=0, tree_match=tm, reduced=1)["err"] == "no kernel for this model / number of task levels"
    assert plan(n=23, nb=18, topo=0)["err"] == "no kernel for this model / number of task levels"
