"""Shared test inputs: the reference's asserted states (tests/dwbc_test.cpp:48-77,152-181,262-308 in
/root/reference) and the seeded synthetic TOCABI batches of SURVEY.md section 8d.  The set-up and the input recipe live in the
package (libdwbc_amd/workloads.py: the bench's product engine imports nothing under tests/); this module re-exports them and adds
what only the tests need (golden readers, the oracle's model, pack / URDF-variant helpers)."""
import os

import numpy as np

from libdwbc_amd.workloads import (  # noqa: F401
    CONTACTS_2, CONTACTS_4, FOOT_POINT, FSTAR_CASE, Q_CASE, TASK_LINK_6D, TASK_LINK_ROTATION, TASKS_2LEVEL, TASKS_3LEVEL_SWING_L,
    TASKS_3LEVEL_SWING_R, TAU_LIM, TOCABI_URDF, synth_batch, yaw_quat,
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
URDF = TOCABI_URDF


def tocabi_model():
    from oracle import urdf_model

    js = os.path.join(GOLDEN, "tocabi_model.json")
    if os.path.exists(js):
        return urdf_model.model_from_json(js)
    return urdf_model.load_urdf(URDF)


def golden(case, name):
    from oracle.dwbc_np import read_golden

    return read_golden(os.path.join(GOLDEN, "cases", str(case), name))


def ensure_pack(model, tree=False):
    """the kernel pack of a model size other than TOCABI's: __graft_entry__.build() makes the ones the tests use; only a missing
    one is compiled here (two minutes of hipcc).  tree=True: the pack built for this model's own kinematic tree"""
    import libdwbc_amd as D
    from libdwbc_amd.batch import tree_tag

    name = f"libdwbc_pack_{model.ndof}_{model.nb}"
    if tree:
        name += "_t" + tree_tag([max(int(p), 0) for p in model.arrays()["parent"]])
    path = os.path.join(os.path.dirname(os.path.abspath(D.__file__)), name + ".so")
    if not os.path.exists(path):
        D.build_pack(model, tree=tree)
    return path


# ---- variants of the TOCABI fixture with joints fixed (models of other sizes for the kernel packs; RBDL merges fixed joints)
HEAD_JOINTS = ["Neck_Joint", "Head_Joint"]


def variant_urdf(path_out, fixed):
    import re

    txt = open(URDF).read()
    for j in fixed:
        txt, n = re.subn(r'(name="%s"\s+type=)"revolute"' % j, r'\1"fixed"', txt)
        assert n == 1, j
    with open(path_out, "w") as f:
        f.write(txt)
    return str(path_out)


# ---- hierarchies of one to four levels on the product kernels (every level at most 6 dof: no general-contact kernel)
TASKS_1LEVEL = [TASKS_2LEVEL[0]]
# pelvis 6D / upper-body rotation / left hand 6D / right hand 6D: 21 task dof
TASKS_4LEVEL = TASKS_2LEVEL + [[(TASK_LINK_6D, 23, (0, 0, 0))], [(TASK_LINK_6D, 33, (0, 0, 0))]]


def hierarchy_batch(B, levels, seed, yaw=False, free=False, mixed=False):
    """synth_batch states posed for a hierarchy of `levels` levels.  Returns (tasks, q, flags, fstar).
    1: pelvis 6D; 2: TASKS_2LEVEL; 3: swing foot (TASKS_3LEVEL_SWING_R, left-foot support: the swing foot cannot also be a
    contact); 4: TASKS_4LEVEL, the hands' f* a seeded uniform.  mixed: LR / L / R flags per instance (ignored at 3 levels);
    free: a third of the instances with no active contact."""
    mode = "L" if levels == 3 else ("mixed" if mixed else "LR")
    q, flags, fstar = synth_batch(B, seed=seed, yaw=yaw, contact_mode=mode, levels=3 if levels == 3 else 2)
    if free:
        flags[::3] = 0
    if levels == 1:
        return TASKS_1LEVEL, q, flags, fstar[:, :6].copy()
    if levels == 2:
        return TASKS_2LEVEL, q, flags, fstar
    if levels == 3:
        return TASKS_3LEVEL_SWING_R, q, flags, fstar
    hands = 0.5 * np.random.default_rng(seed + 1).uniform(-1, 1, size=(B, 12))
    return TASKS_4LEVEL, q, flags, np.concatenate([fstar, hands], axis=1)


# ---- launch routes of the full-model cycle (dwbc_capi.hip launch()): a test that runs an optional path (dump record, warm start,
# trajectories, COM / custom levels, hqp = false) at a small batch gets the wide extras build; `capped` forces the build batches
# beyond four instances per CU run (DWBC_NO_WIDE: the register-capped extras build on the Lds2 map)
CAPPED_EXTRAS = "dwbc::dwbc_cycle_kernel_v2<39, 34, {L}, 64, true, dwbc::TopoTocabi>"


def set_route(monkeypatch, route):
    assert route in ("natural", "capped"), route
    for k in ("DWBC_NO_WIDE", "DWBC_NO_PAIR", "DWBC_NO_LEAN", "DWBC_PAIR_ALWAYS"):
        monkeypatch.delenv(k, raising=False)
    if route == "capped":
        monkeypatch.setenv("DWBC_NO_WIDE", "1")


def check_route(wbc, route, levels):
    """after a solve with an optional path on: the capped route really ran the capped extras build"""
    if route == "capped":
        assert wbc.kernel_name() == CAPPED_EXTRAS.format(L=levels), wbc.kernel_name()
        assert wbc.launch_info()[0] == 64
