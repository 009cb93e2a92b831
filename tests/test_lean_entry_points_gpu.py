"""gpu: what the lean launches share in the C-ABI (libdwbc_amd/csrc/dwbc_capi.hip: one event-bracket timer behind every
dwbc_batch_time_*, one get / bind / bytes / refusal path behind the four output families of dwbc_fields.h), on TOCABI, fp64, B = 4, both
feet registered.

  - the timed launches leave what a single launch leaves, to the bit (the kernels are deterministic and the inputs do not change), and
    return a finite time > 0;
  - one refusal ladder over gravity compensation, the link query, the dynamics and the contact space, with the messages written out
    below as they stood before the four families shared their code -- the differences between the families that had to survive it are
    in the table, one line each."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import cases
from tests import dynamics_cases as dc

pytestmark = pytest.mark.gpu

B = 4
GRAV, LINK_QUERY, DYNAMICS, CONTACT_SPACE = "grav", "link_query", "dynamics", "contact_space"
REDIST = ("redist_tau", "redist_cf", "redist_wrench", "redist_status")


def _batch(tasks=False, dtype="f64"):
    import libdwbc_amd as D

    wbc = D.Batch(D.Model.from_urdf(cases.URDF), B, device=0, dtype=dtype)
    for c in cases.CONTACTS_2:
        wbc.add_contact(c["link"], c["point"], c["lx"], c["ly"], c["mu"], c["muz"])
    if tasks:
        wbc.add_task(0, D.TASK_LINK_6D, 0)
        wbc.add_task(1, D.TASK_LINK_ROTATION, 15)
    wbc.set_torque_limit(np.array(cases.TAU_LIM))
    return wbc


def _posed(tasks=False):
    q, flags, fstar = cases.synth_batch(B, seed=7)
    wbc = _batch(tasks)
    wbc.set_state(q, dc.velocities(B, 39))
    wbc.set_contact(flags)
    if tasks:
        wbc.set_fstar_all(fstar)
    return wbc


def _all(outputs):
    return [k for k in outputs if k != "status"]


def _timed_cases():
    """name -> (tasks, prepare, single launch, read every output, timed launches)"""
    from libdwbc_amd import batch as bt

    tau_in = 20.0 * np.random.default_rng(11).standard_normal((B, 33))
    redist = lambda w: {k: w.get(k) for k in REDIST}
    return dict(
        grav=(False, lambda w: None, lambda w: w.grav_compensation(), lambda w: w.grav_outputs(), lambda w: w.time_grav(3)),
        dynamics=(False, lambda w: w.set_dynamics_outputs(_all(bt.DYNAMICS_OUTPUTS)), lambda w: w.update_dynamics(), lambda w: w.dynamics(), lambda w: w.time_dynamics(3)),
        contact_space=(False, lambda w: w.set_contact_space_outputs(_all(bt.CONTACT_SPACE_OUTPUTS)), lambda w: w.calc_contact_constraint(), lambda w: w.contact_space(),
                       lambda w: w.time_contact_space(3)),
        redistribute=(False, lambda w: w.set_torque_input(tau_in), lambda w: w.redistribute(), redist, lambda w: w.time_redistributes(3)),
        redistribute_add_gravity=(False, lambda w: w.set_torque_input(tau_in), lambda w: w.redistribute(add_gravity=True),
                                  lambda w: dict(redist(w), **{"grav_" + k: v for k, v in w.grav_outputs().items()}), lambda w: w.time_redistributes(3, add_gravity=True)),
        solves=(True, lambda w: None, lambda w: w.solve(), lambda w: {k: w.get(k) for k in ("tau", "wrench", "status", "diag")}, lambda w: w.time_solves(3)),
    )


@pytest.mark.parametrize("case", ["grav", "dynamics", "contact_space", "redistribute", "redistribute_add_gravity", "solves"])
def test_timed_launches_leave_what_a_single_launch_leaves(case):
    tasks, prepare, single, read, timed = _timed_cases()[case]
    wbc = _posed(tasks)
    prepare(wbc)
    single(wbc)
    want = read(wbc)
    assert len(want) >= 3 and all(v.size > 0 for v in want.values())
    assert any(np.abs(v).max() > 0 for k, v in want.items() if not k.endswith("status")), "the single launch wrote nothing"
    ms = timed(wbc)
    got = read(wbc)
    print(f"{case}: {ms:.4f} ms for 3 launches")
    assert math.isfinite(ms) and ms > 0.0
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), k
    wbc.close()


# ---- the refusal ladder.  Per family: entry-point infix, outputs, the request the ladder makes (set), the launch, an output of the
# request and one left out of it (None: the family has no partial request), and its messages.  None: the family has no such refusal.
LADDER = {
    GRAV: dict(
        count=3, asked=0, left_out=None,
        unknown="gravity compensation: unknown output", unknown_bit=None, no_request=None, not_asked=None,
        not_run="no gravity-compensation output yet: call dwbc_batch_grav_compensation (or dwbc_batch_redistribute with DWBC_REDIST_ADD_GRAVITY) first",
        launch_f32="gravity compensation: fp64 batches only"),  # no request to miss: the plan's refusal
    LINK_QUERY: dict(
        count=4, asked=1, left_out=3,
        unknown="link query: unknown output", unknown_bit=None, no_request="no link query: call dwbc_batch_set_link_query first",
        not_asked="link query: set without Jacobians (dwbc_batch_set_link_query with want_jacobians = 1)",
        not_run="no link-query output yet: call dwbc_batch_update_kinematics first",
        launch_f32="no link query: call dwbc_batch_set_link_query first"),  # the missing request before the plan
    DYNAMICS: dict(
        count=7, asked=3, left_out=1,
        unknown="dynamics: unknown output", unknown_bit="dynamics: unknown output bit (the outputs are 1u << DWBC_DYN_A .. 1u << DWBC_DYN_STATUS)",
        no_request="no dynamics request: call dwbc_batch_set_dynamics_outputs first",
        not_asked="dynamics: this output was not asked for (dwbc_batch_set_dynamics_outputs)",
        not_run="no dynamics output yet: call dwbc_batch_update_dynamics first",
        launch_f32="no dynamics request: call dwbc_batch_set_dynamics_outputs first"),  # the missing request before the plan
    CONTACT_SPACE: dict(
        count=11, asked=0, left_out=3,
        unknown="contact space: unknown output", unknown_bit="contact space: unknown output bit (the outputs are 1u << DWBC_CS_J_C .. 1u << DWBC_CS_STATUS)",
        no_request="no contact-space request: call dwbc_batch_set_contact_space_outputs first",
        not_asked="contact space: this output was not asked for (dwbc_batch_set_contact_space_outputs)",
        not_run="no contact-space output yet: call dwbc_batch_calc_contact_constraint first",
        launch_f32="contact space: fp64 batches only"),  # the plan before the missing request
}
TOO_SMALL = "output buffer too small"


class _Family:
    """the entry points of one family on one batch, called through ctypes so that every return value and message is seen"""

    def __init__(self, wbc, fam):
        from libdwbc_amd import _lib

        self.w, self.fam, self.L, self.err = wbc, fam, wbc._L, _lib.last_error
        self.launch_name = {GRAV: "grav_compensation", LINK_QUERY: "update_kinematics", DYNAMICS: "update_dynamics", CONTACT_SPACE: "calc_contact_constraint"}[fam]

    def bytes(self, what):
        return getattr(self.L, f"dwbc_batch_{self.fam}_bytes")(self.w._h, what)

    def get(self, what, nbytes=1 << 20):
        """(return value, message, the output's bytes)"""
        buf = np.zeros(nbytes, np.uint8)
        ok = getattr(self.L, f"dwbc_batch_get_{self.fam}")(self.w._h, what, buf.ctypes.data, C.c_size_t(nbytes))
        return ok, (None if ok else self.err()), buf[: self.bytes(what)].copy()

    def bind(self, what, ptr):
        ok = getattr(self.L, f"dwbc_batch_bind_{self.fam}")(self.w._h, what, C.c_void_p(ptr) if ptr else None)
        return ok, (None if ok else self.err())

    def launch(self):
        ok = getattr(self.L, f"dwbc_batch_{self.launch_name}")(self.w._h)
        return ok, (None if ok else self.err())

    def request(self, partial):
        """the family's request: without (partial) or with the output the ladder leaves out; gravity compensation has none to make"""
        if self.fam == LINK_QUERY:
            self.w.set_link_query([0, 15], jacobians=not partial)
        elif self.fam == DYNAMICS:
            self.w.set_dynamics_outputs(["G"] if partial else ["G", "A_inv"])
        elif self.fam == CONTACT_SPACE:
            self.w.set_contact_space_outputs(["J_C"] if partial else ["J_C", "N_C"])

    def drop(self):
        if self.fam == LINK_QUERY:
            self.w.set_link_query([])
        elif self.fam == DYNAMICS:
            self.w.set_dynamics_outputs([])
        elif self.fam == CONTACT_SPACE:
            self.w.set_contact_space_outputs([])

    def set_mask(self, mask):
        ok = getattr(self.L, f"dwbc_batch_set_{self.fam}_outputs")(self.w._h, C.c_uint(mask))
        return ok, (None if ok else self.err())


@pytest.mark.parametrize("fam", [GRAV, LINK_QUERY, DYNAMICS, CONTACT_SPACE])
def test_refusal_ladder(fam):
    import torch

    s = LADDER[fam]
    asked, left_out = s["asked"], s["left_out"]
    wbc = _posed()
    f = _Family(wbc, fam)
    # an output that does not exist: get, bind, bytes -- before anything else is looked at
    for what in (-1, s["count"]):
        assert f.get(what)[:2] == (0, s["unknown"]) and f.bind(what, None) == (0, s["unknown"]) and f.bytes(what) == 0
    # nothing requested yet
    if s["no_request"]:
        assert f.get(asked)[:2] == (0, s["no_request"]) and f.bind(asked, None) == (0, s["no_request"]) and f.launch() == (0, s["no_request"])
        assert [f.bytes(w) for w in range(s["count"])] == [0] * s["count"]
    f.request(partial=True)
    sizes = [f.bytes(w) for w in range(s["count"])]
    assert sizes[asked] > 0
    # before any launch
    assert f.get(asked)[:2] == (0, s["not_run"])
    # an output that is not part of the request: no size, no get, no bind
    if left_out is not None:
        assert sizes[left_out] == 0
        assert f.get(left_out)[:2] == (0, s["not_asked"]) and f.bind(left_out, None) == (0, s["not_asked"])
    assert f.launch() == (1, None)
    ok, why, want = f.get(asked)
    assert (ok, why) == (1, None) and want.size == sizes[asked] and want.any()
    assert f.get(asked, nbytes=sizes[asked] - 1)[:2] == (0, TOO_SMALL)
    if left_out is not None:
        assert f.get(left_out)[:2] == (0, s["not_asked"])
    # an unknown bit: refused, and the request and its outputs stay as they were
    if s["unknown_bit"]:
        assert f.set_mask((1 << s["count"]) | 1) == (0, s["unknown_bit"])
        assert [f.bytes(w) for w in range(s["count"])] == sizes
        ok, why, again = f.get(asked)
        assert (ok, why) == (1, None) and (again == want).all()
    # an empty request, then a launch; a new request resets what the last launch left
    if s["no_request"]:
        f.drop()
        assert [f.bytes(w) for w in range(s["count"])] == [0] * s["count"]
        assert f.launch() == (0, s["no_request"]) and f.get(asked)[:2] == (0, s["no_request"])
        f.request(partial=False)
        assert f.bytes(left_out) > 0 and f.bytes(asked) == sizes[asked]
        assert f.get(asked)[:2] == (0, s["not_run"]) and f.get(left_out)[:2] == (0, s["not_run"])
        assert f.launch() == (1, None)
        ok, why, want = f.get(asked)
        assert (ok, why) == (1, None) and want.size == sizes[asked] and want.any()
    # bound to a tensor, unbound, launched: the batch's own buffer again, with the unbound result
    t = torch.full((sizes[asked],), 0x55, dtype=torch.uint8, device="cuda:0")
    assert f.bind(asked, t.data_ptr()) == (1, None)
    assert f.get(asked)[:2] == (0, s["not_run"])  # (what the batch's own buffer held is not in the bound one)
    assert f.launch() == (1, None)
    wbc.sync()
    assert (t.cpu().numpy() == want).all()
    t.fill_(0x55)
    assert f.bind(asked, None) == (1, None)
    assert f.get(asked)[:2] == (0, s["not_run"])
    assert f.launch() == (1, None)
    ok, why, again = f.get(asked)
    assert (ok, why) == (1, None) and (again == want).all() and (t.cpu().numpy() == 0x55).all()
    wbc.close()
    # an fp32 batch has no lean kernel: which refusal a launch without a request meets first differs between the families
    f32 = _batch(dtype="f32")
    assert _Family(f32, fam).launch() == (0, s["launch_f32"])
    f32.close()
