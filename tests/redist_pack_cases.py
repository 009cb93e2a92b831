"""Inputs and restatement references of the redistribution tests on models other than TOCABI (tests/test_redistribute_sizes_emu.py,
tests/test_redistribute_packs_gpu.py), computed once per (model, B).

The recipe is redist_cases.state_set's on the models of tests/test_model_packs.py: states of variant_states(mo, B, seed=7) (states_43(B, 7)
for the 43-dof surgery model), contacts CONTACTS_2 on the ankle-roll links, torque limit 300 Nm; tau_in = the restatement's own full-cycle
torque (pelvis 6D over upper-body rotation, both feet down) + NwJw d, d = 10 default_rng(11).standard_normal((B, 6)).  Flags: double
support, every fourth instance (1, 5, 9, ...: left foot and right foot in turn) in single support, and instance 6 with no contact.
The bars are redist_cases' (1e-6 Nm, 1e-5 N), the premises redist_cases.check_premises."""
import functools

import numpy as np

from tests import cases
from tests import redist_cases as rc

TAU_LIM = 300.0
SIZES = {"fixed_head": (37, 32), "fixed_arms": (23, 18), "surgery_43": (43, 38)}
BATCH = {"fixed_head": 48, "fixed_arms": 48, "surgery_43": 32}  # the GPU tests' batch sizes


def flag_mix(B):
    fl = np.ones((B, 2), np.uint8)
    fl[1::8, 1] = 0  # left foot only
    fl[5::8, 0] = 0  # right foot only
    fl[6] = 0        # in the air
    return fl


@functools.lru_cache(maxsize=None)
def model(name):
    """(oracle model dict, (left foot, right foot, upper body) link ids).  The 43-dof model needs the built library (its surgery is
    the library's)."""
    if name == "surgery_43":
        from tests.test_model_packs import model_43

        _, mo = model_43()
        return dict(mo, nb=38, ndof=43), (6, 12, 15)
    import os
    import tempfile

    from oracle import urdf_model
    from tests.test_model_packs import VARIANTS

    if name == "tocabi":  # (39 / 34 itself, for the built-in kernel on TopoGeneric)
        mo = cases.tocabi_model()
    else:
        with tempfile.TemporaryDirectory() as d:
            mo = urdf_model.load_urdf(cases.variant_urdf(os.path.join(d, name + ".urdf"), VARIANTS[name][0]))
    names = list(mo["names"])
    return mo, tuple(names.index(n) for n in ("L_AnkleRoll_Link", "R_AnkleRoll_Link", "Upperbody_Link"))


def contacts_of(links):
    return [dict(cc, link=l) for cc, l in zip(cases.CONTACTS_2, links[:2])]


def cycle_of(mo, links, tau_lim=None, consts=None):
    """the restatement set up for the model; consts: (2, 4) lx, ly, mu, muz of the two contacts (None: CONTACTS_2's)"""
    from oracle.dwbc_np import Cycle

    c = Cycle(mo)
    for i, cc in enumerate(contacts_of(links)):
        v = (cc["lx"], cc["ly"], cc["mu"], cc["muz"]) if consts is None else consts[i]
        c.add_contact(cc["link"], cc["point"], v[0], v[1], v[2], v[3])
    c.add_task(0, 0, 0, (0, 0, 0))
    c.add_task(1, 6, links[2], (0, 0, 0))
    c.set_torque_limit(np.full(mo["ndof"] - 6, TAU_LIM) if tau_lim is None else tau_lim)
    return c


def states(name, mo, B):
    from tests.test_model_packs import states_43, variant_states

    return states_43(B, 7) if name == "surgery_43" else variant_states(mo, B, seed=7)


@functools.lru_cache(maxsize=None)
def state_set(name, B, scale=10.0):
    """dict like redist_cases.state_set (+ fstar): inputs and the restatement's answers; read-only arrays"""
    mo, links = model(name)
    q, fstar = states(name, mo, B)
    flags = flag_mix(B)
    d = scale * np.random.default_rng(11).standard_normal((B, 6))
    cyc = cycle_of(mo, links)
    m = cyc.m
    out = dict(q=q, flags=flags, fstar=fstar, tau_feasible=np.zeros((B, m)), tau_in=np.zeros((B, m)), status=np.zeros(B, np.int32), tau=np.zeros((B, m)),
               cf=np.zeros((B, 6)), wrench=np.zeros((B, 2, 12)), nwjw=np.zeros((B, m, 6)))
    for b in range(B):
        on = [bool(f) for f in flags[b]] if flags[b].any() else [True, True]  # (the instance in the air is handed the standing torque)
        tf = cyc.run(q[b], on, [fstar[b, :6], fstar[b, 6:9]])
        out["tau_feasible"][b] = tf
        out["tau_in"][b] = tf + (cyc.NwJw @ d[b] if cyc.NwJw.shape[1] == 6 and flags[b].all() else 0.0)
        st, dt, c, w, nw = rc.redistribute_ref(cyc, q[b], flags[b], out["tau_in"][b])
        out["status"][b], out["tau"][b], out["cf"][b], out["wrench"][b] = st, dt, c, w
        out["nwjw"][b, :, : nw.shape[1]] = nw
    for v in out.values():
        v.setflags(write=False)
    return out


def check_flag_mix_outputs(got, ref):
    """single support: zero torque, status 1, the wrench of tau_in (six entries) in both rows; no contact: zeros and status 1"""
    nact = ref["flags"].sum(axis=1)
    single, free = nact == 1, nact == 0
    assert single.sum() >= 2 and free.sum() == 1 and (nact == 2).sum() >= len(nact) // 2
    assert (got["status"][single | free] == 1).all()
    assert np.abs(got["tau"][single]).max() == 0.0 and np.abs(got["cf"][single]).max() == 0.0
    assert (got["wrench"][single][:, 0] == got["wrench"][single][:, 1]).all()
    assert np.abs(ref["wrench"][single][:, 0, :6]).max(axis=1).min() > 1.0  # (the reference has a wrench there to compare with)
    assert np.abs(got["wrench"][single][:, 0] - ref["wrench"][single][:, 0]).max() <= rc.TOL_WRENCH
    for k in ("tau", "cf", "wrench"):
        assert np.abs(got[k][free]).max() == 0.0, k
