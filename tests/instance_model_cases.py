"""Inputs and restatement references of the per-instance model tests (tests/test_instance_model_*.py), computed once and left unchanged.

Models: TOCABI with every link randomised per instance.  All draws come from one default_rng(31), instance by instance, and for each
instance in this order, one factor per link: mass x U(0.8, 1.2); the inertia about the COM scaled by the same factor; COM + U(-0.01, 0.01) m
per axis; p_T[1:] x U(0.97, 1.03) (the joint offsets: link lengths).  R_T and the joint axes stay the model's.

States: cases.hierarchy_batch(B, L, seed=20261021 + L, yaw=True), and the same with mixed=True (per-instance LR / L / R flags; not at three
levels, where the swing foot cannot be a contact too).  Contacts CONTACTS_2, limits TAU_LIM; bars: the suite's 1e-6 Nm and 1e-5 N against
the restatement.  The reference is the C restatement (oracle.orc) with orc.make_model(arrays of instance i) per instance.

Every comparison first asserts two premises on the restatement alone: status 1 on at least 0.9 B, and at least half the instances moved by
more than 1e-3 Nm against the shared model."""
import functools

import numpy as np

from tests import cases

B = 24
TOL_TAU = 1e-6     # Nm
TOL_WRENCH = 1e-5  # N
MOVED = 1e-3       # Nm
XTOL = 1e-8        # Nm: the project's bar between two routes / builds on the same states
SETS = ("yaw", "mixed")


def exists(levels, state):
    return not (state == "mixed" and levels == 3)


def _freeze(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def base_arrays():
    m = cases.tocabi_model()
    out = dict(nb=int(m["nb"]), ndof=int(m["ndof"]), parent=np.asarray(m["parent"], np.int32))
    for k, shape in (("R_T", (3, 3)), ("p_T", (3,)), ("axis", (3,)), ("mass", ()), ("com", (3,)), ("inertia", (3, 3))):
        out[k] = np.asarray(m[k], np.float64).reshape((out["nb"],) + shape)
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def fields(n=B):
    """dict of mass (n, nb), inertia (n, nb, 3, 3), com (n, nb, 3), p_T (n, nb, 3): the recipe above"""
    m = base_arrays()
    nb = m["nb"]
    rng = np.random.default_rng(31)
    out = dict(mass=np.zeros((n, nb)), inertia=np.zeros((n, nb, 3, 3)), com=np.zeros((n, nb, 3)), p_T=np.zeros((n, nb, 3)))
    for i in range(n):
        f = rng.uniform(0.8, 1.2, nb)
        out["mass"][i] = m["mass"] * f
        out["inertia"][i] = m["inertia"] * f[:, None, None]
        out["com"][i] = m["com"] + rng.uniform(-0.01, 0.01, (nb, 3))
        out["p_T"][i] = m["p_T"]
        out["p_T"][i, 1:] *= rng.uniform(0.97, 1.03, nb - 1)[:, None]
    return _freeze(out)


def arrays(i, n=B):
    """the model of instance i as a dict of arrays (orc.make_model, Model.from_arrays, oracle.dwbc_np.Cycle)"""
    f = fields(n)
    return dict(base_arrays(), mass=f["mass"][i], inertia=f["inertia"][i], com=f["com"][i], p_T=f["p_T"][i])


def pack(arrs):
    """(nb, 25) body table of a model given as arrays, in the library's layout: R_T[9] p_T[3] axis[3] mass com[3] Icom xx xy xz yy yz zz
    (written out here, independently of Model.instance_model, which the tests compare with it)"""
    nb = int(arrs["nb"])
    t = np.zeros((nb, 25))
    t[:, 0:9] = np.asarray(arrs["R_T"]).reshape(nb, 9)
    t[:, 9:12] = arrs["p_T"]
    t[:, 12:15] = arrs["axis"]
    t[:, 15] = arrs["mass"]
    t[:, 16:19] = arrs["com"]
    t[:, 19:25] = np.asarray(arrs["inertia"]).reshape(nb, 9)[:, [0, 1, 2, 4, 5, 8]]
    return t


@functools.lru_cache(maxsize=None)
def tables(n=B):
    """(n, nb, 25): the record of the batch"""
    t = np.stack([pack(arrays(i, n)) for i in range(n)])
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def states(levels, state, n=B):
    """(tasks, q, flags, fstar)"""
    assert state in SETS and exists(levels, state)
    tasks, q, flags, fstar = cases.hierarchy_batch(n, levels, seed=20261021 + levels, yaw=True, mixed=state == "mixed")
    _freeze((q, flags, fstar))
    return tasks, q, flags, fstar


def orc_cycle(arrs_list, tasks, q, flags, fstar, tau_lim=cases.TAU_LIM):
    """(tau (n, 3, m), wrench (n, 12), status) of the restatement, instance i on the model arrs_list[i]"""
    from oracle import orc

    S = orc.make_setup(cases.CONTACTS_2, tasks, tau_lim)
    outs = [orc.cycle_batch(orc.make_model(a), S, q[i : i + 1], flags[i : i + 1], fstar[i : i + 1], 1)[:3] for i, a in enumerate(arrs_list)]
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(3))


@functools.lru_cache(maxsize=None)
def reference(levels, state, n=B):
    """restatement with the per-instance models; read-only"""
    tasks, q, flags, fstar = states(levels, state, n)
    return _freeze(orc_cycle([arrays(i, n) for i in range(n)], tasks, q, flags, fstar))


@functools.lru_cache(maxsize=None)
def shared_reference(levels, state, n=B):
    """restatement with the one model for all; read-only"""
    from oracle import orc

    tasks, q, flags, fstar = states(levels, state, n)
    return _freeze(orc.cycle_batch(orc.make_model(cases.tocabi_model()), orc.make_setup(cases.CONTACTS_2, tasks, cases.TAU_LIM), q, flags, fstar, 0)[:3])


def check_premises(ref, base, what=""):
    st = ref[2]
    n = len(st)
    assert (st == 1).sum() >= 0.9 * n, f"{what}: restatement status 1 on {(st == 1).sum()} of {n}"
    d = np.abs(ref[0].sum(axis=1) - base[0].sum(axis=1)).max(axis=1)
    moved = d > MOVED
    print(f"{what}: restatement status 1 on {(st == 1).sum()} of {n}; moved by {d.min():.2f} to {d.max():.2f} Nm, more than {MOVED} Nm: {moved.sum()} of {n}")
    assert moved.sum() >= 0.5 * n, f"{what}: only {moved.sum()} of {n} instances differ from the shared model's answer"


def compare(got_tau, got_wr, got_st, ref, what=""):
    tau_r, wr_r, st_r = ref
    assert (got_st == st_r).all(), (what, np.nonzero(got_st != st_r)[0])
    ok = st_r == 1
    assert np.isfinite(got_tau).all(), what
    e_tau = float(np.abs(got_tau[ok] - tau_r[ok]).max())
    e_wr = float(np.abs(got_wr[ok] - wr_r[ok]).max())
    print(f"{what}: worst |d tau| = {e_tau:.3e} Nm, worst |d wrench| = {e_wr:.3e} N over {int(ok.sum())} instances")
    assert e_tau <= TOL_TAU, (what, e_tau)
    assert e_wr <= TOL_WRENCH, (what, e_wr)
    return e_tau, e_wr
