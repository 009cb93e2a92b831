"""Case families and the check of the wave-QP probe (tests/qp_probe): seeded generators, the references they are compared with
(tests/qp_reference.py) and ONE check function, shared by the host test (test_qp_wave_emu.py), the GPU test (test_qp_wave_gpu.py) and
tools/stress_qp.py -- so every build is asked identical things.  TEST INFRASTRUCTURE ONLY.

Discrete outputs (status, steps, working-set size, working set) must equal the oracle's on every family but the three that are degenerate
by design (dependent normals, zero rows, lexicographic edge): there status, the KKT certificate of the returned working set and x are required.
x bars: profiles/qp_probe_tolerances.txt holds, per family and instantiation, the worst |x - x_mp|inf / max(1, |x_mp|inf) of the HOST build
against the 50-digit reference (python -m tests.qp_cases --write-tolerances); the bar is 10 x that value and never below 10 x the unit
round-off of the arithmetic type (the reference itself is rounded to a double; a measured 0 would leave no room for fast_rcp and FMA
contraction on the device).  No bar is derived from GPU output.
"""
import functools
import os
import sys

import numpy as np
import pytest

from tests import qp_reference as ref
from tests.qp_probe import probe

INF = np.inf
N_MP = 64        # problems per family and instantiation certified in mpmath; any further ones are compared with the oracle
VTOL = 1.0e-9    # kQpTol
F32_VTOL, F32_FEAS = 2.0e-5, 1.0e-3  # DWBC_F32_TOL, DWBC_F32_FEAS
DEGENERATE = ("dependent", "zero_rows", "lex_edge")
F32_FAMILIES = ("dense", "product", "infeasible")
ORACLE_OWN_CAP = 2.0e-9  # the largest disagreement of the oracle's x with an exact answer the solver's issue reports (lexicographic problems)
TOL_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "qp_probe_tolerances.txt")


# ------------------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------------------
def svec(nv, t):
    return np.concatenate([np.ones(t), np.full(nv - t, ref.QP_SCALE)])


def problem(nv, t, G2=(), hi2=(), lo2=(), G1=(), hi1=(), vtol=VTOL, max_iter=1000, warm=None, scaled=True, lo_ids=False):
    """two-sided lanes first (id_hi = lane, id_lo = L + lane: the stacked form is [every hi side; the lo sides]), then the one-sided ones; the
    remaining lanes are inert.  scaled: the rows are given on the scaled variables (divided here by the scale of each column).
    lo_ids: the one-sided lanes carry an id for their absent lo side too (nothing may ever match it)"""
    G2, G1 = np.asarray(G2, float).reshape(-1, nv), np.asarray(G1, float).reshape(-1, nv)
    n2, n1 = len(G2), len(G1)
    L = n2 + n1
    assert L <= 64
    G = np.zeros((64, nv))
    hi, lo = np.full(64, INF), np.full(64, INF)
    id_hi, id_lo = np.full(64, -1, np.int32), np.full(64, -1, np.int32)
    G[:n2], G[n2:L] = G2, G1
    if scaled:
        G /= svec(nv, t)
    hi[:n2], lo[:n2], hi[n2:L] = hi2, lo2, hi1
    id_hi[:L] = np.arange(L)
    id_lo[:n2] = L + np.arange(n2)
    if lo_ids:
        id_lo[n2:L] = 1000 + np.arange(n1)
    return dict(nv=nv, t=t, G=G, hi=hi, lo=lo, id_hi=id_hi, id_lo=id_lo, vtol=vtol, max_iter=max_iter, warm=warm, L=L, n2=n2)


def layouts(inst):
    """(nv, t) the instantiation may be given: the standard layout; without lexicographic solve; and, with WS = 1, other splits
    (the lexicographic solve holds KCV contact-null variables at the most: k <= KCV wherever t > 0)"""
    std = (inst.nv, inst.nv - inst.kcv)
    out = [std, (inst.nv, 0), (inst.nv, inst.nv)]
    if inst.ws:
        out += [(inst.nv, inst.nv // 2), (inst.nv - 1, max(2, inst.nv - inst.kcv)), (max(2, inst.nv - 2), max(1, inst.nv - 5))]
    return out


def lex_layouts(inst):
    """the layouts with a lexicographic solve (none for WS = 0 on 6 variables: its standard layout has no task block)"""
    return [(nv, t) for nv, t in layouts(inst) if 0 < t < nv]


def rand_rows(rng, n, nv, t):
    """n rows on the scaled variables; the contact block carries more or less weight than the task block from row set to row set"""
    G = rng.standard_normal((n, nv))
    G[:, t:] *= rng.choice([0.3, 1.0, 5.0])
    return G


def feasible(rng, nv, t, n2, n1, spread=1.5, **kw):
    """rows around a feasible point away from the origin: about half of them are violated at x = 0"""
    xf = rng.standard_normal(nv) * spread
    G2, G1 = rand_rows(rng, n2, nv, t), rand_rows(rng, n1, nv, t)
    m = lambda n: np.abs(rng.standard_normal(n)) * 0.3 + 0.01
    return problem(nv, t, G2, G2 @ xf + m(n2), -(G2 @ xf) + m(n2), G1, G1 @ xf + m(n1), **kw)


def _n(inst, n):
    """problems of a family: half as many on the 18 / 24 variable builds, where the references cost most"""
    return n if inst.nv <= 12 else n // 2


def _vt(inst):
    return F32_VTOL if inst.f32 else VTOL


def fam_dense(inst, n=64, seed=11):
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out = []
    for i in range(n):
        nv, t = lay[i % len(lay)]
        out.append(feasible(rng, nv, t, 0, int(rng.integers(nv, 54)), vtol=_vt(inst)))
    return out


def fam_product(inst, n=64, seed=23):
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    return [feasible(rng, *lay[i % len(lay)], 33, 20, vtol=_vt(inst)) for i in range(n)]


def first_pick(p):
    """(lane, side) of the most violated side at x = 0, as the search normalises"""
    g = p["G"] * svec(p["nv"], p["t"])
    nr = np.linalg.norm(g, axis=1)
    nr[nr < 1e-9] = 1.0
    sh, sl = p["hi"] / nr, p["lo"] / nr
    lane = int(np.argmin(np.minimum(sh, sl)))
    return lane, int(sl[lane] < sh[lane])


def fam_two_sided(inst, n=48, seed=37):
    """narrow slabs: the lo side binds, the hi side binds, and -- kept by the oracle's answer -- the side picked first is dropped and the opposite
    side of the same lane ends in the working set"""
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out, flips, tries = [], 0, 0
    while len(out) < n and tries < 4000:
        tries += 1
        nv, t = lay[tries % len(lay)]
        n2 = int(rng.integers(nv, 40))
        xf = rng.standard_normal(nv) * 1.5
        G2, G1 = rand_rows(rng, n2, nv, t), rand_rows(rng, int(rng.integers(0, 14)), nv, t)
        w = np.abs(rng.standard_normal(n2)) * 0.2 + 0.01  # slab widths
        c = G2 @ xf + (rng.random(n2) - 0.5) * w
        p = problem(nv, t, G2, c + w / 2, -(c - w / 2), G1, G1 @ xf + np.abs(rng.standard_normal(len(G1))) * 0.3 + 0.01)
        st, _, act, _ = ref.oracle(p)
        lane, side = first_pick(p)
        opposite = (p["id_hi"][lane] if side else p["id_lo"][lane]) if lane < p["n2"] else -1
        flip = st == 1 and opposite in act
        lo_binds = any(a >= p["L"] for a in act)
        if flip or (len(out) - flips < n // 2 and lo_binds):
            out.append(p)
            flips += flip
    assert flips >= n // 4, (flips, len(out))
    return out


def vertex(rng, nv, t, extra, cut):
    """q == nv: nv independent rows whose intersection is the closest point of their cone to the origin (positive multipliers), `extra` rows that
    are inactive there and `cut` rows that are satisfied at the origin, violated at the vertex and leave a feasible point"""
    N = rand_rows(rng, nv, nv, t)
    lam = rng.random(nv) + 0.2
    xv = -N.T @ lam
    b = N @ xv
    xf = xv + np.linalg.solve(N, -(rng.random(nv) + 0.1))  # N xf < b
    E = rand_rows(rng, extra, nv, t)
    be = np.maximum(E @ xv, E @ xf) + np.abs(rng.standard_normal(extra)) * 0.3 + 0.05
    C, bc = [], []
    for _ in range(2000):
        if len(C) == cut:
            break
        g = rand_rows(rng, 1, nv, t)[0]
        bb = g @ xf + 0.02
        if bb >= 0 and g @ xv > bb + 0.05:
            C.append(g)
            bc.append(bb)
    assert len(C) == cut
    G1 = np.vstack([N, E] + ([np.array(C)] if cut else []))
    return problem(nv, t, G1=G1, hi1=np.concatenate([b, be, bc]))


def fam_full(inst, n=48, seed=41):
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out = []
    for i in range(n):
        nv, t = lay[i % len(lay)]
        out.append(vertex(rng, nv, t, int(rng.integers(0, 53 - nv - 2)), (i % 3)))  # cut = 0: the vertex stands; 1, 2: it is cut off
    return out


def fam_dependent(inst, n=48, seed=53):
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out = []
    for i in range(n):
        nv, t = lay[i % len(lay)]
        base = feasible(rng, nv, t, 0, int(rng.integers(nv, 40)))
        L = base["L"]
        G = base["G"][:L] * svec(nv, t)
        hi = base["hi"][:L]
        viol = np.argsort(hi / np.linalg.norm(G, axis=1))[:4]  # the most violated rows at the origin: they enter early
        a, b = int(viol[0]), int(viol[1])
        kind = i % 4
        if kind == 0:    # exact duplicates, same and tighter bound
            Gx, hx = [G[a], G[b]], [hi[a], hi[b] - 0.05]
        elif kind == 1:  # anti-parallel pair: with the row it mirrors, a slab (of width 0.1, and of width 0: an equality)
            Gx, hx = [-G[a], -G[b]], [-hi[a] + 0.1, -hi[b]]
        elif kind == 2:  # the sum of two rows, bound a little inside theirs: n lies in the span of the working set when both are active
            Gx, hx = [G[a] + G[b]], [hi[a] + hi[b] - 0.01]
        else:            # a positive multiple, same half-space
            Gx, hx = [3.0 * G[a]], [3.0 * hi[a]]
        out.append(problem(nv, t, G1=np.vstack([G, np.array(Gx)]), hi1=np.concatenate([hi, hx])))
    return out


def fam_zero_rows(inst, n=32, seed=59):
    """exact zero rows (satisfied, and violated by less than vtol), and rows of norm 0.5e-9 / 2e-9 on either side of kQpZeroRow; the tiny rows
    live in the task columns where there are any, so that the scaled and the unscaled row have the same norm"""
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out = []
    for i in range(n):
        nv, t = lay[i % len(lay)]
        base = feasible(rng, nv, t, 0, int(rng.integers(nv, 40)))
        L = base["L"]
        G, hi = base["G"][:L] * svec(nv, t), base["hi"][:L]
        u = np.zeros(nv)
        u[: (t if t > 0 else nv)] = rng.standard_normal(t if t > 0 else nv)
        u /= np.linalg.norm(u)
        # 0.5e-9: a zero row, its bound taken as it is (-5e-10 is within vtol, 1: plainly satisfied); 2e-9: a genuine row -- normalised it asks for
        # u . x <= -0.5 or u . x <= 0.5
        Gx = [np.zeros(nv), np.zeros(nv), 0.5e-9 * u, 0.5e-9 * u, 2e-9 * u, -2e-9 * u]
        hx = [0.0, 1.0, -5e-10, 1.0, (-1e-9 if i % 2 else 1e-9), 1e-9]
        out.append(problem(nv, t, G1=np.vstack([G, np.array(Gx)]), hi1=np.concatenate([hi, hx])))
    return out


def fam_infeasible(inst, n=36, seed=61):
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out = []
    for i in range(n):
        nv, t = lay[i % len(lay)]
        base = feasible(rng, nv, t, int(rng.integers(0, 10)), int(rng.integers(nv, 30)), vtol=_vt(inst))
        L, n2 = base["L"], base["n2"]
        s = svec(nv, t)
        G2, hi2, lo2 = base["G"][:n2] * s, base["hi"][:n2], base["lo"][:n2]
        G1, hi1 = base["G"][n2:L] * s, base["hi"][n2:L]
        kind = i % 3
        if kind == 0:    # empty slab: g.x <= -1 and -g.x <= 0.5
            g = rand_rows(rng, 1, nv, t)
            g /= np.linalg.norm(g)
            G2, hi2, lo2 = np.vstack([G2, g]), np.append(hi2, -1.0), np.append(lo2, 0.5)
        elif kind == 1:  # violated zero row
            G1, hi1 = np.vstack([G1, np.zeros(nv)]), np.append(hi1, -1.0e-3)
        else:            # three half-planes n_i . x <= -1 with normals at 120 degrees in a plane
            e = np.linalg.qr(rng.standard_normal((nv, 2)))[0] if nv >= 2 else None
            if e is None:
                G1, hi1 = np.vstack([G1, [[1.0]], [[-1.0]]]), np.append(hi1, [-1.0, -1.0])
            else:
                nrm = [np.cos(a) * e[:, 0] + np.sin(a) * e[:, 1] for a in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)]
                G1, hi1 = np.vstack([G1] + nrm), np.append(hi1, [-1.0, -1.0, -1.0])
        out.append(problem(nv, t, G2, hi2, lo2, G1, hi1, vtol=_vt(inst)))
    return out


def fam_max_iter(inst, n=24, seed=67):
    n = _n(inst, n)
    out = []
    for p in fam_dense(inst, 2 * n if inst.nv > 12 else n, seed):
        s = ref.oracle(p)[3]
        if s >= 2:
            out += [dict(p, max_iter=s), dict(p, max_iter=s - 1)]
    return out


def fam_layouts(inst, seed=71):
    """every nv in 1..NV; with WS = 1, every t of 0..nv the solver is built for (t = 0, or k = nv - t <= KCV); with WS = 0, no lexicographic
    solve (t = 0, t = nv) and the standard layout.  The 24-variable build has 258 such pairs, two more than a family may hold: (23, 12) and (24, 13), the second
    smallest t > 0 of the two largest nv, are left out, nothing else.  A seeded sample of
    n_mp problems that holds the standard layout comes first -- those are certified in mpmath -- and the others follow, checked against the oracle"""
    rng = np.random.default_rng(seed + inst.index)
    pairs = []
    for nv in range(1, inst.nv + 1):
        if inst.ws:
            ts = [t for t in range(nv + 1) if t == 0 or nv - t <= inst.kcv]  # (k <= KCV wherever there is a lexicographic solve)
        else:
            ts = sorted({0, nv} | ({inst.nv - inst.kcv} if nv == inst.nv else set()))
        pairs += [(nv, t) for t in ts]
    if len(pairs) > 256:
        pairs = [(nv, t) for nv, t in pairs if not (nv >= inst.nv - 1 and t == nv - inst.kcv + 1)]
    out = [feasible(rng, nv, t, int(rng.integers(0, 8)), int(rng.integers(nv, 30))) for nv, t in pairs]
    std = pairs.index((inst.nv, inst.nv - inst.kcv))
    first = [std] + [int(i) for i in rng.permutation(len(out)) if i != std][: n_mp(inst) - 1]
    rest = [i for i in range(len(out)) if i not in set(first)]
    return [out[i] for i in sorted(first) + rest]


def fam_padding(ws, n=40, seed=73):
    """problems of at most 6 variables every build of 6, 9 and 12 variables may be given: the results must not depend on NV"""
    rng = np.random.default_rng(seed + ws)
    out = []
    for i in range(n):
        nv = int(rng.integers(1, 7))
        t = int(rng.integers(0, nv + 1)) if ws else (0 if i % 2 else nv)
        out.append(feasible(rng, nv, t, int(rng.integers(0, 8)), int(rng.integers(nv, 30))))
    return out


def fam_tolerance(inst, n=24, seed=79):
    """a row violated by 5e-8 (normalised): alone at the origin, and at the point where the search of a dense problem ends; each with vtol 1e-9
    (it enters) and 1e-7 (it is left alone).  The search may meet the row earlier on its path, where it is violated by more: kept are the
    problems whose oracle answers differ in that row"""
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out, tries = [], 0
    while len(out) < 2 * n and tries < 20 * n:
        tries += 1
        nv, t = lay[tries % len(lay)]
        s = svec(nv, t)
        g = rand_rows(rng, 1, nv, t)[0]
        if tries % 2 == 0:
            E = rand_rows(rng, 20, nv, t)
            G1, hi1 = np.vstack([E, g]), np.append(np.abs(rng.standard_normal(20)) + 0.1, -5e-8 * np.linalg.norm(g))
        else:
            base = feasible(rng, nv, t, 0, int(rng.integers(nv, 40)))
            L = base["L"]
            st, x, act, _ = ref.oracle(base)
            A, ub = ref.stack(base)
            N = A[act] * s
            xh = N.T @ np.linalg.solve(N @ N.T, ub[act])  # the point the search ends on (the Tikhonov point of the working set)
            G1 = np.vstack([base["G"][:L] * s, g])
            hi1 = np.append(base["hi"][:L], g @ xh - 5e-8 * np.linalg.norm(g))
        pair = [problem(nv, t, G1=G1, hi1=hi1, vtol=vt) for vt in (1.0e-9, 1.0e-7)]
        new = len(G1) - 1
        if new in ref.oracle(pair[0])[2] and new not in ref.oracle(pair[1])[2]:
            out += pair
    return out


def fam_warm(inst, n=20, seed=83):
    """WS = 1: the cold working set, a permutation, a superset with satisfied rows, ids of absent sides and -1 entries"""
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = layouts(inst)
    out = []
    for i in range(n):
        nv, t = lay[i % len(lay)]
        p = feasible(rng, nv, t, int(rng.integers(0, 12)), int(rng.integers(nv, 30)), lo_ids=True)
        st, _, act, _ = ref.oracle(p)
        if st != 1 or not act:
            continue
        R = int(max(p["id_hi"].max(), p["id_lo"][: p["n2"]].max(initial=-1))) + 1
        others = [r for r in range(R) if r not in act]
        qn = inst.qn
        perm = list(rng.permutation(act))
        sup = (perm + list(rng.choice(others, min(len(others), qn - len(act)), replace=False)))[:qn]
        absent = ([1000, 1001, 5000] + perm)[:qn]                   # ids of absent lo sides and ids nobody carries
        holes = [v for a in perm for v in (-1, a)][:qn] if 2 * len(act) <= qn else ([-1] + perm)[:qn]
        for w in (list(act), perm, [int(v) for v in rng.permutation(sup)], absent, holes):
            out.append(dict(p, warm=[int(v) for v in w], cold_act=list(act)))
    return out


def fam_lex_edge(inst, n=40, seed=89):
    """lexicographic solve: contact block rank-deficient by construction (two equal contact columns, a zero contact column), and problems
    whose lexicographic point is infeasible so that the Tikhonov point must be returned (listed first: they are certified in mpmath)"""
    n = _n(inst, n)
    rng = np.random.default_rng(seed + inst.index)
    lay = lex_layouts(inst)
    fall, rest, tries = [], [], 0
    while (len(fall) < 10 or len(rest) < n - 10) and tries < 400:
        tries += 1
        nv, t = lay[tries % len(lay)]
        kind = tries % 3
        xf = rng.standard_normal(nv) * 1.5
        G1 = rand_rows(rng, int(rng.integers(nv, 40)), nv, t)
        if nv - t >= 2 and kind == 1:
            G1[:, nv - 1] = G1[:, t]  # equal columns: c moves freely along e_t - e_(nv-1)
        if nv - t >= 2 and kind == 2:
            G1[:, t + 1] = 0.0        # a contact variable no row touches
        p = problem(nv, t, G1=G1, hi1=G1 @ xf + np.abs(rng.standard_normal(len(G1))) * 0.3 + 0.01)
        st, x, act, _ = ref.oracle(p)
        if st != 1 or not act:
            continue
        r = ref.mp_reference(p, tuple(act))
        p["_mp"] = {tuple(act): r}
        is_fall = r["fallback"]
        if is_fall and len(fall) < 10:
            fall.append(p)
        elif not is_fall and len(rest) < n - 10:
            rest.append(p)
    return fall + rest


FAMILIES = {
    "dense": fam_dense, "product": fam_product, "two_sided": fam_two_sided, "full": fam_full, "dependent": fam_dependent,
    "zero_rows": fam_zero_rows, "infeasible": fam_infeasible, "max_iter": fam_max_iter, "layouts": fam_layouts, "tolerance": fam_tolerance,
    "warm": fam_warm, "lex_edge": fam_lex_edge,
}


def families_of(inst):
    if inst.f32:
        return F32_FAMILIES
    return tuple(f for f in FAMILIES if (inst.ws or f != "warm") and (lex_layouts(inst) or f != "lex_edge"))


@functools.lru_cache(maxsize=None)
def cases(family, inst):
    """(problems, oracle answers) of a family: generated once per process, shared by every test and never changed"""
    ps = FAMILIES[family](inst)
    assert 0 < len(ps) <= 256
    return ps, [ref.oracle(p) for p in ps]


def n_mp(inst):
    return N_MP if inst.nv <= 12 else N_MP // 2  # (a 24-variable problem takes 0.1 s in mpmath)


@functools.lru_cache(maxsize=None)
def _mp_ref(family, inst, b, workset):
    p = cases(family, inst)[0][b]
    if workset in p.get("_mp", {}):  # (a generator that chose the problem by its reference answer)
        return p["_mp"][workset]
    return ref.mp_reference(p, workset, zero_row=inst.zero_row, feas=F32_FEAS if inst.f32 else 1.0e-7)


# ------------------------------------------------------------------------------------------------------------------------------------
# bars
# ------------------------------------------------------------------------------------------------------------------------------------
def unit_roundoff(inst):
    return 2.0 ** -24 if inst.f32 else 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _tolerance_table():
    tab = {}
    with open(TOL_FILE) as f:
        for line in f:
            w = line.split()
            if len(w) >= 3 and not line.startswith("#"):
                tab[(w[0], w[1])] = float(w[2])
    return tab


def x_bar(family, inst):
    return 10.0 * max(_tolerance_table()[(family, inst.name)], unit_roundoff(inst))


# ------------------------------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------------------------------
def relerr(x, xr):
    return float(np.abs(x - xr).max() / max(1.0, np.abs(xr).max()))


def check(family, inst, out, bar=None, label=""):
    """Asserts everything the family requires of the outputs `out` of probe.solve on cases(family, inst).  bar: the x bar (None: x_bar(family, inst);
    inf while the tolerances are being measured).  Returns the figures measured on the way."""
    ps, orc = cases(family, inst)
    if bar is None:
        bar = x_bar(family, inst)
    # (the fp32 build rounds slacks and ratios to 24 bits: a tie the oracle resolves one way may go the other, so its path is not required,
    # its status, certificate and x are)
    strict = family not in DEGENERATE and not inst.f32
    nmp = n_mp(inst)
    u = unit_roundoff(inst)
    feas = F32_FEAS if inst.f32 else 1.0e-7
    worst_mp, worst_orc, orc_own, n_fall = 0.0, 0.0, 0.0, 0
    later = []
    for b, (p, (st_o, x_o, act_o, it_o)) in enumerate(zip(ps, orc)):
        tag = f"{label}{family} {inst.name} problem {b}"
        nv, t, qn = p["nv"], p["t"], inst.qn
        st, it, nact = int(out["status"][b]), int(out["iters"][b]), int(out["nact"][b])
        x, act = out["x"][b], sorted(int(a) for a in out["act"][b] if a >= 0)
        assert st == st_o, (tag, "status", st, st_o)
        assert np.isfinite(out["x"][b]).all() and np.isfinite(out["viol"][b]) and not np.isnan(out["sfin"][b]).any(), (tag, "non-finite output")
        assert (x[nv:] == 0).all(), (tag, "padding of x")
        if inst.ws:
            assert len(act) == nact, (tag, "act entries", act, nact)  # (an inert lane reports id -1: it never entered)
        else:
            assert (out["act"][b] == -1).all(), tag
        if strict and "cold_act" not in p:
            assert it == it_o, (tag, "steps", it, it_o)
            assert nact == len(act_o), (tag, "nact", nact, len(act_o))
            if inst.ws:
                assert act == act_o, (tag, "working set", act, act_o)
        if "cold_act" in p:  # warm start: the path may differ, the end may not
            assert act == p["cold_act"], (tag, "working set of the warm start", act, p["cold_act"])
        # slack of every lane at the returned point, unnormalised; inert lanes: the sentinel
        present = np.isfinite(p["hi"]) | np.isfinite(p["lo"])
        assert (out["sfin"][b][~present] == inst.inf).all(), (tag, "sfin of inert lanes")
        xs = np.where(np.arange(qn) < nv, x, 0.0)[:nv]
        mag = np.abs(p["G"]) @ np.maximum(1.0, np.abs(xs)) + np.where(np.isfinite(p["hi"]), np.abs(p["hi"]), 0) + np.where(np.isfinite(p["lo"]), np.abs(p["lo"]), 0)
        # (a numerically zero row is the constraint 0 <= hi: the solver drops its coefficients)
        Gz = np.where((np.linalg.norm(p["G"] * svec(nv, t), axis=1) < inst.zero_row)[:, None], 0.0, p["G"])
        if b < nmp:
            sref = np.array([float(v) for v in ref.slacks_at(dict(p, G=Gz), xs)])
        else:
            gx = (Gz.astype(np.longdouble) @ xs.astype(np.longdouble))
            sref = np.minimum(p["hi"] - gx, p["lo"] + gx).astype(float)
        serr = np.abs(out["sfin"][b][present] - sref[present])
        assert (serr <= bar * mag[present]).all(), (tag, "sfin", float((serr / np.maximum(mag[present], 1e-300)).max()), bar)
        if st == 0:
            assert (x == 0).all() and nact >= 0, (tag, "x of a failed solve")
            assert out["viol"][b] < -p["vtol"], (tag, "viol of a failed solve", out["viol"][b])
            continue
        if b < nmp:
            # independent certificate and answer, from the problem data and the working set alone
            wset = tuple(act if inst.ws else act_o)
            r = _mp_ref(family, inst, b, wset)
            assert r["lam_min"] >= -1e-9 * max(1.0, r["lam_max"]), (tag, "multiplier", r["lam_min"], r["lam_max"])
            assert r["worst"] >= -p["vtol"], (tag, "row violated at the Tikhonov point of the working set", r["worst"])
            e = relerr(xs, r["x"])
            worst_mp = max(worst_mp, e)
            n_fall += bool(r["fallback"])
            assert e <= bar, (tag, "x against mpmath", e, bar, "fallback" if r["fallback"] else "")
            # |slack error| <= |row|_2 |x error|_2 for a normalised row; and the worst row is chosen on slacks rounded to float (WAVE_ARGMIN_F32,
            # in both arithmetic types): the value reported may be that of a row within 2^-23 relative of the true minimum
            vt = np.sqrt(nv) * bar * max(1.0, np.abs(xs).max()) + 4 * 2.0 ** -23 * abs(r["viol"])
            assert abs(out["viol"][b] - r["viol"]) <= vt, (tag, "viol", out["viol"][b], r["viol"], vt)
            if tuple(act_o) == wset:
                orc_own = max(orc_own, relerr(x_o, r["x"]))
        else:
            later.append((tag, relerr(xs, x_o)))
    # the rest against the oracle: the bar plus ten times the oracle's own error as seen on the problems certified above -- and never more of it
    # than ORACLE_OWN_CAP, so that one certified problem on which the oracle is far off cannot void the bar of the others
    for tag, e in later:
        worst_orc = max(worst_orc, e)
        assert e <= bar + 10.0 * min(max(orc_own, u), ORACLE_OWN_CAP), (tag, "x against the oracle", e, bar, orc_own)
    return dict(worst_mp=worst_mp, worst_orc=worst_orc, orc_own=orc_own, fallbacks=n_fall, n=len(ps))


def check_family_conditions(family, inst):
    """what a family must contain, asserted from the references alone"""
    ps, orc = cases(family, inst)
    if family == "dense":
        assert sum(it > len(act) for _, _, act, it in orc) * 4 >= len(ps), "a quarter of the dense family must drop rows"
    if family == "full":
        assert sum(len(act) == p["nv"] for p, (_, _, act, _) in zip(ps, orc)) * 4 >= len(ps)
        assert sum(it > p["nv"] + 1 for p, (_, _, _, it) in zip(ps, orc)) * 4 >= len(ps), "vertices that are cut off again"
    if family == "two_sided":
        assert sum(any(a >= p["L"] for a in act) for p, (_, _, act, _) in zip(ps, orc)) * 4 >= len(ps)
    if family == "dependent":
        # the added row depends on rows that enter early.  Either it is in the working set in place of one of them, or it stays out; a working
        # set that holds it together with the rows it depends on would be singular.  And the dependent direction is met on the way: rows are
        # dropped (steps > working-set size) on at least a quarter of the family
        for p, (st, _, act, _) in zip(ps, orc):
            if st != 1:  # (an equality may leave nothing feasible: the status alone is compared there)
                continue
            A, _ub = ref.stack(p)
            N = A[act] * svec(p["nv"], p["t"])
            assert np.linalg.matrix_rank(N) == len(act), "dependent rows together in the working set"
        assert sum(it > len(act) for _, _, act, it in orc) * 4 >= len(ps), "dependent normals must force drops"
    if family == "layouts":
        assert {p["nv"] for p in ps} == set(range(1, inst.nv + 1))
        assert any((p["nv"], p["t"]) == (inst.nv, inst.nv - inst.kcv) for p in ps[: n_mp(inst)]), "the standard layout is certified"
        if inst.ws:
            want = {(nv, t) for nv in range(1, inst.nv + 1) for t in range(nv + 1) if t == 0 or nv - t <= inst.kcv}
            missing = want - {(p["nv"], p["t"]) for p in ps}
            assert missing == (set() if inst.nv < 24 else {(23, 12), (24, 13)}), missing
    if family == "infeasible":
        assert all(st == 0 for st, _, _, _ in orc)
    if family == "max_iter":
        assert [st for st, _, _, _ in orc] == [1, 0] * (len(ps) // 2) and len(ps) >= 8
    if family == "tolerance":
        for i in range(0, len(ps), 2):
            new = ps[i]["L"] - 1
            assert new in orc[i][2] and new not in orc[i + 1][2], (i, orc[i][2], orc[i + 1][2])
    if family == "lex_edge":
        nf = sum(bool(_mp_ref(family, inst, b, tuple(orc[b][2]))["fallback"]) for b in range(min(n_mp(inst), len(ps))) if orc[b][0] == 1)
        assert nf >= min(8, n_mp(inst)), ("Tikhonov fallbacks among the certified problems", nf)


def run_family(build, family, inst, threads=64, bar=None, label=""):
    ps, _ = cases(family, inst)
    return check(family, inst, probe.solve(build, inst, ps, threads), bar, label)


def check_refusals(build):
    """the entry validates every size before anything runs: each of these batches is refused with a message and leaves the outputs untouched"""
    ws0, ws1 = probe.INSTANTIATIONS[4], probe.INSTANTIATIONS[5]  # 12 variables, KCV = 6
    rng = np.random.default_rng(5)
    ok = feasible(rng, 12, 6, 4, 20)
    assert (probe.solve(build, ws0, [ok])["status"] == 1).all()
    bad = [
        (ws0, [feasible(rng, 12, 7, 4, 20)], "standard layout"),        # WS = 0 off the standard layout
        (ws0, [feasible(rng, 11, 5, 4, 20)], "standard layout"),
        (ws1, [feasible(rng, 12, 3, 4, 20)], "contact-null"),           # k = 9 > KCV with a lexicographic solve
        (ws1, [dict(ok, t=13)], "t 13"),
        (ws1, [dict(ok, t=-1)], "t -1"),
        (ws1, [dict(ok, max_iter=0)], "max_iter"),
        (ws1, [dict(ok, max_iter=2001)], "max_iter"),
        (ws1, [dict(ok, vtol=float("nan"))], "vtol"),
        (ws0, [dict(ok, warm=[1, 2])], "warm"),
        (ws1, [ok] * 1025, "batch"),
    ]
    for inst, ps, word in bad:
        with pytest.raises(RuntimeError, match=word):
            probe.solve(build, inst, ps)
    # (nv beyond QN is a record the packer cannot lay out: hand the entry a valid record with that size alone changed)
    rows, ids, par, vtol, warm = probe.pack(ws1, [ok])
    par[0, 0] = 13
    with pytest.raises(RuntimeError, match="nv 13"):
        probe.solve_packed(build, ws1, 64, rows, ids, par, vtol, warm)
    with pytest.raises(RuntimeError, match="threads"):
        probe.solve(build, ws1, [ok], threads=96)


def write_tolerances(path=TOL_FILE):
    lines = ["# worst |x - x_mp|inf / max(1, |x_mp|inf) of the HOST build of the wave-QP probe against the 50-digit mpmath reference, per family and",
             "# instantiation (python -m tests.qp_cases --write-tolerances).  tests/qp_cases.py sets the bar of both builds at 10 x this value, and",
             "# never below 10 x the unit round-off of the arithmetic type.  oracle_own: the same figure of the oracle's x; fallbacks: certified",
             "# problems that return the Tikhonov point because the lexicographic point is infeasible.",
             "# family instantiation worst_x_vs_mp worst_x_vs_oracle oracle_own certified fallbacks problems"]
    for inst in probe.instantiations("emu"):
        for fam in families_of(inst):
            r = run_family("emu", fam, inst, bar=1e300)
            lines.append(f"{fam} {inst.name} {r['worst_mp']:.3e} {r['worst_orc']:.3e} {r['orc_own']:.3e} {min(n_mp(inst), r['n'])} {r['fallbacks']} {r['n']}")
            print(lines[-1], flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--write-tolerances" in sys.argv:
        write_tolerances()
