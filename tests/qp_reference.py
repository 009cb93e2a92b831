"""References for the wave-QP probe (tests/qp_probe): the canon oracle on the stacked one-sided form of a probe problem, and an independent
reference in 50-digit mpmath that never calls the oracle.  TEST INFRASTRUCTURE ONLY.

The QP (DESIGN.md "QP canon"):  lexmin(1/2 |x[:t]|^2, 1/2 |x[t:]|^2)  s.t.  A x <= ub, searched on the scaled variables x^ = x / s
(s = 1 for the t task variables, QP_SCALE for the k contact-null ones) as the strictly convex problem min 1/2 |x^|^2 ("Tikhonov").
The point returned is the lexicographic least-norm point ON THE FINAL WORKING SET if every row holds there to `feas` (normalised by the
row norm), else the Tikhonov point.
"""
import numpy as np
from mpmath import mp, mpf

from oracle import orc

mp.dps = 50
QP_SCALE = 1.0e4
RANK_ABS = mpf(10) ** -30  # absolute rank threshold of the pseudo-inverses: a relative one turns an exactly zero projector (working set
                           # with q <= k rows of full rank) into a full-rank matrix of round-off


def stack(p):
    """the stacked one-sided form A x <= ub of a probe problem: row `id` of A is the side of the lane that carries that id"""
    ids = np.concatenate([p["id_hi"][np.isfinite(p["hi"])], p["id_lo"][np.isfinite(p["lo"])]])  # (of the sides that are present)
    R = int(ids.max()) + 1 if (ids >= 0).any() else 0
    A = np.zeros((R, p["nv"]))
    ub = np.zeros(R)
    seen = np.zeros(R, bool)
    for lane in range(64):
        ih, il = int(p["id_hi"][lane]), int(p["id_lo"][lane])
        if ih >= 0 and np.isfinite(p["hi"][lane]):
            A[ih], ub[ih], seen[ih] = p["G"][lane], p["hi"][lane], True
        if il >= 0 and np.isfinite(p["lo"][lane]):
            A[il], ub[il], seen[il] = -p["G"][lane], p["lo"][lane], True
    assert seen.all(), "row ids of the present sides must be 0..R-1"
    return A, ub


def oracle(p):
    """(status, x, sorted working set, steps) of oracle.orc.solve_qp on the stacked form, searched with the problem's vtol"""
    A, ub = stack(p)
    if A.shape[0] == 0:
        return 1, np.zeros(p["nv"]), [], 0
    st, x, act, it = orc.solve_qp(A, ub, p["t"], p["max_iter"], tol=p["vtol"])
    return st, x, act, it


# ---- 50-digit linear algebra on lists of mpf rows
def _dot(a, b):
    return mp.fdot(a, b)


def _matvec(M, v):
    return [_dot(r, v) for r in M]


def _T(M):
    return [list(c) for c in zip(*M)] if M else []


def _solve(M, b):
    return list(mp.lu_solve(mp.matrix(M), mp.matrix(b)))


class Pinv:
    """M^+ and the projector on range(M), the rank decided by an ABSOLUTE threshold: modified Gram-Schmidt with column pivoting gives
    M = Q^T F (Q: r orthonormal vectors, F = Q M: r x n of full row rank), so M^+ = F^T (F F^T)^-1 Q"""

    def __init__(self, M):
        self.m, self.n = len(M), len(M[0]) if M else 0
        self.Q, self.F = [], []
        if self.m == 0 or self.n == 0:
            return
        cols = _T(M)
        res = [list(c) for c in cols]
        for _ in range(min(self.m, self.n)):
            nr = [_dot(c, c) for c in res]
            j = max(range(self.n), key=lambda i: nr[i])
            if mp.sqrt(nr[j]) <= RANK_ABS:
                break
            q = [e / mp.sqrt(nr[j]) for e in res[j]]
            self.Q.append(q)
            for i in range(self.n):
                c = _dot(q, res[i])
                res[i] = [a - c * b for a, b in zip(res[i], q)]
            res[j] = [mpf(0)] * self.m
        if self.Q:
            self.F = [[_dot(q, c) for c in cols] for q in self.Q]
            self.FFt = mp.matrix([[_dot(a, b) for b in self.F] for a in self.F])

    def apply(self, v):
        if not self.Q:
            return [mpf(0)] * self.n
        y = list(mp.lu_solve(self.FFt, mp.matrix(_matvec(self.Q, v))))
        return _matvec(_T(self.F), y)

    def off_range(self, v):
        """(I - M M^+) v"""
        for q in self.Q:
            c = _dot(q, v)
            v = [a - c * b for a, b in zip(v, q)]
        return list(v)


def _row_norm(a, zero_row):
    n = mp.sqrt(_dot(a, a))
    return mpf(1) if n < zero_row else n


def slacks_at(p, x, scale=QP_SCALE):
    """min(hi - g.x, lo + g.x) of the unnormalised row of every lane at x, in mpmath; +inf where both sides are absent"""
    xm = [mpf(float(v)) for v in x[: p["nv"]]]
    out = []
    for lane in range(64):
        gx = _dot([mpf(float(v)) for v in p["G"][lane]], xm)
        sh = mpf(float(p["hi"][lane])) - gx if np.isfinite(p["hi"][lane]) else mp.inf
        sl = mpf(float(p["lo"][lane])) + gx if np.isfinite(p["lo"][lane]) else mp.inf
        out.append(min(sh, sl))
    return out


def mp_reference(p, workset, zero_row=1.0e-9, feas=1.0e-7, scale=QP_SCALE):
    """The answer on the working set `workset` (row ids of the stacked form), from the problem data alone.

    Returns dict: x (the canon's point, floats), x_tik, x_lex, fallback (lexicographic point infeasible), lam_min / lam_max (multipliers of the
    Tikhonov problem), worst (least normalised slack of any row at the Tikhonov point), viol (what the solver reports for this answer)."""
    A, ub = stack(p)
    nv, t = p["nv"], p["t"]
    k = nv - t
    s = [mpf(1)] * t + [mpf(scale)] * k
    Am = [[mpf(float(v)) for v in row] for row in A]
    Gm = [[a * sj for a, sj in zip(row, s)] for row in Am]  # scaled variables
    um = [mpf(float(v)) for v in ub]
    ws = list(workset)
    q = len(ws)
    zr = mpf(zero_row)
    # a numerically zero row (norm of the scaled row below zero_row) is the constraint 0 <= ub: its coefficients are dropped and its slack is
    # taken as it is (dwbc_qp_wave.h).  The oracle keeps the coefficients: its slack of such a row differs by 1e-9 |x| at the most, its x does not.
    # (Where the oracle's x is far from this reference on the zero-row family -- 0.1 relative on two problems -- the cause is another one: an
    # ACTIVE row of norm 2e-9, a genuine row just above the threshold.  The oracle's lexicographic stage solves the normal equations
    # (Ab Ab^T) y = b by Cholesky; their condition number is the squared ratio of the row norms, 1e18 here, the residual of the small row divided
    # by its norm exceeds QP_FEAS_TOL, and the oracle discards its own lexicographic point for the Tikhonov point.  Scaling that row and its
    # bound by 1e6 brings the oracle back to 2e-11 of the lexicographic point.  The point is feasible to 5e-10, so by the canon it is the answer:
    # this reference and the solver, which works on unit-normalised rows, return it.  DESIGN.md, "The solver on its own".)
    zero = [mp.sqrt(_dot(g, g)) < zr for g in Gm]
    Am = [[mpf(0)] * nv if z else a for a, z in zip(Am, zero)]
    Gm = [[mpf(0)] * nv if z else g for g, z in zip(Gm, zero)]
    gn = [_row_norm(g, zr) for g in Gm]   # as the search normalises (scaled row)
    an = [_row_norm(a, zr) for a in Am]   # as the acceptance test of the lexicographic point normalises (row as the reference states it)
    out = {}
    if q == 0:
        xh, lam = [mpf(0)] * nv, []
    else:
        N = [Gm[i] for i in ws]
        b = [um[i] for i in ws]
        y = _solve([[_dot(r1, r2) for r2 in N] for r1 in N], b)  # (N N^T) y = b, x^ = N^T y, multipliers -y
        xh = _matvec(_T(N), y)
        lam = [-v for v in y]
    sl_t = [(um[i] - _dot(Gm[i], xh)) / gn[i] for i in range(len(Gm))]
    out["lam_min"] = float(min(lam)) if lam else 0.0
    out["lam_max"] = float(max(abs(v) for v in lam)) if lam else 0.0
    out["worst"] = float(min(sl_t)) if sl_t else 0.0
    x_tik = [a * sj for a, sj in zip(xh, s)]
    out["x_tik"] = np.array([float(v) for v in x_tik])
    rest = [sl_t[i] for i in range(len(Gm)) if i not in ws]
    viol_t = min(rest) if rest else mpf(0)
    x, viol, fallback = x_tik, viol_t, False
    out["x_lex"] = None
    if k > 0 and t > 0 and q > 0:
        Ad = [Am[i][:t] for i in ws]
        Ac = [Am[i][t:] for i in ws]
        b = [um[i] for i in ws]
        Pc = Pinv(Ac)
        PAd = _T([Pc.off_range(col) for col in _T(Ad)])                              # (I - Ac Ac^+) Ad
        dl = Pinv(PAd).apply(Pc.off_range(b))                                        # stage 1: min |delta|
        c = Pc.apply([bi - _dot(r, dl) for bi, r in zip(b, Ad)])                     # stage 2: min |c|
        x_lex = list(dl) + list(c)
        out["x_lex"] = np.array([float(v) for v in x_lex])
        sl_l = [(um[i] - _dot(Am[i], x_lex)) / an[i] for i in range(len(Am))]
        wl = min(sl_l)
        out["lex_worst"] = float(wl)
        if wl < -mpf(feas):
            fallback = True
        else:
            x, viol = x_lex, wl
    out["fallback"] = fallback
    out["viol"] = float(viol) if viol != mp.inf else 0.0
    out["x"] = np.array([float(v) for v in x])
    return out
