"""Cases, 50-digit mpmath references and checks of the wave-routine probe (tests/wave_probe): the device-only bodies behind the
DWBC_HOST_EMU forks -- cross-lane primitives, scalar math, wave_gemm, the inverses and the batched row products -- and the routines
of the general-contact kernel (section 6: the rank-revealing pseudo-inverse, the pivoted Gauss-Jordan inverse, the register-sweep
inverses, the run-time sized matrix-core product) and the two in-place matrix-core tiles of the cycle (section 7: contact_gram and
wrench_maps), each alone.

Both builds of the probe run the same cases against the same references: tests/test_wave_probe_emu.py (host emulation: validates the
cases and the references, and is where the bars of the inverses come from) and tests/test_wave_probe_gpu.py (the device bodies).
Every bar is either exactness, a bound derived from the arithmetic (written next to it), a figure the issue of this probe sets, or --
the inverses -- 10 x the worst figure of the HOST build on the same instantiation and never below 10 (the rule of tests/qp_cases.py;
profiles/wave_probe_tolerances.txt, written by ``python -m tests.wave_cases --write-tolerances``).  No bar comes from GPU output.

Each ``check_*`` runs ONE launch per instantiation (the unit matrices of wave_gemm take three: 1275 problems) and returns the figures
it measured.
"""
import functools
import os
import sys

import numpy as np
from mpmath import mp, mpf

from tests.wave_probe import probe

mp.dps = 50
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_FILE = os.path.join(ROOT, "profiles", "wave_probe_tolerances.txt")
DEV_FILE = os.path.join(ROOT, "profiles", "wave_probe_device_figures.txt")
U64, U32 = 2.0 ** -53, 2.0 ** -24
LANE = np.arange(64)


def unit(f32):
    return U32 if f32 else U64


def rnd(a, f32):
    """the values as the build's arithmetic type holds them (the references take the SAME inputs)"""
    return np.asarray(a, np.float32).astype(np.float64) if f32 else np.asarray(a, np.float64)


def mpv(a):
    return [mpf(float(v)) for v in np.ravel(a)]


def gamma(n, u=U64):
    return n * u / (1.0 - n * u)


# ====================================================================================================================================
# 1. cross-lane primitives
# ====================================================================================================================================
def _lane_record(val, src=None, flag=None, usrc=0):
    key = LANE.astype(float)  # every call site passes key = lane (see wave_probe_body.h): asserted below for every case
    src = (LANE * 7 + 3) % 64 if src is None else src
    flag = np.zeros(64) if flag is None else flag
    return np.concatenate([val, key, src.astype(float), flag]), usrc


@functools.lru_cache(maxsize=None)
def lanes_cases(f32):
    """list of (group, record, usrc, extra).  Groups: onehot, ones, ints, reals (sums and scans); min_each, inf63, near_tie, tie, zeros
    (arg-min); nan (WAVE_ARGMIN_F32 with no lane comparing equal)"""
    rng = np.random.default_rng(101)
    out = []
    for b in range(64):
        v = np.zeros(64)
        v[b] = -2.5
        out.append(("onehot", *_lane_record(v, src=(LANE * 7 + b) % 64, flag=(LANE == b).astype(float), usrc=b), None))
    out.append(("ones", *_lane_record(np.ones(64), usrc=63), None))
    top = 2 ** 17 if f32 else 2 ** 20  # (fp32: 64 x 2^17 = 2^23 keeps every partial sum exact in 24 bits)
    for _ in range(32):
        out.append(("ints", *_lane_record(rng.integers(-top + 1, top, 64).astype(float), usrc=int(rng.integers(64))), None))
    for _ in range(32):
        v = rnd(rng.standard_normal(64) * 2.0 ** rng.integers(-40, 41, 64), f32)
        out.append(("reals", *_lane_record(v, src=rng.integers(0, 64, 64), usrc=int(rng.integers(64))), None))
    for b in range(64):  # the minimum in each lane in turn; negative and mixed-sign values; a smaller value outside row 1 for most b
        v = np.round(rng.uniform(-10.0, 10.0, 64) * 1024.0) / 1024.0
        v += LANE * 2.0 ** -12  # (distinct: multiples of 2^-10 plus a lane mark below that grid)
        v[b] = -20.0 - b
        out.append(("min_each", *_lane_record(v, usrc=b), None))
    for b in range(64):
        v = np.full(64, 1.0e300)  # (DWBC_QP_INF in the build's type once loaded)
        v[b] = 0.75 * b - 10.0
        out.append(("inf63", *_lane_record(v, usrc=b), None))
    if not f32:  # (a float widened to double has no set bit among the 7 the device drops: no such pair exists in the fp32 build)
        for t in range(32):
            lo_lane, n_lane = (16, 16) if t % 2 else (0, 64)  # (half of the pairs inside row 1)
            i, j = sorted(lo_lane + rng.choice(n_lane, 2, replace=False))
            base = np.float64(rng.uniform(0.5, 4.0) * (1 if rng.random() < 0.5 else -1)).view(np.uint64) & ~np.uint64(127)
            lo = rng.choice(128, 2, replace=False).astype(np.uint64)
            v = rng.uniform(5.0, 9.0, 64)
            v[i], v[j] = (base | lo[0]).view(np.float64), (base | lo[1]).view(np.float64)
            out.append(("near_tie", *_lane_record(v), (int(i), int(j))))
    for _ in range(32):
        lanes = np.sort(rng.choice(64, int(rng.integers(2, 6)), replace=False))
        v = rng.uniform(1.0, 2.0, 64)
        v[lanes] = -3.25 if rng.random() < 0.5 else 0.375
        out.append(("tie", *_lane_record(rnd(v, f32)), tuple(int(l) for l in lanes)))
    for _ in range(16):
        lanes = np.sort(rng.choice(64, 4, replace=False))
        v = rng.uniform(1.0, 2.0, 64)
        v[lanes] = [0.0, -0.0, 0.0, -0.0]
        rng.shuffle(v[lanes])
        out.append(("zeros", *_lane_record(rnd(v, f32)), tuple(int(l) for l in lanes)))
    out.append(("nan", *_lane_record(np.full(64, np.nan)), None))
    for g, rec, usrc, extra in out:
        assert (rec[64:128] == LANE).all(), "keys increase with the lane"
    return out


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def check_lanes(build, f32, threads=64):
    cs = lanes_cases(f32)
    name = "lanes_f32" if f32 else "lanes"
    o = probe.run(build, name, np.stack([c[1] for c in cs]), np.array([[c[2]] for c in cs]), threads)
    u = unit(f32)
    inf = float(np.float32(1.0e30)) if f32 else 1.0e300
    worst = 0.0
    for b, (g, rec, usrc, extra) in enumerate(cs):
        tag = f"{build} {name} t{threads} problem {b} ({g})"
        val = rec[:64].copy()
        val[val >= inf] = inf
        src, flag = rec[128:192].astype(int), rec[192:256]
        r = o[b]
        assert (r[10:16] == probe.SENTINEL).all(), tag
        assert (r[208:272] == -1.0).all(), (tag, "element 0 of the scanned array")
        # broadcasts and shuffles move bits
        assert np.array_equal(_bits(r[80:144]), _bits(val[src])), (tag, "SHFL")
        assert np.array_equal(_bits(r[144:208]), _bits(val[src])), (tag, "SHFLA")
        assert _bits(r[7]) == _bits(val[usrc]) and _bits(r[8]) == _bits(val[usrc]) and r[9] == usrc, (tag, "BCAST")
        assert r[1] == (1.0 if flag.any() else 0.0), (tag, "WAVE_ANY")
        if g in ("onehot", "ones", "ints", "reals"):
            S = mpf(0)
            Sa = mpf(0)
            for l in range(64):
                S += mpf(float(val[l]))
                Sa += abs(mpf(float(val[l])))
                # any association order: each result passes through at most 63 additions -> 64 u sum|x| (componentwise, first order
                # bound gamma_63 <= 64 u); exact inputs whose partial sums are all representable give the exact result
                bar = 0.0 if g != "reals" else 64.0 * u * float(Sa)
                e = float(abs(mpf(float(r[16 + l])) - S))
                assert e <= bar, (tag, "WAVE_PREFIX_A", l, r[16 + l], float(S), e, bar)
                worst = max(worst, e / (u * float(Sa))) if g == "reals" and Sa > 0 else worst
            e = float(abs(mpf(float(r[0])) - S))
            assert e <= bar, (tag, "WAVE_SUM", r[0], float(S), e, bar)
        if g == "ones":
            assert r[0] == 64.0 and (r[16:80] == LANE + 1.0).all(), tag
        if g in ("onehot", "ones", "ints", "min_each", "inf63", "tie"):
            # exact arg-min, ties to the smaller lane (= the smaller key); fp32-distinct values, so WAVE_ARGMIN_F32 picks the same lane
            w = int(np.argmin(val))
            assert (r[2], r[3]) == (val[w], w), (tag, "WAVE_ARGMIN", r[2:4], val[w], w)
            w1 = 16 + int(np.argmin(val[16:32]))
            assert (r[4], r[5]) == (val[w1], w1), (tag, "WAVE_ARGMIN_ROW1", r[4:6], val[w1], w1)
            with np.errstate(over="ignore"):
                v32 = val.astype(np.float32)
            assert r[6] == int(np.argmin(v32)), (tag, "WAVE_ARGMIN_F32", r[6], int(np.argmin(v32)))
        if g == "near_tie":
            i, j = extra
            assert r[3] in (i, j) and _bits(r[2]) == _bits(val[int(r[3])]), (tag, "WAVE_ARGMIN", r[2:4])
            if 16 <= i < 32:
                assert r[5] in (i, j) and _bits(r[4]) == _bits(val[int(r[5])]), (tag, "WAVE_ARGMIN_ROW1", r[4:6])
            assert r[6] == min(i, j), (tag, "WAVE_ARGMIN_F32: equal floats, first lane")
        if g == "zeros":
            assert int(r[3]) in extra and _bits(r[2]) == _bits(val[int(r[3])]), (tag, "WAVE_ARGMIN", r[2:4])
            assert r[6] == extra[0], (tag, "WAVE_ARGMIN_F32: zeros of either sign compare equal, first lane")
        if g == "nan":
            assert r[6] == 0, (tag, "WAVE_ARGMIN_F32 with no lane comparing equal")
    return dict(worst_sum=worst, n=len(cs))


def check_lanes_refusals(build):
    import pytest

    idx, fam, nin, nip, nout = probe.table(build)["lanes"]
    good = np.stack([lanes_cases(False)[0][1]])
    for kw, word in ((dict(threads=96), "threads"), (dict(B=0), "batch"), (dict(B=probe.MAX_B + 1), "batch"), (dict(index=999), "out of range"),
                     (dict(ip=64), "source lane"), (dict(ip=-1), "source lane"), (dict(nin=nin - 1), "input record"),
                     (dict(nout=nout + 1), "output record"), (dict(fam=3), "family")):
        B = kw.get("B", 1)
        din = np.zeros(max(B, 1) * kw.get("nin", nin))
        din[:nin - 1] = good[0, :nin - 1]
        ip = np.full(max(B, 1) * nip, kw.get("ip", 0), np.int32)
        out = np.full(max(B, 1) * kw.get("nout", nout), probe.SENTINEL)
        with pytest.raises(RuntimeError, match=word):
            probe.run_raw(build, kw.get("fam", fam), kw.get("index", idx), kw.get("threads", 64), B, din, ip, out)
        assert (out == probe.SENTINEL).all()
    for name, ip in (("spd_small", [13]), ("spd_small", [0]), ("chol6", [7]), ("chol6_x3", [1, 7, 0]), ("math", [3])):
        sz = probe.sizes(build, name)
        with pytest.raises(RuntimeError, match="outside"):
            probe.run(build, name, np.zeros((1, sz[0])), np.array([ip]))


# ====================================================================================================================================
# 2. scalar math
# ====================================================================================================================================
def _pad64(x, fill=1.0):
    x = np.asarray(x, np.float64)
    n = (-len(x)) % 64
    return np.concatenate([x, np.full(n, fill)]).reshape(-1, 64), len(x)


@functools.lru_cache(maxsize=None)
def rcp_inputs(f32, both_signs):
    rng = np.random.default_rng(211)
    one = np.float32(1.0) if f32 else np.float64(1.0)
    two = one + one
    mant = [float(one), float(np.nextafter(one, two)), 1.5, float(np.nextafter(two, one))]
    emax = 60 if f32 else 200
    xs = []
    for e in range(-emax, emax + 1):
        ms = mant + list(rnd(rng.uniform(1.0, 2.0, 4), f32))
        xs += [m * 2.0 ** e for m in ms]
    xs = np.array(xs)
    return np.concatenate([xs, -xs]) if both_signs else xs


def check_rcp_rsqrt(build, f32, op, threads=64):
    """fast_rcp (op 0) / fast_rsqrt (op 1).  Bars: 2 u and 4 u relative (fp32: 4 u32) -- the last Newton step with an exact residual FMA
    leaves the rounding of the final FMA (u) plus what the squared error of the step before adds; set by the issue of this probe"""
    x = rcp_inputs(f32, op == 0)
    X, n = _pad64(x)
    name = "math_f32" if f32 else "math"
    o = probe.run(build, name, X, np.full((len(X), 1), op), threads)[:, :64].ravel()[:n]
    u = unit(f32)
    bar = (4.0 if (f32 or op == 1) else 2.0) * u
    worst, wx = 0.0, None
    for xi, ri in zip(x, o):
        ref = 1 / mpf(float(xi)) if op == 0 else 1 / mp.sqrt(mpf(float(xi)))
        e = float(abs(mpf(float(ri)) - ref) / abs(ref))
        if e > worst:
            worst, wx = e, xi
    print(f"{build} {name} op {op} t{threads}: worst relative error {worst / u:.3f} u at x = {wx!r} (bar {bar / u:.0f} u, {n} arguments)")
    assert worst <= bar, (build, name, op, worst / u, wx)
    return dict(worst_u=worst / u, n=n)


@functools.lru_cache(maxsize=None)
def sincos_inputs():
    rng = np.random.default_rng(223)
    base = [0.0, 1e-300, -1e-300, 2.0 ** -27, -(2.0 ** -27)]
    k = 1
    while k * np.pi / 4 <= 33.0:
        base += [k * np.pi / 4, -k * np.pi / 4]
        k += 1
    xs = []
    for v in base:
        xs += [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]
    n_special = len(xs)
    xs += list(rng.uniform(-np.pi, np.pi, 4096)) + list(rng.uniform(-33.0, 33.0, 4096))
    wide = rng.uniform(-1.0e5, 1.0e5, 4096)  # recorded, not asserted
    return np.array(xs), n_special, wide


@functools.lru_cache(maxsize=None)
def _sincos_ref():
    xs, _, wide = sincos_inputs()
    return [(mp.sin(mpf(float(v))), mp.cos(mpf(float(v)))) for v in np.concatenate([xs, wide])]


def check_sincos(build, threads=64):
    """sincos_r in double.  Bar: the header's own claim, 1.3e-16 absolute, plus half an ulp of 1.0 (the reference is exact, the claim was
    measured against long double); |s^2 + c^2 - 1| <= 4 u.  The worst case over +-1e5 rad is returned, not asserted."""
    xs, nsp, wide = sincos_inputs()
    allx = np.concatenate([xs, wide])
    X, n = _pad64(allx)
    o = probe.run(build, "math", X, np.full((len(X), 1), 2), threads)
    s, c = o[:, :64].ravel()[:n], o[:, 64:].ravel()[:n]
    ref = _sincos_ref()
    bar = 1.3e-16 + 2.0 ** -53
    worst = worst_wide = worst_unit = 0.0
    wx = None
    for i in range(n):
        e = max(float(abs(mpf(float(s[i])) - ref[i][0])), float(abs(mpf(float(c[i])) - ref[i][1])))
        if i < len(xs):
            un = float(abs(mpf(float(s[i])) ** 2 + mpf(float(c[i])) ** 2 - 1))
            worst_unit = max(worst_unit, un)
            if e > worst:
                worst, wx = e, allx[i]
        else:
            worst_wide = max(worst_wide, e)
    print(f"{build} sincos_r t{threads}: worst |error| {worst:.3e} at x = {wx!r} (bar {bar:.3e}); |s^2+c^2-1| {worst_unit / U64:.2f} u (bar 4 u); "
          f"over +-1e5 rad {worst_wide:.3e} (recorded)")
    assert worst <= bar, (build, worst, wx)
    assert worst_unit <= 4.0 * U64, (build, worst_unit / U64)
    return dict(worst=worst, worst_unit_u=worst_unit / U64, worst_wide=worst_wide, n=n)


# ====================================================================================================================================
# 3. wave_gemm
# ====================================================================================================================================
GEMM_SHAPES = [(16, 16, 4), (17, 15, 5), (1, 1, 1), (12, 12, 39), (33, 6, 12), (6, 9, 33), (39, 16, 12), (39, 7, 18)]
GEMM_INSTS = [(f"gemm_{m}_{n}_{k}" + ("_fc" if fc else ""), m, n, k, fc, False) for m, n, k in GEMM_SHAPES for fc in (False, True)]
GEMM_INSTS.append(("gemm_12_12_39_fc_over", 12, 12, 39, True, True))


@functools.lru_cache(maxsize=None)
def gemm_cases(MR, NCV, KV):
    """(kind, A, B, C0): small integers (exact), 1e300 in the last row of A and the last column of B (what the clamped duplicate rows
    and columns compute must not be stored), reals with an exponent spread and cancelling rows"""
    rng = np.random.default_rng(1000 * MR + 31 * NCV + KV)
    cs = []
    for _ in range(4):
        cs.append(("ints", rng.integers(-9, 10, (MR, KV)).astype(float), rng.integers(-9, 10, (KV, NCV)).astype(float),
                   rng.integers(-99, 100, (MR, NCV)).astype(float)))
    for _ in range(2):
        A, B = rng.integers(1, 10, (MR, KV)).astype(float), rng.integers(1, 10, (KV, NCV)).astype(float)
        A[-1, :] = 1.0e300
        B[:, -1] = 1.0e300
        cs.append(("huge", A, B, rng.integers(1, 100, (MR, NCV)).astype(float)))
    for _ in range(6):
        A = rng.standard_normal((MR, KV)) * 2.0 ** rng.integers(-20, 21, (MR, KV))
        B = rng.standard_normal((KV, NCV)) * 2.0 ** rng.integers(-20, 21, (KV, NCV))
        C0 = rng.standard_normal((MR, NCV))
        if MR > 1 and KV > 1:  # a row whose products cancel against each other and against C0
            A[0, 1:] = A[0, 0]
            B[1:, :] = -B[:1, :] / (KV - 1)
            C0[0, :] = 0.0
        cs.append(("reals", A, B, C0))
    return cs


@functools.lru_cache(maxsize=None)
def _gemm_ref(MR, NCV, KV, fc):
    """per case: the exact result and the exact |C0| + |A||B|, both as mp matrices (nested lists)"""
    out = []
    for kind, A, B, C0 in gemm_cases(MR, NCV, KV):
        Am, Bm = [[mpf(float(v)) for v in r] for r in A], [[mpf(float(v)) for v in r] for r in B]
        D = [[(mpf(float(C0[i, j])) if fc else mpf(0)) + sum(Am[i][k] * Bm[k][j] for k in range(KV)) for j in range(NCV)] for i in range(MR)]
        Ab = [[(abs(mpf(float(C0[i, j]))) if fc else mpf(0)) + sum(abs(Am[i][k] * Bm[k][j]) for k in range(KV)) for j in range(NCV)] for i in range(MR)]
        out.append((D, Ab))
    return out


def _gemm_unpack(o, MR, NCV, KV, over, tag, A=None):
    """checks the frame, the index notes and what lies outside MR x NCV; returns the result block"""
    NF = (MR + 2) * ((KV if over else NCV) + 2)
    F = o[:NF].reshape(MR + 2, -1)
    idx = o[NF:].reshape(64, 6)
    assert (idx[:, :3].min(0) == 0).all() and (idx[:, 3:].max(0) == [MR - 1, KV - 1, NCV - 1]).all(), (tag, "accessor indices", idx.min(0), idx.max(0))
    assert (idx[:, :3] >= 0).all() and (idx[:, 3:] <= [MR - 1, KV - 1, NCV - 1]).all(), (tag, "an accessor was called outside the matrices")
    border = np.ones_like(F, bool)
    border[1:-1, 1:-1] = False
    if over:
        assert np.isnan(F[border]).all(), (tag, "the frame of A")
        assert np.array_equal(F[1:-1, 1 + NCV:-1], A[:, NCV:]), (tag, "columns of A beyond the result")
    else:
        assert (F[border] == probe.FRAME_SENTINEL).all(), (tag, "stored outside MR x NCV")
    return F[1:-1, 1:1 + NCV]


def check_gemm(build, name, MR, NCV, KV, fc, over, threads=64):
    cs = gemm_cases(MR, NCV, KV)
    din = np.stack([np.concatenate([A.ravel(), B.ravel(), C0.ravel()]) for _, A, B, C0 in cs])
    o = probe.run(build, name, din, None, threads)
    ref = _gemm_ref(MR, NCV, KV, fc)
    g = gamma(KV + 1)  # KV products and KV additions onto C0 in ANY order the matrix core takes: gamma_{KV+1} (|C0| + |A||B|)
    worst = 0.0
    for b, (kind, A, B, C0) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind})"
        D = _gemm_unpack(o[b], MR, NCV, KV, over, tag, A)
        Dr, Ab = ref[b]
        for i in range(MR):
            for j in range(NCV):
                if kind == "ints":
                    assert D[i, j] == float(Dr[i][j]), (tag, i, j, D[i, j], float(Dr[i][j]))
                elif Dr[i][j] > mpf(1.7e308):
                    assert D[i, j] == np.inf, (tag, i, j, D[i, j])
                else:
                    assert np.isfinite(D[i, j]), (tag, i, j, D[i, j])
                    e = float(abs(mpf(float(D[i, j])) - Dr[i][j]))
                    bar = g * float(Ab[i][j])
                    assert e <= bar, (tag, i, j, D[i, j], float(Dr[i][j]), e, bar)
                    if Ab[i][j] > 0:
                        worst = max(worst, e / (U64 * float(Ab[i][j])))
    return dict(worst_u=worst, n=len(cs))


def check_gemm_units(build, threads=64):
    """e_i e_k^T . e_k e_j^T for every (i, k, j) of (17, 15, 5): exactly e_i e_j^T -- a transposed or permuted operand layout moves the one"""
    MR, NCV, KV = 17, 15, 5
    trip = [(i, k, j) for i in range(MR) for k in range(KV) for j in range(NCV)]
    for c0 in range(0, len(trip), 425):
        part = trip[c0:c0 + 425]
        din = np.zeros((len(part), MR * KV + KV * NCV + MR * NCV))
        for b, (i, k, j) in enumerate(part):
            din[b, i * KV + k] = 1.0
            din[b, MR * KV + k * NCV + j] = 1.0
        o = probe.run(build, "gemm_17_15_5", din, None, threads)
        for b, (i, k, j) in enumerate(part):
            D = _gemm_unpack(o[b], MR, NCV, KV, False, f"{build} unit ({i},{k},{j}) t{threads}")
            E = np.zeros((MR, NCV))
            E[i, j] = 1.0
            assert np.array_equal(D, E), (build, "unit matrices", (i, k, j), np.argwhere(D != E))
    return dict(n=len(trip))


# ====================================================================================================================================
# 5. lds_rows_dot / lds_rows_axpy
# ====================================================================================================================================
# name: NR, NC, MODE, OFF, NO
DOT_INSTS = {"dot_33_6_6_3_0": (33, 6, 0, 0, 33), "dot_1_33_34_1_0": (1, 33, 0, 0, 1), "dot_12_12_12_4_0": (12, 12, 0, 0, 12),
             "dot_39_12_12_2_1": (39, 12, 1, 0, 39), "dot_6_33_34_3_0_off6_no14": (6, 33, 0, 6, 14), "dot_12_12_12_4_0_unaligned": (12, 12, 0, 0, 12)}
AXPY_INSTS = {"axpy_6_14_14_3": (6, 14), "axpy_6_8_8_3": (6, 8)}


def check_rows_dot(build, name, threads=64):
    NR, NC, MODE, OFF, NO = DOT_INSTS[name]
    rng = np.random.default_rng(7000 + 97 * NR + NC + MODE + OFF)
    cs = []
    for kind in ("ints",) * 3 + ("reals",) * 5:
        if kind == "ints":
            A, x, o0 = rng.integers(-99, 100, (NR, NC)), rng.integers(-99, 100, (64, NC)), rng.integers(-999, 1000, (64, NO))
        else:
            A = rng.standard_normal((NR, NC)) * 2.0 ** rng.integers(-12, 13, (NR, NC))
            x = rng.standard_normal((64, NC)) * 2.0 ** rng.integers(-12, 13, (64, NC))
            o0 = rng.standard_normal((64, NO))
        cs.append((kind, A.astype(float), x.astype(float), o0.astype(float)))
    o = probe.run(build, name, np.stack([np.concatenate([A.ravel(), x.ravel(), o0.ravel()]) for _, A, x, o0 in cs]), None, threads)
    worst = 0.0
    for b, (kind, A, x, o0) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind})"
        R = o[b].reshape(64, NO)
        keep = np.ones(NO, bool)
        keep[OFF:OFF + NR] = False
        assert np.array_equal(R[:, keep], o0[:, keep]), (tag, "entries outside the output slice")
        Am = [[mpf(float(v)) for v in r] for r in A]
        for lane in range(0, 64, 1 if kind == "ints" else 7):
            xm = mpv(x[lane])
            for r in range(NR):
                d = sum(Am[r][i] * xm[i] for i in range(NC))
                da = sum(abs(Am[r][i] * xm[i]) for i in range(NC))
                exp = -d + mpf(float(o0[lane, OFF + r])) if MODE else d
                expa = da + abs(mpf(float(o0[lane, OFF + r]))) if MODE else da
                got = R[lane, OFF + r]
                assert np.isfinite(got), (tag, lane, r, got)
                e = float(abs(mpf(float(got)) - exp))
                # NC products, each through fewer than NC additions (+ the subtraction of MODE 1), in any order: gamma_NC (gamma_{NC+1})
                bar = 0.0 if kind == "ints" else gamma(NC + MODE) * float(expa)
                assert e <= bar, (tag, lane, r, got, float(exp), e, bar)
                if kind == "reals" and expa > 0:
                    worst = max(worst, e / (U64 * float(expa)))
    return dict(worst_u=worst, n=len(cs))


def check_rows_axpy(build, name, threads=64):
    NR, NC = AXPY_INSTS[name]
    rng = np.random.default_rng(8000 + 97 * NR + NC)
    cs = []
    for kind in ("ints",) * 3 + ("reals",) * 5:
        if kind == "ints":
            A, x, a0 = rng.integers(-99, 100, (NR, NC)), rng.integers(-99, 100, (64, NR)), rng.integers(-999, 1000, (64, NC))
        else:
            A = rng.standard_normal((NR, NC)) * 2.0 ** rng.integers(-12, 13, (NR, NC))
            x = rng.standard_normal((64, NR)) * 2.0 ** rng.integers(-12, 13, (64, NR))
            a0 = rng.standard_normal((64, NC))
        cs.append((kind, A.astype(float), x.astype(float), a0.astype(float)))
    o = probe.run(build, name, np.stack([np.concatenate([A.ravel(), x.ravel(), a0.ravel()]) for _, A, x, a0 in cs]), None, threads)
    worst = 0.0
    for b, (kind, A, x, a0) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind})"
        R = o[b].reshape(64, NC)
        Am = [[mpf(float(v)) for v in r] for r in A]
        for lane in range(0, 64, 1 if kind == "ints" else 7):
            xm = mpv(x[lane])
            for p in range(NC):
                exp = mpf(float(a0[lane, p])) + sum(Am[r][p] * xm[r] for r in range(NR))
                expa = abs(mpf(float(a0[lane, p]))) + sum(abs(Am[r][p] * xm[r]) for r in range(NR))
                got = R[lane, p]
                assert np.isfinite(got), (tag, lane, p, got)
                e = float(abs(mpf(float(got)) - exp))
                bar = 0.0 if kind == "ints" else gamma(NR + 1) * float(expa)  # NR products accumulated onto acc: gamma_{NR+1}
                assert e <= bar, (tag, lane, p, got, float(exp), e, bar)
                if kind == "reals" and expa > 0:
                    worst = max(worst, e / (U64 * float(expa)))
    return dict(worst_u=worst, n=len(cs))


# ====================================================================================================================================
# 4. inverses
# ====================================================================================================================================
SWEEP_INSTS = {"sweep_tree39": 39, "sweep_tree_lds39": 39, "sweep_tree_lds_multi39": 39, "sweep_dense33": 33, "sweep_lds33": 33}
SMALL_INSTS = ("spd_small", "spd12_lds", "spd12_lds_inplace", "chol6", "chol6_x3")


def _mp_inverse(A):
    return np.array(mp.inverse(mp.matrix([[mpf(float(v)) for v in r] for r in A])).tolist(), dtype=object)


def _f(M):
    return np.array([[float(v) for v in r] for r in M]) if M.ndim == 2 else np.array([float(v) for v in M])


def _gfig(X, Xm, kappa):
    """g = |X - X_mp|max / (u kappa_2(A) |X_mp|max)"""
    err = max(float(abs(mpf(float(X[i, j])) - Xm[i, j])) for i in range(X.shape[0]) for j in range(X.shape[1]))
    nrm = max(float(abs(v)) for v in Xm.ravel())
    return err / (U64 * kappa * nrm), nrm


def tocabi_model():
    """the oracle's TOCABI model (read from the stored json, without loading the library as tests/cases.py does)"""
    from oracle import urdf_model

    return urdf_model.model_from_json(os.path.join(ROOT, "tests", "golden", "tocabi_model.json"))


def tocabi_relatives():
    """the coupling pattern of TOCABI's mass matrix (dof i and dof j couple iff one's body is an ancestor of the other's), from the model"""
    par = list(tocabi_model()["parent"])
    nb = len(par)
    body = [0] * 6 + list(range(1, nb))

    def anc(a, b):
        while b > a:
            b = max(par[b], 0)
        return a == b

    n = nb + 5
    return np.array([[anc(body[i], body[j]) or anc(body[j], body[i]) for j in range(n)] for i in range(n)])


@functools.lru_cache(maxsize=None)
def sweep_cases(NN):
    """(kind, A, rhs): A (NN x NN) SPD with the pattern the sweep assumes, rhs (NN x (64 - NN)) riding along; the last one indefinite"""
    from oracle import dwbc_np

    rng = np.random.default_rng(4000 + NN)
    model = tocabi_model()
    qrng = np.random.default_rng(29)  # (the same 16 joint states for both widths)
    mass = []
    for _ in range(16):  # q = [x y z qx qy qz joints.. qw]: random base pose, joints within +-1.2 rad
        quat = qrng.standard_normal(4)
        quat /= np.linalg.norm(quat)
        q = np.concatenate([qrng.uniform(-1.0, 1.0, 3), quat[:3], qrng.uniform(-1.2, 1.2, model["ndof"] - 6), quat[3:]])
        mass.append(dwbc_np.crba(model, q))
    cs = []
    if NN == 39:
        rel = tocabi_relatives()
        assert all(((np.abs(A) > 0) <= rel).all() for A in mass), "the oracle's mass matrices carry TopoTocabi's pattern"
        cs += [("mass", A) for A in mass]
        for shift in (0.05, 1.0, 30.0):
            G = rng.standard_normal((39, 39))
            S = np.where(rel, G + G.T, 0.0)
            S += np.diag(np.abs(S).sum(1) * (1.0 + shift))  # (diagonally dominant: SPD whatever the mask leaves)
            cs.append(("synthetic", S))
    else:
        cs += [("mass_joints", A[6:, 6:].copy()) for A in mass[:8]]
        for cond in (1.0e2, 1.0e5, 1.0e8):
            Q, _ = np.linalg.qr(rng.standard_normal((33, 33)))
            S = (Q * np.geomspace(1.0, cond, 33)) @ Q.T
            cs.append(("synthetic", 0.5 * (S + S.T)))
    bad = cs[0][1].copy()
    bad[NN // 2, NN // 2] = -bad[NN // 2, NN // 2]
    cs.append(("indefinite", bad))
    return [(k, A, rng.standard_normal((NN, 64 - NN))) for k, A in cs]


@functools.lru_cache(maxsize=None)
def _sweep_ref(NN):
    out = []
    for kind, A, rhs in sweep_cases(NN):
        if kind == "indefinite":
            out.append(None)
            continue
        Xm = _mp_inverse(A)
        Ym = Xm.dot(np.array([[mpf(float(v)) for v in r] for r in rhs], dtype=object))
        out.append((Xm, Ym, float(np.linalg.cond(A))))
    return out


def check_sweep(build, name, threads=64, bar=None):
    NN = SWEEP_INSTS[name]
    cs = sweep_cases(NN)
    din = np.stack([np.concatenate([A, rhs], axis=1).T.ravel() for _, A, rhs in cs])  # lane-major: column `lane`, NN entries
    o = probe.run(build, name, din, None, threads)
    ref = _sweep_ref(NN)
    bar = inverse_bar(name) if bar is None else bar
    worst = worst_sym = 0.0
    for b, (kind, A, rhs) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind})"
        S = o[b, :64 * NN].reshape(64, NN)
        ok = o[b, 64 * NN + 64]
        if kind == "indefinite":
            assert ok == 0, (tag, "ok", ok)
            continue
        assert ok == 1, (tag, "ok", ok)
        Xm, Ym, kappa = ref[b]
        X = S[:NN].T
        Y = -S[NN:].T  # (the riding columns come out negated like the matrix lanes before their epilogue: dwbc_cycle2p.h stores -s)
        assert np.isfinite(S).all(), tag
        assert np.array_equal(np.diag(X), o[b, 64 * NN:64 * NN + NN]), (tag, "dg is the diagonal of the inverse")
        g, nrm = _gfig(X, Xm, kappa)
        gy, _ = _gfig(Y, Ym, kappa)
        sym = float(np.abs(X - X.T).max())
        worst, worst_sym = max(worst, g, gy), max(worst_sym, sym / (U64 * kappa * nrm))
        assert max(g, gy) <= bar, (tag, "g", g, gy, bar)
        assert sym <= 2.0 * bar * U64 * kappa * nrm, (tag, "|X - X^T|", sym)  # (both halves are within the bar of the symmetric X_mp)
    return dict(worst_g=worst, worst_sym=worst_sym, n=len(cs))


def _spd(rng, n, spread=0.0):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    S = (Q * rng.uniform(0.5, 2.0, n)) @ Q.T
    S = 0.5 * (S + S.T)
    d = 10.0 ** rng.uniform(-spread, spread, n)
    return S * d[:, None] * d[None, :]


@functools.lru_cache(maxsize=None)
def small_cases(name):
    """(kind, n, A): n is a tuple for chol6_x3.  kind 'bad': a pivot that is not positive (ok == 0, values not asserted)"""
    base = name.replace("_inplace", "")  # (the in-place form takes the cases of the out-of-place one)
    rng = np.random.default_rng(5000 + len(base) * 13 + sum(map(ord, base)))
    cs = []
    if name in ("spd12_lds", "spd12_lds_inplace", "spd_small"):
        for _ in range(6):
            cs.append(("spread", 12, _spd(rng, 12, 4.0)))  # diagonals over 1e-8 .. 1e8: force and moment rows mix
        for es in ([-7, -5, -3, -1, 1, 3, 5, 7, 9, 11, -9, -11], [-8, -6, -4, -2, 0, 2, 4, 6, -1, -3, 5, 7], [-21, -20, -19, -1, -2, -3, 1, 2, 3, -41, 40, 41]):
            S = _spd(rng, 12)
            d = np.sqrt(2.0 ** np.array(es, float) / np.diag(S))
            S = S * d[:, None] * d[None, :]
            S[np.diag_indices(12)] = 2.0 ** np.array(es, float)  # diagonals that are exact powers of two, odd and negative exponents
            cs.append(("pow2", 12, S))
        Z = _spd(rng, 12)
        Z[4, 4] = 0.0
        cs.append(("bad", 12, Z))
        Ng = _spd(rng, 12)
        Ng[7, 7] = -Ng[7, 7]
        cs.append(("bad", 12, Ng))
        Id = _spd(rng, 12) - 1.2 * np.eye(12)
        Id[np.diag_indices(12)] = np.abs(np.diag(Id)) + 0.1  # positive diagonal, indefinite
        cs.append(("bad", 12, Id))
        if name == "spd_small":
            for n in range(1, 12):  # n < 12: partial pivots of the 12-wide sweep; n <= 6: the Cholesky form
                cs.append(("partial", n, _spd(rng, n, 2.0)))
                cs.append(("partial", n, _spd(rng, n)))
            B7 = _spd(rng, 9)
            B7[5, 5] = -1.0
            cs.append(("bad", 9, B7))
    elif name == "chol6":
        for n in range(1, 7):
            for sp in (0.0, 0.0, 3.0):
                cs.append(("spd", n, _spd(rng, n, sp)))
        B = _spd(rng, 5) - 1.1 * np.eye(5)
        B[np.diag_indices(5)] = np.abs(np.diag(B)) + 0.1
        cs.append(("bad", 5, B))
    else:
        for ns in ((6, 6, 6), (0, 0, 0), (6, 0, 3), (0, 5, 0), (1, 2, 3), (3, 6, 0), (2, 4, 6), (6, 5, 4), (0, 0, 1), (4, 4, 4)):
            cs.append(("spd", ns, [(_spd(rng, n, 1.0) if n else np.zeros((0, 0))) for n in ns]))
        bad = [_spd(rng, 4), _spd(rng, 6), _spd(rng, 3)]
        bad[1] = bad[1] - 1.1 * np.eye(6)
        bad[1][np.diag_indices(6)] = np.abs(np.diag(bad[1])) + 0.1
        cs.append(("bad", (4, 6, 3), bad))
    return cs


def _is_spd(M):
    """definiteness, decided on the Jacobi-scaled matrix (the diagonals of the cases spread over 2^+-41: unscaled, eigvalsh rounds the
    smallest eigenvalue of a definite matrix below zero); every case is far from the border"""
    d = np.diag(M)
    if (d <= 0).any():
        return False
    lam = np.linalg.eigvalsh(M / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]).min()
    assert abs(lam) > 1.0e-3, ("a case too close to singular to call", lam)
    return lam > 0


@functools.lru_cache(maxsize=None)
def _small_ref(name):
    out = []
    for kind, n, A in small_cases(name):
        mats = A if isinstance(n, tuple) else [A]
        out.append([None if (M.size == 0 or not _is_spd(M)) else (_mp_inverse(M), float(np.linalg.cond(M))) for M in mats])
    return out


def check_small(build, name, threads=64, bar=None):
    """(ok is asserted against the definiteness of the case in BOTH builds: the device flag equals the host's)"""
    cs = small_cases(name)
    ref = _small_ref(name)
    bar = inverse_bar(name) if bar is None else bar
    nin, nip, nout = probe.sizes(build, name)
    din = np.full((len(cs), nin), np.nan)  # (NaN outside n x n: a padding row that leaks into the result shows)
    ip = np.zeros((len(cs), nip), np.int32)
    for b, (kind, n, A) in enumerate(cs):
        if name == "chol6_x3":
            for q in range(3):
                din[b, 36 * q:36 * q + n[q] * n[q]] = A[q].ravel()
            ip[b] = n
        else:
            ld = 6 if name == "chol6" else 12
            M = np.full((ld, ld), np.nan)
            M[:n, :n] = A
            din[b] = M.ravel()
            ip[b, 0] = n
    o = probe.run(build, name, din, ip, threads)
    worst = worst_sym = 0.0
    oks = []
    for b, (kind, n, A) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind}, n = {n})"
        if name == "chol6_x3":
            blocks = []
            for q in range(3):
                blk = o[b, 36 * q:36 * q + 36]
                rest = blk[n[q] * n[q]:]
                assert (np.isnan(rest).all() if q == 2 else (rest == probe.FRAME_SENTINEL).all()), (tag, q, "written beyond n x n")
                blocks.append(blk[:n[q] * n[q]].reshape(n[q], n[q]))
            ok = [int(v) for v in o[b, 108:111]]
        else:
            ld = 6 if name == "chol6" else 12
            F = o[b, :ld * ld].reshape(ld, ld)
            out_mask = np.ones((ld, ld), bool)
            out_mask[:n, :n] = False
            if name == "spd12_lds_inplace":
                assert not out_mask.any()
            else:
                assert (F[out_mask] == probe.FRAME_SENTINEL).all(), (tag, "written beyond n x n")
            blocks = [F[:n, :n]]
            ok = [int(o[b, ld * ld])]
        oks.append(ok)
        for q, (X, r) in enumerate(zip(blocks, ref[b])):
            if r is None:
                assert ok[q] == (1 if X.size == 0 else 0), (tag, q, "ok", ok)
                continue
            assert ok[q] == 1, (tag, q, "ok", ok)
            Xm, kappa = r
            assert np.isfinite(X).all(), (tag, q)
            g, nrm = _gfig(X, Xm, kappa)
            sym = float(np.abs(X - X.T).max())
            worst, worst_sym = max(worst, g), max(worst_sym, sym / (U64 * kappa * nrm))
            assert g <= bar, (tag, q, "g", g, bar)
            assert sym <= 2.0 * bar * U64 * kappa * nrm, (tag, q, "|X - X^T|", sym)
    return dict(worst_g=worst, worst_sym=worst_sym, n=len(cs), ok=oks)


# ====================================================================================================================================
# 6. the routines of the general-contact kernel: pinv_cod_small / qr_small, gj_inverse_rows, spd_inverse_reg, spd_inverse_scaled, mmg
# ====================================================================================================================================
COD_THR = 1.0e-6  # kCodThreshold of the fp64 build (dwbc_cycle.h), COD_THRESHOLD of the reference
COD_CHECK = 1.0e-4  # kCodCheck
PINV_TS = tuple(range(1, 13))
GJ_INSTS = {"gj_rows6": 6, "gj_rows12": 12, "gj_rows18": 18}
SPD_REG_INSTS = {"spd_reg39_lds": 39, "spd_reg33_lds": 33, "spd_reg33_rl": 33}
# name: MAXM, MAXN, MAXK, OP -- the bounds of the TG = 12 kernel's calls (dwbc_cycle_gc.h stage 3)
MMG_INSTS = {"mmg_12_39_39_nn": (12, 39, 39, 0), "mmg_12_12_39_nt": (12, 12, 39, 1), "mmg_33_12_12_tn": (33, 12, 12, 2),
             "mmg_12_33_12_nn": (12, 33, 12, 0)}
GC_INVERSE_INSTS = ("pinv_cod12",) + tuple(GJ_INSTS) + tuple(SPD_REG_INSTS) + ("spd_scaled12",)


def _mpm(A):
    return [[mpf(float(v)) for v in r] for r in np.atleast_2d(A)]


def _mp_qrcp(A):
    """Householder QR with column pivoting in 50 digits: the largest remaining column norm first (the first of equal ones), reflector
    sign against the pivot.  A (nested lists of mpf) = Q R Pi^T; returns Q, R, piv (piv[j] = the original column in position j) and,
    per step, the ratio of the largest to the second largest remaining column norm"""
    m, n = len(A), len(A[0])
    R = [r[:] for r in A]
    Q = [[mpf(1) if i == j else mpf(0) for j in range(m)] for i in range(m)]
    piv = list(range(n))
    gaps = []
    for s in range(min(m, n)):
        nr = [sum(R[i][j] ** 2 for i in range(s, m)) for j in range(s, n)]
        order = sorted(range(len(nr)), key=lambda j: (-nr[j], j))
        best = s + order[0]
        if len(nr) > 1:
            gaps.append(mp.sqrt(nr[order[0]] / nr[order[1]]) if nr[order[1]] > 0 else mp.inf)
        if best != s:
            for i in range(m):
                R[i][s], R[i][best] = R[i][best], R[i][s]
            piv[s], piv[best] = piv[best], piv[s]
        v = [R[i][s] for i in range(s, m)]
        nrm = mp.sqrt(sum(x * x for x in v))
        if nrm == 0:
            continue
        v[0] -= -nrm if v[0] > 0 else nrm
        vn = sum(x * x for x in v)
        if vn == 0:
            continue
        beta = 2 / vn
        for j in range(s, n):
            d = beta * sum(v[i - s] * R[i][j] for i in range(s, m))
            for i in range(s, m):
                R[i][j] -= d * v[i - s]
        for i in range(m):
            d = beta * sum(Q[i][k] * v[k - s] for k in range(s, m))
            for k in range(s, m):
                Q[i][k] -= d * v[k - s]
    return Q, R, piv, gaps


def _mp_pinv_cod(M, thr=COD_THR):
    """the reference's rule (PinvCODWB, src/wbd.cpp:5-30) restated in 50 digits: column-pivoted Householder QR, rank = #{|R_ii| > thr
    max |R_ii|}, the pseudo-inverse of the kept rows R1 = R[:rank] permuted back: P = Pi R1^+ Q1^T.  NOT an SVD truncation (the two
    differ at O(dropped pivot / kept pivot)).  Returns P (object array of mpf), rank, room (the factor by which the closest |R_ii|
    clears thr max |R_ii|, on its side) and the pivot gaps of _mp_qrcp"""
    t = M.shape[0]
    Q, R, piv, gaps = _mp_qrcp(_mpm(M))
    d = [abs(R[i][i]) for i in range(t)]
    bar = mpf(thr) * max(d)
    rank = sum(1 for x in d if x > bar)
    room = min([mp.inf] + [(x / bar if x > bar else (bar / x if x > 0 else mp.inf)) for x in d if bar > 0])
    assert all(d[i] > bar for i in range(rank)), "the kept pivots lead"
    P = np.array([[mpf(0)] * t for _ in range(t)], dtype=object)
    if rank > 0:
        R1 = mp.matrix(R[:rank])
        R1p = R1.T * mp.inverse(R1 * R1.T)  # t x rank: the minimum-norm solution operator of the kept rows
        for i in range(t):
            for j in range(t):
                P[piv[i], j] = sum(R1p[i, k] * Q[j][k] for k in range(rank))
    return P, rank, float(room), [float(g) for g in gaps]


def _orth(rng, t, r):
    Q, _ = np.linalg.qr(rng.standard_normal((t, t)))
    return Q[:, :r]


@functools.lru_cache(maxsize=None)
def pinv_cases(t):
    """(kind, M, rank or None).  deficient: M = F diag(s) F^T with t x rank orthonormal F, s within a factor 4, at three overall scales
    (the rule is relative); zero; full (SPD: the verdict leaves the caller's inverse alone); nonsym: F1 diag(s) F2^T (t = 7 and 12);
    thr_kept / thr_dropped: M = Q R with the smallest pivot at 1e-5 / 1e-7 of the largest and column norms a factor >= 1.3 apart"""
    rng = np.random.default_rng(6000 + t)
    cs = []
    for r in range(1, t):
        for scale in (1.0e-3, 1.0, 1.0e3):
            F = _orth(rng, t, r)
            M = (F * (scale * rng.uniform(1.0, 4.0, r))) @ F.T
            cs.append(("deficient", 0.5 * (M + M.T), r))
    cs.append(("zero", np.zeros((t, t)), 0))
    cs.append(("full", _spd(rng, t), t))
    if t in (7, 12):
        for r in (t - 3, 2):
            cs.append(("nonsym", (_orth(rng, t, r) * rng.uniform(1.0, 4.0, r)) @ _orth(rng, t, r).T, r))
    if t >= 2:
        for kind, last in (("thr_kept", 1.0e-5), ("thr_dropped", 1.0e-7)):
            d = np.concatenate([np.geomspace(1.0, 1.0e-2, t - 1), [last]]) if t > 2 else np.array([1.0, last])
            if t > 2:
                assert (d[:-1] / d[1:]).min() >= 1.3
            R = np.diag(d) + np.triu(rng.uniform(-1.0, 1.0, (t, t)), 1) * d[None, :] * (0.3 / np.sqrt(t))
            cs.append((kind, _orth(rng, t, t) @ R, t if kind == "thr_kept" else t - 1))
    return cs


@functools.lru_cache(maxsize=None)
def _pinv_ref(t):
    """per case (P_mp, rank, kappa_r); asserts of the CASES: the rank the case was built for, a factor 10 of room in every rank
    decision, a 10 % gap of the column norms wherever the pivot order matters (a dropped pivot that is not round-off), and that the
    reference rounded to double scores g <= 1"""
    out = []
    for kind, M, rank in pinv_cases(t):
        P, rk, room, gaps = _mp_pinv_cod(M)
        assert rk == rank, (t, kind, rk, rank)
        assert room >= 9.99, (t, kind, "room of the rank decision", room)  # (the threshold pairs sit AT the factor 10, up to the rounding of M)
        if kind.startswith("thr"):
            assert min(gaps) >= 1.1, (t, kind, "pivot order", gaps)
        sv = np.linalg.svd(M, compute_uv=False)
        kappa = float(sv[0] / sv[rank - 1]) if rank > 0 else 1.0
        if 0 < rank < t:
            assert _gfig(_f(P), P, kappa)[0] <= 1.0
        out.append((P, rk, kappa))
    return out


def check_pinv_cod(build, ts=PINV_TS, threads=64, bar=None):
    """pinv_cod_small at t = ts, one launch per t.  Asserts: the rank of the 50-digit rule; g = |P - P_mp|max / (u kappa_r |P_mp|max),
    kappa_r over the KEPT singular values; on the exactly deficient cases both Penrose identities, independent of the restated rule:
    with P = M^+ + E, |E| <= bar u kappa_r |P|max, M P M - M = M E M and P M P - P = E M P + P M E to first order, |M|max |P|max <=
    kappa_r, so t^2 bar u kappa_r^2 |M|max and 2 t^2 bar u kappa_r^2 |P|max bound them (+ 4 t u kappa_r |.|max for the round-off
    the deficient directions of M itself carry)"""
    bar = inverse_bar("pinv_cod12") if bar is None else bar
    worst = worst_pen = 0.0
    ncase = 0
    for t in ts:
        cs, ref = pinv_cases(t), _pinv_ref(t)
        din = np.full((len(cs), 144), np.nan)
        for b, (kind, M, rank) in enumerate(cs):
            din[b, :t * t] = M.ravel()
        o = probe.run(build, "pinv_cod12", din, np.full((len(cs), 1), t), threads)
        ncase += len(cs)
        for b, (kind, M, rank) in enumerate(cs):
            tag = f"{build} pinv_cod12 t{threads} t = {t} case {b} ({kind}, rank {rank})"
            Pm, rk, kappa = ref[b]
            assert np.isnan(o[b, 145:]).all(), (tag, "written behind vec")
            assert (o[b, t * t:144] == probe.FRAME_SENTINEL).all(), (tag, "written beyond t x t")
            assert o[b, 144] == rk, (tag, "rank", o[b, 144], rk)
            P = o[b, :t * t].reshape(t, t)
            if rk == t:
                assert (P == probe.FRAME_SENTINEL).all(), (tag, "a full-rank verdict leaves Out alone")
                continue
            if rk == 0:
                assert (P == 0.0).all(), tag
                continue
            assert np.isfinite(P).all(), tag
            g, nrm = _gfig(P, Pm, kappa)
            worst = max(worst, g)
            assert g <= bar, (tag, "g", g, bar)
            if kind in ("deficient", "nonsym"):
                Ml, Pl = M.astype(np.longdouble), P.astype(np.longdouble)
                p1 = float(np.abs(Ml @ Pl @ Ml - Ml).max()) / (U64 * np.abs(M).max())
                p2 = float(np.abs(Pl @ Ml @ Pl - Pl).max()) / (U64 * np.abs(P).max())
                b1, b2 = t * t * bar * kappa ** 2 + 4 * t * kappa, 2 * t * t * bar * kappa ** 2 + 4 * t * kappa
                worst_pen = max(worst_pen, p1 / b1, p2 / b2)
                assert p1 <= b1 and p2 <= b2, (tag, "Penrose", p1, b1, p2, b2)
    return dict(worst_g=worst, worst_sym=0.0, worst_penrose=worst_pen, n=ncase)


def _mp_gj_pivots(A, first=None):
    """Gauss-Jordan with partial pivoting in 50 digits (the largest remaining element of the column; `first`: the row forced at column
    0): the pivot magnitudes, and the smallest ratio of the largest to the second largest candidate over the unforced steps"""
    n = A.shape[0]
    R = _mpm(A)
    free = list(range(n))
    pivs, margin = [], mp.inf
    for c in range(n):
        cand = sorted(((abs(R[i][c]), -i) for i in free), reverse=True)
        p = -cand[0][1]
        if c == 0 and first is not None:
            p = first
        elif len(cand) > 1 and cand[0][0] > 0:
            margin = min(margin, cand[0][0] / cand[1][0] if cand[1][0] > 0 else mp.inf)
        pivs.append(abs(R[p][c]))
        free.remove(p)
        if R[p][c] == 0:
            return pivs, mpf(0)
        for i in free:
            f = R[i][c] / R[p][c]
            for j in range(c, n):
                R[i][j] -= f * R[p][j]
    return pivs, margin


@functools.lru_cache(maxsize=None)
def gj_cases(NMAX):
    """(kind, n, A, extra): general, NON-symmetric matrices, each run out of place and in place.  random (every n); zero_lead (A[0][0] =
    0) and zero_diag (pivoting is needed from the first column on); permdiag (a permutation times a diagonal over 1e-6 .. 1e6); tie
    (the two largest entries of column 0 agree in all but the 7 lowest mantissa bits, which the device's arg-min drops: either row is
    a valid pivot; extra = the two rows); singular (two equal rows)"""
    rng = np.random.default_rng(6100 + NMAX)
    cs = []
    for n in range(1, NMAX + 1):
        cs.append(("random", n, rng.standard_normal((n, n)) + 2.0 * np.eye(n)[rng.permutation(n)], None))
    Z = rng.standard_normal((NMAX, NMAX))
    Z[0, 0] = 0.0
    cs.append(("zero_lead", NMAX, Z, None))
    Z = rng.standard_normal((NMAX, NMAX)) + 3.0 * np.eye(NMAX)[np.roll(np.arange(NMAX), 1)]
    Z[np.diag_indices(NMAX)] = 0.0
    cs.append(("zero_diag", NMAX, Z, None))
    cs.append(("permdiag", NMAX, np.eye(NMAX)[rng.permutation(NMAX)] * np.geomspace(1.0e-6, 1.0e6, NMAX)[rng.permutation(NMAX)], None))
    for k in range(4):
        A = rng.standard_normal((NMAX, NMAX)) + 2.0 * np.eye(NMAX)
        A[:, 0] = np.clip(A[:, 0], -1.5, 1.5)
        i, j = sorted(int(v) for v in rng.choice(NMAX, 2, replace=False))
        base = np.float64(rng.uniform(3.0, 4.0)).view(np.uint64) & ~np.uint64(127)
        lo = rng.choice(128, 2, replace=False).astype(np.uint64)
        A[i, 0], A[j, 0] = (base | lo[0]).view(np.float64), (base | lo[1]).view(np.float64) * (-1.0 if k % 2 else 1.0)
        cs.append(("tie", NMAX, A, (i, j)))
    n = NMAX // 2 + 2
    S = rng.standard_normal((n, n))
    S[n - 2] = S[1]
    cs.append(("singular", n, S, None))
    return cs


@functools.lru_cache(maxsize=None)
def _gj_ref(NMAX):
    """per case (X_mp, kappa, the valid pivot ratios, whether the pivot order is unambiguous)"""
    out = []
    for kind, n, A, extra in gj_cases(NMAX):
        if kind == "singular":
            pivs, _ = _mp_gj_pivots(A)
            assert min(pivs) == 0
            out.append(None)
            continue
        Xm, kappa = _mp_inverse(A), float(np.linalg.cond(A))
        assert _gfig(_f(Xm), Xm, kappa)[0] <= 1.0
        ratios, clear = [], False
        for first in (extra if kind == "tie" else (None,)):
            pivs, margin = _mp_gj_pivots(A, first)
            ratios.append(float(min(pivs) / max(pivs)))
            clear = kind != "tie" and margin >= 1.0 + 1.0e-6
            if kind == "tie":
                assert margin >= 1.0 + 1.0e-6, "the tie is the only ambiguous pivot"
        out.append((Xm, kappa, ratios, clear))
    return out


def check_gj_rows(build, name, threads=64, bar=None):
    """gj_inverse_rows<NMAX>: g against the 50-digit inverse; the returned pivot ratio against the pivots of the 50-digit elimination to
    1e-10 relative where the pivot order is unambiguous, within 2^-45 of one of the two valid values on the tie cases; nothing written
    outside n x n; the singular case returns a ratio below kCodCheck (values not asserted)"""
    NMAX = GJ_INSTS[name]
    cs, ref = gj_cases(NMAX), _gj_ref(NMAX)
    bar = inverse_bar(name) if bar is None else bar
    din = np.full((2 * len(cs), NMAX * NMAX), np.nan)
    ip = np.zeros((2 * len(cs), 2), np.int32)
    for b, (kind, n, A, extra) in enumerate(cs):
        for inplace in (0, 1):
            din[2 * b + inplace, :n * n] = A.ravel()
            ip[2 * b + inplace] = (n, inplace)
    o = probe.run(build, name, din, ip, threads)
    worst = worst_ratio = 0.0
    for b, (kind, n, A, extra) in enumerate(cs):
        for inplace in (0, 1):
            tag = f"{build} {name} t{threads} case {b} ({kind}, n = {n}, {'in place' if inplace else 'out of place'})"
            r = o[2 * b + inplace]
            rest = r[n * n:NMAX * NMAX]
            assert (np.isnan(rest).all() if inplace else (rest == probe.FRAME_SENTINEL).all()), (tag, "written beyond n x n")
            ratio = r[NMAX * NMAX]
            if ref[b] is None:
                assert 0.0 <= ratio < COD_CHECK, (tag, "pivot ratio of a singular matrix", ratio)
                continue
            Xm, kappa, ratios, clear = ref[b]
            X = r[:n * n].reshape(n, n)
            assert np.isfinite(X).all(), tag
            g, _ = _gfig(X, Xm, kappa)
            worst = max(worst, g)
            assert g <= bar, (tag, "g", g, bar)
            rel = min(abs(ratio - v) / v for v in ratios)
            if kind == "tie":
                assert rel <= 2.0 ** -45, (tag, "pivot ratio", ratio, ratios)
            elif clear:
                worst_ratio = max(worst_ratio, rel)
                assert rel <= 1.0e-10, (tag, "pivot ratio", ratio, ratios)
    return dict(worst_g=worst, worst_sym=0.0, worst_ratio=worst_ratio, n=len(cs))


def check_spd_reg(build, name, threads=64, bar=None):
    """spd_inverse_reg<NN> in place on sweep_cases(NN) without the riding columns, checked as check_sweep does"""
    NN = SPD_REG_INSTS[name]
    cs, ref = sweep_cases(NN), _sweep_ref(NN)
    bar = inverse_bar(name) if bar is None else bar
    o = probe.run(build, name, np.stack([A.ravel() for _, A, _ in cs]), None, threads)
    worst = worst_sym = 0.0
    for b, (kind, A, _) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind})"
        ok = o[b, NN * NN]
        if kind == "indefinite":
            assert ok == 0, (tag, "ok", ok)
            continue
        assert ok == 1, (tag, "ok", ok)
        Xm, _, kappa = ref[b]
        X = o[b, :NN * NN].reshape(NN, NN)
        assert np.isfinite(X).all(), tag
        g, nrm = _gfig(X, Xm, kappa)
        sym = float(np.abs(X - X.T).max())
        worst, worst_sym = max(worst, g), max(worst_sym, sym / (U64 * kappa * nrm))
        assert g <= bar, (tag, "g", g, bar)
        assert sym <= 2.0 * bar * U64 * kappa * nrm, (tag, "|X - X^T|", sym)
    return dict(worst_g=worst, worst_sym=worst_sym, n=len(cs))


def check_spd_scaled(build, threads=64, bar=None):
    """spd_inverse_scaled<12> in place on the cases of spd_small (diagonals over 1e+-8 and 2^+-41 with odd and negative exponents, n =
    1..12, pivots that are not positive), densely stored (row stride n), checked as check_small does"""
    name = "spd_scaled12"
    cs, ref = small_cases("spd_small"), _small_ref("spd_small")
    bar = inverse_bar(name) if bar is None else bar
    din = np.full((len(cs), 144), np.nan)
    for b, (kind, n, A) in enumerate(cs):
        din[b, :n * n] = A.ravel()
    o = probe.run(build, name, din, np.array([[n] for _, n, _ in cs]), threads)
    worst = worst_sym = 0.0
    for b, (kind, n, A) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind}, n = {n})"
        assert np.isnan(o[b, n * n:144]).all(), (tag, "written beyond n x n")
        ok, r = o[b, 144], ref[b][0]
        if r is None:
            assert kind == "bad" and ok == 0, (tag, "ok", ok)
            continue
        assert ok == 1, (tag, "ok", ok)
        Xm, kappa = r
        X = o[b, :n * n].reshape(n, n)
        assert np.isfinite(X).all(), tag
        g, nrm = _gfig(X, Xm, kappa)
        sym = float(np.abs(X - X.T).max())
        worst, worst_sym = max(worst, g), max(worst_sym, sym / (U64 * kappa * nrm))
        assert g <= bar, (tag, "g", g, bar)
        assert sym <= 2.0 * bar * U64 * kappa * nrm, (tag, "|X - X^T|", sym)
    return dict(worst_g=worst, worst_sym=worst_sym, n=len(cs))


def check_gc_inverse(build, name, threads=64, bar=None):
    if name == "pinv_cod12":
        return check_pinv_cod(build, PINV_TS, threads, bar)
    if name in GJ_INSTS:
        return check_gj_rows(build, name, threads, bar)
    if name in SPD_REG_INSTS:
        return check_spd_reg(build, name, threads, bar)
    return check_spd_scaled(build, threads, bar)


@functools.lru_cache(maxsize=None)
def mmg_cases(name):
    """(kind, m, kk, n, A, B) with A, B in the shapes OP reads: run-time sizes (1, 1, 1), the full bounds, n at 15, 16, 17 and 33 (the
    borders of the 16-wide column tiles) where MAXN allows, kk that is no multiple of 4 (the depth of an MFMA step), odd m"""
    MAXM, MAXN, MAXK, OP = MMG_INSTS[name]
    rng = np.random.default_rng(6200 + 1000 * MAXM + 31 * MAXN + MAXK + OP)
    sizes = [(1, 1, 1), (MAXM, MAXK, MAXN), (MAXM, MAXK - 1, MAXN), (MAXM - 1, 5, MAXN - 1), (3, 7, 2), (MAXM, 1, MAXN), (1, MAXK, 1)]
    sizes += [(MAXM - (i % 2), MAXK - 2 * i, n) for i, n in enumerate((15, 16, 17, 33)) if n <= MAXN]
    cs = []
    for c, (m, kk, n) in enumerate(sizes):
        sa, sb = ((kk, m) if OP == 2 else (m, kk)), ((n, kk) if OP == 1 else (kk, n))
        for kind in ("ints", "reals") if c < 5 else ("reals",):
            if kind == "ints":
                A, B = rng.integers(-9, 10, sa).astype(float), rng.integers(-9, 10, sb).astype(float)
            else:
                A, B = rng.standard_normal(sa) * 2.0 ** rng.integers(-20, 21, sa), rng.standard_normal(sb) * 2.0 ** rng.integers(-20, 21, sb)
            cs.append((kind, m, kk, n, A, B))
    return cs


@functools.lru_cache(maxsize=None)
def _mmg_ref(name):
    """per case the exact product and the exact |A||B| (as _gemm_ref), floats of the 50-digit sums"""
    OP = MMG_INSTS[name][3]
    out = []
    for kind, m, kk, n, A, B in mmg_cases(name):
        if kind == "ints":  # (exact in int64; no bar to scale)
            D = (A.T if OP == 2 else A).astype(np.int64) @ (B.T if OP == 1 else B).astype(np.int64)
            out.append(([[mpf(int(v)) for v in r] for r in D], None))
            continue
        Am, Bm = _mpm(A.T if OP == 2 else A), _mpm(B.T if OP == 1 else B)
        Bc = [[Bm[k][j] for k in range(kk)] for j in range(n)]
        D = [[mp.fdot(Am[i], Bc[j]) for j in range(n)] for i in range(m)]
        Ab = [[mp.fsum(abs(x * y) for x, y in zip(Am[i], Bc[j])) for j in range(n)] for i in range(m)]
        out.append((D, Ab))
    return out


def check_mmg(build, name, threads=64):
    """mmg at run-time sizes inside its compile-time bounds.  Bar: gamma_{kk+1} (|A||B|), as check_gemm derives it; integers exactly;
    nothing stored outside m x n (the operands are NaN outside the run-time sizes: an unmasked read shows in the result)"""
    MAXM, MAXN, MAXK, OP = MMG_INSTS[name]
    cs, ref = mmg_cases(name), _mmg_ref(name)
    SA, SB = MAXM * MAXK, MAXK * MAXN
    din = np.full((len(cs), SA + SB), np.nan)
    for b, (kind, m, kk, n, A, B) in enumerate(cs):
        din[b, :A.size] = A.ravel()
        din[b, SA:SA + B.size] = B.ravel()
    o = probe.run(build, name, din, np.array([[m, kk, n] for _, m, kk, n, _, _ in cs]), threads)
    worst = 0.0
    for b, (kind, m, kk, n, A, B) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind}, m kk n = {m} {kk} {n})"
        assert (o[b, m * n:] == probe.FRAME_SENTINEL).all(), (tag, "stored outside m x n")
        D = o[b, :m * n].reshape(m, n)
        assert np.isfinite(D).all(), tag
        Dr, Ab = ref[b]
        g = gamma(kk + 1)
        for i in range(m):
            for j in range(n):
                e = float(abs(mpf(float(D[i, j])) - Dr[i][j]))
                bar = 0.0 if kind == "ints" else g * float(Ab[i][j])
                assert e <= bar, (tag, i, j, D[i, j], float(Dr[i][j]), e, bar)
                if kind == "reals" and Ab[i][j] > 0:
                    worst = max(worst, e / (U64 * float(Ab[i][j])))
    return dict(worst_u=worst, n=len(cs))


# ====================================================================================================================================
# 7. the two in-place matrix-core tiles of the cycle: contact_gram and wrench_maps (dwbc_cycle2.h)
# ====================================================================================================================================
# Both families return the wave's whole LDS slice (wave_probe_body.h, section 7), so every check sees the guards, the operands as they
# read back and the output block.  Bars: integers exactly; reals gamma_{K+3} sum_c (|R||J|)_c |rhs_c| -- the bound of check_gemm with
# three more roundings for the three-term row of A_rot (contact_gram has no such row: its bound is the looser for it), K = N for the
# Gram tile and K = M for the wrench maps, in ANY order of summation; the sum is taken in mpmath.
GRAM_INSTS = {"gram_39": 39, "gram_37": 37, "gram_23": 23, "gram_24": 24, "gram_50": 50}
WRENCH_INSTS = {"wrench_39": 39, "wrench_37": 37, "wrench_23": 23, "wrench_24": 24, "wrench_50": 50}
TILE_INSTS = tuple(GRAM_INSTS) + tuple(WRENCH_INSTS)
# (cd, k, t_dof): 1 + sum t + k columns -- one full tile (BASELINE's shape), one partial tile, a partial second tile ([6, 6, 3]: the
# third level's block, columns 13..15, ends at the tile boundary), a block across the boundary ([3, 6, 6]: the null block, columns
# 16..21, starts the second tile; [6, 3, 6]: the third level's block is columns 10..15, offsets 0, 6, 9), the maximum of 31 (its third
# level's block, columns 13..18, straddles column 16, the tile boundary), two single-contact shapes without a null block
WRENCH_HIER = [(12, 6, (6, 3)), (12, 6, (3,)), (12, 6, (6, 6, 3)), (12, 6, (3, 6, 6)), (12, 6, (6, 3, 6)), (12, 6, (6, 6, 6, 6)),
               (6, 0, (6, 3)), (6, 0, (3,))]
WRENCH_LAYOUT_HIER = [(12, 6, (6, 6, 6, 6)), (6, 0, (6, 3))]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def _spread(rng, shape):
    return rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 21, shape)


# ---- contact_gram
def _gram_offsets(N):
    oY = 2
    oJ = oY + 12 * N + 2
    oO = oJ + 12 * N + 2
    return oY, oJ, oO, oO + 144 + 2


@functools.lru_cache(maxsize=None)
def gram_cases(N):
    """(kind, cd, Yt, JCt), both N x 12 with the columns >= cd zero (the contract of contact_gram): small integers, reals with an exponent
    spread and one cancelling row, 1e300 in the last reduction row of either or both operands (what the masked duplicate of that row
    computes must not be added), each at cd = 12 and at cd = 6 (one contact)"""
    rng = np.random.default_rng(7100 + N)
    cs = []

    def cut(A, cd):
        A[:, cd:] = 0.0
        return A

    for c in range(4):
        cd = 12 if c < 2 else 6
        cs.append(("ints", cd, cut(rng.integers(-9, 10, (N, 12)).astype(float), cd), cut(rng.integers(-9, 10, (N, 12)).astype(float), cd)))
    for c in range(6):
        cd = 12 if c < 4 else 6
        Y, J = _spread(rng, (N, 12)), _spread(rng, (N, 12))
        Y[1:, 0] = Y[0, 0]  # row 0 of Y J^T: equal factors against a column sum that cancels
        J[1:, :] = -J[:1, :] / (N - 1)
        cs.append(("reals", cd, cut(Y, cd), cut(J, cd)))
    for c, (hy, hj) in enumerate(((True, True), (True, False), (False, True), (True, False))):
        cd = 12 if c < 3 else 6
        Y, J = rng.integers(1, 10, (N, 12)).astype(float), rng.integers(1, 10, (N, 12)).astype(float)
        if hy:
            Y[N - 1, :] = 1.0e300
        if hj:
            J[N - 1, :] = 1.0e300
        cs.append(("huge", cd, cut(Y, cd), cut(J, cd)))
    return cs


@functools.lru_cache(maxsize=None)
def _gram_ref(N):
    """per case the exact Y J^T and the exact sum_c |Y_ci J_cj| over cd x cd (zero outside), nested lists of mpf"""
    out = []
    for kind, cd, Y, J in gram_cases(N):
        Yc, Jc = [mpv(Y[:, i]) for i in range(cd)], [mpv(J[:, j]) for j in range(cd)]
        D = [[mp.fdot(Yc[i], Jc[j]) for j in range(cd)] for i in range(cd)]
        Ab = [[mp.fsum(abs(a * b) for a, b in zip(Yc[i], Jc[j])) for j in range(cd)] for i in range(cd)]
        out.append((D, Ab))
    return out


def _gram_unpack(o, N, Y, J, tag):
    """the footprint: guards, operands bit for bit; returns the 12 x 12 block"""
    oY, oJ, oO, LDS = _gram_offsets(N)
    assert o.shape == (LDS,), (tag, o.shape)
    guard = np.r_[0:oY, oJ - 2:oJ, oO - 2:oO, LDS - 2:LDS]
    assert np.isnan(o[guard]).all(), (tag, "guard words", o[guard])
    assert _bits_equal(o[oY:oY + 12 * N], Y.ravel()) and _bits_equal(o[oJ:oJ + 12 * N], J.ravel()), (tag, "an operand changed")
    return o[oO:oO + 144].reshape(12, 12)


def _check_block(tag, kind, D, Dr, Ab, rows, cols, g):
    """D[i, j] against the exact Dr over rows x cols; returns the worst error in units of u Ab"""
    worst = 0.0
    for i in range(rows):
        for j in range(cols):
            if kind == "ints":
                assert D[i, j] == float(Dr[i][j]), (tag, i, j, D[i, j], float(Dr[i][j]))
            elif abs(Dr[i][j]) > mpf(1.7e308):
                assert D[i, j] == (np.inf if Dr[i][j] > 0 else -np.inf), (tag, i, j, D[i, j])
            else:
                assert np.isfinite(D[i, j]), (tag, i, j, D[i, j])
                e = float(abs(mpf(float(D[i, j])) - Dr[i][j]))
                bar = g * float(Ab[i][j])
                assert e <= bar, (tag, i, j, D[i, j], float(Dr[i][j]), e, bar)
                if kind == "reals" and Ab[i][j] > 0:
                    worst = max(worst, e / (U64 * float(Ab[i][j])))
    return worst


def _gram_unit_cs(N):
    """the reduction indices of the unit sweep: the first four, the last two, and one per K step (a different lane group in each)"""
    return sorted({0, 1, 2, 3, N - 2, N - 1} | {min(4 * s + s % 4, N - 1) for s in range((N + 3) // 4)})


def check_gram(build, name, threads=64):
    """contact_gram<N, 12>: the cases of gram_cases against Y J^T (zero outside cd x cd, exactly), then the exhaustive layout sweep:
    Yt = e_(c,i), JCt = e_(c,j) gives exactly e_i e_j^T -- a transposed or permuted operand layout, a K step that reads another row,
    a padding lane that stores, each moves the one"""
    N = GRAM_INSTS[name]
    cs, ref = gram_cases(N), _gram_ref(N)
    din = np.stack([np.concatenate([Y.ravel(), J.ravel()]) for _, _, Y, J in cs])
    o = probe.run(build, name, din, np.array([[cd] for _, cd, _, _ in cs]), threads)
    g = gamma(N + 3)
    worst = 0.0
    for b, (kind, cd, Y, J) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({kind}, cd {cd})"
        D = _gram_unpack(o[b], N, Y, J, tag)
        outside = np.ones((12, 12), bool)
        outside[:cd, :cd] = False
        assert (D[outside] == 0.0).all(), (tag, "not zero outside cd x cd", D)
        worst = max(worst, _check_block(tag, kind, D, ref[b][0], ref[b][1], cd, cd, g))
    units = [(c, i, j) for c in _gram_unit_cs(N) for i in range(12) for j in range(12)]
    for c0 in range(0, len(units), probe.MAX_B):
        part = units[c0:c0 + probe.MAX_B]
        din = np.zeros((len(part), 24 * N))
        for b, (c, i, j) in enumerate(part):
            din[b, c * 12 + i] = 1.0
            din[b, 12 * N + c * 12 + j] = 1.0
        o = probe.run(build, name, din, np.full((len(part), 1), 12), threads)
        for b, (c, i, j) in enumerate(part):
            tag = f"{build} {name} t{threads} unit (c, i, j) = ({c}, {i}, {j})"
            D = _gram_unpack(o[b], N, din[b, :12 * N], din[b, 12 * N:], tag)
            E = np.zeros((12, 12))
            E[i, j] = 1.0
            assert np.array_equal(D, E), (tag, np.argwhere(D != E))
    return dict(worst_u=worst, n=len(cs), n_units=len(units))


# ---- wrench_maps
def _wrench_offsets(N):
    """the probe's LDS map (WpWrenchMap of wave_probe_body.h): offset of Rc, tg, U, NwJw, JbT, WM and the slice length"""
    M = N - 6
    Rc = 2
    tg = Rc + 18 + 2
    U = tg + ((M + 1) & ~1) + 2
    Nw = U + 24 * M + 2
    Jb = Nw + 6 * M + 2
    wm = Jb + 12 * N + 2
    return Rc, tg, U, Nw, Jb, wm, wm + 384 + 2


def wrench_rhs(M, k, t_dof, tg, U, NwJw):
    """the right-hand operand [ tg | U_0 | U_1 ... | NwJw ] (M x (1 + sum t_l + k)), restated from the comment above wrench_maps:
    column 0 is the gravity torque, level l contributes the leading t_l columns of its M x 6 block, the contact-null block its k columns"""
    return np.hstack([tg.reshape(M, 1)] + [U[l][:, :t] for l, t in enumerate(t_dof)] + [NwJw[:, :k]])


def _wrench_record(N, R, JbT, tg, U, NwJw):
    return np.concatenate([R.ravel(), JbT.ravel(), tg.ravel(), U.ravel(), NwJw.ravel()])


def _wrench_ip(cd, k, t_dof):
    return [cd, k, len(t_dof)] + list(t_dof) + [0] * (4 - len(t_dof))


def _wrench_poison(M, cd, k, t_dof, U, NwJw):
    """NaN in every word of U and NwJw that no column of the hierarchy addresses: a stride, a level or a block taken wrongly reads one"""
    for l in range(4):
        U[l][:, (t_dof[l] if l < len(t_dof) else 0):] = np.nan
    NwJw[:, k:] = np.nan


@functools.lru_cache(maxsize=None)
def wrench_cases(N):
    """(kind, cd, k, t_dof, R (2, 3, 3), JbT (12, N), tg (M), U (4, M, 6), NwJw (M, 6)) over every hierarchy of WRENCH_HIER: four integer
    cases, six of reals with an exponent spread (three of them with rows 0..2 cancelling), three with 1e300 in the last reduction row
    (of J0, of every right-hand block, of both) and, with one contact, two integer and two real cases with NaN in R_1 and in rows 6..11
    of Jbar^T (kinds "ints1" / "reals1").  R need not be a rotation: the function is bilinear.  The words of U / NwJw beyond the
    hierarchy's columns hold NaN; columns 0..5 of Jbar^T, which the function never reads, too."""
    M = N - 6
    rng = np.random.default_rng(7300 + N)
    cs = []

    def add(kind, cd, k, t_dof, R, J, tg, U, Nw):
        _wrench_poison(M, cd, k, t_dof, U, Nw)
        J[:, :6] = np.nan
        if kind.endswith("1"):
            R[1] = np.nan
            J[6:, :] = np.nan
        cs.append((kind, cd, k, t_dof, R, J, tg, U, Nw))

    for cd, k, t_dof in WRENCH_HIER:
        ints = lambda lo, shape: rng.integers(lo, 10, shape).astype(float)
        for _ in range(4):
            add("ints", cd, k, t_dof, ints(-9, (2, 3, 3)), ints(-9, (12, N)), ints(-9, M), ints(-9, (4, M, 6)), ints(-9, (M, 6)))
        for c in range(6):
            R, J, tg, U, Nw = _spread(rng, (2, 3, 3)), _spread(rng, (12, N)), _spread(rng, M), _spread(rng, (4, M, 6)), _spread(rng, (M, 6))
            if c < 3:  # rows 0..2 of A_rot Jbar are constant along the reduction, every right-hand column sums to zero
                J[0:3, 7:] = J[0:3, 6:7]
                tg[1:] = -tg[0] / (M - 1)
                U[:, 1:, :] = -U[:, :1, :] / (M - 1)
                Nw[1:, :] = -Nw[:1, :] / (M - 1)
            add("reals", cd, k, t_dof, R, J, tg, U, Nw)
        for hj, hr in ((True, False), (False, True), (True, True)):
            R, J, tg, U, Nw = ints(1, (2, 3, 3)), ints(1, (12, N)), ints(1, M), ints(1, (4, M, 6)), ints(1, (M, 6))
            if hj:
                J[:, N - 1] = 1.0e300
            if hr:
                tg[M - 1], U[:, M - 1, :], Nw[M - 1, :] = 1.0e300, 1.0e300, 1.0e300
            add("huge", cd, k, t_dof, R, J, tg, U, Nw)
        if cd == 6:
            for _ in range(2):
                add("ints1", cd, k, t_dof, ints(-9, (2, 3, 3)), ints(-9, (12, N)), ints(-9, M), ints(-9, (4, M, 6)), ints(-9, (M, 6)))
                add("reals1", cd, k, t_dof, _spread(rng, (2, 3, 3)), _spread(rng, (12, N)), _spread(rng, M), _spread(rng, (4, M, 6)), _spread(rng, (M, 6)))
    return cs


def _wrench_terms(R, JbT, i, N):
    """row i of A_rot Jbar[:, 6:] as its three terms: contact a = i / 6, force / moment half h, axis x; the row is column x of R_a
    (A_rot = blockdiag(R_a^T, R_a^T)) against rows 6 a + 3 h .. + 2 of Jbar^T"""
    a, h, x = i // 6, (i % 6) // 3, i % 3
    return [(R[a][y][x], JbT[6 * a + 3 * h + y, 6:]) for y in range(3)]


@functools.lru_cache(maxsize=None)
def _wrench_ref(N):
    """per case the exact WM[:cd, :ncols] and the exact sum_c (|R||J|)_c |rhs_c| (nested lists of mpf; the integer cases in int64, no bar)"""
    M = N - 6
    out = []
    for kind, cd, k, t_dof, R, J, tg, U, Nw in wrench_cases(N):
        rhs = wrench_rhs(M, k, t_dof, tg, U, Nw)
        assert np.isfinite(rhs).all() and rhs.shape == (M, 1 + sum(t_dof) + k)
        if kind.startswith("ints"):
            AJ = np.array([sum(int(r) * t.astype(np.int64) for r, t in _wrench_terms(R, J, i, N)) for i in range(cd)])
            out.append(([[mpf(int(v)) for v in row] for row in AJ @ rhs.astype(np.int64)], None))
            continue
        cols = [mpv(rhs[:, c]) for c in range(rhs.shape[1])]
        acols = [[abs(v) for v in col] for col in cols]
        D, Ab = [], []
        for i in range(cd):
            terms = [[mpf(float(r)) * v for v in mpv(t)] for r, t in _wrench_terms(R, J, i, N)]
            row = [t0 + t1 + t2 for t0, t1, t2 in zip(*terms)]
            arow = [abs(t0) + abs(t1) + abs(t2) for t0, t1, t2 in zip(*terms)]
            D.append([mp.fdot(row, col) for col in cols])
            Ab.append([mp.fdot(arow, col) for col in acols])
        out.append((D, Ab))
    return out


def _wrench_unpack(o, build, N, cd, ncols, rec, tag):
    """the footprint: guard words, operands bit for bit, nothing stored beyond the last tile (device) or outside cd x ncols (host);
    returns the 12 x 32 block"""
    M = N - 6
    Rc, tg, U, Nw, Jb, wm, LDS = _wrench_offsets(N)
    assert o.shape == (LDS,), (tag, o.shape)
    blocks = ((Rc, 18), (Jb, 12 * N), (tg, M), (U, 24 * M), (Nw, 6 * M))  # (in the order of the input record)
    guard = np.ones(LDS, bool)
    guard[wm:wm + 384] = False
    at = 0
    for off, n in blocks:
        guard[off:off + n] = False
        assert _bits_equal(o[off:off + n], rec[at:at + n]), (tag, "an operand changed", off)
        at += n
    assert at == rec.size and np.isnan(o[guard]).all(), (tag, "guard words", np.flatnonzero(guard & ~np.isnan(o)))
    W = o[wm:wm + 384].reshape(12, 32)
    ntile = (ncols + 15) // 16
    assert (W[:, 16 * ntile:] == probe.FRAME_SENTINEL).all(), (tag, "stored beyond the last tile")
    if build == "emu":
        assert (W[:, ncols:] == probe.FRAME_SENTINEL).all() and (W[cd:, :] == probe.FRAME_SENTINEL).all(), (tag, "host: stored outside cd x ncols")
    return W


def check_wrench(build, name, threads=64):
    """wrench_maps<N, NT, Map> over every hierarchy: rows 0..cd-1 and columns 0..ncols-1 against the reference.  Rows 6..11 with one
    contact are not asserted (the host leaves the sentinel, the device stores what the stale operands give); rows 0..5 must meet the
    bars and be finite with NaN standing in R_1 and in rows 6..11 of Jbar^T"""
    N = WRENCH_INSTS[name]
    M = N - 6
    cs, ref = wrench_cases(N), _wrench_ref(N)
    assert len(cs) <= probe.MAX_B
    din = np.stack([_wrench_record(N, *c[4:]) for c in cs])
    o = probe.run(build, name, din, np.array([_wrench_ip(cd, k, t) for _, cd, k, t, *_ in cs]), threads)
    g = gamma(M + 3)
    worst = 0.0
    for b, (kind, cd, k, t_dof, *_) in enumerate(cs):
        ncols = 1 + sum(t_dof) + k
        tag = f"{build} {name} t{threads} case {b} ({kind}, cd {cd}, k {k}, t {t_dof})"
        W = _wrench_unpack(o[b], build, N, cd, ncols, din[b], tag)
        base = kind.rstrip("1")
        if kind.endswith("1"):
            assert np.isfinite(W[:cd, :ncols]).all(), (tag, "a stale operand of the inactive contact reached rows 0..5")
        worst = max(worst, _check_block(tag, base, W[:cd, :ncols], ref[b][0], ref[b][1], cd, ncols, g))
    return dict(worst_u=worst, n=len(cs))


def check_wrench_layout(build, threads=64, names=tuple(WRENCH_INSTS)):
    """exhaustive layout sweep of wrench_maps: R and Jbar^T of distinct integers, the right-hand side e_c in exactly ONE column, for
    every column and every c < M of the 31-column hierarchy and of (6, 0, [6, 3]).  That column of WM must be exactly column c of
    A_rot Jbar[:, 6:], every other live column exactly zero: a transposed rotation, a swapped h / x split, a wrong stride or a level
    off by one each move a number (the unaddressed words of U / NwJw hold NaN)"""
    n = 0
    for name in names:
        N = WRENCH_INSTS[name]
        M = N - 6
        R = (1.0 + np.arange(18)).reshape(2, 3, 3)
        J = (20.0 + np.arange(12 * N)).reshape(12, N)
        J[:, :6] = np.nan
        AJ = np.array([sum(r * t for r, t in _wrench_terms(R, J, i, N)) for i in range(12)])  # (12, M): integers far below 2^53, exact
        for cd, k, t_dof in WRENCH_LAYOUT_HIER:
            ncols = 1 + sum(t_dof) + k
            # where column `col` lives: (block, level, column inside the block)
            where = [("tg", 0, 0)] + [("U", l, j) for l, t in enumerate(t_dof) for j in range(t)] + [("N", 0, j) for j in range(k)]
            assert len(where) == ncols
            todo = [(col, c) for col in range(ncols) for c in range(M)]
            for c0 in range(0, len(todo), probe.MAX_B):
                part = todo[c0:c0 + probe.MAX_B]
                recs = []
                for col, c in part:
                    tg, U, Nw = np.zeros(M), np.zeros((4, M, 6)), np.zeros((M, 6))
                    _wrench_poison(M, cd, k, t_dof, U, Nw)
                    blk, l, j = where[col]
                    if blk == "tg":
                        tg[c] = 1.0
                    elif blk == "U":
                        U[l][c, j] = 1.0
                    else:
                        Nw[c, j] = 1.0
                    rhs = wrench_rhs(M, k, t_dof, tg, U, Nw)
                    assert rhs.sum() == 1.0 and rhs[c, col] == 1.0
                    recs.append(_wrench_record(N, R, J, tg, U, Nw))
                din = np.stack(recs)
                o = probe.run(build, name, din, np.array([_wrench_ip(cd, k, t_dof)] * len(part)), threads)
                for b, (col, c) in enumerate(part):
                    tag = f"{build} {name} t{threads} layout cd {cd} t {t_dof}: e_{c} in column {col}"
                    W = _wrench_unpack(o[b], build, N, cd, ncols, din[b], tag)
                    E = np.zeros((cd, ncols))
                    E[:, col] = AJ[:cd, c]
                    assert np.array_equal(W[:cd, :ncols], E), (tag, np.argwhere(W[:cd, :ncols] != E)[:8], W[:cd, col], AJ[:cd, c])
                n += len(part)
    return dict(n=n)


def check_gc_refusals(build):
    import pytest

    for name, ip in (("pinv_cod12", [0]), ("pinv_cod12", [13]), ("gj_rows6", [7, 0]), ("gj_rows12", [0, 1]), ("gj_rows18", [19, 0]),
                     ("gj_rows18", [4, 2]), ("spd_scaled12", [0]), ("spd_scaled12", [13]), ("mmg_12_39_39_nn", [0, 1, 1]),
                     ("mmg_12_39_39_nn", [13, 39, 39]), ("mmg_12_12_39_nt", [12, 40, 12]), ("mmg_33_12_12_tn", [33, 12, 13]),
                     ("mmg_12_33_12_nn", [12, 0, 33]), ("gram_39", [0]), ("gram_23", [7]), ("gram_50", [13]),
                     ("wrench_39", [12, 0, 2, 6, 3, 0, 0]), ("wrench_39", [6, 6, 2, 6, 3, 0, 0]), ("wrench_37", [0, 0, 1, 3, 0, 0, 0]),
                     ("wrench_23", [12, 6, 0, 6, 3, 0, 0]), ("wrench_24", [12, 6, 5, 6, 6, 6, 6]), ("wrench_50", [12, 6, 2, 6, 4, 0, 0]),
                     ("wrench_50", [6, 0, 1, 0, 3, 3, 3]), ("wrench_39", [12, 6, 4, 6, 6, 6, 12])):
        sz = probe.sizes(build, name)
        with pytest.raises(RuntimeError, match="outside"):
            probe.run(build, name, np.zeros((1, sz[0])), np.array([ip]))


# ------------------------------------------------------------------------------------------------------------------------------------
# bars of the inverses
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tolerance_table():
    tab = {}
    with open(TOL_FILE) as f:
        for line in f:
            w = line.split()
            if len(w) >= 2 and not line.startswith("#"):
                tab[w[0]] = float(w[1])
    return tab


def inverse_bar(name):
    return 10.0 * max(_tolerance_table()[name], 1.0)


def check_inverse(build, name, threads=64, bar=None):
    if name in GC_INVERSE_INSTS:
        return check_gc_inverse(build, name, threads, bar)
    return check_sweep(build, name, threads, bar) if name in SWEEP_INSTS else check_small(build, name, threads, bar)


def write_tolerances(path=TOL_FILE):
    lines = ["# worst g = |X - X_mp|max / (u kappa_2(A) |X_mp|max) of the HOST build of the wave-routine probe against the 50-digit mpmath inverse,",
             "# per instantiation (python -m tests.wave_cases --write-tolerances; riding right-hand sides included).  tests/wave_cases.py sets the",
             "# bar of both builds at 10 x this value and never below 10.  sym: |X - X^T|max in the same unit (0: a general matrix).",
             "# pinv_cod12: g against the 50-digit restatement of the reference's rank rule, kappa over the kept singular values.",
             "# instantiation worst_g sym cases"]
    for name in list(SWEEP_INSTS) + list(SMALL_INSTS) + list(GC_INVERSE_INSTS):
        r = check_inverse("emu", name, bar=1e300)
        lines.append(f"{name} {r['worst_g']:.3e} {r['worst_sym']:.3e} {r['n']}")
        print(lines[-1], flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_device_figures(path=DEV_FILE):
    """on a GPU: the worst figure of the DEVICE build per family, next to the host-derived bars (for the reader; no bar comes from here)"""
    lines = ["# worst figures of the DEVICE build (gfx950) of the wave-routine probe, 64 and 128 threads per block (python -m tests.wave_cases",
             "# --write-device-figures on a GPU).  For the reader: the bars stay host-derived or derived from the arithmetic (tests/wave_cases.py).",
             "# family / instantiation: figure"]
    both = lambda f: [f(t) for t in (64, 128)]
    for f32 in (False, True):
        r = both(lambda t: check_lanes("gpu", f32, t))
        lines.append(f"lanes{'_f32' if f32 else ''}: worst sum / scan error {max(x['worst_sum'] for x in r):.3f} u sum|x| (bar 64)")
        for op, nm, bar in ((0, "fast_rcp", 4 if f32 else 2), (1, "fast_rsqrt", 4)):
            r = both(lambda t: check_rcp_rsqrt("gpu", f32, op, t))
            lines.append(f"{nm}{'_f32' if f32 else ''}: worst relative error {max(x['worst_u'] for x in r):.3f} u (bar {bar})")
    r = both(lambda t: check_sincos("gpu", t))
    lines.append(f"sincos_r: worst |error| {max(x['worst'] for x in r):.3e} (bar {1.3e-16 + U64:.3e}); |s^2+c^2-1| {max(x['worst_unit_u'] for x in r):.2f} u "
                 f"(bar 4); over +-1e5 rad {max(x['worst_wide'] for x in r):.3e} (recorded, no bar)")
    for name, m, n, k, fc, over in GEMM_INSTS:
        r = both(lambda t: check_gemm("gpu", name, m, n, k, fc, over, t))
        lines.append(f"{name}: worst error {max(x['worst_u'] for x in r):.3f} u (|C0| + |A||B|) (bar gamma_{k + 1} ~ {k + 1})")
    for name in DOT_INSTS:
        r = both(lambda t: check_rows_dot("gpu", name, t))
        lines.append(f"{name}: worst error {max(x['worst_u'] for x in r):.3f} u sum|a||x| (bar ~ {DOT_INSTS[name][1] + DOT_INSTS[name][2]})")
    for name in AXPY_INSTS:
        r = both(lambda t: check_rows_axpy("gpu", name, t))
        lines.append(f"{name}: worst error {max(x['worst_u'] for x in r):.3f} u (|acc| + sum|a||x|) (bar ~ {AXPY_INSTS[name][0] + 1})")
    for name in list(SWEEP_INSTS) + list(SMALL_INSTS) + list(GC_INVERSE_INSTS):
        r = both(lambda t: check_inverse("gpu", name, t))
        lines.append(f"{name}: worst g {max(x['worst_g'] for x in r):.3e}, sym {max(x['worst_sym'] for x in r):.3e} (bar {inverse_bar(name):.3g})")
    for name in MMG_INSTS:
        r = both(lambda t: check_mmg("gpu", name, t))
        lines.append(f"{name}: worst error {max(x['worst_u'] for x in r):.3f} u |A||B| (bar gamma_(kk+1) <= ~ {MMG_INSTS[name][2] + 1})")
    for name, N in GRAM_INSTS.items():
        r = both(lambda t: check_gram("gpu", name, t))
        lines.append(f"{name}: worst error {max(x['worst_u'] for x in r):.3f} u |Y||J^T| (bar gamma_{N + 3} ~ {N + 3})")
    for name, N in WRENCH_INSTS.items():
        r = both(lambda t: check_wrench("gpu", name, t))
        lines.append(f"{name}: worst error {max(x['worst_u'] for x in r):.3f} u sum_c (|R||J|)_c |rhs_c| (bar gamma_{N - 3} ~ {N - 3})")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if "--write-tolerances" in sys.argv:
        write_tolerances()
    if "--write-device-figures" in sys.argv:
        at = sys.argv.index("--write-device-figures")
        write_device_figures(sys.argv[at + 1] if at + 1 < len(sys.argv) else DEV_FILE)
