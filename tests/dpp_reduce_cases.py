"""Cases and numpy expectations for the one-instruction DPP reductions of dwbc_wave.h (WAVE_ARGMIN_F32, WAVE_ARGMIN_ROW1) and for
ROW_REPLICATE followed by the row-broadcast dot product, run through the existing probes (tests/wave_probe family ``lanes`` /
``lanes_f32``, tests/rowbc_probe kinds 0 and 2 - 4), unchanged.  One wavefront per case, one launch per check.

Every expectation is worked out here from the contracts written in dwbc_wave.h and wave_probe_body.h, never from a probe's output:
  WAVE_ARGMIN_F32   first lane whose value, rounded to float, is the smallest; lane 0 when no lane compares equal (all NaN)
  WAVE_ARGMIN_ROW1  over lanes 16..31, keys = lanes.  Host build: exact minimum, first lane.  Device build: minimum of the order-
                    preserving 64-bit image of the double with its 7 lowest bits replaced by the lane (so values that differ only in
                    those bits tie, first lane wins, and -0.0 sorts below +0.0); value and key returned are the winner's own
  WAVE_ARGMIN       the same over the 64 lanes
  ROW_REPLICATE     lanes 16..63 take the bits of lane (lane & 15)
  ROWBC_DOT         acc = +0.0, then one term per j = 0 .. N-1 in this order: fused multiply-add on the device, product rounded and
                    then added in the host emulation
"""
import functools
from fractions import Fraction

import numpy as np

from tests.rowbc_probe import probe as rprobe
from tests.wave_probe import probe

LANE = np.arange(64)
ROW1 = np.arange(16, 32)


def _f(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def _u(vals):
    return np.asarray(vals, np.float64).view(np.uint64)


def _rec(val):
    return np.concatenate([val, LANE.astype(float), ((LANE * 7 + 3) % 64).astype(float), np.zeros(64)])


@functools.lru_cache(maxsize=None)
def cases():
    """list of (group, val[64]).  Unless the group says otherwise the values are distinct after rounding to float."""
    rng = np.random.default_rng(2024)
    out = []

    def distinct():  # multiples of 2^-6 below 64 in magnitude, all different: exact and distinct as floats
        return rng.choice(np.arange(-4000, 4001), 64, replace=False) / 64.0

    for b in range(64):  # the minimum in each of the 64 lanes in turn
        v = distinct()
        v[b] = -100.0 - b
        out.append(("min_lane", v))
    for b in range(16):  # ... and in each lane of row 1, with smaller values in the other rows and above the rest of row 1
        for sign in (1.0, -1.0):
            v = distinct()
            v[ROW1] = sign * 200.0 + rng.choice(np.arange(1, 400), 16, replace=False) / 8.0
            v[16 + b] = sign * 200.0
            out.append(("min_row1", v))
    for t in range(48):  # the minimum shared: inside one row, across rows, inside row 1
        v = distinct()
        if t % 3 == 0:
            r = int(rng.integers(4))
            lanes = 16 * r + rng.choice(16, int(rng.integers(2, 6)), replace=False)
        elif t % 3 == 1:
            lanes = rng.choice(64, int(rng.integers(2, 8)), replace=False)
        else:
            lanes = 16 + rng.choice(16, int(rng.integers(2, 6)), replace=False)
            v[ROW1] += 300.0
        v[lanes] = -77.5 if t % 2 else 0.015625
        if t % 2 == 0:
            v[v < 0.015625] += 200.0
        out.append(("tie", v))
    for t in range(48):  # row 1: two or three lanes share the smallest HIGH word and differ in the low word; others carry a larger high
        v = distinct()   # word over a SMALLER low word, which must not win the second stage
        neg = t % 2 == 1
        hi = np.uint64(0x40091EB8) + np.uint64(rng.integers(0, 1 << 8))
        hi_w = hi | np.uint64(0x80000000) if neg else hi
        n = 2 + t % 2
        lanes = 16 + rng.choice(16, n, replace=False)
        bit = (7, 8, 16, 31, 20, 12)[t % 6]  # lowest kept bit, top bit of the low word, some between
        lows = rng.choice(np.arange(1, 1 << 12), n, replace=False).astype(np.uint64) << np.uint64(max(bit - 11, 7))
        lows |= np.uint64(1) << np.uint64(bit)
        lows[0] ^= np.uint64(1) << np.uint64(bit)  # (lane lanes[0] differs from the others in that very bit, too)
        others = np.setdiff1d(ROW1, lanes)
        step = -1 if neg else 1  # (a negative double grows downward with its bits)
        oh = (hi_w.astype(np.int64) + step * rng.integers(1, 5, others.size)).astype(np.uint64)
        ol = rng.integers(0, 64, others.size).astype(np.uint64) << np.uint64(7)
        ol = np.where(rng.random(others.size) < 0.5, ol, np.uint64(0xFFFFFF80) - ol)  # (either end: the image of a negative double is inverted)
        v[others] = _f((oh << np.uint64(32)) | ol)
        v[lanes] = _f((hi_w << np.uint64(32)) | lows)
        rest = np.setdiff1d(LANE, ROW1)
        v[rest] = np.where(rng.random(rest.size) < 0.5, v[lanes[0]], v[rest])  # (copies of a contender outside the row change nothing in it)
        out.append(("low_word", v))
    for t in range(32):  # two lanes that differ only in the last bit / inside the 7 bits the device drops
        v = distinct() + 500.0
        i, j = 16 + rng.choice(16, 2, replace=False) if t % 2 else rng.choice(64, 2, replace=False)
        base = _u([rng.uniform(1.0, 2.0) * (-1.0 if t % 4 < 2 else 1.0)])[0] & ~np.uint64(127)
        a, b = (0, 1) if t % 8 < 4 else tuple(int(x) for x in rng.choice(128, 2, replace=False))
        v[i], v[j] = _f(base | np.uint64(a)), _f(base | np.uint64(b))
        out.append(("last_bits", v))
    for t in range(32):  # doubles that differ but round to the same float; the exact minimum sits in the LATER lane
        v = distinct() + 500.0
        i, j = np.sort(16 + rng.choice(16, 2, replace=False) if t % 2 else rng.choice(64, 2, replace=False))
        x = float(np.float32(rng.uniform(1.0, 2.0))) * (-1.0 if t % 4 < 2 else 1.0)
        v[i], v[j] = x + 2.0 ** -30, x - 2.0 ** -31
        out.append(("same_float", v))
    for t in range(16):  # zeros of either sign among positive values
        v = np.abs(distinct()) + 1.0
        lanes = np.sort(16 + rng.choice(16, 3, replace=False) if t % 2 else rng.choice(64, 4, replace=False))
        v[lanes] = rng.permutation([0.0, -0.0, 0.0, -0.0])[:lanes.size]
        out.append(("zeros", v))
    for t in range(16):  # -inf in one lane (twice: the first wins), +inf in all lanes but a few
        v = distinct()
        i, j = np.sort(rng.choice(64, 2, replace=False))
        v[i] = -np.inf
        if t % 2:
            v[j] = -np.inf
        out.append(("minus_inf", v))
        v = np.full(64, np.inf)
        v[rng.choice(64, 3, replace=False)] = [3.0, 2.0, 2.5]
        v[16 + rng.choice(16, 2, replace=False)] = [7.0, 6.5]
        out.append(("plus_inf", v))
    for t in range(16):  # denormals: of the double format (zero as floats: a tie with the zeros), of the float format (distinct floats)
        v = np.abs(distinct()) + 1.0
        lanes = np.sort(rng.choice(64, 6, replace=False))
        if t % 2:
            v[lanes] = [5e-324, 0.0, 2.5e-310, 1e-320, 0.0, 4e-315]
        else:
            v[lanes] = np.array([3.0, 7.0, 2.0, 11.0, 5.0, 13.0]) * 2.0 ** -140 * (-1.0 if t % 4 == 0 else 1.0)
        v[16 + rng.choice(16, 2, replace=False)] = [2.0 ** -1040, 2.0 ** -1030]
        out.append(("denormal", v))
    out.append(("sentinel", np.full(64, 1.0e300)))  # every lane at DWBC_QP_INF: +inf as float, lane 0
    out.append(("sentinel", np.full(64, np.inf)))
    for b in (0, 15, 16, 31, 32, 63):
        v = np.full(64, 1.0e300)
        v[b] = 1.0e299 if b % 2 else -1.0e-3
        out.append(("sentinel", v))
    out.append(("nan", np.full(64, np.nan)))  # no lane compares equal to the minimum: lane 0
    assert len(out) <= 512
    return out


def _held(val, f32):
    """the values as the probe's build holds them after its load (wave_probe_body.h: sentinel clamp, then the arithmetic type)"""
    if f32:
        inf = np.float32(1.0e30)
        with np.errstate(over="ignore"):
            h = np.where(val >= float(inf), inf, val.astype(np.float32))
        return h.astype(np.float64)
    return np.where(val >= 1.0e300, 1.0e300, val)


def _key(v):
    """order-preserving image of a double, the 7 lowest bits replaced by the lane (dwbc_wave.h, argmin_key)"""
    b = _u(v)
    b = np.where(b >> np.uint64(63) != 0, ~b, b | (np.uint64(1) << np.uint64(63)))
    return (b & ~np.uint64(127)) | LANE.astype(np.uint64)


def expected(val, f32, build):
    """(lane of WAVE_ARGMIN_F32, lane of WAVE_ARGMIN_ROW1, lane of WAVE_ARGMIN) for one case"""
    v = _held(val, f32)
    with np.errstate(over="ignore"):
        v32 = v.astype(np.float32)
    fl = 0 if np.isnan(v32).all() else int(np.argmin(v32))
    if build == "gpu":
        k = _key(v)
        return fl, 16 + int(np.argmin(k[16:32])), int(np.argmin(k))
    return fl, 16 + int(np.argmin(v[16:32])), int(np.argmin(v))


def check_argmin(build, f32, threads=64):
    cs = cases()
    name = "lanes_f32" if f32 else "lanes"
    o = probe.run(build, name, np.stack([_rec(v) for _, v in cs]), np.zeros((len(cs), 1), np.int32), threads)
    seen = set()
    for b, (g, val) in enumerate(cs):
        tag = f"{build} {name} t{threads} case {b} ({g})"
        r = o[b]
        fl, rl, wl = expected(val, f32, build)
        v = _held(val, f32)
        assert r[6] == fl, (tag, "WAVE_ARGMIN_F32", r[6], fl)
        if g != "nan":
            assert r[5] == rl and _u(r[4]) == _u(v[rl]), (tag, "WAVE_ARGMIN_ROW1", r[4:6], rl, v[rl])
            assert r[3] == wl and _u(r[2]) == _u(v[wl]), (tag, "WAVE_ARGMIN", r[2:4], wl, v[wl])
        seen.add((g, fl))
    assert {l for g, l in seen if g == "min_lane"} == set(range(64))
    return len(cs)


# ---- ROW_REPLICATE, alone and in front of the row-broadcast dot product
@functools.lru_cache(maxsize=None)
def replicate_cases():
    rng = np.random.default_rng(77)
    out = [LANE + 1.0, -(LANE + 1.0) * 2.0 ** -1030, _f((LANE.astype(np.uint64) + np.uint64(1)) * np.uint64(0x0101010101010101))]
    for _ in range(29):  # distinct bit patterns in both dwords of all 64 lanes
        out.append(_f(rng.permutation(1 << 16)[:64].astype(np.uint64) * np.uint64(0x0001000100010001) ^ (LANE.astype(np.uint64) << np.uint64(33))))
    return np.stack(out)


def check_replicate(build, threads=64):
    x = replicate_cases()
    o = rprobe.run(build, rprobe.REPLICATE, x, threads)
    assert np.array_equal(_u(o), _u(x[:, LANE & 15])), (build, threads)
    return len(x)


@functools.lru_cache(maxsize=None)
def dot_cases():
    """(g (B, 64, 12), m (B, 64)): distinct m in all 64 lanes (a source lane outside the own row, or outside 0..NV-1, shows).  The first
    half holds small integers (every partial sum exact: one expectation whatever the rounding of the terms), the second half reals"""
    rng = np.random.default_rng(78)
    g, m = [], []
    for t in range(8):
        g.append(rng.integers(-512, 513, (64, 12)).astype(float))
        m.append(rng.permutation(np.arange(-40, 41)[np.arange(-40, 41) != 0])[:64].astype(float))
    for t in range(8):
        g.append(rng.standard_normal((64, 12)) * 2.0 ** rng.integers(-8, 9, (64, 12)))
        mm = rng.standard_normal(64)
        assert np.unique(mm).size == 64
        m.append(mm)
    return np.stack(g), np.stack(m)


def _dot_ref(g, m, nv, fused):
    out = np.zeros(g.shape[:2])
    for b in range(g.shape[0]):
        for l in range(64):
            acc = 0.0
            for j in range(nv):
                if fused:
                    acc = float(Fraction(m[b, j]) * Fraction(g[b, l, j]) + Fraction(acc))  # one rounding (float(Fraction) rounds to nearest even)
                else:
                    acc = acc + m[b, j] * g[b, l, j]
            out[b, l] = acc
    return out


def check_replicate_dot(build, nv, threads=64):
    g, m = dot_cases()
    kind = {6: rprobe.DZ6, 9: rprobe.DZ9, 12: rprobe.DZ12}[nv]
    o = rprobe.run(build, kind, np.concatenate([g.reshape(len(g), 768), m], axis=1), threads)
    ref = _dot_ref(g, m, nv, fused=build == "gpu")
    assert np.array_equal(ref[:8], np.einsum("blj,bj->bl", g[:8, :, :nv], m[:8, :nv])), "integer cases are exact"
    assert np.array_equal(_u(o[:, :64]), _u(ref)), (build, nv, threads, "replicate + ROWBC_DOT")
    assert np.array_equal(_u(o[:, 64:]), _u(ref)), (build, nv, threads, "the v_readlane form")
    return len(g)
