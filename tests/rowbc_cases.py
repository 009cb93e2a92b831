"""Cases and checks of the row-broadcast probe (tests/rowbc_probe), shared by its host and device tests.

Every check is exact.  The device forms move values and form ONE fused multiply-add per product, so the expected bits come from the
C library's fma on the host (correctly rounded, as v_fmac_f64 is) or from a second route compiled in the same probe.  The host
emulation forms are `acc += a * b` in the host compiler's arithmetic, like every other product of the emulation (a fused form would
move the emulated solver off the results tests/test_qp_wave_emu.py pins): there the expected bits are the rounded product plus the
accumulator (``madd``).  Launches are 64 or 128 threads per block and one to three blocks (``chunks``); a wave takes one problem.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

from tests.rowbc_probe import probe

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
fma = np.frompyfunc(lambda a, b, c: _libm.fma(float(a), float(b), float(c)), 3, 1)
ROW = (np.arange(64) & ~15)


def madd(build, a, b, c):
    """a * b + c as the build under test forms it: fused on the device, product rounded first in the host emulation"""
    with np.errstate(invalid="ignore"):
        return fma(a, b, c).astype(np.float64) if build == "gpu" else np.asarray(a, float) * np.asarray(b, float) + np.asarray(c, float)


# one planted lane per DPP row, all different
PLANT = tuple((3 + 5 * r) % 16 for r in range(4))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def chunks(build, kind, din, threads):
    """the batch in launches of 1, 2 and 3 blocks in turn (128 threads: the odd counts leave the last block's second wave without a problem)"""
    wpb = threads // 64
    sizes = (1, 2 * wpb, 3 * wpb - (wpb - 1))
    out, b, i = [], 0, 0
    while b < len(din):
        n = sizes[i % 3]
        out.append(probe.run(build, kind, din[b:b + n], threads))
        b, i = b + n, i + 1
    return np.concatenate(out)


def check_replicate(build, threads):
    lanes = np.arange(64, dtype=np.uint64)
    rng = np.random.default_rng(11)
    cs = []
    for k in range(6):
        hi = np.uint64(0x3FF00000 + 0x1111 * k) + lanes * np.uint64(0x101)  # 64 distinct values in EACH half of the double
        lo = np.uint64(0x00012345 + 0x777 * k) + lanes * np.uint64(0x10001)
        cs.append(((hi << np.uint64(32)) | lo).view(np.float64))
    cs.append(rng.standard_normal(64))
    x = np.array(cs)
    assert all(len(set(bits(r) >> np.uint64(32))) == 64 and len(set(bits(r) & np.uint64(0xffffffff))) == 64 for r in x[:6])
    o = chunks(build, probe.REPLICATE, x, threads)
    assert np.array_equal(bits(o), bits(x[:, np.arange(64) & 15])), (build, threads)


@functools.lru_cache(maxsize=None)
def fma_cases():
    """(tag, x, y, acc): integers (exact), reals on accumulators +0.0 / -0.0 / real, signed-zero products, planted NaN and inf * 0"""
    rng = np.random.default_rng(12)
    cs = []
    cs.append(("int", rng.integers(-1000, 1000, 64).astype(float), rng.integers(-1000, 1000, 64).astype(float),
               rng.integers(-10**6, 10**6, 64).astype(float)))
    for acc0 in (0.0, -0.0):
        cs.append(("int", rng.integers(-1000, 1000, 64).astype(float), rng.integers(-1000, 1000, 64).astype(float), np.full(64, acc0)))
        cs.append(("real", rng.standard_normal(64) * 10.0 ** rng.uniform(-3, 3, 64), rng.standard_normal(64), np.full(64, acc0)))
        # products that are zeros of either sign: the sign of the sum depends on the accumulator's zero
        x = rng.standard_normal(64)
        x[rng.random(64) < 0.5] = 0.0
        x[rng.random(64) < 0.3] *= -1.0
        y = np.where(rng.random(64) < 0.5, 0.0, rng.standard_normal(64)) * np.where(rng.random(64) < 0.5, -1.0, 1.0)
        cs.append(("zeros", x, y, np.full(64, acc0)))
    cs.append(("real", rng.standard_normal(64), rng.standard_normal(64), rng.standard_normal(64)))
    x, y = rng.standard_normal(64), rng.standard_normal(64)
    for r in range(4):
        x[16 * r + PLANT[r]] = np.nan
    cs.append(("nan", x, y, rng.standard_normal(64)))
    x, y = rng.standard_normal(64), rng.standard_normal(64)
    for r in range(4):
        x[16 * r + PLANT[r]] = np.inf if r & 1 else -np.inf
    y[16:32] = 0.0  # inf * 0 in row 1 only; the other rows get a signed infinity
    cs.append(("inf0", x, y, rng.standard_normal(64)))
    return cs


def check_fma(build, threads):
    cs = fma_cases()
    din = np.array([np.concatenate([x, y, a]) for _, x, y, a in cs])
    o = chunks(build, probe.FMA, din, threads).reshape(len(cs), 16, 64)
    for b, (tag, x, y, a) in enumerate(cs):
        for J in range(16):
            src = x[ROW | J]
            ref = madd(build, src, y, a)
            got = o[b, J]
            where = (build, threads, b, tag, J)
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan), where
            assert np.array_equal(bits(got)[~nan], bits(ref)[~nan]), where
            if tag == "int":
                assert np.array_equal(got, src * y + a), where  # (exact in double: |.| < 2^21)
            if tag == "nan":  # the planted lane reaches the 16 lanes of its own row when J names it, and nothing else
                assert np.array_equal(nan, np.repeat([J == PLANT[r] for r in range(4)], 16)), where
            if tag == "inf0":
                want_nan = np.zeros(64, bool)
                want_nan[16:32] = J == PLANT[1]
                assert np.array_equal(nan, want_nan), where
                for r in (0, 2, 3):
                    assert np.array_equal(np.isinf(got[16 * r:16 * r + 16]), np.full(16, J == PLANT[r])), where


@functools.lru_cache(maxsize=None)
def dz_cases(nv):
    """product-shaped rows (dwbc_qp_wave.h): 53 row owners with unit rows over nv variables, the rest zero rows; z in lanes 0..nv-1 of m,
    the multipliers r of the slot lanes (16..16+nv-1) beside it -- they must NOT reach the product"""
    rng = np.random.default_rng(20 + nv)
    cs = []
    for k in range(5):
        g = np.zeros((64, 12))
        g[:53, :nv] = rng.standard_normal((53, nv))
        g[:53] /= np.linalg.norm(g[:53], axis=1, keepdims=True)
        if k == 1:
            g[:53, :nv][rng.random((53, nv)) < 0.3] = 0.0  # sparse rows (torque-limit rows have few entries)
        m = np.zeros(64)
        m[:nv] = rng.standard_normal(nv) * (1e-9 if k == 2 else 1.0)  # (k = 2: |z| small, the re-projection case)
        m[16:16 + nv] = rng.standard_normal(nv) * 1e3
        m[32:] = rng.standard_normal(32) * 1e6
        if k == 3:
            m[:nv] = -0.0  # z = -0: every product is a signed zero onto the +0.0 start
        cs.append((g, m))
    return cs


def check_dz(build, nv, threads):
    kind = {6: probe.DZ6, 9: probe.DZ9, 12: probe.DZ12}[nv]
    cs = dz_cases(nv)
    o = chunks(build, kind, np.array([np.concatenate([g.ravel(), m]) for g, m in cs]), threads)
    for b, (g, m) in enumerate(cs):
        ref = np.zeros(64)
        for j in range(nv):
            ref = madd(build, np.full(64, m[j]), g[:, j], ref)
        where = (build, nv, threads, b)
        assert np.array_equal(bits(o[b, :64]), bits(o[b, 64:])), (where, "row broadcast against the readlane-fed form")
        assert np.array_equal(bits(o[b, :64]), bits(ref)), (where, "against the host's own sum")
        assert not o[b, 53:64].any(), where


def check_sweep(build, threads):
    """the 12-pivot sweep fed by row broadcast against the LDS-fed lds_pivot<12, 11, 0> kept in the probe: same bits, on the spd12 family of
    tests/wave_cases.py (its values against 50-digit references: tests/test_wave_probe_gpu.py)"""
    from tests import wave_cases as wc

    cs = wc.small_cases("spd12_lds")
    o = chunks(build, probe.SWEEP, np.array([A.ravel() for _, _, A in cs]), threads)
    n_ok = 0
    for b, (kind, _, A) in enumerate(cs):
        new, old = o[b, :145], o[b, 145:]
        where = (build, threads, b, kind)
        assert old[144] == (0.0 if kind == "bad" else 1.0), where
        assert new[144] == old[144], where
        assert np.array_equal(np.isnan(new), np.isnan(old)), where
        k = ~np.isnan(new)
        assert np.array_equal(bits(new)[k], bits(old)[k]), where
        if kind != "bad":
            assert np.isfinite(new).all() and not (new[:144] == -7777.0).any(), where
            n_ok += 1
    assert n_ok >= 9
