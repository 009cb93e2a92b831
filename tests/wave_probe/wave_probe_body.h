// wave_probe_body.h -- TEST HARNESS ONLY.  Runs the shipped text of the device-only wave routines (libdwbc_amd/csrc/dwbc_wave.h,
// dwbc_cycle2.h, dwbc_cycle2p.h, dwbc_cycle_gc.h) alone, on operands of the caller's choosing: one set of templates, compiled for the device
// (wave_probe.hip -> libdwbc_wave_probe.so, one wavefront per problem, 64 or 128 threads per block -- the two-wave kernel runs these
// routines in wave 1, where lane = threadIdx.x & 63) and for the host (the same files with DWBC_HOST_EMU -> libdwbc_wave_probe_emu.so).
// The probe includes the shipped headers and calls the shipped functions; it holds no copy of any of them, and nothing of it is
// linked into libdwbc_hip.so.  Included once per arithmetic type: wave_probe.hip (double, every family) and wave_probe_f32.hip
// (WAVE_PROBE_F32: DWBC_REAL = float, namespace renamed; the cross-lane primitives and the scalar routines -- wave_gemm, the LDS-fed
// sweeps, the batched row products and the two matrix-core tiles of the cycle, contact_gram and wrench_maps, are fp64-only on the
// device, their fp32 build takes the same plain code as the host).
//
// A family is a struct: NIN doubles and NIP ints in, NOUT doubles out per problem, LDS reals of scratch per wave (even: every wave's
// slice and every operand in it starts at a 16-byte boundary, as the kernels place theirs), check(ip) for the run-time sizes and
// problem(in, ip, out, L).  Outputs are the caller's, pre-filled with its sentinel: what a problem does not write keeps it.
// Every loop of every routine under test has compile-time bounds; the probe's own copy loops run over compile-time counts.
//
// Rules the cross-lane arg-min relies on (read off the call sites: dwbc_qp_wave.h ratio test, dwbc_cycle_gc.h QR pivot):
//   WAVE_ARGMIN / WAVE_ARGMIN_ROW1: every caller passes key = lane, i.e. keys INCREASE with the lane.  Under that contract the
//     host rule (ties to the smaller key) and the device rule (ties to the smaller lane) agree; tests/wave_cases.py asserts it of its
//     cases.  The device compares with the 7 lowest mantissa bits dropped: of two values that close either may win, and the value
//     and key returned are the winner's own.  The device orders -0.0 below +0.0, the host does not: of zeros of mixed sign either
//     lane may win (the callers form -fabs(x), all -0.0, or a step length that is equally valid at either lane).
//   WAVE_ARGMIN_F32: first lane whose value, rounded to float, is the smallest.  The callers pass no NaN; when no lane compares
//     equal to the minimum (all NaN) both builds return lane 0.  With NaN in SOME lanes the builds differ (fminf skips a NaN, the
//     host's `<` never leaves a NaN in lane 0): not relied on, not tested.
#pragma once
#include <limits>

#ifdef WAVE_PROBE_F32
#include "../../libdwbc_amd/csrc/dwbc_cycle.h"
#else
#include "../../libdwbc_amd/csrc/dwbc_cycle_gc.h"
#endif

namespace dwbc {

struct WpArgs {
    int B;
    const double *in;
    const int *ip;
    double *out;
};

constexpr double kWpSentinel = -7777.0;
constexpr int wp_ev(int x) { return (x + 1) & ~1; }
#define WP_NAN std::numeric_limits<real_t>::quiet_NaN()

// ---- 1. cross-lane primitives.  in: val[64] key[64] src[64] flag[64]; ip: the uniform source lane.
// out: 0 sum, 1 any, 2/3 arg-min value/key, 4/5 the same over lanes 16..31, 6 WAVE_ARGMIN_F32's lane, 7 BCAST, 8 BCASTA, 9 BCASTI;
// 16.. WAVE_PREFIX_A of element 1, 80.. SHFL, 144.. SHFLA (per-lane source), 208.. element 0 of the prefix array (must stay -1)
struct WpLanes {
    static constexpr int NIN = 256, NIP = 1, NOUT = 272, LDS = 2;
    static const char *check(const int *ip) { return (ip[0] < 0 || ip[0] > 63) ? "source lane outside 0..63" : nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *) {
        DWBC_LANE_DECL;
        PL(real_t, val);
        PL(int, key);
        PL(int, src);
        PL(int, flag);
        PLA(real_t, arr, 2);
        PL(real_t, sh);
        PL(real_t, sha);
#ifdef DWBC_HOST_EMU
        const int usrc = ip[0];
#else
        const int usrc = __builtin_amdgcn_readfirstlane(ip[0]);
#endif
        LANES {
            const double v = in[lane];
            LV(val) = v >= (double)DWBC_QP_INF ? DWBC_QP_INF : (real_t)v;
            LV(key) = (int)in[64 + lane];
            LV(src) = (int)in[128 + lane] & 63;
            LV(flag) = in[192 + lane] != 0.0 ? 1 : 0;
            LV(arr)[0] = real_t(-1.0);
            LV(arr)[1] = LV(val);
        }
        real_t sum, av, rv;
        int ak, rk, fl;
        bool any;
        WAVE_SUM(val, sum);
        WAVE_ANY(flag, any);
        WAVE_ARGMIN(val, key, av, ak);
        WAVE_ARGMIN_ROW1(val, key, rv, rk);
        WAVE_ARGMIN_F32(val, fl);
        const real_t bc = BCAST(val, usrc), bca = BCASTA(arr, 1, usrc);
        const int bci = BCASTI(key, usrc);
        LANES {
            LV(sh) = SHFL(val, LV(src));
            LV(sha) = SHFLA(arr, 1, LV(src));
        }
        WAVE_PREFIX_A(arr, 1);
        LANES {
            if (lane == 0) {
                out[0] = (double)sum, out[1] = any ? 1.0 : 0.0, out[2] = (double)av, out[3] = ak, out[4] = (double)rv, out[5] = rk;
                out[6] = fl, out[7] = (double)bc, out[8] = (double)bca, out[9] = bci;
            }
            out[16 + lane] = (double)LV(arr)[1];
            out[80 + lane] = (double)LV(sh);
            out[144 + lane] = (double)LV(sha);
            out[208 + lane] = (double)LV(arr)[0];
        }
    }
};

// ---- 2. scalar math, one argument per lane.  ip: 0 fast_rcp, 1 fast_rsqrt, 2 sincos_r.  out: result[64], second result[64] (cos)
struct WpMath {
    static constexpr int NIN = 64, NIP = 1, NOUT = 128, LDS = 2;
    static const char *check(const int *ip) { return (ip[0] < 0 || ip[0] > 2) ? "operation outside 0..2" : nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *) {
        DWBC_LANE_DECL;
        const int op = ip[0];
        LANES {
            const real_t x = (real_t)in[lane];
            real_t a = real_t(0.0), b = real_t(0.0);
            if (op == 0) a = fast_rcp(x);
            else if (op == 1) a = fast_rsqrt(x);
            else sincos_r(x, &a, &b);
            out[lane] = (double)a;
            out[64 + lane] = (double)b;
        }
    }
};

#ifndef WAVE_PROBE_F32
// (range clamp of an address only: the index the accessor was CALLED with is noted unclamped and asserted by the tests)
DWBC_WDEV int wp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- 3. wave_gemm.  in: A (MR x KV), B (KV x NCV), C0 (MR x NCV), row-major.  In LDS each sits inside a frame of NaN (one guard
// row / column on every side); the result goes to a framed block pre-filled with the sentinel -- or, OVER (with SYNC_STORE), over
// the leading NCV columns of A.  out: that whole framed block, then per lane the smallest (3) and largest (3) row, reduction and
// column index any accessor was called with.
template <int MR, int NCV, int KV, bool FC, bool OVER>
struct WpGemm {
    static constexpr int AC = KV + 2, BC = NCV + 2, CC = NCV + 2;
    static constexpr int oA = 0, oB = oA + wp_ev((MR + 2) * AC), oC = oB + wp_ev((KV + 2) * BC), oD = oC + wp_ev((MR + 2) * CC);
    static constexpr int LDS = oD + wp_ev((MR + 2) * CC);
    static constexpr int NF = OVER ? (MR + 2) * AC : (MR + 2) * CC;
    static constexpr int NIN = MR * KV + KV * NCV + MR * NCV, NIP = 1, NOUT = NF + 64 * 6;
    static_assert(oB % 2 == 0 && oC % 2 == 0 && oD % 2 == 0 && LDS % 2 == 0, "16-byte aligned operands");
    static_assert(!OVER || NCV <= KV, "the result fits over A");
    static const char *check(const int *) { return nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *, double *out, real_t *L) {
        DWBC_LANE_DECL;
        real_t *Af = L + oA, *Bf = L + oB, *Cf = L + oC, *Df = L + oD;
        LANES {
            for (int x = lane; x < LDS; x += 64) L[x] = (x >= oD && x < oD + (MR + 2) * CC) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int x = lane; x < MR * KV; x += 64) Af[(x / KV + 1) * AC + x % KV + 1] = (real_t)in[x];
            for (int x = lane; x < KV * NCV; x += 64) Bf[(x / NCV + 1) * BC + x % NCV + 1] = (real_t)in[MR * KV + x];
            for (int x = lane; x < MR * NCV; x += 64) Cf[(x / NCV + 1) * CC + x % NCV + 1] = (real_t)in[MR * KV + KV * NCV + x];
        }
        WSYNC();
        DWBC_SYNC();
        int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-(1 << 30), -(1 << 30), -(1 << 30)};
        auto note = [&](int d, int v) {
            lo[d] = v < lo[d] ? v : lo[d];
            hi[d] = v > hi[d] ? v : hi[d];
        };
        auto fa = [&](auto, auto, int i, int k) {
            note(0, i), note(1, k);
            return Af[(wp_clampi(i, -1, MR) + 1) * AC + wp_clampi(k, -1, KV) + 1];
        };
        auto fb = [&](auto, int k, int j) {
            note(1, k), note(2, j);
            return Bf[(wp_clampi(k, -1, KV) + 1) * BC + wp_clampi(j, -1, NCV) + 1];
        };
        auto fc = [&](int i, int j) {
            note(0, i), note(2, j);
            return Cf[(wp_clampi(i, -1, MR) + 1) * CC + wp_clampi(j, -1, NCV) + 1];
        };
        auto fs = [&](int i, int j, real_t v) {
            note(0, i), note(2, j);
            const int ci = wp_clampi(i, -1, MR) + 1, cj = wp_clampi(j, -1, NCV) + 1;
            if (OVER) Af[ci * AC + cj] = v; else Df[ci * CC + cj] = v;
        };
        if constexpr (FC) wave_gemm<MR, NCV, KV, OVER>(fa, fb, fs, fc);
        else wave_gemm<MR, NCV, KV, OVER>(fa, fb, fs);
        DWBC_SYNC();
        WSYNC();
        LANES {
            const real_t *F = OVER ? Af : Df;
            for (int x = lane; x < NF; x += 64) out[x] = (double)F[x];
            for (int d = 0; d < 3; d++) out[NF + lane * 6 + d] = lo[d], out[NF + lane * 6 + 3 + d] = hi[d];
        }
    }
};

// ---- 5. lds_rows_dot / lds_rows_axpy.  The matrix sits at a 16-byte aligned offset inside NaN: two reals before it, its padding
// columns NC .. RS-1, and everything behind its last row (the element just past it included).
// dot: in A (NR x NC), x (64 x NC: the lane's register column), out0 (64 x NO: what `out` holds before);  out: 64 x NO
template <int NR, int NC, int RS, int CH, int MODE, bool AL, int OFF, int NO>
struct WpRowsDot {
    static constexpr int oA = 2, LDS = oA + wp_ev(NR * RS) + 4;
    static constexpr int NIN = NR * NC + 64 * NC + 64 * NO, NIP = 1, NOUT = 64 * NO;
    static_assert(oA % 2 == 0 && LDS % 2 == 0, "16-byte aligned matrix");
    static const char *check(const int *) { return nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *, double *out, real_t *L) {
        DWBC_LANE_DECL;
        PLA(real_t, x, NC);
        PLA(real_t, o, NO);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < NR * NC; e += 64) L[oA + (e / NC) * RS + e % NC] = (real_t)in[e];
#pragma unroll
            for (int i = 0; i < NC; i++) LV(x)[i] = (real_t)in[NR * NC + lane * NC + i];
#pragma unroll
            for (int i = 0; i < NO; i++) LV(o)[i] = (real_t)in[NR * NC + 64 * NC + lane * NO + i];
        }
        WSYNC();
        DWBC_SYNC();
        LANES { lds_rows_dot<NR, NC, RS, CH, MODE, AL, OFF, NO>(L + oA, LV(x), LV(o)); }
        LANES {
#pragma unroll
            for (int i = 0; i < NO; i++) out[lane * NO + i] = (double)LV(o)[i];
        }
    }
};
// axpy: in A (NR x NC), x (64 x NR), acc0 (64 x NC);  out: 64 x NC
template <int NR, int NC, int RS, int CH, bool AL>
struct WpRowsAxpy {
    static constexpr int oA = 2, LDS = oA + wp_ev(NR * RS) + 4;
    static constexpr int NIN = NR * NC + 64 * NR + 64 * NC, NIP = 1, NOUT = 64 * NC;
    static_assert(oA % 2 == 0 && LDS % 2 == 0, "16-byte aligned matrix");
    static const char *check(const int *) { return nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *, double *out, real_t *L) {
        DWBC_LANE_DECL;
        PLA(real_t, x, NR);
        PLA(real_t, o, NC);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < NR * NC; e += 64) L[oA + (e / NC) * RS + e % NC] = (real_t)in[e];
#pragma unroll
            for (int i = 0; i < NR; i++) LV(x)[i] = (real_t)in[NR * NC + lane * NR + i];
#pragma unroll
            for (int i = 0; i < NC; i++) LV(o)[i] = (real_t)in[NR * NC + 64 * NR + lane * NC + i];
        }
        WSYNC();
        DWBC_SYNC();
        LANES { lds_rows_axpy<NR, NC, RS, CH, AL>(L + oA, LV(x), LV(o)); }
        LANES {
#pragma unroll
            for (int i = 0; i < NC; i++) out[lane * NC + i] = (double)LV(o)[i];
        }
    }
};

// ---- 4. inverses.
// The register / LDS-fed sweeps on a column-per-lane matrix.  KIND 0: sweep_inverse_tree<TopoTocabi, 39>, 1: sweep_inverse_tree_lds,
// 2: sweep_inverse_tree_lds_multi<.., DWBC_SWEEP_W>, 3: sweep_inverse_tree<TopoDense<33>, 33>, 4: sweep_inverse_lds<33>.
// in: 64 x NN, the register column of every lane: lanes < NN a column of the matrix (its diagonal goes to dg), lanes >= NN a
// right-hand side riding along with dg = 1, as the two-wave cycle loads them (dwbc_cycle2p.h, phase 1b).
// out: the 64 columns after the sweep, dg[64], ok
#ifndef DWBC_SWEEP_W
#define DWBC_SWEEP_W 4
#endif
template <int KIND>
struct WpSweep {
    static constexpr int NN = KIND < 3 ? 39 : 33;
    static constexpr int LDS = DWBC_SWEEP_W * 2 * ((NN + 1) / 2) + 2;  // (>= 64: the single-pivot sweeps give every lane a slot)
    static constexpr int NIN = 64 * NN, NIP = 1, NOUT = 64 * NN + 64 + 1;
    static_assert(LDS >= 66 && LDS % 2 == 0, "column buffer");
    static const char *check(const int *) { return nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *, double *out, real_t *L) {
        DWBC_LANE_DECL;
        PLA(real_t, s, NN);
        PL(real_t, dg);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = WP_NAN;
#pragma unroll
            for (int i = 0; i < NN; i++) LV(s)[i] = (real_t)in[lane * NN + i];
            LV(dg) = lane < NN ? (real_t)in[lane * NN + (lane < NN ? lane : 0)] : real_t(1.0);
        }
        WSYNC();
        DWBC_SYNC();
        int ok;
        if constexpr (KIND == 0) ok = sweep_inverse_tree<TopoTocabi, 39>(s, dg);
        else if constexpr (KIND == 1) ok = sweep_inverse_tree_lds<TopoTocabi, 39>(s, dg, L);
        else if constexpr (KIND == 2) ok = sweep_inverse_tree_lds_multi<TopoTocabi, 39, DWBC_SWEEP_W>(s, dg, L);
        else if constexpr (KIND == 3) ok = sweep_inverse_tree<TopoDense<33>, 33>(s, dg);
        else ok = sweep_inverse_lds<33>(s, dg, L);
        DWBC_SYNC();
        LANES {
#pragma unroll
            for (int i = 0; i < NN; i++) out[lane * NN + i] = (double)LV(s)[i];
            out[64 * NN + lane] = (double)LV(dg);
            if (lane == 0) out[64 * NN + 64] = ok;
        }
    }
};

// The LDS-resident small inverses.  KIND 0: spd_inverse_small (ip: n = 1..12, row stride 12 -- n < 12 leaves pivots out of the
// 12-wide sweep, n <= 6 goes to the Cholesky form), 1: spd_inverse12_lds out of place, 2: the same with Out == Mx,
// 3: spd_inverse_chol6 (ip: n = 1..6, row stride 6, with the pivot ratio).  in: 12 x 12 (KIND 3: 6 x 6).
// out: the output block (pre-filled with the sentinel where it is not the input), ok, pivot ratio
template <int KIND>
struct WpSmall {
    static constexpr int LD = KIND == 3 ? 6 : 12;
    static constexpr int oM = 0, oO = 144, oS = 288, LDS = 288 + 12 + 2;
    static constexpr int NIN = LD * LD, NIP = 1, NOUT = LD * LD + 2;
    static const char *check(const int *ip) {
        if (KIND == 0 && (ip[0] < 1 || ip[0] > 12)) return "n outside 1..12";
        if (KIND == 3 && (ip[0] < 1 || ip[0] > 6)) return "n outside 1..6";
        return nullptr;
    }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int n = ip[0];
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= oO && e < oO + 144) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < LD * LD; e += 64) L[oM + e] = (real_t)in[e];
        }
        WSYNC();
        DWBC_SYNC();
        real_t *Mx = L + oM, *Out = KIND == 2 ? L + oM : L + oO;
        real_t pr = real_t(-1.0);
        int ok;
        if constexpr (KIND == 0) ok = spd_inverse_small(Mx, 12, n, Out, 12, L + oS);
        else if constexpr (KIND == 3) ok = spd_inverse_chol6(Mx, 6, n, Out, 6, &pr);
        else ok = spd_inverse12_lds(Mx, Out, L + oS);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < LD * LD; e += 64) out[e] = (double)Out[e];
            if (lane == 0) out[LD * LD] = ok, out[LD * LD + 1] = (double)pr;
        }
    }
};

// spd_inverse_chol6_x3 as the helper wave calls it: three densely stored matrices (row stride n_q; ip: n0 n1 n2, each 0..6), the first
// two out of place, the third in place.  in: 3 x 36;  out: 3 x 36 (the three output blocks), ok[3]
struct WpChol3 {
    static constexpr int LDS = 5 * 36 + 2;
    static constexpr int NIN = 108, NIP = 3, NOUT = 111;
    static const char *check(const int *ip) {
        for (int q = 0; q < 3; q++)
            if (ip[q] < 0 || ip[q] > 6) return "n outside 0..6";
        return nullptr;
    }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= 108 && e < 180) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < 108; e += 64) L[e] = (real_t)in[e];
        }
        WSYNC();
        DWBC_SYNC();
        int ok3[3] = {-1, -1, -1};
        spd_inverse_chol6_x3(L, ip[0], L + 108, L + 36, ip[1], L + 144, L + 72, ip[2], L + 72, ok3);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < 72; e += 64) out[e] = (double)L[108 + e];
            for (int e = lane; e < 36; e += 64) out[72 + e] = (double)L[72 + e];
            if (lane == 0) out[108] = ok3[0], out[109] = ok3[1], out[110] = ok3[2];
        }
    }
};
// ---- 6. the routines of the general-contact kernel (dwbc_cycle_gc.h) and the rank-revealing pseudo-inverse it shares with the
// product kernels (dwbc_cycle2.h).  fp64 only: that kernel refuses fp32.  Instantiated in wave_probe_gc.hip.
// The thread-strided routines take Thr{lane} with NT = 64 on the device and Thr{0} with NT = 1 on the host, as the kernels do.
#ifdef DWBC_HOST_EMU
constexpr int kWpNT = 1;
#define WP_THR Thr{0}
inline int wp_uni(int v) { return v; }
#else
constexpr int kWpNT = 64;
#define WP_THR Thr{lane}
__device__ __forceinline__ int wp_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }  // (run-time sizes are wave-uniform in the kernels)
#endif

// pinv_cod_small with the scratch its callers give it: three 12 x 12 blocks and 3 x 12 reals.  ip: t = 1..12.  in: 144, the block
// densely (row stride t) in the leading t t words.  out: Out (144: t x t densely, the rest keeps the frame sentinel -- all of it on a
// full-rank verdict), the returned rank, and the 36 words behind vec (must stay NaN)
struct WpPinvCod {
    static constexpr int oM = 0, oO = 144, oQ = 288, oG = 432, oT = 576, oV = 720, oGd = 756, LDS = 792;
    static constexpr int NIN = 144, NIP = 1, NOUT = 144 + 1 + 36;
    static const char *check(const int *ip) { return (ip[0] < 1 || ip[0] > 12) ? "t outside 1..12" : nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int t = wp_uni(ip[0]);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= oO && e < oO + 144) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < 144; e += 64) L[oM + e] = (real_t)in[e];
        }
        WSYNC();
        DWBC_SYNC();
        int rank = -1;
        rank = pinv_cod_small<kWpNT, 12>(WP_THR, L + oM, t, kCodThreshold, L + oO, L + oQ, L + oG, L + oT, L + oV);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < 144; e += 64) out[e] = (double)L[oO + e];
            for (int e = lane; e < 36; e += 64) out[145 + e] = (double)L[oGd + e];
            if (lane == 0) out[144] = rank;
        }
    }
};

// gj_inverse_rows<NMAX>.  ip: n = 1..NMAX, in place (0 / 1).  in: NMAX^2, the matrix densely (row stride n) in the leading n n
// words.  out: the output block (NMAX^2: out of place the frame sentinel behind n n words, in place what the input held), pivot ratio
template <int NMAX>
struct WpGjRows {
    static constexpr int SZ = NMAX * NMAX, oA = 0, oO = wp_ev(SZ), oW = 2 * wp_ev(SZ), LDS = oW + 2 * NMAX + 2;
    static constexpr int NIN = SZ, NIP = 2, NOUT = SZ + 1;
    static const char *check(const int *ip) {
        if (ip[0] < 1 || ip[0] > NMAX) return "n outside 1..NMAX";
        if (ip[1] < 0 || ip[1] > 1) return "in-place flag outside 0..1";
        return nullptr;
    }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int n = wp_uni(ip[0]);
        real_t *Ai = wp_uni(ip[1]) ? L + oA : L + oO;
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= oO && e < oO + SZ) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < SZ; e += 64) L[oA + e] = (real_t)in[e];
        }
        WSYNC();
        DWBC_SYNC();
        const real_t ratio = gj_inverse_rows<NMAX, kWpNT>(WP_THR, L + oA, n, n, Ai, n, L + oW);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < SZ; e += 64) out[e] = (double)Ai[e];
            if (lane == 0) out[SZ] = (double)ratio;
        }
    }
};

// spd_inverse_reg<NN> in place, as the kernel calls it.  LDSFEED: the pivot column through colbuf (sweep_inverse_lds), else the
// v_readlane feed (sweep_inverse_rl).  in: NN x NN.  out: NN x NN, ok
template <int NN, bool LDSFEED>
struct WpSpdReg {
    static constexpr int oC = wp_ev(NN * NN), LDS = oC + 64 + 2;
    static constexpr int NIN = NN * NN, NIP = 1, NOUT = NN * NN + 1;
    static const char *check(const int *) { return nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *, double *out, real_t *L) {
        DWBC_LANE_DECL;
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < NN * NN; e += 64) L[e] = (real_t)in[e];
        }
        WSYNC();
        DWBC_SYNC();
        const int ok = spd_inverse_reg<NN>(L, NN, L, NN, LDSFEED ? L + oC : nullptr);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < NN * NN; e += 64) out[e] = (double)L[e];
            if (lane == 0) out[NN * NN] = ok;
        }
    }
};

// spd_inverse_scaled<12> in place.  ip: n = 1..12.  in: 144, the matrix densely (row stride n) in the leading n n words.  out: 144, ok
struct WpSpdScaled {
    static constexpr int oC = 144, LDS = 144 + 12 + 2;
    static constexpr int NIN = 144, NIP = 1, NOUT = 145;
    static const char *check(const int *ip) { return (ip[0] < 1 || ip[0] > 12) ? "n outside 1..12" : nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int n = wp_uni(ip[0]);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < 144; e += 64) L[e] = (real_t)in[e];
        }
        WSYNC();
        DWBC_SYNC();
        const int ok = spd_inverse_scaled<12>(L, n, n, L, n, L + oC);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < 144; e += 64) out[e] = (double)L[e];
            if (lane == 0) out[144] = ok;
        }
    }
};

// mmg<MAXM, MAXN, MAXK, OP>.  ip: m, kk, n (1 .. the bounds).  in: A then B, each densely in the leading words of its MAXM MAXK /
// MAXK MAXN block (OP 0: A m x kk, B kk x n;  1: A m x kk, B n x kk;  2: A kk x m, B kk x n), NaN behind.  out: the C block
// (MAXM MAXN: m x n densely, the frame sentinel behind)
template <int MAXM, int MAXN, int MAXK, int OP>
struct WpMmg {
    static constexpr int SA = MAXM * MAXK, SB = MAXK * MAXN, SC = MAXM * MAXN;
    static constexpr int oA = 0, oB = wp_ev(SA), oC = oB + wp_ev(SB), LDS = oC + wp_ev(SC);
    static constexpr int NIN = SA + SB, NIP = 3, NOUT = SC;
    static const char *check(const int *ip) {
        if (ip[0] < 1 || ip[0] > MAXM) return "m outside 1..MAXM";
        if (ip[1] < 1 || ip[1] > MAXK) return "kk outside 1..MAXK";
        if (ip[2] < 1 || ip[2] > MAXN) return "n outside 1..MAXN";
        return nullptr;
    }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int m = wp_uni(ip[0]), kk = wp_uni(ip[1]), n = wp_uni(ip[2]);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= oC && e < oC + SC) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < SA; e += 64) L[oA + e] = (real_t)in[e];
            for (int e = lane; e < SB; e += 64) L[oB + e] = (real_t)in[SA + e];
        }
        WSYNC();
        DWBC_SYNC();
        mmg<MAXM, MAXN, MAXK, OP>(L + oC, n, L + oA, OP == 2 ? m : kk, L + oB, OP == 1 ? kk : n, m, kk, n);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < SC; e += 64) out[e] = (double)L[oC + e];
        }
    }
};
// ---- 7. the two in-place matrix-core tiles of the cycle (dwbc_cycle2.h): contact_gram (stage 1 of every cycle kernel, the
// redistribution and the gravity-compensation kernels) and wrench_maps (the cascade).  fp64 only: on the device the fp32 build takes the
// plain loops of the host.  Instantiated in wave_probe_gc.hip.  Every block sits at a 16-byte aligned offset with two NaN words in
// front of it and behind it (and one more where its length is odd); the output block is pre-filled with the frame sentinel.
// out (both families): the wave's WHOLE slice of LDS after the call -- guards, operands as they read back, the output block.

// contact_gram<N, 12, NT, OUT>.  ip: cd (6 or 12).  in: Yt then JCt, each N x 12 (rows of the transposed blocks; the caller keeps the
// entries of the rows >= cd of Y / J_C, i.e. columns >= cd here, zero: the function's contract)
template <int N>
struct WpGram {
    static constexpr int C = 12;
    static constexpr int oY = 2, oJ = oY + N * C + 2, oO = oJ + N * C + 2, LDS = oO + C * C + 2;
    static constexpr int NIN = 2 * N * C, NIP = 1, NOUT = LDS;
    static_assert(oY % 2 == 0 && oJ % 2 == 0 && oO % 2 == 0 && LDS % 2 == 0, "16-byte aligned blocks");
    static const char *check(const int *ip) { return (ip[0] != 6 && ip[0] != 12) ? "cd outside {6, 12}" : nullptr; }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int cd = wp_uni(ip[0]);
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= oO && e < oO + C * C) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            for (int e = lane; e < N * C; e += 64) L[oY + e] = (real_t)in[e], L[oJ + e] = (real_t)in[N * C + e];
        }
        WSYNC();
        DWBC_SYNC();
        contact_gram<N, C, kWpNT, oO>(WP_THR, L + oY, L + oJ, cd, L);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < LDS; e += 64) out[e] = (double)L[e];
        }
    }
};

// wrench_maps<N, NT, Map> with an LDS map of the probe's own: nothing but the members the function reads.
// ip: cd, k ((12, 6) or (6, 0)), n_levels (1..4), t_dof[4] (3 or 6 each; beyond n_levels ignored); 1 + sum t + k <= 31 columns.
// The Setup is built here from ip: n_levels, fstar_off[] and fstar_total, the only members the function reads.
// in: R_0, R_1 (18), JbT (12 x N), tg (M), U (4 levels x M x 6), NwJw (M x 6)
template <int N>
struct WpWrenchMap {
    static constexpr int M = N - 6, T = 6, WLD = 32, C = 12;
    static constexpr int Rc = 2, tg = Rc + 18 + 2, U = tg + wp_ev(M) + 2, NwJw = U + kMaxLevels * M * T + 2;
    static constexpr int JbT = NwJw + M * 6 + 2, wm = JbT + C * N + 2, total = wm + C * WLD + 2;
    static_assert(Rc % 2 == 0 && tg % 2 == 0 && U % 2 == 0 && NwJw % 2 == 0 && JbT % 2 == 0 && wm % 2 == 0 && total % 2 == 0, "16-byte aligned blocks");
};
template <int N>
struct WpWrench {
    using S = WpWrenchMap<N>;
    static constexpr int M = S::M, C = S::C;
    static constexpr int LDS = S::total;
    static constexpr int NIN = 18 + C * N + M + kMaxLevels * M * S::T + M * 6, NIP = 3 + kMaxLevels, NOUT = LDS;
    static const char *check(const int *ip) {
        if (!((ip[0] == 12 && ip[1] == 6) || (ip[0] == 6 && ip[1] == 0))) return "(cd, k) outside {(12, 6), (6, 0)}";
        if (ip[2] < 1 || ip[2] > kMaxLevels) return "n_levels outside 1..4";
        int ftot = 0;
        for (int l = 0; l < ip[2]; l++) {
            if (ip[3 + l] != 3 && ip[3 + l] != 6) return "t_dof outside {3, 6}";
            ftot += ip[3 + l];
        }
        return 1 + ftot + ip[1] > 31 ? "1 + sum t_dof + k outside 1..31" : nullptr;
    }
    DWBC_WDEV static void problem(const double *in, const int *ip, double *out, real_t *L) {
        DWBC_LANE_DECL;
        const int cd = wp_uni(ip[0]), k = wp_uni(ip[1]);
        Setup su;  // (only what wrench_maps reads is set)
        su.n_levels = wp_uni(ip[2]);
        int off = 0;
        for (int l = 0; l < kMaxLevels; l++) {
            su.fstar_off[l] = off;
            off += l < su.n_levels ? wp_uni(ip[3 + l]) : 0;
        }
        su.fstar_total = off;
        LANES {
            for (int e = lane; e < LDS; e += 64) L[e] = (e >= S::wm && e < S::wm + C * S::WLD) ? (real_t)kWpSentinel : WP_NAN;
        }
        WSYNC();
        LANES {
            const double *p = in;
            for (int e = lane; e < 18; e += 64) L[S::Rc + e] = (real_t)p[e];
            p += 18;
            for (int e = lane; e < C * N; e += 64) L[S::JbT + e] = (real_t)p[e];
            p += C * N;
            for (int e = lane; e < M; e += 64) L[S::tg + e] = (real_t)p[e];
            p += M;
            for (int e = lane; e < kMaxLevels * M * S::T; e += 64) L[S::U + e] = (real_t)p[e];
            p += kMaxLevels * M * S::T;
            for (int e = lane; e < M * 6; e += 64) L[S::NwJw + e] = (real_t)p[e];
        }
        WSYNC();
        DWBC_SYNC();
        wrench_maps<N, kWpNT, S>(WP_THR, su, L, L + S::JbT, cd, k, L + S::wm);
        DWBC_SYNC();
        WSYNC();
        LANES {
            for (int e = lane; e < LDS; e += 64) out[e] = (double)L[e];
        }
    }
};
#endif  // !WAVE_PROBE_F32

#ifndef DWBC_HOST_EMU
template <class F>
__global__ __launch_bounds__(128) void wp_kernel(const WpArgs a) {
    __shared__ __attribute__((aligned(16))) real_t Ls[2 * F::LDS];
    static_assert(F::LDS % 2 == 0 && 2 * F::LDS * sizeof(real_t) <= 60000, "wave slices of LDS");
    const int wave = (int)(threadIdx.x >> 6);
    const int b = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (b >= a.B) return;  // (the whole wave: the routines hold no block-wide barrier)
    F::problem(a.in + (size_t)b * F::NIN, a.ip + (size_t)b * F::NIP, a.out + (size_t)b * F::NOUT, Ls + wave * F::LDS);
}
#endif

// runs the batch; nullptr or the error text.  The caller (wave_probe.hip) has checked every size; on the device `a` holds device pointers
template <class F>
static const char *wp_run(const WpArgs &a, int threads) {
#ifdef DWBC_HOST_EMU
    (void)threads;
    static real_t L[F::LDS];
    for (int b = 0; b < a.B; b++) F::problem(a.in + (size_t)b * F::NIN, a.ip + (size_t)b * F::NIP, a.out + (size_t)b * F::NOUT, L);
    return nullptr;
#else
    const int per = threads / 64;
    hipLaunchKernelGGL((wp_kernel<F>), dim3((a.B + per - 1) / per), dim3(threads), 0, 0, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
#endif
}

}  // namespace dwbc
