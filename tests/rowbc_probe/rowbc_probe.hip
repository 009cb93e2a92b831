// rowbc_probe.hip -- TEST HARNESS ONLY: the row-broadcast primitives of dwbc_wave.h (ROWBC_FMA, ROWBC_DOT, ROW_REPLICATE) and the
// 12-pivot sweep built on them (rowbc_pivot12 inside spd_inverse12_lds, dwbc_cycle2p.h) alone, on operands of the caller's choosing.
//   hipcc --offload-arch=gfx950            -> libdwbc_rowbc_probe.so      (device: one wavefront per problem, 64 or 128 threads per block)
//   g++ -x c++ -DDWBC_HOST_EMU             -> libdwbc_rowbc_probe_emu.so  (host emulation of the same text; kinds 0 - 4)
// The probe includes the shipped headers and calls the shipped macros and functions.  The one thing it keeps a copy of is what the
// product no longer has: the body of spd_inverse12_lds with the pivot column fed through LDS (the shipped lds_pivot<12, 11, 0> of
// dwbc_cycle2.h), the form the row-broadcast sweep must reproduce bit for bit.
// Kinds (doubles in / out per problem):
//   0  replicate   in x[64]                        out x[64] after ROW_REPLICATE
//   1  fma         in x[64] y[64] acc[64]          out 16 x 64: for J = 0..15 the accumulator after ROWBC_FMA(J, acc, x, y)
//   2, 3, 4  dz    in g[64][12] m[64]              out dz[64] by row broadcast (copy of m, replicate, ROWBC_DOT over NV = 6, 9, 12),
//                                                      dz[64] with z read out by BCAST into uniform values, `s_ += g[j] * zu[j]` (the
//                                                      v_readlane form of the solver: the device compiler contracts it to the same FMAs)
//   5  sweep       in A[12][12]                    out Lambda[12][12], ok by spd_inverse12_lds; the same by the LDS-fed copy  (device only)
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../libdwbc_amd/csrc/dwbc_cycle2p.h"

using namespace dwbc;

namespace {

constexpr int kNIn[6] = {64, 192, 832, 832, 832, 144};
constexpr int kNOut[6] = {64, 1024, 128, 128, 128, 290};
constexpr int kLds = 304;  // per wave: two 12 x 12 blocks, 12 scale factors, padded to a 16-byte multiple
constexpr int kMaxB = 512;

struct RbArgs {
    int B;
    const double *in;
    double *out;
};

DWBC_WDEV void rb_replicate(const double *in, double *out) {
    DWBC_LANE_DECL;
    PL(real_t, x);
    LANES { LV(x) = in[lane]; }
    ROW_REPLICATE(x);
    LANES { out[lane] = LV(x); }
}

DWBC_WDEV void rb_fma(const double *in, double *out) {
    DWBC_LANE_DECL;
    PL(real_t, x);
    PL(real_t, y);
    PL(real_t, a0);
    PL(real_t, a);
    LANES { LV(x) = in[lane], LV(y) = in[64 + lane], LV(a0) = in[128 + lane]; }
#define RB_ONE(J)                                  \
    LANES { LV(a) = LV(a0); }                      \
    ROWBC_FMA(J, a, x, y);                         \
    LANES { out[(J) * 64 + lane] = LV(a); }
    RB_ONE(0) RB_ONE(1) RB_ONE(2) RB_ONE(3) RB_ONE(4) RB_ONE(5) RB_ONE(6) RB_ONE(7)
    RB_ONE(8) RB_ONE(9) RB_ONE(10) RB_ONE(11) RB_ONE(12) RB_ONE(13) RB_ONE(14) RB_ONE(15)
#undef RB_ONE
}

// the dz product of qp_solve_wave (dwbc_qp_wave.h): z = m of lanes 0..NV-1, every lane's own row g
template <int NV>
DWBC_WDEV void rb_dz(const double *in, double *out) {
    DWBC_LANE_DECL;
    PLA(real_t, g, 12);
    PL(real_t, m);
    PL(real_t, mz);
    PL(real_t, dz);
    PL(real_t, dr);
    LANES {
#pragma unroll
        for (int j = 0; j < 12; j++) LV(g)[j] = in[lane * 12 + j];
        LV(m) = in[768 + lane];
    }
    LANES { LV(mz) = LV(m); LV(dz) = real_t(0.0); }
    ROW_REPLICATE(mz);
    ROWBC_DOT(NV, dz, mz, g);
    real_t zu[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) zu[i] = BCAST(m, i);
    LANES {
        real_t s_ = real_t(0.0);
#pragma unroll
        for (int j = 0; j < NV; j++) s_ += LV(g)[j] * zu[j];
        LV(dr) = s_;
    }
    LANES { out[lane] = LV(dz), out[64 + lane] = LV(dr); }
}

#ifndef DWBC_HOST_EMU
// spd_inverse12_lds as it was with the pivot column fed through LDS: the matrix block is the column buffer during the sweep
__device__ __forceinline__ int spd_inverse12_ldsfed(double *Mx, double *Out, double *scl) {
    const int lane = (int)(threadIdx.x & 63u);
    DWBC_SYNC();
    double s[12], dg, dsc;
    {
        const int col = lane < 12 ? lane : 0;
        const double a = Mx[col * 12 + col];
        int e2 = 0;
        (void)frexp(a > 0.0 ? a : 1.0, &e2);
        dsc = (lane < 12 && a > 0.0) ? ldexp(1.0, -(e2 >> 1)) : 1.0;
        if (lane < 12) scl[lane] = dsc;
    }
    DWBC_SYNC();
    {
        const int col = lane < 12 ? lane : 0;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const double v_ = Mx[i * 12 + col] * scl[i] * dsc;
            s[i] = lane < 12 ? v_ : 0.0;
        }
        const double d_ = Mx[col * 12 + col] * dsc * dsc;
        dg = lane < 12 ? d_ : 1.0;
    }
    DWBC_SYNC();
    int ok = 1;
    {
        DWBC_LANE_OPAQUE(lp);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = (i == lp) ? dg - 1.0 : s[i];
    }
    double dg2 = dg - 2.0;
    lds_pivot<12, 11, 0>(s, dg2, ok, (unsigned)(size_t)Mx, lane);
    ok = DWBC_FLAG_UNIFORM(ok);
    DWBC_SYNC();
    if (lane < 12) {
        DWBC_LANE_OPAQUE(le);
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const double v_ = (i == le) ? -dg2 : -s[i];
            Out[i * 12 + lane] = v_ * scl[i] * dsc;
        }
    }
    DWBC_SYNC();
    return ok;
}

__device__ __forceinline__ void rb_sweep(const double *in, double *out, double *L) {
    const int lane = (int)(threadIdx.x & 63u);
    double *Mx = L, *Out = L + 144, *scl = L + 288;
    for (int pass = 0; pass < 2; pass++) {
        for (int e = lane; e < 144; e += 64) Mx[e] = in[e], Out[e] = -7777.0;
        DWBC_SYNC();
        const int ok = pass == 0 ? spd_inverse12_lds(Mx, Out, scl) : spd_inverse12_ldsfed(Mx, Out, scl);
        DWBC_SYNC();
        for (int e = lane; e < 144; e += 64) out[pass * 145 + e] = Out[e];
        if (lane == 0) out[pass * 145 + 144] = ok;
        DWBC_SYNC();
    }
}

template <int KIND>
__global__ __launch_bounds__(128) void rowbc_probe_kernel(RbArgs a) {
    __shared__ double lds[2][kLds];
    const int w = (int)(threadIdx.x >> 6);
    const int b = (int)blockIdx.x * (int)(blockDim.x >> 6) + w;
    if (b >= a.B) return;  // (whole waves: the routines below run convergent)
    const double *in = a.in + (size_t)b * kNIn[KIND];
    double *out = a.out + (size_t)b * kNOut[KIND];
    if constexpr (KIND == 0) rb_replicate(in, out);
    if constexpr (KIND == 1) rb_fma(in, out);
    if constexpr (KIND == 2) rb_dz<6>(in, out);
    if constexpr (KIND == 3) rb_dz<9>(in, out);
    if constexpr (KIND == 4) rb_dz<12>(in, out);
    if constexpr (KIND == 5) rb_sweep(in, out, lds[w]);
}
#endif

thread_local char g_err[256];
int fail(const char *fmt, long a = 0, long b = 0) {
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return 0;
}

}  // namespace

extern "C" {

const char *rowbc_probe_error() { return g_err; }

// 1: run, outputs written.  0: nothing was run or the run failed; rowbc_probe_error() says why.
int rowbc_probe_run(int kind, int threads, int B, const double *in, long n_in, double *out, long n_out) {
    g_err[0] = 0;
    if (kind < 0 || kind > 5) return fail("kind %ld outside 0..5", kind);
    if (threads != 64 && threads != 128) return fail("threads per block %ld: 64 or 128", threads);
    if (B < 1 || B > kMaxB) return fail("batch %ld outside 1..%ld", B, kMaxB);
    if (!in || !out) return fail("null record");
    if (n_in != (long)B * kNIn[kind]) return fail("input record: %ld doubles, the kind takes %ld per problem", n_in, kNIn[kind]);
    if (n_out != (long)B * kNOut[kind]) return fail("output record: %ld doubles, the kind writes %ld per problem", n_out, kNOut[kind]);
#ifdef DWBC_HOST_EMU
    if (kind == 5) return fail("the 12-pivot sweep is device text: the host emulation of spd_inverse12_lds is spd_inverse_small");
    for (int b = 0; b < B; b++) {
        const double *pi = in + (size_t)b * kNIn[kind];
        double *po = out + (size_t)b * kNOut[kind];
        if (kind == 0) rb_replicate(pi, po);
        else if (kind == 1) rb_fma(pi, po);
        else if (kind == 2) rb_dz<6>(pi, po);
        else if (kind == 3) rb_dz<9>(pi, po);
        else rb_dz<12>(pi, po);
    }
    return 1;
#else
#define RB_HIP(call)                                                                       \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                            \
            snprintf(g_err, sizeof(g_err), "%s: %s", #call, hipGetErrorString(e_));        \
            if (din) (void)hipFree(din);                                                   \
            if (dout) (void)hipFree(dout);                                                 \
            return 0;                                                                      \
        }                                                                                  \
    } while (0)
    double *din = nullptr, *dout = nullptr;
    RB_HIP(hipMalloc(&din, (size_t)n_in * sizeof(double)));
    RB_HIP(hipMalloc(&dout, (size_t)n_out * sizeof(double)));
    RB_HIP(hipMemcpy(din, in, (size_t)n_in * sizeof(double), hipMemcpyHostToDevice));
    RB_HIP(hipMemcpy(dout, out, (size_t)n_out * sizeof(double), hipMemcpyHostToDevice));  // (what nobody writes keeps the caller's fill)
    RbArgs a{B, din, dout};
    const int wpb = threads / 64, grid = (B + wpb - 1) / wpb;
    switch (kind) {
        case 0: rowbc_probe_kernel<0><<<grid, threads>>>(a); break;
        case 1: rowbc_probe_kernel<1><<<grid, threads>>>(a); break;
        case 2: rowbc_probe_kernel<2><<<grid, threads>>>(a); break;
        case 3: rowbc_probe_kernel<3><<<grid, threads>>>(a); break;
        case 4: rowbc_probe_kernel<4><<<grid, threads>>>(a); break;
        default: rowbc_probe_kernel<5><<<grid, threads>>>(a); break;
    }
    RB_HIP(hipGetLastError());
    RB_HIP(hipDeviceSynchronize());
    RB_HIP(hipMemcpy(out, dout, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(din);
    (void)hipFree(dout);
#undef RB_HIP
    return 1;
#endif
}

}  // extern "C"
