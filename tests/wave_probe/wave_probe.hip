// wave_probe.hip -- TEST HARNESS ONLY: the C entries of the wave-routine probe (wave_probe_body.h) and its fp64 instantiations.
//   hipcc --offload-arch=gfx950            -> libdwbc_wave_probe.so      (device: allocates, copies, launches, synchronises, copies back)
//   g++ -x c++ -DDWBC_HOST_EMU             -> libdwbc_wave_probe_emu.so  (host emulation of the same text)
// The 39- and 33-wide sweeps are instantiated in wave_probe_sweeps.hip (they are most of the compile time), the routines of the
// general-contact kernel in wave_probe_gc.hip, the fp32 forms in wave_probe_f32.hip.  The instantiation table below is what tests/wave_probe/probe.py looks its names up in.
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "wave_probe_body.h"

using namespace dwbc;

extern "C" const char *wave_probe_run_f32(int which, const void *args, int threads);     // wave_probe_f32.hip: 0 lanes, 1 math
extern "C" const char *wave_probe_run_sweep(int kind, const void *args, int threads);    // wave_probe_sweeps.hip
extern "C" const char *wave_probe_run_gc(int kind, const void *args, int threads);       // wave_probe_gc.hip

namespace {

enum Family { kLanes = 1, kMath, kGemm, kInverse, kRows };

struct Inst {
    const char *name;
    int family, nin, nip, nout;
    const char *(*check)(const int *);
    const char *(*run)(const WpArgs &, int);
};
template <int W>
const char *run_f32(const WpArgs &a, int threads) { return wave_probe_run_f32(W, &a, threads); }
template <int K>
const char *run_sweep(const WpArgs &a, int threads) { return wave_probe_run_sweep(K, &a, threads); }
template <int K>
const char *run_gc(const WpArgs &a, int threads) { return wave_probe_run_gc(K, &a, threads); }
const char *no_check(const int *) { return nullptr; }

#define WP_INST(name, fam, ...) Inst{name, fam, __VA_ARGS__::NIN, __VA_ARGS__::NIP, __VA_ARGS__::NOUT, &__VA_ARGS__::check, &wp_run<__VA_ARGS__>}
#define WP_GEMM(MR, NCV, KV) \
    WP_INST("gemm_" #MR "_" #NCV "_" #KV, kGemm, WpGemm<MR, NCV, KV, false, false>), WP_INST("gemm_" #MR "_" #NCV "_" #KV "_fc", kGemm, WpGemm<MR, NCV, KV, true, false>)
#define WP_SWEEP(name, K) Inst{name, kInverse, WpSweep<K>::NIN, WpSweep<K>::NIP, WpSweep<K>::NOUT, &no_check, &run_sweep<K>}
#define WP_GC(name, fam, K, ...) Inst{name, fam, __VA_ARGS__::NIN, __VA_ARGS__::NIP, __VA_ARGS__::NOUT, &__VA_ARGS__::check, &run_gc<K>}
const Inst kInst[] = {
    WP_INST("lanes", kLanes, WpLanes),
    Inst{"lanes_f32", kLanes, WpLanes::NIN, WpLanes::NIP, WpLanes::NOUT, &WpLanes::check, &run_f32<0>},
    WP_INST("math", kMath, WpMath),
    Inst{"math_f32", kMath, WpMath::NIN, WpMath::NIP, WpMath::NOUT, &WpMath::check, &run_f32<1>},
    WP_GEMM(16, 16, 4), WP_GEMM(17, 15, 5), WP_GEMM(1, 1, 1), WP_GEMM(12, 12, 39), WP_GEMM(33, 6, 12), WP_GEMM(6, 9, 33),
    WP_GEMM(39, 16, 12), WP_GEMM(39, 7, 18),
    WP_INST("gemm_12_12_39_fc_over", kGemm, WpGemm<12, 12, 39, true, true>),
    // the shapes the kernels use: V_b^T g (dwbc_cycle2.h), the 33-wide row with an odd count in an even stride, Lambda_c Y and
    // s -= Y^T Jbar^T (dwbc_cycle2_stage1.inc / dwbc_cycle2p.h), Lambda_c y through the plain loads (dwbc_redistribute.h), a slice
    WP_INST("dot_33_6_6_3_0", kRows, WpRowsDot<33, 6, 6, 3, 0, true, 0, 33>),
    WP_INST("dot_1_33_34_1_0", kRows, WpRowsDot<1, 33, 34, 1, 0, true, 0, 1>),
    WP_INST("dot_12_12_12_4_0", kRows, WpRowsDot<12, 12, 12, 4, 0, true, 0, 12>),
    WP_INST("dot_39_12_12_2_1", kRows, WpRowsDot<39, 12, 12, 2, 1, true, 0, 39>),
    WP_INST("dot_6_33_34_3_0_off6_no14", kRows, WpRowsDot<6, 33, 34, 3, 0, true, 6, 14>),
    WP_INST("dot_12_12_12_4_0_unaligned", kRows, WpRowsDot<12, 12, 12, 4, 0, false, 0, 12>),
    WP_INST("axpy_6_14_14_3", kRows, WpRowsAxpy<6, 14, 14, 3, true>),
    WP_INST("axpy_6_8_8_3", kRows, WpRowsAxpy<6, 8, 8, 3, true>),
    WP_SWEEP("sweep_tree39", 0), WP_SWEEP("sweep_tree_lds39", 1), WP_SWEEP("sweep_tree_lds_multi39", 2), WP_SWEEP("sweep_dense33", 3),
    WP_SWEEP("sweep_lds33", 4),
    WP_INST("spd_small", kInverse, WpSmall<0>), WP_INST("spd12_lds", kInverse, WpSmall<1>), WP_INST("spd12_lds_inplace", kInverse, WpSmall<2>),
    WP_INST("chol6", kInverse, WpSmall<3>), WP_INST("chol6_x3", kInverse, WpChol3),
    // the general-contact kernel's routines (K: the case of wave_probe_run_gc), mmg at the bounds of the TG = 12 build
    WP_GC("pinv_cod12", kInverse, 0, WpPinvCod),
    WP_GC("gj_rows6", kInverse, 1, WpGjRows<6>), WP_GC("gj_rows12", kInverse, 2, WpGjRows<12>), WP_GC("gj_rows18", kInverse, 3, WpGjRows<18>),
    WP_GC("spd_reg39_lds", kInverse, 4, WpSpdReg<39, true>), WP_GC("spd_reg33_lds", kInverse, 5, WpSpdReg<33, true>),
    WP_GC("spd_reg33_rl", kInverse, 6, WpSpdReg<33, false>), WP_GC("spd_scaled12", kInverse, 7, WpSpdScaled),
    WP_GC("mmg_12_39_39_nn", kGemm, 8, WpMmg<12, 39, 39, 0>), WP_GC("mmg_12_12_39_nt", kGemm, 9, WpMmg<12, 12, 39, 1>),
    WP_GC("mmg_33_12_12_tn", kGemm, 10, WpMmg<33, 12, 12, 2>), WP_GC("mmg_12_33_12_nn", kGemm, 11, WpMmg<12, 33, 12, 0>),
    // the two in-place matrix-core tiles of the cycle at the built-in size, two pack sizes, a size without K padding and the largest model
    WP_GC("gram_39", kGemm, 12, WpGram<39>), WP_GC("gram_37", kGemm, 13, WpGram<37>), WP_GC("gram_23", kGemm, 14, WpGram<23>),
    WP_GC("gram_24", kGemm, 15, WpGram<24>), WP_GC("gram_50", kGemm, 16, WpGram<50>),
    WP_GC("wrench_39", kGemm, 17, WpWrench<39>), WP_GC("wrench_37", kGemm, 18, WpWrench<37>), WP_GC("wrench_23", kGemm, 19, WpWrench<23>),
    WP_GC("wrench_24", kGemm, 20, WpWrench<24>), WP_GC("wrench_50", kGemm, 21, WpWrench<50>),
};
constexpr int kNInst = (int)(sizeof(kInst) / sizeof(kInst[0]));
constexpr int kMaxB = 512;

thread_local char g_err[256];
int fail(const char *fmt, long a = 0, long b = 0, long c = 0) {
    snprintf(g_err, sizeof(g_err), fmt, a, b, c);
    return 0;
}

#ifndef DWBC_HOST_EMU
// device copies of the records of one call, freed on every path
struct DevBufs {
    void *p[3] = {nullptr, nullptr, nullptr};
    ~DevBufs() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
};
#endif

// 1: run, outputs written.  0: nothing was run or the run failed; wave_probe_error() says why.  n_in, n_ip, n_out: the lengths of the
// caller's arrays, which must be B times the instantiation's record sizes; `out` arrives pre-filled with the caller's sentinel
int run_inst(int family, int inst, int threads, int B, const double *in, long n_in, const int *ip, long n_ip, double *out, long n_out) {
    g_err[0] = 0;
    if (inst < 0 || inst >= kNInst) return fail("instantiation %ld out of range", inst);
    const Inst &I = kInst[inst];
    if (I.family != family) return fail("instantiation %ld belongs to family %ld, not %ld", inst, I.family, family);
    if (threads != 64 && threads != 128) return fail("threads per block %ld: 64 or 128", threads);
    if (B < 1 || B > kMaxB) return fail("batch %ld outside 1..%ld", B, kMaxB);
    if (!in || !ip || !out) return fail("null record");
    if (n_in != (long)B * I.nin) return fail("input record: %ld doubles, the instantiation takes %ld per problem", n_in, I.nin);
    if (n_ip != (long)B * I.nip) return fail("parameter record: %ld ints, the instantiation takes %ld per problem", n_ip, I.nip);
    if (n_out != (long)B * I.nout) return fail("output record: %ld doubles, the instantiation writes %ld per problem", n_out, I.nout);
    for (int b = 0; b < B; b++) {
        const char *e = I.check(ip + (size_t)b * I.nip);
        if (e) {
            snprintf(g_err, sizeof(g_err), "problem %d: %s", b, e);
            return 0;
        }
    }
    WpArgs a{};
    a.B = B;
#ifdef DWBC_HOST_EMU
    a.in = in, a.ip = ip, a.out = out;
    const char *e = I.run(a, threads);
    if (e) {
        snprintf(g_err, sizeof(g_err), "%s", e);
        return 0;
    }
    return 1;
#else
    DevBufs d;
    const void *src[3] = {in, ip, out};
    const size_t bytes[3] = {(size_t)n_in * sizeof(double), (size_t)n_ip * sizeof(int), (size_t)n_out * sizeof(double)};
#define WP_HIP(call)                                                                       \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                            \
            snprintf(g_err, sizeof(g_err), "%s: %s", #call, hipGetErrorString(e_));        \
            return 0;                                                                      \
        }                                                                                  \
    } while (0)
    for (int i = 0; i < 3; i++) {
        WP_HIP(hipMalloc(&d.p[i], bytes[i]));
        WP_HIP(hipMemcpy(d.p[i], src[i], bytes[i], hipMemcpyHostToDevice));  // (the outputs too: what nobody writes keeps the sentinel)
    }
    a.in = (const double *)d.p[0], a.ip = (const int *)d.p[1], a.out = (double *)d.p[2];
    const char *e = I.run(a, threads);
    if (e) {
        snprintf(g_err, sizeof(g_err), "kernel: %s", e);
        return 0;
    }
    WP_HIP(hipMemcpy(out, d.p[2], bytes[2], hipMemcpyDeviceToHost));
#undef WP_HIP
    return 1;
#endif
}

}  // namespace

extern "C" {

int wave_probe_inst_count() { return kNInst; }
const char *wave_probe_inst_name(int inst) { return (inst >= 0 && inst < kNInst) ? kInst[inst].name : nullptr; }
// info: family, doubles in, ints in, doubles out (per problem)
int wave_probe_inst_info(int inst, int *info) {
    if (inst < 0 || inst >= kNInst) return fail("instantiation %ld out of range", inst);
    info[0] = kInst[inst].family, info[1] = kInst[inst].nin, info[2] = kInst[inst].nip, info[3] = kInst[inst].nout;
    return 1;
}
const char *wave_probe_error() { return g_err; }

// one entry per routine family (each takes the instantiations of its own family only)
#define WP_ENTRY(name, fam)                                                                                                              \
    int name(int inst, int threads, int B, const double *in, long n_in, const int *ip, long n_ip, double *out, long n_out) {             \
        return run_inst(fam, inst, threads, B, in, n_in, ip, n_ip, out, n_out);                                                          \
    }
WP_ENTRY(wave_probe_lanes, kLanes)
WP_ENTRY(wave_probe_math, kMath)
WP_ENTRY(wave_probe_gemm, kGemm)
WP_ENTRY(wave_probe_inverse, kInverse)
WP_ENTRY(wave_probe_rows, kRows)

}  // extern "C"
