// qp_probe.hip -- TEST HARNESS ONLY: the C entry of the wave-QP probe (qp_probe_body.h) and its fp64 instantiations.
//   hipcc --offload-arch=gfx950            -> libdwbc_qp_probe.so      (device: allocates, copies, launches, synchronises, copies back)
//   g++ -x c++ -DDWBC_HOST_EMU             -> libdwbc_qp_probe_emu.so  (host emulation of the same text)
// The instantiations (WS, NV, QN, KCV) are the ones the product instantiates: dwbc_cycle.h / dwbc_cycle2p.h (6, 9 and 12 variables,
// with and without the working-set report), dwbc_cycle_gc.h (18 variables with three contacts, 24 with the 12-dof task block) and the
// fp32 translation unit (qp_probe_f32.hip).
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "qp_probe_body.h"

using namespace dwbc;

extern "C" double qp_probe_scale_f32();
extern "C" const char *qp_probe_run_f32(const void *args, int threads);  // qp_probe_f32.hip: (1, 12, 12, 6) in float; args: its own QpProbeArgs (same layout)

namespace {

struct Inst {
    int ws, nv, qn, kcv, f32;
    const char *(*run)(const QpProbeArgs &, int);
};
const char *run_f32(const QpProbeArgs &a, int threads) { return qp_probe_run_f32(&a, threads); }
#define QP_PROBE_INST(WS, NV, QN, KCV) Inst{WS, NV, QN, KCV, 0, &qp_probe_run<WS, NV, QN, KCV>}
const Inst kInst[] = {
    QP_PROBE_INST(0, 6, 12, 6),  QP_PROBE_INST(1, 6, 12, 6),  QP_PROBE_INST(0, 9, 12, 6),   QP_PROBE_INST(1, 9, 12, 6),
    QP_PROBE_INST(0, 12, 12, 6), QP_PROBE_INST(1, 12, 12, 6), QP_PROBE_INST(1, 18, 18, 12), QP_PROBE_INST(1, 24, 24, 12),
    Inst{1, 12, 12, 6, 1, &run_f32},
};
constexpr int kNInst = (int)(sizeof(kInst) / sizeof(kInst[0]));
constexpr int kMaxB = 1024, kMaxIter = 2000;

thread_local char g_err[256];
int fail(const char *fmt, int a = 0, int b = 0, int c = 0) {
    snprintf(g_err, sizeof(g_err), fmt, a, b, c);
    return 0;
}

#ifndef DWBC_HOST_EMU
// device copies of the records of one call, freed on every path
struct DevBufs {
    void *p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~DevBufs() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
};
#endif

}  // namespace

extern "C" {

int qp_probe_inst_count() { return kNInst; }

// info: ws, nv, qn, kcv, f32
int qp_probe_inst_info(int inst, int *info) {
    if (inst < 0 || inst >= kNInst) return fail("instantiation %d out of range", inst);
    const Inst &I = kInst[inst];
    info[0] = I.ws, info[1] = I.nv, info[2] = I.qn, info[3] = I.kcv, info[4] = I.f32;
    return 1;
}

// kQpScaleGI of the instantiation's arithmetic type: the factor the probe puts on the contact columns (the references must use the same)
double qp_probe_inst_scale(int inst) { return (inst >= 0 && inst < kNInst && kInst[inst].f32) ? qp_probe_scale_f32() : (double)kQpScaleGI; }

const char *qp_probe_error() { return g_err; }

// 1: solved, outputs written.  0: nothing was run or the run failed; qp_probe_error() says why.
int qp_probe_solve(int inst, int threads, int B, const double *rows, const int *ids, const int *par, const double *vtol, const int *warm, int *oi, double *od) {
    g_err[0] = 0;
    if (inst < 0 || inst >= kNInst) return fail("instantiation %d out of range", inst);
    const Inst &I = kInst[inst];
    if (threads != 64 && threads != 128) return fail("threads per block %d: 64 or 128", threads);
    if (B < 1 || B > kMaxB) return fail("batch %d outside 1..%d", B, kMaxB);
    if (!rows || !ids || !par || !vtol || !oi || !od) return fail("null record");
    for (int b = 0; b < B; b++) {
        const int nv = par[4 * b], t = par[4 * b + 1], mi = par[4 * b + 2], hw = par[4 * b + 3];
        if (nv < 1 || nv > I.nv) return fail("problem %d: nv %d outside 1..%d", b, nv, I.nv);
        if (t < 0 || t > nv) return fail("problem %d: t %d outside 0..%d", b, t, nv);
        if (mi < 1 || mi > kMaxIter) return fail("problem %d: max_iter %d outside 1..%d", b, mi, kMaxIter);
        if (!(vtol[b] >= 0.0) || !isfinite(vtol[b])) return fail("problem %d: vtol", b);
        if (hw && (!I.ws || !warm)) return fail("problem %d: warm start needs WS = 1 and the warm record", b);
        // WS = 0: the lexicographic solve reads the contact block at its standard positions whatever (t, k) is
        const int k = nv - t;
        // the lexicographic solve (t > 0 and k > 0) holds KCV contact-null variables at the most
        if (t > 0 && k > I.kcv) return fail("problem %d: k %d contact-null variables, the instantiation holds %d", b, k, I.kcv);
        if (!I.ws && !(t == 0 || k == 0 || (t == I.nv - I.kcv && k == I.kcv)))
            return fail("problem %d: WS = 0 solves the standard layout only (t %d, k %d)", b, t, k);
    }
    const size_t n_rows = (size_t)B * 64 * (I.qn + 2), n_ids = (size_t)B * 64 * 2, n_par = (size_t)B * 4, n_warm = (size_t)B * I.qn;
    const size_t n_oi = (size_t)B * (4 + I.qn), n_od = (size_t)B * (1 + I.qn + 64);
    QpProbeArgs a{};
    a.B = B;
#ifdef DWBC_HOST_EMU
    a.rows = rows, a.ids = ids, a.par = par, a.vtol = vtol, a.warm = warm, a.oi = oi, a.od = od;
    const char *e = I.run(a, threads);
    if (e) {
        snprintf(g_err, sizeof(g_err), "%s", e);
        return 0;
    }
    return 1;
#else
    DevBufs d;
    const void *src[5] = {rows, ids, par, vtol, warm};
    const size_t bytes[7] = {n_rows * sizeof(double), n_ids * sizeof(int), n_par * sizeof(int), (size_t)B * sizeof(double), n_warm * sizeof(int),
                             n_oi * sizeof(int), n_od * sizeof(double)};
#define QP_PROBE_HIP(call)                                                                 \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                            \
            snprintf(g_err, sizeof(g_err), "%s: %s", #call, hipGetErrorString(e_));        \
            return 0;                                                                      \
        }                                                                                  \
    } while (0)
    for (int i = 0; i < 7; i++) {
        if (i == 4 && !warm) continue;
        QP_PROBE_HIP(hipMalloc(&d.p[i], bytes[i]));
        if (i < 5) QP_PROBE_HIP(hipMemcpy(d.p[i], src[i], bytes[i], hipMemcpyHostToDevice));
        else QP_PROBE_HIP(hipMemset(d.p[i], 0xff, bytes[i]));  // (an output nobody writes reads as -1 / NaN)
    }
    a.rows = (const double *)d.p[0], a.ids = (const int *)d.p[1], a.par = (const int *)d.p[2], a.vtol = (const double *)d.p[3];
    a.warm = (const int *)d.p[4], a.oi = (int *)d.p[5], a.od = (double *)d.p[6];
    const char *e = I.run(a, threads);
    if (e) {
        snprintf(g_err, sizeof(g_err), "kernel: %s", e);
        return 0;
    }
    QP_PROBE_HIP(hipMemcpy(oi, d.p[5], bytes[5], hipMemcpyDeviceToHost));
    QP_PROBE_HIP(hipMemcpy(od, d.p[6], bytes[6], hipMemcpyDeviceToHost));
#undef QP_PROBE_HIP
    return 1;
#endif
}

}  // extern "C"
