// qp_probe_body.h -- TEST HARNESS ONLY.  Runs the shipped text of qp_solve_wave (libdwbc_amd/csrc/dwbc_qp_wave.h) on rows of the
// caller's own choosing: one function template, compiled for the device (qp_probe.hip -> libdwbc_qp_probe.so, one wavefront per
// problem) and for the host (the same files with DWBC_HOST_EMU -> libdwbc_qp_probe_emu.so, the lanes of a wave run in turn).
// Nothing of it is linked into libdwbc_hip.so.  Included once per arithmetic type: qp_probe.hip (double) and qp_probe_f32.hip
// (DWBC_REAL = float, namespace renamed as the library's fp32 translation unit does).
//
// Records (every array is the caller's, in host memory; doubles at the boundary in both arithmetic types):
//   rows  B x 64 x (QN + 2)   per lane  g[QN] (as given: the probe multiplies the contact columns j >= t by kQpScaleGI, as
//                             qp_rows_and_solve does), hi, lo   (+inf: side absent)
//   ids   B x 64 x 2          id_hi, id_lo
//   par   B x 4               nv, t, max_iter, has_warm
//   vtol  B
//   warm  B x QN              ids of a previous working set, -1 = empty (read where has_warm; WS = 1 only)
//   oi    B x (4 + QN)        status, iters, nact, 0, act[QN]
//   od    B x (1 + QN + 64)   viol, x[QN], sfin of the 64 lanes
#pragma once
#include <limits>

#include "../../libdwbc_amd/csrc/dwbc_cycle.h"

namespace dwbc {

struct QpProbeArgs {
    int B;
    const double *rows;
    const int *ids, *par;
    const double *vtol;
    const int *warm;
    int *oi;
    double *od;
};

// problem b on the LDS scratch V (QN reals of this wave's own)
template <int WS, int NV, int QN, int KCV>
DWBC_WDEV void qp_probe_problem(const QpProbeArgs &a, int b, real_t *V) {
    DWBC_LANE_DECL;
    const int nv = a.par[4 * b + 0], t = a.par[4 * b + 1], max_iter = a.par[4 * b + 2], has_warm = a.par[4 * b + 3];
    const real_t vtol = (real_t)a.vtol[b];
    QpRowsT<QN> R;
    QpResultT<QN> out;
    PL(real_t, sfin);
    LANES {
        const double *rec = a.rows + ((size_t)b * 64 + lane) * (QN + 2);
#pragma unroll
        for (int j = 0; j < QN; j++) LV(R.g)[j] = (real_t)rec[j] * (j >= t ? kQpScaleGI : real_t(1.0));
        LV(R.hi) = rec[QN] >= (double)DWBC_QP_INF ? DWBC_QP_INF : (real_t)rec[QN];
        LV(R.lo) = rec[QN + 1] >= (double)DWBC_QP_INF ? DWBC_QP_INF : (real_t)rec[QN + 1];
        LV(R.id_hi) = a.ids[((size_t)b * 64 + lane) * 2 + 0];
        LV(R.id_lo) = a.ids[((size_t)b * 64 + lane) * 2 + 1];
        LV(sfin) = std::numeric_limits<real_t>::quiet_NaN();
        if (lane < QN) V[lane] = std::numeric_limits<real_t>::quiet_NaN();  // a read of scratch nobody wrote shows up
    }
    WSYNC();
    int warm[QN];
#pragma unroll
    for (int i = 0; i < QN; i++) warm[i] = (WS && has_warm) ? a.warm[(size_t)b * QN + i] : -1;
    qp_solve_wave<WS, NV, QN, KCV>(R, nv, t, max_iter, out, V, (WS && has_warm) ? warm : nullptr, vtol, sfin);
    int *oi = a.oi + (size_t)b * (4 + QN);
    double *od = a.od + (size_t)b * (1 + QN + 64);
    LANES {
        if (lane == 0) {
            oi[0] = out.status;
            oi[1] = out.iters;
            oi[2] = out.nact;
            oi[3] = 0;
            od[0] = (double)out.viol;
#pragma unroll
            for (int i = 0; i < QN; i++) {
                oi[4 + i] = out.act[i];
                od[1 + i] = (double)out.x[i];
            }
        }
        od[1 + QN + lane] = (double)LV(sfin);
    }
}

#ifndef DWBC_HOST_EMU
// one wavefront per problem; 64 or 128 threads per block (the two-wave cycle runs the solver in a 128-thread block), each wave on
// its own slice of V
template <int WS, int NV, int QN, int KCV>
__global__ __launch_bounds__(128) void qp_probe_kernel(const QpProbeArgs a) {
    __shared__ real_t Vs[2 * QN];
    const int wave = (int)(threadIdx.x >> 6);
    const int b = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (b >= a.B) return;  // (the whole wave: the solver holds no block-wide barrier)
    qp_probe_problem<WS, NV, QN, KCV>(a, b, Vs + wave * QN);
}
#endif

// runs the batch; returns nullptr or the error text.  The caller (qp_probe.hip: qp_probe_solve) has checked every size; on the
// device `a` holds device pointers
template <int WS, int NV, int QN, int KCV>
static const char *qp_probe_run(const QpProbeArgs &a, int threads) {
#ifdef DWBC_HOST_EMU
    (void)threads;
    real_t V[QN];
    for (int b = 0; b < a.B; b++) qp_probe_problem<WS, NV, QN, KCV>(a, b, V);
    return nullptr;
#else
    const int per = threads / 64;
    hipLaunchKernelGGL((qp_probe_kernel<WS, NV, QN, KCV>), dim3((a.B + per - 1) / per), dim3(threads), 0, 0, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
#endif
}

}  // namespace dwbc
