// dwbc_task_qp.h -- RobotData::CalcSingleTaskTorqueWithQP (reference include/dwbc.h:354, src/dwbc.cpp:941-1127) for ONE task level in a
// launch of its own, one wavefront per instance: the step CalcTaskControlTorque takes once per level (src/dwbc.cpp:830-852) between
// CalcTaskSpace and the level's torque, for a caller that closes its own hierarchy in torch --
//   in    the level l, torque_prev (m), task_null_matrix (m x m; none: the identity, as the reference passes for level 0), f* of the level
//   out   f_star_qp (t)   contact_qp (k)   torque_h = J_kt Lambda (f* + f_star_qp) (dwbc.cpp:839)   torque_null_h = N torque_h (:840, :849)
//         torque_contact = NwJw contact_qp (:851)   status
// NwJw, J_C_INV_T, P_C, J_kt and Lambda_task are formed here from the state.  It is the task-space kernel's front for the one level and the
// cycle's row fill and solver behind it:
//   stage 0 (dwbc_cycle2_stage0.inc, shared text)          kinematics, CRBA, A in register columns
//   task points of level l, COM Jacobian                   while the link rotations stand; jac_com_ only where the level is on the COM link
//   contact stage (dwbc_contact_space_body.inc, shared)    with kCsWInv | kCsNwJw: Jbar^T, NwJw, s <- A^-1 N_c, G^-1, W^+
//   ahead of the W^+ sweep                                 the level's J_task, T1, Lambda (dwbc_task_space_level_front.inc, shared); Jbar^T[:, 6:],
//                                                          P_C = Jbar^T G and the contact frames move behind the map (the staged W overwrites them)
//   behind it                                              Q, Q W^+, J_kt, X = J_kt Lambda (dwbc_task_space_level_back.inc, shared)
//   operands of the rows                                   P1 = N X (N staged from global memory, lane-contiguous, over the dead staged W),
//                                                          base = torque_prev + P1 f*, RJ = A_rot Jbar[:, 6:] in place, W1 = RJ P1, W2 = RJ NwJw,
//                                                          fv = RJ base - A_rot P_C: plain thread-strided loops (wrench_maps of dwbc_cycle2.h reads
//                                                          its right-hand sides at the cycle's offsets for every level at once: its contract does not fit)
//   QP                                                     qp_rows_and_solve<N, NB, 0> (dwbc_cycle.h) on x = [f_star_qp (t); contact_qp (k)], cold start,
//                                                          the cycle's canon: kQpTol, kQpScaleGI on the contact columns, acceptance at kQpFeasTol
// No new DWBC_HOST_EMU fork: every device-only body reached here (the sweeps, the DPP primitives, contact_gram, the wave QP) has its own;
// what is added around them is plain code that the host emulation runs as written.
// status 0: more flags than two, a failed Lambda_c, a bad pivot of the W sweep, a rejected t x t block, or the QP's failure (dwbc.cpp:1117-1125);
// every other output of the instance is then zero.
#pragma once
#include "dwbc_task_space.h"

namespace dwbc {

// bits of TqIO::mask: 1u << dwbc_task_qp_output (include/dwbc_batch.h; dwbc_capi.hip asserts the two agree)
enum : unsigned { kTqFstarQp = 1u << 0, kTqContactQp = 1u << 1, kTqTorqueH = 1u << 2, kTqTorqueNullH = 1u << 3, kTqTorqueContact = 1u << 4 };
// what the launch needs of the contact stage: W^+ (with the columns A^-1 N_c and G^-1) and NwJw
constexpr unsigned kTqContactStageMask = kCsWInv | kCsNwJw;
constexpr int kTqMaxIter = 1000;  // nWSR of the one call (reference src/dwbc.cpp:1080), as the restatement's solve_qp takes it

// device pointers of a single-level task-QP launch, batch-major; the kernel's own argument struct beside BatchIO (whose layout is pack ABI and
// stays).  An output pointer whose bit is clear is never dereferenced.
struct TqIO {
    unsigned mask;
    int level;
    const io_t *torque_prev;  // B x M
    const io_t *null;         // B x M x M row-major, or nullptr: the identity
    io_t *f_star_qp;          // B x 6, zero beyond t
    io_t *contact_qp;         // B x 6, zero beyond k
    io_t *torque_h;           // B x M
    io_t *torque_null_h;      // B x M
    io_t *torque_contact;     // B x M, zero when k = 0
    int *status;              // B   always written
    unsigned cs_mask;         // kTqContactStageMask: CsIO::mask of the contact stage this launch runs (see task_qp_instance)
    io_t *cs_out;             // where another output of that stage would go: never written, NULL
};

// LDS map: LdsCs's (stage 0 and the contact stage are the same text), then the blocks of the ONE level under way, as LdsTs lays them out
// per level, then what the QP reads of the contact stage and its own operands.  W^+ and the staged null matrix move into the map itself
// as in LdsTs (c_Wp, c_Null).  Life times (block : front | W^+ sweep | level back | operands | QP and outputs):
//   Pt, Jcm    : task points, jac_com_ ..... | .      | .                | .                          | .
//   T1         : six base rows of A, then T1 ......... | Y = T1[:, 6:]    | .                          | .
//   Lt, G      : Lambda, Lambda^-1 ................... | read             | .                          | .
//   Q          : J_task (transposed, with QW) | .      | Q, then X ...... | X (P1 without null matrix) . | torque_h
//   QW         : (J_task)                    | .      | Q W^+, then free | P1 = N X ................... | rows, torque_null_h
//   Jk, Pi, s2, cod : (Pi, cod: Newton scratch) | .   | J_kt, pinv, scratch | .                       | .
//   Jb         : Jbar^T[:, 6:] ....................................... | RJ = A_rot Jbar[:, 6:]      | .
//   Nw         : NwJw (zero when k = 0) ................................................................ | rows, torque_contact
//   PC, Rc     : P_C, contact frames ................................. | A_rot P_C                   | .
//   base, fv, wm : .                         | .      | .                | base, fv, [W1 | W2]         | rows
//   V, x       : .                           | .      | .                | .                          | solver row, solution
//   c_Null     : (LdsCs: head .. NwJw, staged W) ..... | .                | N (M x M)                  | .
// Bytes (N / NB: total_bytes):  23 / 18: 24 048    37 / 32: 36 144    39 / 34: 37 872 (four workgroups per CU; LdsTs<39, 34>: 38 656)
// 43 / 38: 52 280 (W^+ behind the blocks)    50 / 45: 64 032
template <int N, int NB>
struct LdsTq : LdsCs<N, NB> {
    using B = LdsCs<N, NB>;
    using R = LdsRd<N, NB>;
    static constexpr int M = R::M, C = R::C, T = kMaxTaskDof;
    static constexpr int WLD = 2 * T;  // row stride of [W1 | W2]: W1 in columns 0 .. T - 1, W2 in columns T .. T + K - 1
    static constexpr int e_Pt = R::ev(R::total);
    static constexpr int e_Jcm = e_Pt + kMaxTaskLinks * 3;
    static constexpr int e_T1 = R::ev(e_Jcm + 6 * N + 3);
    static constexpr int e_Lt = e_T1 + T * N;
    static constexpr int e_G = e_Lt + T * T;
    static constexpr int e_Q = e_G + T * T;
    static constexpr int e_QW = e_Q + T * M;
    static constexpr int e_Jt = e_Q;
    static_assert(T * N <= 2 * T * M, "J_task of the level over Q and QW");
    static constexpr int e_Jk = e_QW + T * M;
    static constexpr int e_Pi = e_Jk + M * T;
    static constexpr int e_s2 = e_Pi + T * T;
    static constexpr int e_cod = e_s2 + T * T;
    static constexpr int q_Jb = R::ev(e_cod + 3 * T * T + 3 * T);  // C x M
    static constexpr int q_Nw = q_Jb + C * M;                       // M x K
    static constexpr int q_PC = q_Nw + M * R::K;                    // C
    static constexpr int q_Rc = q_PC + C;                           // 2 x 9
    static constexpr int q_base = q_Rc + kMaxActiveContacts * 9;    // M
    static constexpr int q_fv = q_base + M;                         // C
    static constexpr int q_wm = R::ev(q_fv + C);                    // C x WLD
    static constexpr int q_V = q_wm + C * WLD;                      // kQpLd (the row a drop step passes through LDS)
    static constexpr int q_x = q_V + kQpLd;                         // kQpLd
    static constexpr int e_end = R::ev(q_x + kQpLd);
    static_assert(R::K <= T && T + R::K <= kQpLd, "W2 behind W1 in a row of the maps");
    static constexpr bool wp_inside = B::c_Ws + M * B::w_rs + M * M <= R::c_s1;
    static constexpr int c_Wp = wp_inside ? B::c_Ws + M * B::w_rs : e_end;
    static constexpr int c_Null = B::c_Ws;
    static_assert(M * M <= M * B::w_rs, "the null matrix over the staged W");
    static constexpr int total = wp_inside ? e_end : e_end + M * M;
    static constexpr int total_bytes = total * (int)sizeof(real_t) + 64;
};
static_assert(LdsTq<39, 34>::total_bytes <= LdsTs<39, 34>::total_bytes, "one live level: not more than the task-space kernel's map");

template <int N, int NB, int NT, class Topo>
DWBC_DEV void task_qp_instance(Thr th, const Setup &su, const BatchIO &io, const TqIO &qio, int inst, real_t *L) {
    using S = LdsTq<N, NB>;
    constexpr bool kExtras = false;
    constexpr int M = S::M, C = S::C, T = kMaxTaskDof, WLD = S::WLD;
    DWBC_LANE_DECL;
    constexpr bool kTree = !std::is_same<Topo, TopoGeneric>::value;
    const int nb = kTree ? NB : su.nb;
    const real_t *body = DWBC_BODY(io, inst, nb);
    const int *topo = io.topo;  // parent[nb] depth[nb] subtree[nb]
    const io_t *qin = io.q + (size_t)inst * (N + 1);
    const DumpLayout dl = DumpLayout::make(N);
    real_t *dump = nullptr;  // no dump record, no diagnostics: the cycle's stay as its last launch left them
    int *diag = nullptr;
    DWBC_STAMP_INIT();
    const int lv = qio.level, ls = 0;  // the level, and the index of its blocks in the map (there is one set)
    constexpr unsigned want = 0u;      // (of the shared level text: no J_task store)
    auto put_j_task = [](int) {};

    PLA(real_t, s, N);  // column `lane` of A -> A^-1 -> A^-1 N_c
    PL(real_t, dg);     // its diagonal element

#define DWBC_STAGE0_FRONT_ONLY
#include "dwbc_cycle2_stage0.inc"
#undef DWBC_STAGE0_FRONT_ONLY

    // ================= world points of the level's links (dwbc.cpp:685-793) and jac_com_ (dwbc.cpp:318-353), while the link rotations stand =================
    bool com_level = false;
    for (int li = 0; li < su.t_nlinks[lv]; li++) com_level = com_level || su.t_link[lv][li] == nb;
    for (int idx = th.tid; idx < kMaxTaskLinks * 3; idx += NT) {
        const int a = idx % 3, li = idx / 3;
        real_t v = real_t(0.0);
        if (li < su.t_nlinks[lv] && su.t_link[lv][li] < nb) {
            const int mode = su.t_mode[lv][li], link = su.t_link[lv][li];
            real_t pl[3] = {0, 0, 0};
            if (mode == TASK_LINK_6D_COM_FRAME || mode == TASK_LINK_POSITION_COM_FRAME)
                for (int x = 0; x < 3; x++) pl[x] = body[link * kBodyStride + BF_COM + x];
            else if (mode == TASK_LINK_6D_CUSTOM_FRAME || mode == TASK_LINK_POSITION_CUSTOM_FRAME)
                for (int x = 0; x < 3; x++) pl[x] = su.t_point[lv][li][x];
            const real_t *R = L + S::Rw + link * 9;
            v = L[S::pw + link * 3 + a] + R[a * 3] * pl[0] + R[a * 3 + 1] * pl[1] + R[a * 3 + 2] * pl[2];
        }
        L[S::e_Pt + idx] = v;
    }
    if (com_level) {  // the six base rows of A out of the register columns, as the task-space kernel stages them
        real_t *A6 = L + S::e_T1;
        LANES {
            if (lane < N) {
#pragma unroll
                for (int a = 0; a < 6; a++) A6[a * N + lane] = LV(s)[a];
            }
        }
        DWBC_SYNC();
        com_jacobian<N, NT>(th, A6, N, L + S::Rw, L + S::q, L + S::e_Jcm);
    }
    DWBC_SYNC();

    real_t *Jt = L + S::e_Jt;
    int st_task = 1;
    // ================= while the columns A^-1 N_c and the link positions stand: J_task, T1, Lambda_task of the level (wbd.cpp:210) =================
    auto level_front = [&]() __attribute__((always_inline)) {
#include "dwbc_task_space_level_front.inc"
    };
    const unsigned mask = qio.cs_mask;
    // (the mask and the pointer the stage's other stores would go through are kernel arguments, for the reason given in task_space_instance:
    // with either a constant -- a null pointer folds the branches on its bits as a constant mask does -- the stage's blocks merge and the
    // scheduler's hoisting costs 954 spilled VGPRs, 3.4 KB of scratch per lane, under the register cap; with the branches kept, none)
    io_t *o_JC = qio.cs_out, *o_Lam = o_JC, *o_JbT = o_JC, *o_NC = o_JC, *o_AiNc = o_JC, *o_W = o_JC, *o_pos = o_JC, *o_rot = o_JC;
    static_assert(sizeof(io_t) == sizeof(real_t) || N < 0, "NwJw and W^+ go to LDS through the contact stage's output pointers: fp64 only");
    io_t *o_Nw = reinterpret_cast<io_t *>(L + S::q_Nw);  // the stage's store of NwJw (zeros when k = 0) lands behind the map, where the rows read it
    io_t *o_Wi = reinterpret_cast<io_t *>(L + S::c_Wp);  // W^+ stays in LDS, row stride M
    // what the rows read of the contact stage, taken behind the map before the staged W overwrites head, Jbar^T and NwJw: Jbar^T[:, 6:]
    // (zero rows beyond cd), P_C = Jbar^T G (wbd.cpp:192) and the contact frames
    auto save_contact_stage = [&](const real_t *JbT_, int cd_, int nc_) __attribute__((always_inline)) {
        DWBC_SYNC();
        for (int idx = th.tid; idx < C * M; idx += NT) {
            const int i = idx / M, c = idx - i * M;
            L[S::q_Jb + idx] = i < cd_ ? JbT_[i * N + 6 + c] : real_t(0.0);
        }
        for (int i = th.tid; i < C; i += NT) {
            real_t acc = real_t(0.0);
            if (i < cd_) {
                _Pragma("unroll 8")
                for (int j = 0; j < N; j++) acc += JbT_[i * N + j] * L[S::G + j];
            }
            L[S::q_PC + i] = acc;
        }
        for (int r = th.tid; r < kMaxActiveContacts * 9; r += NT) L[S::q_Rc + r] = r < 9 * nc_ ? L[S::Rc + r] : real_t(0.0);
        DWBC_SYNC();
    };
#define DWBC_CS_BEFORE_W_INV level_front(); save_contact_stage(JbT, cd, nc);
#include "dwbc_contact_space_body.inc"
#undef DWBC_CS_BEFORE_W_INV
    DWBC_SYNC();
    if (!st_contact) st_task = 0;

    // ================= behind W^+: J_kt (wbd.cpp:212-214, CalculateJKT) and X = J_kt Lambda of the level =================
    const int t = su.t_dof[lv];
    const real_t *Wp = L + S::c_Wp, *T1 = L + S::e_T1, *Lt = L + S::e_Lt;
    real_t *Q = L + S::e_Q, *QW = L + S::e_QW, *Jk = L + S::e_Jk, *Pi = L + S::e_Pi, *s2 = L + S::e_s2, *cod = L + S::e_cod;
    if (st_task) do {
        DWBC_SYNC();
#include "dwbc_task_space_level_back.inc"
    } while (0);
    DWBC_SYNC();

    // ================= operands of the rows (dwbc.cpp:1001-1053) =================
    const real_t *X = Q, *Nw = L + S::q_Nw;
    const real_t *P1 = X;  // Ntorque_task = N J_kt Lambda; without a null matrix it is X itself
    real_t *base = L + S::q_base, *fv = L + S::q_fv, *WM = L + S::q_wm, *RJ = L + S::q_Jb, *RPC = L + S::q_PC;
    const real_t *xq = L + S::q_x;
    const io_t *tprev = qio.torque_prev + (size_t)inst * M;
    real_t f6[T];  // f* of the level (wave-uniform), zero beyond t
    {
        const io_t *fs = io.fstar + (size_t)inst * su.fstar_total + su.fstar_off[lv];
#pragma unroll
        for (int j = 0; j < T; j++) f6[j] = j < t ? (real_t)fs[j < t ? j : 0] : real_t(0.0);
    }
    if (st_task) {
        if (qio.null) {
            // the null matrix, lane-contiguous from global memory, over the staged W (dead behind the Newton step on W^+); P1 over Q W^+ (dead behind J_kt)
            const io_t *Ng = qio.null + (size_t)inst * M * M;
            real_t *Nl = L + S::c_Null;
            for (int idx = th.tid; idx < M * M; idx += NT) Nl[idx] = (real_t)Ng[idx];
            DWBC_SYNC();
            mm_nn<NT>(th, QW, t, Nl, M, X, t, M, M, t);
            P1 = QW;
            DWBC_SYNC();
        }
        for (int i = th.tid; i < M; i += NT) {  // torque the level starts from (dwbc.cpp:1001-1016)
            real_t acc = (real_t)tprev[i];
#pragma unroll
            for (int j = 0; j < T; j++) acc += j < t ? P1[i * t + j] * f6[j] : real_t(0.0);  // (f6 stays in registers: no run-time index)
            base[i] = acc;
        }
        // contact-local frames, in place: rows 3 g .. 3 g + 2 of Jbar[:, 6:] and of P_C times R_a^T (A_rot = blockdiag(R_a^T, R_a^T), dwbc.cpp:1018-1039)
        const int ng = cd / 3;
        for (int idx = th.tid; idx < ng * (M + 1); idx += NT) {
            const int g = idx / (M + 1), c = idx - g * (M + 1);
            const real_t *R = L + S::q_Rc + (g / 2) * 9;
            real_t *p = c < M ? RJ + 3 * g * M + c : RPC + 3 * g;
            const int st = c < M ? M : 1;
            const real_t v0 = p[0], v1 = p[st], v2 = p[2 * st];
#pragma unroll
            for (int x = 0; x < 3; x++) p[x * st] = R[x] * v0 + R[3 + x] * v1 + R[6 + x] * v2;
        }
        DWBC_SYNC();
        // [W1 | W2] = RJ [P1 | NwJw] and fv = RJ base - A_rot P_C (dwbc.cpp:1041-1053), zero rows beyond cd and zero columns beyond t / k
        for (int idx = th.tid; idx < C * (WLD + 1); idx += NT) {
            const int i = idx / (WLD + 1), col = idx - i * (WLD + 1);
            const bool left = col < T, fvc = col == WLD;
            const int j = left ? col : col - T;
            const bool in = i < cd && (fvc || (left ? j < t : j < k));
            const real_t *rhs = fvc ? base : left ? P1 + j : Nw + j;
            const int rs = fvc ? 1 : left ? t : 6;
            real_t acc = fvc ? -RPC[i] : real_t(0.0);
            if (in) {
                _Pragma("unroll 8")
                for (int c = 0; c < M; c++) acc += RJ[i * M + c] * rhs[c * rs];
            } else {
                acc = real_t(0.0);
            }
            if (fvc) fv[i] = acc; else WM[i * WLD + col] = acc;
        }
        DWBC_SYNC();

        // ================= the QP in [f_star_qp (t); contact_qp (k)], started cold (dwbc.cpp:1055-1127) =================
        const int nlim = su.has_tau_lim ? 2 * M : 0, ncone = 10 * nc;
        QpResult qres;
        PL(real_t, sfin);
        qp_rows_and_solve<N, NB, 0>(su, L, nlim, ncone, act_c[0], act_c[1], P1, t, t, Nw, 6, k, kQpScaleGI, WM, WLD, WM + T, WLD, fv, base, t,
                                    kTqMaxIter, qres, L + S::q_V, L + S::q_x, nullptr, nullptr, kQpTol, sfin, io.inst_par, inst);
        if (!qres.status) st_task = 0;  // dwbc.cpp:1117-1125
    }

    // ================= outputs: zero on a failed instance =================
    const bool ok = st_task != 0;
    real_t fx[T], xc[T];  // f* + f_star_qp, contact_qp (wave-uniform), zero beyond t / k and on failure
#pragma unroll
    for (int j = 0; j < T; j++) {
        fx[j] = (ok && j < t) ? f6[j] + xq[j < t ? j : 0] : real_t(0.0);
        xc[j] = (ok && j < k) ? xq[t + (j < k ? j : 0)] : real_t(0.0);
    }
    if (qio.mask & kTqFstarQp) {
        io_t *o = qio.f_star_qp + (size_t)inst * T;
        for (int j = th.tid; j < T; j += NT) o[j] = (ok && j < t) ? xq[j < t ? j : 0] : real_t(0.0);
    }
    if (qio.mask & kTqContactQp) {
        io_t *o = qio.contact_qp + (size_t)inst * T;
        for (int j = th.tid; j < T; j += NT) o[j] = (ok && j < k) ? xq[t + (j < k ? j : 0)] : real_t(0.0);
    }
    auto put_torque = [&](unsigned bit, io_t *out, const real_t *A, int lda, const real_t *v, int n) {
        if (!(qio.mask & bit)) return;
        io_t *o = out + (size_t)inst * M;
        for (int i = th.tid; i < M; i += NT) {
            real_t acc = real_t(0.0);
#pragma unroll
            for (int j = 0; j < T; j++) acc += (ok && j < n) ? A[i * lda + j] * v[j] : real_t(0.0);
            o[i] = acc;
        }
    };
    put_torque(kTqTorqueH, qio.torque_h, X, t, fx, t);           // J_kt Lambda (f* + f_star_qp)          (dwbc.cpp:839)
    put_torque(kTqTorqueNullH, qio.torque_null_h, P1, t, fx, t); // N torque_h                            (dwbc.cpp:840, :849)
    put_torque(kTqTorqueContact, qio.torque_contact, Nw, 6, xc, k);  // NwJw contact_qp; k = 0: zero       (dwbc.cpp:851)
    if (th.tid == 0) qio.status[inst] = ok ? 1 : 0;
}

}  // namespace dwbc
