// dwbc_task_space.h -- RobotData::SetTaskSpace + CalcTaskSpace (reference src/dwbc.cpp:795-816, src/task.cpp:90-93,202-211,
// src/wbd.cpp:207-261) in a launch of its own, one wavefront per instance: what a caller reads off ts_[i] between CalcTaskSpace and a
// torque law of its own --
//   J_task_ (t x n)   Lambda_task_ (t x t)   J_kt_ (m x t)   Null_task_ (m x m, every level but the last)
// -- per level, written to buffers of their own, selected by a mask.  It is the contact-space kernel's front and the level loop of the
// restatement (oracle/dwbc_np.py, Cycle.calc_task_torque) behind it:
//   stage 0 (dwbc_cycle2_stage0.inc, shared text)        kinematics, CRBA, A in register columns
//   task points, COM Jacobian                            while the link rotations stand; jac_com_ from the six base rows of A (com_jacobian)
//   contact stage (dwbc_contact_space_body.inc, shared)  A^-1 sweep, J_C, Lambda_c, Jbar^T, s <- A^-1 N_c, G^-1, W^+ (with its Newton step)
//   ahead of the W^+ sweep, per level                    J_task, T1 = J_task (A^-1 N_c) one column per lane, Lambda^-1 = T1 J_task^T, Lambda
//                                                        (the columns die in the sweep; the link positions and axes under the staged W)
//   behind it, per level                                 Q = (Lambda T1)[:, 6:], Q W^+, J_kt = (Q W^+)^T pinv(Q W^+ Q^T) -- the route the cycle
//                                                        takes when its shortcut does not apply -- and, below the last level,
//                                                        Null_l = Null_{l-1} - (Null_{l-1} X_l) Y_l,  X_l = J_kt Lambda,  Y_l = T1[:, 6:]
// Every step sits behind a wave-uniform branch on the mask (a kernel argument):
//   only J_TASK                  nothing behind the kinematics: no A^-1 sweep, no contact stage
//   neither J_KT nor NULL_TASK   nothing behind Lambda of each level: no internal-wrench basis, no G^-1, no W^+ sweep
//   no NULL_TASK                 no projector is formed, no m x m store
// No f*, no trajectory, no QP; of BatchIO it reads q, flags, body and topo, of Setup the tree, the contacts and the task levels.
// The per-level text ahead of and behind the W^+ sweep is dwbc_task_space_level_front.inc / dwbc_task_space_level_back.inc: the single-level
// task-QP kernel (dwbc_task_qp.h) runs the same text for its one level.
#pragma once
#include "dwbc_contact_space.h"

namespace dwbc {

// bits of TsIO::mask: 1u << dwbc_task_space_output (include/dwbc_batch.h; dwbc_capi.hip asserts the two agree)
enum : unsigned { kTsJTask = 1u << 0, kTsLambda = 1u << 1, kTsJkt = 1u << 2, kTsNull = 1u << 3 };
constexpr unsigned kTsNeedsW = kTsJkt | kTsNull;  // anything behind Lambda_task
// TsIO::cs_mask of a request: what the levels need of the contact stage
constexpr unsigned ts_contact_stage_mask(unsigned mask) { return (mask & kTsNeedsW) ? kCsWInv : kCsW; }

// device pointers of a task-space launch, batch-major and per level, with t the level's task dof; the kernel's own argument struct beside
// BatchIO (whose layout is pack ABI and stays).  A pointer whose bit is clear, or whose level does not exist, is never dereferenced.
struct TsIO {
    unsigned mask;
    io_t *J_task[kMaxLevels];  // B x t x N
    io_t *Lambda[kMaxLevels];  // B x t x t
    io_t *J_kt[kMaxLevels];    // B x M x t
    io_t *Null[kMaxLevels];    // B x M x M, levels 0 .. L - 2
    int *status;               // B   always written: 0 = more flags than two, a failed Lambda_c, a bad pivot of the W sweep, or a t x t block of
                               //     some level that the small inverses reject (every asked-for output of the instance is then zero)
    unsigned cs_mask;          // CsIO::mask of the contact stage this launch runs: kCsWInv with J_kt or Null_task in the request, else kCsW (see
                               // task_space_instance: ts_contact_stage_mask)
    io_t *cs_out;              // where an output of that stage would go: never written, NULL
};

// LDS map: LdsCs's (stage 0 and the contact stage are the same text), then this kernel's own blocks behind it.  Two tenants move into the
// map itself once the contact stage is through:
//   W^+ (M x M, row stride M)   behind the staged W where that ends below the pivot column of the W sweep (everything there is dead once
//                               the projector P is in registers), else behind the blocks below
//   Null (M x M)                over the staged W, which is dead behind the Newton step on W^+
// Behind the map:
//   Pt    world points of the task links (taken while the link rotations stand, as the compact cycle does)
//   Jcm   jac_com_ and com_pos (com_jacobian's record), for levels on the COM link
//   T1    per level T x N: J_task (A^-1 N_c); first, the six base rows of A for com_jacobian
//   Lt, G per level t x t: Lambda_task and what it inverts, J_task A^-1 N_c J_task^T
//   Q, QW T x M each; ahead of the W^+ sweep J_task of the level under way (T x N) lies over both; behind J_kt, X over Q and Null X over QW
//   Jk    M x t: J_kt
//   Pi, s2, cod   t x t blocks: pinv(Q W^+ Q^T), its input (and the input of Lambda), the scratch of pinv_cod_small
// Bytes (N / NB: total_bytes):  23 / 18: 24 960    37 / 32: 36 944    39 / 34: 38 656 (four workgroups per CU)    43 / 38: 53 032 (W^+ behind
// the blocks)    50 / 45: 64 736
template <int N, int NB>
struct LdsTs : LdsCs<N, NB> {
    using B = LdsCs<N, NB>;
    using R = LdsRd<N, NB>;
    static constexpr int M = R::M, T = kMaxTaskDof, LV = kMaxLevels;
    static constexpr int e_Pt = R::ev(R::total);
    static constexpr int e_Jcm = e_Pt + LV * kMaxTaskLinks * 3;
    static constexpr int e_T1 = R::ev(e_Jcm + 6 * N + 3);
    static constexpr int e_Lt = e_T1 + LV * T * N;
    static constexpr int e_G = e_Lt + LV * T * T;   // per level t x t: Lambda_task^-1 = J_task A^-1 N_c J_task^T
    static constexpr int e_Q = e_G + LV * T * T;
    static constexpr int e_QW = e_Q + T * M;
    static constexpr int e_Jt = e_Q;
    static_assert(T * N <= 2 * T * M, "J_task of the level under way over Q and QW");
    static constexpr int e_Jk = e_QW + T * M;
    static constexpr int e_Pi = e_Jk + M * T;
    static constexpr int e_s2 = e_Pi + T * T;
    static constexpr int e_cod = e_s2 + T * T;
    static constexpr int e_end = R::ev(e_cod + 3 * T * T + 3 * T);
    static constexpr bool wp_inside = B::c_Ws + M * B::w_rs + M * M <= R::c_s1;
    static constexpr int c_Wp = wp_inside ? B::c_Ws + M * B::w_rs : e_end;
    static constexpr int c_Null = B::c_Ws;
    static_assert(M * M <= M * B::w_rs, "Null over the staged W");
    static constexpr int total = wp_inside ? e_end : e_end + M * M;
    static constexpr int total_bytes = total * (int)sizeof(real_t) + 64;
};

// J_task of one level, TRANSPOSED (N x T, as the cycle keeps it) with zero columns beyond t (reference src/dwbc.cpp:685-793; the modes as
// Cycle.task_jacobian of the restatement tells them apart).  R0: the pelvis rotation; Pt: the world points of the level's links
template <int N, int NB, int NT>
DWBC_DEV void task_jacobian_rows(Thr th, const Setup &su, int lv, const real_t *R0, const real_t *pw, const real_t *aw, const int *topo, int nb,
                                 const real_t *Pt, const real_t *Jcm, real_t *Jtt) {
    constexpr int T = kMaxTaskDof;
    DWBC_SYNC();
    for (int idx = th.tid; idx < T * N; idx += NT) Jtt[idx] = real_t(0.0);
    DWBC_SYNC();
    int row = 0;
    for (int li = 0; li < su.t_nlinks[lv]; li++) {
        const int mode = su.t_mode[lv][li], link = su.t_link[lv][li];
        const int rsel = mode <= TASK_LINK_6D_CUSTOM_FRAME ? 0 : (mode <= TASK_LINK_POSITION_CUSTOM_FRAME ? 1 : 2);
        if (link == nb) com_task_rows<N, NT>(th, Jcm, Jtt, row, rsel, T);  // the COM link: jac_ = jac_com_ (dwbc.cpp:352-353)
        else point_jacobian<N, NB, NT>(th, R0, pw, aw, topo, nb, link, Pt + li * 3, Jtt, 1, row, rsel == 0 ? 6 : 3, rsel, T);
        row += rsel == 0 ? 6 : 3;
    }
    DWBC_SYNC();
}

// One Newton step on the inverse X of a small SPD block G (t x t, row stride t both), X <- X - X (G X - I), as the contact stage takes on
// Lambda_c: a caller of this launch multiplies Lambda_task and J_kt back onto what they invert.  E, Xn: t x t scratch each
template <int NT>
DWBC_DEV void newton_step_small(Thr th, const real_t *G, real_t *X, int t, real_t *E, real_t *Xn) {
    DWBC_SYNC();
    for (int idx = th.tid; idx < t * t; idx += NT) {
        const int i = idx / t, j = idx - i * t;
        real_t acc = (i == j) ? real_t(-1.0) : real_t(0.0);
        for (int c = 0; c < t; c++) acc += G[i * t + c] * X[c * t + j];
        E[idx] = acc;
    }
    DWBC_SYNC();
    for (int idx = th.tid; idx < t * t; idx += NT) {
        const int i = idx / t, j = idx - i * t;
        real_t acc = X[idx];
        for (int c = 0; c < t; c++) acc -= X[i * t + c] * E[c * t + j];
        Xn[idx] = acc;
    }
    DWBC_SYNC();
    for (int idx = th.tid; idx < t * t; idx += NT) X[idx] = Xn[idx];
    DWBC_SYNC();
}

template <int N, int NB, int NT, class Topo>
DWBC_DEV void task_space_instance(Thr th, const Setup &su, const BatchIO &io, const TsIO &tio, int inst, real_t *L) {
    using S = LdsTs<N, NB>;
    constexpr bool kExtras = false;
    constexpr int M = S::M, C = S::C, T = kMaxTaskDof;
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
    const unsigned want = tio.mask;
    const int nlv = su.n_levels;

    PLA(real_t, s, N);  // column `lane` of A -> A^-1 -> A^-1 N_c
    PL(real_t, dg);     // its diagonal element

#define DWBC_STAGE0_FRONT_ONLY
#include "dwbc_cycle2_stage0.inc"
#undef DWBC_STAGE0_FRONT_ONLY

    // ================= world points of the task links (dwbc.cpp:685-793) and jac_com_ (dwbc.cpp:318-353), while the link rotations stand =================
    for (int idx = th.tid; idx < nlv * kMaxTaskLinks * 3; idx += NT) {
        const int a = idx % 3, li = (idx / 3) % kMaxTaskLinks, lv = idx / (3 * kMaxTaskLinks);
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
    if (su.has_com_task) {  // the six base rows of A out of the register columns, as the link query stages them
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
    auto put_j_task = [&](int lv) {
        io_t *o = tio.J_task[lv] + (size_t)inst * su.t_dof[lv] * N;
        for (int idx = th.tid; idx < su.t_dof[lv] * N; idx += NT) o[idx] = Jt[(idx % N) * T + idx / N];
    };
    int st_task = 1;

    if (!(want & ~kTsJTask)) {
        // ================= only J_task: nothing behind the kinematics =================
        const unsigned char *flj = io.flags + (size_t)inst * su.n_contacts;
        int nfl = 0;
        for (int i = 0; i < su.n_contacts; i++) nfl += flj[i] ? 1 : 0;
        if (nfl > kMaxActiveContacts) st_task = 0;  // as every other tier: such an instance fails
        for (int lv = 0; lv < nlv && st_task; lv++) {
            task_jacobian_rows<N, NB, NT>(th, su, lv, L + S::Rw, L + S::pw, L + S::aw, topo, nb, L + S::e_Pt + lv * kMaxTaskLinks * 3, L + S::e_Jcm, Jt);
            if (want & kTsJTask) put_j_task(lv);  // (a request of the status alone asks for no J_task either)
        }
    } else {
        // ================= per level, while the columns A^-1 N_c and the link positions stand: J_task, T1, Lambda_task (wbd.cpp:210) =================
        auto levels_front = [&]() __attribute__((always_inline)) {
            for (int lv = 0; lv < nlv; lv++) {
                const int ls = lv;
#include "dwbc_task_space_level_front.inc"
            }
        };
        // of the contact stage: kCsWInv -- the columns s <- A^-1 N_c, G^-1 and W^+ -- where J_kt or Null_task is asked for, else kCsW -- the
        // columns alone: no internal-wrench basis, no G^-1, no W^+ sweep; none of its outputs to memory.  A kernel argument, like the
        // pointer its other output stores would go through: with the mask a constant the stage's wave-uniform branches fold away, its
        // blocks merge and the scheduler's hoisting costs 754 spilled VGPRs (3.5 KB of scratch per lane) under the register cap; with the
        // branches kept, none
        const unsigned mask = tio.cs_mask;
        io_t *o_JC = tio.cs_out, *o_Lam = o_JC, *o_JbT = o_JC, *o_NC = o_JC, *o_AiNc = o_JC, *o_Nw = o_JC, *o_pos = o_JC, *o_rot = o_JC;
        static_assert(sizeof(io_t) == sizeof(real_t) || N < 0, "W and W^+ go to LDS through the contact stage's output pointers: fp64 only");
        static_assert(S::e_end - S::e_T1 >= M * M || N < 0, "W of the kCsW tier over the level blocks, which are all written behind it");
        io_t *o_W = reinterpret_cast<io_t *>(L + S::e_T1);   // kCsW: the stage's store of W lands in LDS that nothing reads (the columns are what is wanted)
        io_t *o_Wi = reinterpret_cast<io_t *>(L + S::c_Wp);  // W^+ stays in LDS, row stride M
#define DWBC_CS_BEFORE_W_INV levels_front();
#include "dwbc_contact_space_body.inc"
#undef DWBC_CS_BEFORE_W_INV
        DWBC_SYNC();
        if (!st_contact) st_task = 0;

        // ================= per level, behind W^+: J_kt (wbd.cpp:212-214, CalculateJKT) and Null_task (dwbc.cpp:804-813) =================
        const real_t *Wp = L + S::c_Wp;
        real_t *Nl = L + S::c_Null, *Q = L + S::e_Q, *QW = L + S::e_QW, *Jk = L + S::e_Jk, *Pi = L + S::e_Pi, *s2 = L + S::e_s2, *cod = L + S::e_cod;
        if (st_task && (want & kTsNull))
            for (int idx = th.tid; idx < M * M; idx += NT) Nl[idx] = (idx / M == idx % M) ? real_t(1.0) : real_t(0.0);
        for (int lv = 0; lv < nlv && st_task; lv++) {
            const int t = su.t_dof[lv];
            const real_t *T1 = L + S::e_T1 + lv * T * N, *Lt = L + S::e_Lt + lv * T * T;
            DWBC_SYNC();
            if (want & kTsLambda) {
                io_t *o = tio.Lambda[lv] + (size_t)inst * t * t;
                for (int idx = th.tid; idx < t * t; idx += NT) o[idx] = Lt[idx];
            }
            if (!(want & kTsNeedsW)) continue;
            const int ls = lv;
#include "dwbc_task_space_level_back.inc"
            if (want & kTsJkt) {
                io_t *o = tio.J_kt[lv] + (size_t)inst * M * t;
                for (int idx = th.tid; idx < M * t; idx += NT) o[idx] = Jk[idx];
            }
            if ((want & kTsNull) && lv < nlv - 1) {
                mm_nn<NT>(th, U, t, Nl, M, X, t, M, M, t);   // U = Null_{l-1} X
                DWBC_SYNC();
                for (int idx = th.tid; idx < M * M; idx += NT) {  // Null_l = Null_{l-1} - U Y, Y = T1[:, 6:]
                    const int i = idx / M, j = idx - i * M;
                    real_t acc = Nl[idx];
                    for (int r = 0; r < t; r++) acc -= U[i * t + r] * T1[r * N + 6 + j];
                    Nl[idx] = acc;
                }
                DWBC_SYNC();
                io_t *o = tio.Null[lv] + (size_t)inst * M * M;
                for (int idx = th.tid; idx < M * M; idx += NT) o[idx] = Nl[idx];
            }
        }
    }

    // ================= a failed instance: what was written goes back to zero =================
    if (!st_task) {
        for (int lv = 0; lv < nlv; lv++) {
            const int t = su.t_dof[lv];
            auto zero = [&](unsigned bit, io_t *p, int cnt) {
                if (want & bit)
                    for (int idx = th.tid; idx < cnt; idx += NT) p[(size_t)inst * cnt + idx] = real_t(0.0);
            };
            zero(kTsJTask, tio.J_task[lv], t * N);
            zero(kTsLambda, tio.Lambda[lv], t * t);
            zero(kTsJkt, tio.J_kt[lv], M * t);
            if (lv < nlv - 1) zero(kTsNull, tio.Null[lv], M * M);
        }
    }
    if (th.tid == 0) tio.status[inst] = st_task ? 1 : 0;
}

}  // namespace dwbc
