// dwbc_redistribute.h -- contact redistribution of a CALLER-SUPPLIED joint torque, one wavefront per instance:
//   RobotData::CalcContactRedistribute(torque_input, hqp = true, init)   reference include/dwbc.h:297, src/dwbc.cpp:1377-1568
//   RobotData::getContactForce(command_torque)                           reference include/dwbc.h:303, src/wbd.cpp:268-271
// The torque comes from anywhere (a policy, a clipped command, another controller); the kernel returns the contact-null-space torque
// NwJw c that brings the contact wrenches back inside the ZMP / friction rows and the torque limits, the QP's answer c, and the contact
// wrench before and after the correction.  It is the front half of the fused cycle and one QP of k = cd - 6 variables:
//   stage 0 (dwbc_cycle2_stage0.inc, shared text)   kinematics, CRBA, tree-sparse A^-1 sweep
//   stage 1 (below)                                 contact frames, J_C, Y = J_C A^-1, Lambda_c, Jbar^T = Lambda_c Y, P_C = Jbar^T G
//   NwJw                                            closed form from the internal-wrench basis (as dwbc_cycle2.h forms it)
//   wrench maps                                     FN = Jbar[:, 6:] [tau_in | NwJw]  (cd x 7), rotated into the contact frames for the cone rows
//   QP                                              min |c|^2  s.t.  +-NwJw c <= tau_lim -+ tau_in,  10 cone rows per active contact
//                                                   (dwbc.cpp:1458-1517; qp_solve_wave, cold start at c = 0, accepted at kQpFeasTol)
// What the cycle needs beyond that is never formed here: no A^-1 N_c (the register columns stay A^-1), no W, no W^+, no gravity torque,
// no task block.
// The GRAV build of the same text (redistribute_instance<.., true>, dwbc_gravcomp_kernel) is RobotData::CalcGravCompensation() as a launch
// of its own and ahead of the redistribution: torque_grav_ is formed behind P_C from blocks stage 1 already holds (see above GravIO), the
// redistribution then runs on torque_grav_ + tau_in, or is skipped when there is no tau_in.  Every GRAV branch is `if constexpr` or folds
// on a constant in the plain build, whose instantiations compile to what they were.
#pragma once
#include "dwbc_cycle2.h"

namespace dwbc {

// device pointers of a redistribution launch that BatchIO has no member for (BatchIO's layout is part of the kernel-pack ABI and stays)
struct RedistIO {
    const io_t *tau_in;  // B x M   torque_input
    io_t *tau;           // B x M   NwJw c (what the reference adds to torque_contact_)
    io_t *cf;            // B x 6   c (cf_redis_qp_), zero beyond k
    io_t *wrench;        // B x 2 x 12: getContactForce(tau_in), getContactForce(tau_in + NwJw c); zero padded
    int *status;         // B       1 ok / 0 failed
};

// LDS map: the order of the compact map's stage-0 / stage-1 / NwJw blocks (Lds3 at one task level, dwbc_cycle2.h) -- those stages are
// the same text -- with the blocks behind them named for what this kernel keeps there.  Life times (region : stage 0 | stage 1 | NwJw | maps + QP):
//   head : q, G ............. G (P_C) | .    | .
//   JbT  : k_S k_F          | J_C, then Jbar^T .......................... (maps, wrench outputs)
//   NwJw : .                | .              | NwJw .................... (QP rows, torque output)
//   U    : Rw               | Rw (contact frames, pelvis rotation)  | . | .
//   RE   : pw aw ........................... | .    | tau_in, rotated maps, fv, QP scratch
//   RF   : k_Iw k_Ic (k_Rl, k_A over them) | Vb ........... | (QP scratch reaches into it)
//   RG   : (k_Ic, k_A)      | Y              | .    | .
//   RX   : (k_A), sweep column | Lambda_c, small-inverse scratch ... | FN (unrotated maps, kept for the wrench outputs)
// The map is laid out for every model size a kernel runs at (N = NB + 5 <= 50), not for TOCABI's alone.  Lds3 sizes its regions for the
// tenants of the CYCLE, and three of its borrowings do not carry over: the QP scratch outgrows RE .. RG below 39 dof (RE .. RG shrinks
// with M, the C x WLD wrench maps do not), Y fills RG .. RX to the last double at every even N, and the packed mass matrix runs past
// the end of the map from 46 dof on.  So every region here is as large as the largest of ITS tenants: U holds the link rotations or
// 2 M T, the QP scratch may run on through RG (Y is dead by then) and pushes RX back where it would reach FN, and the map ends behind
// the last of the small-inverse block, the staged mass matrix and the composite inertias.  The blocks this kernel never writes (FNl, the
// task points, G^-1) keep their places, so that at 39 / 34 every offset is the compact map's and TOCABI's kernel is the one it was
// (asserted below the struct).
// Bytes (N / NB: total_bytes, workgroups that fit a CU's 160 KB):  23 / 18: 12 880, 12    37 / 32: 19 488, 8    39 / 34: 20 432, 8
//                                                                  43 / 38: 22 320, 7     50 / 45: 26 792, 6
// (the register cap of two waves per SIMD allows eight one-wave workgroups per CU whatever the map says)
template <int N, int NB>
struct LdsRd {
    static constexpr bool compact = true;
    static constexpr int M = N - 6;
    static constexpr int C = 6 * kMaxActiveContacts;
    static constexpr int K = C - 6;
    static constexpr int T = kMaxTaskDof;
    static constexpr int max2(int a, int b) { return a > b ? a : b; }
    static constexpr int ev(int a) { return (a + 1) & ~1; }
    // ---- head: the stage-0 text clears tg .. tc and fills fs; PC, Rc, Pc live to the end
    static constexpr int tg = 0;
    static constexpr int tt = tg + M;
    static constexpr int tc = tt + M;
    static constexpr int PC = tc + M;
    static constexpr int Rc = PC + C;
    static constexpr int Pc = Rc + kMaxActiveContacts * 9;
    static constexpr int fs = Pc + kMaxActiveContacts * 3;
    static constexpr int comp = fs + kMaxLevels * kMaxTaskDof;
    static constexpr int q = ev(comp + 4);                     // N+1, stage 0 only
    static constexpr int G = q + ev(N + 1);                    // N
    static constexpr int hend = G + ev(N);
    // ---- long-lived blocks
    static constexpr int JbT = hend;                           // C x N
    static constexpr int c_JC = JbT;                           // N x C, until Jbar^T is written over it
    static constexpr int k_S = JbT;                            // N x 6
    static constexpr int k_F = k_S + N * 6;                    // N x 6
    static_assert(k_F + N * 6 <= JbT + C * N, "S and F borrow the Jbar^T region");
    static constexpr int NwJw = JbT + C * N;                   // M x K
    static constexpr int FNl = NwJw + M * K;                   // (C x K of the cycle: not formed here)
    static constexpr int U = FNl + C * K;
    static constexpr int Rw = U;                               // NB x 9, until the contact frames are taken
    static constexpr int RE = U + max2(2 * M * T, NB * 9);
    static_assert(Rw + NB * 9 <= RE, "the link rotations");
    static constexpr int pw = RE;
    static constexpr int aw = pw + NB * 3;
    static constexpr int Rw0 = aw + NB * 3;                    // 9 (+1)
    static constexpr int RF = ev(Rw0 + 10 + kMaxLevels * kMaxTaskLinks * 3);  // (behind the task points of the cycle)
    static constexpr int c_Vb = RF;                            // M x K
    static constexpr int RG = c_Vb + M * K + K * K;            // (behind G^-1 of the cycle)
    // ---- stage 0
    static constexpr int k_Iw = RF;                            // NB x 10 (first the ping-pong partner of pw)
    static constexpr int k_Ic = k_Iw + NB * 10;                // NB x 10
    static constexpr int k_Rl = k_Iw + NB * 3;                 // NB x 9: local rotations / ping-pong partner of Rw, dead before Iw and Ic are written
    static constexpr int k_anc = k_Ic + NB * 10 - 2 * NB;      // ancestor indices at the tail of k_Ic
    static_assert(k_Rl + NB * 9 <= k_anc, "local rotations must not reach the ancestor indices");
    static constexpr bool a_overlay = false, a_packed = true;
    static constexpr int k_A = RF;                             // N (N + 1) / 2, written after Ic has been consumed
    static constexpr int Jcm = 0;                              // (COM task levels: full build of the cycle only)
    // ---- the wrench maps and the QP (RE onwards; pw, aw, Vb and Y are dead by then)
    static constexpr int WLD = 32;
    static constexpr int FLD = 8;                              // row stride of FN: 1 + K columns, padded to an even number
    static constexpr int t_in = RE;                            // M: tau_in (the `base` of the QP's torque rows)
    static constexpr int wm = ev(t_in + M);                    // C x WLD
    static constexpr int t_fv = wm + C * WLD;                  // C
    static constexpr int qp_V = t_fv + C + C + K;              // kQpLd (the row a drop step passes through LDS; behind the cascade's t_wacc, t_cl)
    static constexpr int qp_x = qp_V + kQpLd;
    static constexpr int qp_end = qp_x + kQpLd;
    // ---- stage 1
    static constexpr int c_Y = RG;                             // N x C, dead once Jbar^T is written
    static constexpr int RX = max2(c_Y + C * ev(N), ev(qp_end));
    static_assert(c_Y + C * N <= RX, "Y ends before the small-inverse block");
    static constexpr int c_s1 = RX;                            // max(C x K, 64): small-inverse scratch, sweep column (one double per lane)
    static_assert(c_s1 % 2 == 0, "the sweep column is read in 16-byte pieces");
    static constexpr int c_s2 = c_s1 + max2(C * K, 64);        // C x C: input of the small inverses, the four 6 x 6 blocks of NwJw
    static constexpr int c_Lam = c_s2;
    static constexpr int fn = c_s2;                            // C x FLD: Jbar[:, 6:] [tau_in | NwJw], world frame, kept for the wrench outputs
    static constexpr int RXend = c_s2 + C * C;
    static_assert(4 * K * K <= C * C, "JV, G^-1, B and S of the NwJw closed form");
    static_assert(C * FLD <= C * C, "FN borrows the input block of the small inverses");
    static_assert(qp_end <= fn, "QP scratch must not reach FN");
    static_assert(1 + K <= FLD && 1 + K <= WLD, "columns of the wrench maps");
    static constexpr int total = max2(RXend, max2(k_A + N * (N + 1) / 2, k_Ic + NB * 10));
    static_assert(k_Ic + NB * 10 <= total && k_A + N * (N + 1) / 2 <= total, "stage-0 scratch");
    static constexpr int total_bytes = total * (int)sizeof(real_t) + 64;
};
// at TOCABI's size this IS the compact map: nothing of the built-in constant-tree kernel moves
#define DWBC_RD_SAME(X) (LdsRd<39, 34>::X == Lds3<39, 34, 1>::X)
static_assert(DWBC_RD_SAME(tg) && DWBC_RD_SAME(PC) && DWBC_RD_SAME(Rc) && DWBC_RD_SAME(Pc) && DWBC_RD_SAME(fs) && DWBC_RD_SAME(comp) && DWBC_RD_SAME(q) &&
                  DWBC_RD_SAME(G) && DWBC_RD_SAME(JbT) && DWBC_RD_SAME(c_JC) && DWBC_RD_SAME(k_S) && DWBC_RD_SAME(k_F) && DWBC_RD_SAME(NwJw) && DWBC_RD_SAME(Rw) &&
                  DWBC_RD_SAME(pw) && DWBC_RD_SAME(aw) && DWBC_RD_SAME(Rw0) && DWBC_RD_SAME(c_Vb) && DWBC_RD_SAME(k_Iw) && DWBC_RD_SAME(k_Ic) && DWBC_RD_SAME(k_Rl) &&
                  DWBC_RD_SAME(k_anc) && DWBC_RD_SAME(k_A) && DWBC_RD_SAME(wm) && DWBC_RD_SAME(t_fv) && DWBC_RD_SAME(qp_V) && DWBC_RD_SAME(qp_x) && DWBC_RD_SAME(c_Y) &&
                  DWBC_RD_SAME(c_s1) && DWBC_RD_SAME(c_s2) && DWBC_RD_SAME(c_Lam) && DWBC_RD_SAME(total) && LdsRd<39, 34>::t_in == Lds3<39, 34, 1>::t_base,
              "LdsRd<39, 34> is Lds3<39, 34, 1>");
#undef DWBC_RD_SAME

// ---- gravity compensation (GRAV = true): RobotData::CalcGravCompensation, reference include/dwbc.h:246-247, src/dwbc.cpp:875-889,
// src/wbd.cpp:186-192 -- torque_grav_ = W^+ (A^-1 N_c G)[6:] without W or W^+.  W^+ a is constrained inverse dynamics, and
// for a = G it collapses onto the blocks stage 1 holds, because Lambda_c (J_C A^-1 G) IS P_C.  With J_Cb / J_Cj the base / joint columns of J_C:
//     cv = G_b - J_Cb^T P_C        y = (J_Cb^T J_Cb)^-1 cv       E = P_C + J_Cb y     (the contact wrench that balances the base rows; min norm)
//     tau_any = G_j - J_Cj^T E     torque_grav_ = tau_any - Vb (Vb^T Vb)^-1 Vb^T tau_any   (two contacts: off the internal-wrench torques)
// The launch has two forms.  Gravity only (GravIO::tau_in == nullptr): torque_grav_ and getContactForce(torque_grav_); NwJw and the QP are
// skipped by a wave-uniform branch.  With a torque input: the redistribution below runs on torque_grav_ + tau_in, and torque_grav_ is
// written as well.  No contact: torque_grav_ = 0 exactly (G = 9.81 A[2, :], so G_j - A_jb A_bb^-1 G_b = 0).
// Device pointers of such a launch; the kernel's own argument struct beside BatchIO (RedistIO keeps its layout)
struct GravIO {
    const io_t *tau_in;  // B x M   command on top of gravity compensation, or nullptr: gravity only
    io_t *rd_tau, *rd_cf, *rd_wrench;  // the redistribution's outputs as RedistIO has them (never written without tau_in)
    int *rd_status;
    io_t *tau;           // B x M   torque_grav_
    io_t *wrench;        // B x 12  getContactForce(torque_grav_), zero padded
    int *status;         // B       1 ok / 0: more flags than the capacity, or a failed contact stage
};

// Tenants of the gravity stage on LdsRd: every one moves into a block that is dead between P_C and NwJw, so the map and its bytes are
// LdsRd's at every size (region : what it held : the tenant)
//   tg    : zeros of stage 0 (the cycle's gravity torque)  : torque_grav_, to the end
//   tt    : zeros of stage 0                               : tau_any
//   c_Y   : Y = J_C A^-1, dead once Jbar^T is written      : J_C^T formed again (Jbar^T stands where stage 1 formed it)
//   c_s1  : small-inverse scratch                          : cv, y, E, Vb^T tau_any and its solve (36 doubles)
//   c_s2  : Lambda_c, dead once Jbar^T is written          : J_Cb^T J_Cb, Vb^T Vb and their inverses (4 x 36)
//   fn    : column 7 of FN (padding of the 1 + K columns)  : Jbar[:, 6:] torque_grav_
template <int N, int NB>
struct LdsGc : LdsRd<N, NB> {
    using R = LdsRd<N, NB>;
    static constexpr int g_tau = R::tg, g_any = R::tt, g_JC = R::c_Y, g_v = R::c_s1, g_Q = R::c_s2;
    static constexpr int g_col = R::FLD - 1;  // column of FN
    static_assert(g_JC + R::C * N <= R::RX, "J_C again where Y was");
    static_assert(36 <= R::c_s2 - R::c_s1 && 4 * 36 <= R::C * R::C, "vectors and 6 x 6 blocks of the gravity stage");
    static_assert(g_col > R::K, "the padding column of FN");
};

template <int N, int NB, int NT, class Topo, bool GRAV = false>
DWBC_DEV void redistribute_instance(Thr th, const Setup &su, const BatchIO &io, const RedistIO &rio, int inst, real_t *L, const GravIO *gio = nullptr) {
    using S = LdsRd<N, NB>;
    const bool has_in = !GRAV || rio.tau_in != nullptr;  // (the plain build: a constant)
    constexpr bool kExtras = false;
    constexpr int M = S::M, C = S::C, WLD = S::WLD, FLD = S::FLD;
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

    PLA(real_t, s, N);  // column `lane` of A -> A^-1
    PL(real_t, dg);     // its diagonal element

#include "dwbc_cycle2_stage0.inc"

    // ================= stage 1: contacts (dwbc.h:432-474, dwbc.cpp:433-478, wbd.cpp:108-143), without A^-1 N_c =================
    const unsigned char *fl = io.flags + (size_t)inst * su.n_contacts;
    int act_c[kMaxActiveContacts] = {0, 0};
    int nc = 0, nflag = 0;
    for (int i = 0; i < su.n_contacts; i++) {
        if (fl[i] && nc < kMaxActiveContacts) act_c[nc++] = i;
        nflag += fl[i] ? 1 : 0;
    }
    const bool too_many = nflag > kMaxActiveContacts;  // as the cycle: never solved with a subset, the instance fails
    if (too_many) st_contact = 0;
    const int cd = 6 * nc, k = cd > 6 ? cd - 6 : 0;
    DWBC_SYNC();
    for (int a = 0; a < nc; a++) {
        const int ci = act_c[a], link = su.c_link[ci];
        const real_t *R = L + S::Rw + link * 9;
        for (int r = th.tid; r < 12; r += NT) {
            if (r < 9) L[S::Rc + a * 9 + r] = R[r];
            else {
                const int x = r - 9;
                L[S::Pc + a * 3 + x] = L[S::pw + link * 3 + x] + R[x * 3] * su.c_point[ci][0] + R[x * 3 + 1] * su.c_point[ci][1] + R[x * 3 + 2] * su.c_point[ci][2];
            }
        }
    }
    for (int r = th.tid; r < 9; r += NT) L[S::Rw0 + r] = L[S::Rw + r];  // pelvis rotation for the base columns of the point Jacobians
    DWBC_SYNC();
    // J_C and Y = J_C A^-1 TRANSPOSED in LDS (N x C), as in the cycle; Jbar^T (C x N) is written over J_C once Y and Lambda_c are done
    real_t *JCt = L + S::c_JC, *Yt = L + S::c_Y, *Lam = L + S::c_Lam, *JbT = L + S::JbT, *Vb = L + S::c_Vb;
    for (int idx = th.tid; idx < C * N; idx += NT) { JCt[idx] = real_t(0.0); Yt[idx] = real_t(0.0); }
    DWBC_SYNC();
    for (int a = 0; a < nc; a++)
        point_jacobian<N, NB, NT>(th, L + S::Rw0, L + S::pw, L + S::aw, topo, nb, su.c_link[act_c[a]], L + S::Pc + a * 3, JCt, 1, 6 * a, 6, 0, C);
    DWBC_SYNC();
    if (k > 0) internal_wrench_basis<N, NT>(th, L + S::Pc, JCt, Vb);  // the only later reader of J_C
    DWBC_SYNC();
    const unsigned long long cm0 = nc > 0 ? su.c_dofmask[act_c[0]] : 0ull, cm1 = nc > 1 ? su.c_dofmask[act_c[1]] : 0ull;
    static_assert(C == 12, "two 6D contacts");
    LANES {
        real_t yc[C];
#pragma unroll
        for (int p = 0; p < C; p++) yc[p] = real_t(0.0);
#pragma unroll
        for (int ib = 0; ib < N; ib += 3) {  // one uniform branch per 3 columns and contact: the zero columns of J_C are skipped
            if ((cm0 >> ib) & 7) {
#pragma unroll
                for (int i = ib; i < ib + 3 && i < N; i++)
#pragma unroll
                    for (int p = 0; p < 6; p++) yc[p] += JCt[i * C + p] * LV(s)[i];
            }
            if ((cm1 >> ib) & 7) {
#pragma unroll
                for (int i = ib; i < ib + 3 && i < N; i++)
#pragma unroll
                    for (int p = 6; p < C; p++) yc[p] += JCt[i * C + p] * LV(s)[i];
            }
        }
        if (lane < N) {
#pragma unroll
            for (int p = 0; p < C; p++) Yt[lane * C + p] = yc[p];
        }
    }
    DWBC_SYNC();
    // J A^-1 J^T = Y J_C^T in a C x C block, zero outside cd x cd (contact_gram, dwbc_cycle2.h: the tile stage 1 of the cycle takes)
    contact_gram<N, C, NT, S::c_s2>(th, Yt, JCt, cd, L);
    if (cd > 0) {
        if (!spd_inverse_small(L + S::c_s2, C, cd, Lam, C, L + S::c_s1)) st_contact = 0;  // Lambda_c (wbd.cpp:115)
    }
    DWBC_SYNC();
    // Jbar^T = Lambda_c J A^-1 (wbd.cpp:116) over J_C; the columns of A^-1 are dead after this
    LANES {
        real_t yc[C], jb[C];
        const int col = lane < N ? lane : 0;
#pragma unroll
        for (int p = 0; p < C; p++) yc[p] = Yt[col * C + p];
        lds_rows_dot<C, C, C, 4, 0, false>(Lam, yc, jb);
#pragma unroll
        for (int p = 0; p < C; p++)
            if (lane < N && p < cd) JbT[p * N + lane] = jb[p];
    }
    DWBC_SYNC();
    mv_n<NT>(th, L + S::PC, JbT, N, L + S::G, cd, N);  // P_C = Jbar^T G (wbd.cpp:192)
    DWBC_SYNC();

    if constexpr (GRAV) {
        // ================= torque_grav_ (wbd.cpp:186-191) from P_C, J_C and Vb: see above GravIO =================
        using Sg = LdsGc<N, NB>;
        real_t *JC2 = L + Sg::g_JC, *gv = L + Sg::g_v, *gq = L + Sg::g_Q, *tgv = L + Sg::g_tau, *tany = L + Sg::g_any;
        real_t *cv = gv, *yv = gv + 6, *Ev = gv + 12, *wv = gv + 24, *zv = gv + 30;
        const real_t *Gv = L + S::G, *PCv = L + S::PC;
        if (nc > 0 && st_contact) {
            for (int idx = th.tid; idx < C * N; idx += NT) JC2[idx] = real_t(0.0);
            DWBC_SYNC();
            for (int a = 0; a < nc; a++)
                point_jacobian<N, NB, NT>(th, L + S::Rw0, L + S::pw, L + S::aw, topo, nb, su.c_link[act_c[a]], L + S::Pc + a * 3, JC2, 1, 6 * a, 6, 0, C);
            DWBC_SYNC();
            for (int idx = th.tid; idx < 42; idx += NT) {  // J_Cb^T J_Cb (6 x 6) and cv
                if (idx < 36) {
                    const int r = idx / 6, c = idx - r * 6;
                    real_t acc = real_t(0.0);
                    for (int p = 0; p < cd; p++) acc += JC2[r * C + p] * JC2[c * C + p];
                    gq[idx] = acc;
                } else {
                    const int r = idx - 36;
                    real_t acc = Gv[r];
                    for (int p = 0; p < cd; p++) acc -= JC2[r * C + p] * PCv[p];
                    cv[r] = acc;
                }
            }
            DWBC_SYNC();
            if (!spd_inverse_small(gq, 6, 6, gq + 36, 6, gv + 36)) st_contact = 0;
            mv_n<NT>(th, yv, gq + 36, 6, cv, 6, 6);
            DWBC_SYNC();
            for (int p = th.tid; p < cd; p += NT) {
                real_t acc = PCv[p];
#pragma unroll
                for (int r = 0; r < 6; r++) acc += JC2[r * C + p] * yv[r];
                Ev[p] = acc;
            }
            DWBC_SYNC();
            real_t *tdst = k > 0 ? tany : tgv;
            for (int j = th.tid; j < M; j += NT) {
                real_t acc = Gv[6 + j];
                for (int p = 0; p < cd; p++) acc -= JC2[(6 + j) * C + p] * Ev[p];
                tdst[j] = acc;
            }
            DWBC_SYNC();
            if (k > 0) {
                mm_tn<NT>(th, gq + 72, 6, Vb, 6, Vb, 6, 6, M, 6);  // Vb^T Vb
                for (int a = th.tid; a < 6; a += NT) {
                    real_t acc = real_t(0.0);
                    _Pragma("unroll 8")
                    for (int j = 0; j < M; j++) acc += Vb[j * 6 + a] * tany[j];
                    wv[a] = acc;
                }
                DWBC_SYNC();
                if (!spd_inverse_small(gq + 72, 6, 6, gq + 108, 6, gv + 36)) st_contact = 0;
                mv_n<NT>(th, zv, gq + 108, 6, wv, 6, 6);
                DWBC_SYNC();
                for (int j = th.tid; j < M; j += NT) {
                    real_t acc = tany[j];
#pragma unroll
                    for (int a = 0; a < 6; a++) acc -= Vb[j * 6 + a] * zv[a];
                    tgv[j] = acc;
                }
                DWBC_SYNC();
            }
        }
    }

    // ================= NwJw from the closed-form internal-wrench basis (see dwbc_cycle2.h): NwJw = Vb G^-1 X^T, X = S^-1 JV =================
    if (k > 0 && has_in) {
        static_assert(kMaxActiveContacts == 2, "k in {0, 6}");
        constexpr int K6 = 6;
        for (int idx = th.tid; idx < K6 * K6; idx += NT) {
            const int i = idx / 6, j = idx - i * 6;
            real_t acc = real_t(0.0);
            _Pragma("unroll 8")
            for (int c = 0; c < M; c++) acc += JbT[i * N + 6 + c] * Vb[c * K6 + j];
            L[S::c_s2 + idx] = acc;
        }
        real_t *JV = L + S::c_s2, *Gi = L + S::c_s2 + 36, *Bm = L + S::c_s2 + 72, *Sm6 = L + S::c_s2 + 108;  // 4 x (6 x 6) in C * C
        mm_tn<NT>(th, Gi, K6, Vb, K6, Vb, K6, K6, M, K6);                  // G = Vb^T Vb
        DWBC_SYNC();
        spd_inverse_small(Gi, K6, K6, Gi, K6, L + S::c_s1);                // G^-1
        mm_nn<NT>(th, Bm, K6, JV, K6, Gi, K6, K6, K6, K6);                 // B = JV G^-1
        DWBC_SYNC();
        mm_nt<NT>(th, Sm6, K6, Bm, K6, JV, K6, K6, K6, K6);                // S = B JV^T (SPD)
        DWBC_SYNC();
        if (!spd_inverse_small(Sm6, K6, K6, Sm6, K6, L + S::c_s1)) st_contact = 0;
        mm_nn<NT>(th, Bm, K6, Sm6, K6, JV, K6, K6, K6, K6);                // X = S^-1 JV
        DWBC_SYNC();
        mm_nt<NT>(th, JV, K6, Gi, K6, Bm, K6, K6, K6, K6);                 // G^-1 X^T (JV is dead)
        DWBC_SYNC();
        mm_nn<NT>(th, L + S::NwJw, K6, Vb, K6, JV, K6, M, K6, K6);         // NwJw = Vb (G^-1 X^T)
        DWBC_SYNC();
    }

    // ================= the wrench maps of [tau_in | NwJw] and the QP (dwbc.cpp:1458-1517) =================
    const io_t *tin_g = rio.tau_in + (size_t)inst * M;
    real_t *tin = L + S::t_in, *FN = L + S::fn, *WM = L + S::wm, *fv = L + S::t_fv;
    if constexpr (GRAV) {  // the torque that is redistributed: torque_grav_ + the command (gravity only: torque_grav_)
        for (int i = th.tid; i < M; i += NT) tin[i] = L[LdsGc<N, NB>::g_tau + i] + (has_in ? (real_t)tin_g[i] : real_t(0.0));
    } else
    for (int i = th.tid; i < M; i += NT) tin[i] = (real_t)tin_g[i];
    DWBC_SYNC();
    const int ncol = has_in ? 1 + k : 1;
    constexpr int gcol = GRAV ? LdsGc<N, NB>::g_col : -1;  // the wrench map of torque_grav_ alone, in the padding column of FN
    for (int idx = th.tid; idx < cd * FLD; idx += NT) {
        const int i = idx / FLD, col = idx - i * FLD;
        real_t acc = real_t(0.0);
        if (col < ncol || col == gcol) {
            const real_t *rhs = col == 0 ? tin : col == gcol ? L + S::tg : L + S::NwJw + (col - 1);
            const int rs = (col == 0 || col == gcol) ? 1 : 6;
            _Pragma("unroll 8")
            for (int c = 0; c < M; c++) acc += JbT[i * N + 6 + c] * rhs[c * rs];
        }
        FN[idx] = acc;
    }
    DWBC_SYNC();
    // contact-local frames for the cone rows: WM = A_rot FN, fv = A_rot (FN[:, 0] - P_C), A_rot = blockdiag(R_a^T, R_a^T)
    for (int idx = th.tid; idx < cd * FLD; idx += NT) {
        const int i = idx / FLD, col = idx - i * FLD;
        const int a = i / 6, h = (i % 6) / 3, x = i % 3;
        const real_t *R = L + S::Rc + a * 9;
        const real_t *src = FN + (6 * a + 3 * h) * FLD + col;
        const real_t v = R[x] * src[0] + R[3 + x] * src[FLD] + R[6 + x] * src[2 * FLD];
        WM[i * WLD + col] = v;
        if (col == 0) {
            const real_t *pc3 = L + S::PC + 6 * a + 3 * h;
            fv[i] = v - (R[x] * pc3[0] + R[3 + x] * pc3[1] + R[6 + x] * pc3[2]);
        }
    }
    DWBC_SYNC();
    int st_redis = 1;
    real_t xq[6] = {real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0)};
    if (k > 0 && st_contact && has_in) {
        const int nlim = su.has_tau_lim ? 2 * M : 0, ncone = 10 * nc;
        QpResult qres;
        PL(real_t, sfin);
        // x = c (k), H = I: rows [NwJw] against the torque limits, cone(WM[:, 1:]) against cone(fv); no second block
        qp_rows_and_solve<N, NB, 0>(su, L, nlim, ncone, act_c[0], act_c[1], L + S::NwJw, 6, k, L + S::NwJw, 6, 0, real_t(1.0), WM + 1, WLD, WM + 1, WLD,
                                    fv, tin, k, su.qp_max_iter_contact, qres, L + S::qp_V, L + S::qp_x, nullptr, nullptr, kQpFeasTol, sfin, io.inst_par, inst);
        if (qres.status) {
#pragma unroll
            for (int j = 0; j < 6; j++) xq[j] = j < k ? L[S::qp_x + j] : real_t(0.0);
        } else {
            st_redis = 0;  // dwbc.cpp:1553-1559: zero torque
        }
    }

    // ================= outputs =================
    const bool ok = st_contact && st_redis;
    if constexpr (GRAV) {
        io_t *gt = gio->tau + (size_t)inst * M;
        for (int i = th.tid; i < M; i += NT) gt[i] = st_contact ? L[LdsGc<N, NB>::g_tau + i] : real_t(0.0);
        io_t *gw = gio->wrench + (size_t)inst * 12;
        for (int i = th.tid; i < 12; i += NT) gw[i] = (i < cd && st_contact) ? FN[i * FLD + gcol] - L[S::PC + i] : real_t(0.0);  // wbd.cpp:268-271
        if (th.tid == 0) gio->status[inst] = st_contact ? 1 : 0;
        if (!has_in) return;
    }
    io_t *tau = rio.tau + (size_t)inst * M;
    for (int i = th.tid; i < M; i += NT) {
        real_t c = real_t(0.0);
        if (k > 0 && ok) {
#pragma unroll
            for (int j = 0; j < 6; j++) c += L[S::NwJw + i * 6 + j] * xq[j];  // NwJw c (dwbc.cpp:1549)
        }
        tau[i] = c;
    }
    io_t *cf = rio.cf + (size_t)inst * 6;
    for (int j = th.tid; j < 6; j += NT) {
        real_t v = real_t(0.0);
#pragma unroll
        for (int a = 0; a < 6; a++) v = (a == j) ? xq[a] : v;
        cf[j] = ok ? v : real_t(0.0);
    }
    // getContactForce(tau) = Jbar[:, 6:] tau - P_C (wbd.cpp:268-271) for tau_in and for tau_in + NwJw c: columns of FN
    io_t *wr = rio.wrench + (size_t)inst * 24;
    for (int i = th.tid; i < 12; i += NT) {
        real_t w0 = real_t(0.0), w1 = real_t(0.0);
        if (i < cd && st_contact) {
            w0 = FN[i * FLD] - L[S::PC + i];
            w1 = w0;
#pragma unroll
            for (int j = 0; j < 6; j++) w1 += (j < k) ? FN[i * FLD + 1 + j] * xq[j] : real_t(0.0);
        }
        wr[i] = w0;
        wr[12 + i] = w1;
    }
    if (th.tid == 0) rio.status[inst] = ok ? 1 : 0;
}

}  // namespace dwbc
