// dwbc_contact_space.h -- the contact space of RobotData::SetContact + CalcContactConstraint (reference include/dwbc.h:432-474,
// src/dwbc.cpp:433-478, src/wbd.cpp:108-143) in a launch of its own, one wavefront per instance: what a caller reads off RobotData
// between UpdateKinematics and SetTaskSpace --
//   J_C (dwbc.cpp:445-453)   Lambda_contact (wbd.cpp:115)   J_C_INV_T (:116)   N_C (:117)   A_inv_N_C (:118)   W (:119)
//   W_inv (:124, :140)   NwJw (:128)   cc_[i].xc_pos / rotm
// -- written to buffers of their own, selected by a mask.  It is the front of the one-wave kernels and nothing behind it:
//   stage 0 (dwbc_cycle2_stage0.inc up to the column-per-lane load, shared text)   kinematics, CRBA, A in register columns
//   A^-1 (sweep_inverse_tree, dwbc_cycle2.h)                                       the register sweep of the dynamics kernel (see there and below)
//   contact stage (the text of dwbc_redistribute.h, which is dwbc_cycle2_stage1.inc without the gravity vectors and the task points)
//                                                                                  active contacts, J_C, Y = J_C A^-1, Lambda_c, Jbar^T
//   N_C = I - J_C^T Jbar^T                                                         column `lane` from the lane's column of Jbar^T, while J_C stands
//   s <- A^-1 N_c                                                                  the register columns, as stage 1 of the cycle updates them
//   G^-1 = (Vb^T Vb)^-1, NwJw                                                      closed form from the internal-wrench basis (dwbc_redistribute.h)
//   W^+ = (W + alpha P)^-1 - P / alpha                                             the 33-pivot sweep of the cycle (dwbc_cycle2.h); k = 0: a plain inverse
// Every step sits behind a wave-uniform branch on the mask (a kernel argument):
//   only J_C and / or the contact frames      no A^-1 sweep, nothing behind J_C
//   no A_INV_N_C, W, W_INV                    the columns stay A^-1 (the redistribution kernel's situation)
//   no W_INV                                  no W + alpha P, no 33-pivot sweep
//   neither NWJW nor W_INV                    no internal-wrench basis (W^+ needs the projector P = Vb G^-1 Vb^T on two contacts; without
//                                             NWJW the closed form stops behind G^-1)
//   no N_C                                    no n x n product
// No task level, no gravity vector, no QP; of BatchIO it reads q, flags, body and topo, of Setup the tree and the contacts.
#pragma once
#include "dwbc_redistribute.h"

namespace dwbc {

// bits of CsIO::mask: 1u << dwbc_contact_space_output (include/dwbc_batch.h; dwbc_capi.hip asserts the two agree)
enum : unsigned {
    kCsJC = 1u << 0, kCsLambda = 1u << 1, kCsJCInvT = 1u << 2, kCsNC = 1u << 3, kCsAInvNC = 1u << 4, kCsW = 1u << 5, kCsWInv = 1u << 6,
    kCsNwJw = 1u << 7, kCsPos = 1u << 8, kCsRot = 1u << 9
};
constexpr unsigned kCsNeedsCols = kCsAInvNC | kCsW | kCsWInv;                                   // s <- A^-1 N_c
constexpr unsigned kCsNeedsLambda = kCsLambda | kCsJCInvT | kCsNC | kCsNwJw | kCsNeedsCols;      // the A^-1 sweep, Y, Lambda_c, Jbar^T
constexpr unsigned kCsNeedsBasis = kCsNwJw | kCsWInv;                                           // Vb and G^-1

// device pointers of a contact-space launch, batch-major; the kernel's own argument struct beside BatchIO (whose layout is pack ABI and
// stays).  A pointer whose bit is clear is never dereferenced.  Every shape is fixed, whatever the support: zero beyond the active cd.
struct CsIO {
    unsigned mask;
    io_t *J_C;        // B x 12 x N
    io_t *Lambda_c;   // B x 12 x 12, row stride 12
    io_t *J_C_INV_T;  // B x 12 x N
    io_t *N_C;        // B x N x N
    io_t *A_inv_N_C;  // B x N x N
    io_t *W;          // B x M x M
    io_t *W_inv;      // B x M x M
    io_t *NwJw;       // B x M x 6
    io_t *pos;        // B x 2 x 3   in the order of the active contacts
    io_t *rot;        // B x 2 x 9
    int *status;      // B           always written: 0 = more flags than two, a failed Lambda_c or a bad pivot of the W sweep (every
                      //             asked-for output of the instance is then zero)
};

// LDS map: LdsRd's (dwbc_redistribute.h) -- stage 0 and the contact stage are the same text, and every region there is as large as the
// largest of its tenants at every size -- with this kernel's tenants in blocks that are dead when they move in (region : what it held :
// the tenant):
//   G            : G_, which nothing here reads                         : the diagonal of W (alpha), M doubles
//   c_Vb + M K   : (G^-1 of the cycle: the redistribution leaves it)    : G^-1 = (Vb^T Vb)^-1, 36 doubles, for the projector of W^+
//   NwJw, FNl, U : nothing yet (NwJw is formed later), dead link rotations      : the Gram matrix J A^-1 J^T and G X - I of the Newton step on Lambda_c
//   0 .. M ev(M) : everything below c_s1, dead once P is in registers   : W, then W^+, row-major, for the Newton step on W^+
//   c_s1         : small-inverse scratch                                : the pivot column of the W sweep (64 doubles)
//   JbT / c_JC   : J_C, then Jbar^T over it                             : J_C is written out and N_C formed before the overwrite
// Bytes (N / NB: total_bytes) are LdsRd's:  23 / 18: 12 880    37 / 32: 19 488    39 / 34: 20 432    43 / 38: 22 320    50 / 45: 26 792
template <int N, int NB>
struct LdsCs : LdsRd<N, NB> {
    using R = LdsRd<N, NB>;
    static constexpr int c_Gi = R::c_Vb + R::M * R::K;  // K x K
    static constexpr int c_col = R::G;                  // M
    static constexpr int c_Gm = R::NwJw;                // C x C: the Gram matrix J A^-1 J^T beside its inverse, before NwJw is formed
    static_assert(c_Gm + 2 * R::C * R::C <= R::RE, "the Gram matrix and the residual of the Newton step in the NwJw, FNl and U blocks (the link rotations are dead)");
    static constexpr int c_Ws = 0, w_rs = R::ev(R::M);   // M x ev(M): W, then W^+, staged for the Newton step behind the W sweep
    static_assert(c_Ws + R::M * w_rs <= R::c_s1, "the staged W ends below the pivot column of the W sweep");
    static_assert(c_Gi + R::K * R::K <= R::RG && R::RG <= R::c_Y, "G^-1 sits between Vb and Y");
    static_assert(R::M <= N, "the diagonal of W where G_ was");
    static_assert(R::c_s2 - R::c_s1 >= 64, "the pivot column of the W sweep");
    static_assert(R::K == 6 && 4 * 36 <= R::C * R::C, "the four 6 x 6 blocks of the NwJw closed form");
    static_assert(R::c_JC == R::JbT, "Jbar^T is written over J_C: J_C and N_C leave first");
};

template <int N, int NB, int NT, class Topo>
DWBC_DEV void contact_space_instance(Thr th, const Setup &su, const BatchIO &io, const CsIO &cio, int inst, real_t *L) {
    using S = LdsCs<N, NB>;
    constexpr bool kExtras = false;
    constexpr int M = S::M, C = S::C;
    DWBC_LANE_DECL;
    constexpr bool kTree = !std::is_same<Topo, TopoGeneric>::value;
    const int nb = kTree ? NB : su.nb;
    const real_t *body = io.body;
    const int *topo = io.topo;  // parent[nb] depth[nb] subtree[nb]
    const io_t *qin = io.q + (size_t)inst * (N + 1);
    const DumpLayout dl = DumpLayout::make(N);
    real_t *dump = nullptr;  // no dump record, no diagnostics: the cycle's stay as its last launch left them
    int *diag = nullptr;
    DWBC_STAMP_INIT();
    const unsigned mask = cio.mask;

    PLA(real_t, s, N);  // column `lane` of A -> A^-1 -> A^-1 N_c
    PL(real_t, dg);     // its diagonal element

#define DWBC_STAGE0_FRONT_ONLY
#include "dwbc_cycle2_stage0.inc"
#undef DWBC_STAGE0_FRONT_ONLY

    io_t *o_JC = cio.J_C + (size_t)inst * C * N, *o_Lam = cio.Lambda_c + (size_t)inst * C * C, *o_JbT = cio.J_C_INV_T + (size_t)inst * C * N;
    io_t *o_NC = cio.N_C + (size_t)inst * N * N, *o_AiNc = cio.A_inv_N_C + (size_t)inst * N * N, *o_W = cio.W + (size_t)inst * M * M;
    io_t *o_Wi = cio.W_inv + (size_t)inst * M * M, *o_Nw = cio.NwJw + (size_t)inst * M * 6;
    io_t *o_pos = cio.pos + (size_t)inst * kMaxActiveContacts * 3, *o_rot = cio.rot + (size_t)inst * kMaxActiveContacts * 9;

    // ================= active contacts and their frames (dwbc.h:432-474, dwbc.cpp:433-444) =================
    const unsigned char *fl = io.flags + (size_t)inst * su.n_contacts;
    int act_c[kMaxActiveContacts] = {0, 0};
    int nc = 0, nflag = 0;
    for (int i = 0; i < su.n_contacts; i++) {
        if (fl[i] && nc < kMaxActiveContacts) act_c[nc++] = i;
        nflag += fl[i] ? 1 : 0;
    }
    if (nflag > kMaxActiveContacts) { st_contact = 0; nc = 0; }  // as the cycle: never solved with a subset, the instance fails
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
    if (mask & kCsPos)
        for (int r = th.tid; r < kMaxActiveContacts * 3; r += NT) o_pos[r] = (r < 3 * nc) ? L[S::Pc + r] : real_t(0.0);
    if (mask & kCsRot)
        for (int r = th.tid; r < kMaxActiveContacts * 9; r += NT) o_rot[r] = (r < 9 * nc) ? L[S::Rc + r] : real_t(0.0);

    // ================= J_C (dwbc.cpp:445-453), TRANSPOSED in LDS (N x C) as in the cycle =================
    real_t *JCt = L + S::c_JC, *Yt = L + S::c_Y, *Lam = L + S::c_Lam, *JbT = L + S::JbT, *Vb = L + S::c_Vb;
    if (mask & (kCsJC | kCsNeedsLambda)) {
        for (int idx = th.tid; idx < C * N; idx += NT) { JCt[idx] = real_t(0.0); Yt[idx] = real_t(0.0); }
        DWBC_SYNC();
        for (int a = 0; a < nc; a++)
            point_jacobian<N, NB, NT>(th, L + S::Rw0, L + S::pw, L + S::aw, topo, nb, su.c_link[act_c[a]], L + S::Pc + a * 3, JCt, 1, 6 * a, 6, 0, C);
        DWBC_SYNC();
        if (mask & kCsJC)
            for (int idx = th.tid; idx < C * N; idx += NT) o_JC[idx] = JCt[(idx % N) * C + idx / N];
        if ((mask & kCsNeedsBasis) && k > 0) internal_wrench_basis<N, NT>(th, L + S::Pc, JCt, Vb);  // the only later reader of J_C
        DWBC_SYNC();
    }

    if ((mask & kCsNeedsLambda) && st_contact) {
        // ================= A_inv (dwbc.cpp:307): tree-sparse on a constant tree, dense leaves-first on any tree =================
        {
            using SweepTopo = typename std::conditional<kTree, Topo, TopoDense<N>>::type;
            // The register sweep (pivot column by v_readlane), as in the dynamics kernel, not the LDS-fed one of the redistribution kernel:
            // that one carries the diagonal shifted by two and leaves A^-1 less symmetric, which J_C (A^-1 N_c) = 0 shows -- Y = J_C A^-1 is
            // formed from the columns, Lambda_c from Y J_C^T.  On an MI355X, TOCABI: 1.8e-14 against a bar of 1.8e-14 (ten times the
            // restatement's 1.8e-15) with the LDS-fed sweep, 2.1e-15 with this one.  DWBC_CS_LDS_SWEEP (development) builds the other.
#ifdef DWBC_CS_LDS_SWEEP
            DWBC_SYNC();
            if (!sweep_inverse_tree_lds<SweepTopo, N>(s, dg, L + S::c_s1)) st_contact = 0;
            DWBC_SYNC();
#else
            if (!sweep_inverse_tree<SweepTopo, N>(s, dg)) st_contact = 0;
            DWBC_SYNC();
#endif
        }
        // ================= Y = J_C A^-1, Lambda_c, Jbar^T (wbd.cpp:115-116) =================
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
        // J A^-1 J^T = Y J_C^T in a C x C block, zero outside cd x cd (contact_gram, dwbc_cycle2.h); Lambda_c in place
        contact_gram<N, C, NT, S::c_s2>(th, Yt, JCt, cd, L);
        if (cd > 0) {
            // A caller of this launch reads Lambda_c and Jbar^T themselves and multiplies them back: one Newton step on the sweep's inverse,
            // X <- X - X (G X - I) with the Gram matrix G kept aside, brings |Jbar^T J_C^T - I| and |N_C N_C - N_C| from 3 - 5e-14 down to the
            // level of an LU inverse (host emulation, TOCABI; the cycle, which only multiplies Lambda_c on, does without)
            real_t *Gm = L + S::c_Gm;
            for (int idx = th.tid; idx < C * C; idx += NT) Gm[idx] = L[S::c_s2 + idx];
            if (!spd_inverse_small(L + S::c_s2, C, cd, Lam, C, L + S::c_s1)) st_contact = 0;
            DWBC_SYNC();
            real_t *Eb = Gm + C * C;
            for (int idx = th.tid; idx < C * C; idx += NT) {  // E = G X - I
                const int i = idx / C, j = idx - i * C;
                real_t acc = (i == j) ? real_t(-1.0) : real_t(0.0);
#pragma unroll
                for (int c = 0; c < C; c++) acc += Gm[i * C + c] * Lam[c * C + j];
                Eb[idx] = acc;
            }
            DWBC_SYNC();
            for (int idx = th.tid; idx < C * C; idx += NT) {  // X - X E, beside X
                const int i = idx / C, j = idx - i * C;
                real_t acc = Lam[idx];
#pragma unroll
                for (int c = 0; c < C; c++) acc -= Lam[i * C + c] * Eb[c * C + j];
                Gm[idx] = acc;
            }
            DWBC_SYNC();
            for (int idx = th.tid; idx < C * C; idx += NT) Lam[idx] = Gm[idx];
        }
        DWBC_SYNC();
        if (mask & kCsLambda)
            for (int idx = th.tid; idx < C * C; idx += NT) o_Lam[idx] = Lam[idx];
        // column `lane` of Jbar^T = Lambda_c Y in registers; N_C = I - J_C^T Jbar^T (wbd.cpp:117) from it while J_C stands
        PLA(real_t, jb, C);
        LANES {
            real_t yc[C];
            const int col = lane < N ? lane : 0;
#pragma unroll
            for (int p = 0; p < C; p++) yc[p] = Yt[col * C + p];
            lds_rows_dot<C, C, C, 4, 0, false>(Lam, yc, LV(jb));
            if (mask & kCsNC) {
                DWBC_LANE_OPAQUE(ln);
#pragma unroll 3
                for (int i = 0; i < N; i++) {
                    real_t acc = real_t(0.0);
#pragma unroll
                    for (int p = 0; p < C; p++) acc += JCt[i * C + p] * LV(jb)[p];
                    if (lane < N) o_NC[i * N + lane] = (i == ln ? real_t(1.0) : real_t(0.0)) - acc;
                }
            }
        }
        DWBC_SYNC();
        LANES {
#pragma unroll
            for (int p = 0; p < C; p++)
                if (lane < N) JbT[p * N + lane] = LV(jb)[p];
        }
        DWBC_SYNC();
        if (mask & kCsJCInvT)
            for (int idx = th.tid; idx < C * N; idx += NT) o_JbT[idx] = JbT[idx];

        // ================= A^-1 N_c = A^-1 - Y^T Jbar^T (wbd.cpp:118) in the register columns; W its joint block (:119) =================
        if (mask & kCsNeedsCols) {
            LANES {
                real_t yc[C];
                const int col = lane < N ? lane : 0;
                real_t dsub = real_t(0.0);
#pragma unroll
                for (int p = 0; p < C; p++) { yc[p] = Yt[col * C + p]; dsub += yc[p] * LV(jb)[p]; }
                LV(dg) -= dsub;
                lds_rows_dot<N, C, C, 2, 1, false>(Yt, LV(jb), LV(s));  // s[i] -= Y^T[i, :] . Jbar^T[:, lane]
            }
            if (mask & kCsAInvNC) {
                LANES {
                    if (lane < N) {
#pragma unroll
                        for (int i = 0; i < N; i++) o_AiNc[i * N + lane] = LV(s)[i];
                    }
                }
            }
            if (mask & kCsW) {
                LANES {
                    if (lane >= 6 && lane < N) {
#pragma unroll
                        for (int i = 0; i < M; i++) o_W[i * M + lane - 6] = LV(s)[6 + i];
                    }
                }
            }
        }

        // ================= G^-1 and NwJw (wbd.cpp:128) from the closed-form internal-wrench basis: NwJw = Vb G^-1 X^T, X = S^-1 JV =================
        if ((mask & kCsNeedsBasis) && k > 0) {
            static_assert(kMaxActiveContacts == 2, "k in {0, 6}");
            constexpr int K6 = 6;
            real_t *JV = L + S::c_s2, *Gi = L + S::c_s2 + 36, *Bm = L + S::c_s2 + 72, *Sm6 = L + S::c_s2 + 108;  // 4 x (6 x 6) in C * C (Lambda_c is dead)
            DWBC_SYNC();
            mm_tn<NT>(th, Gi, K6, Vb, K6, Vb, K6, K6, M, K6);                  // G = Vb^T Vb
            DWBC_SYNC();
            if (!spd_inverse_small(Gi, K6, K6, Gi, K6, L + S::c_s1)) st_contact = 0;  // G^-1
            for (int idx = th.tid; idx < K6 * K6; idx += NT) L[S::c_Gi + idx] = Gi[idx];
            DWBC_SYNC();
            if (mask & kCsNwJw) {
                for (int idx = th.tid; idx < K6 * K6; idx += NT) {
                    const int i = idx / 6, j = idx - i * 6;
                    real_t acc = real_t(0.0);
                    _Pragma("unroll 8")
                    for (int c = 0; c < M; c++) acc += JbT[i * N + 6 + c] * Vb[c * K6 + j];
                    JV[idx] = acc;
                }
                DWBC_SYNC();
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
        }
        if (mask & kCsNwJw)
            for (int idx = th.tid; idx < M * 6; idx += NT) o_Nw[idx] = k > 0 ? L[S::NwJw + idx] : real_t(0.0);

        // ================= W^+ = (W + alpha P)^-1 - P / alpha (wbd.cpp:124, :140): the sweep of dwbc_cycle2.h; k = 0: a plain inverse =================
        if (mask & kCsWInv) {
            PLA(real_t, w, M);  // column c of W held by lane c (moved down from lane 6 + c)
            PL(real_t, dw);
            LANES {
                const int src = lane < M ? lane + 6 : lane;
#pragma unroll
                for (int i = 0; i < M; i++) LV(w)[i] = SHFLA(s, 6 + i, src);
                LV(dw) = SHFL(dg, src);
            }
            DWBC_SYNC();
            LANES {
                if (lane < M) L[S::c_col + lane] = LV(dw);
            }
            DWBC_SYNC();
            real_t alpha = real_t(0.0);
            for (int i = 0; i < M; i++) alpha += L[S::c_col + i];
            alpha /= M;
            const real_t ialpha = alpha != real_t(0.0) ? real_t(1.0) / alpha : real_t(0.0);
            DWBC_SYNC();
            PLA(real_t, pc, M);  // column `lane` of the projector P = Vb G^-1 Vb^T: kept in registers across the sweep for the correction
            LANES {
#pragma unroll
                for (int i = 0; i < M; i++) LV(pc)[i] = real_t(0.0);
                if (k > 0) {
                    DWBC_LANE_OPAQUE(lw);
                    real_t dp = real_t(0.0);
                    real_t vbr[6], gv[6] = {real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0)};
#pragma unroll
                    for (int a = 0; a < 6; a++) vbr[a] = lane < M ? Vb[lane * 6 + a] : real_t(0.0);
#pragma unroll
                    for (int b = 0; b < 6; b++)
#pragma unroll
                        for (int a = 0; a < 6; a++) gv[b] += L[S::c_Gi + b * 6 + a] * vbr[a];
                    lds_rows_dot<M, 6, 6, 3, 0, false>(Vb, gv, LV(pc));
#pragma unroll
                    for (int i = 0; i < M; i++) {
                        const real_t pij = LV(pc)[i];
                        LV(w)[i] += alpha * pij;
                        dp = (i == lw) ? pij : dp;
                    }
                    LV(dw) += alpha * dp;
                }
                if (lane >= M) {
#pragma unroll
                    for (int i = 0; i < M; i++) LV(w)[i] = real_t(0.0);
                    LV(dw) = real_t(1.0);
                }
            }
            // W itself goes to LDS for the Newton step behind the sweep (everything below the sweep's pivot column is dead by now): the
            // columns s die here, so that the sweep runs with w and pc alone in registers, as in the cycle
            DWBC_SYNC();
            LANES {
                if (lane >= 6 && lane < N) {
#pragma unroll
                    for (int i = 0; i < M; i++) L[S::c_Ws + i * S::w_rs + lane - 6] = LV(s)[6 + i];
                }
            }
            DWBC_SYNC();
            if (!sweep_inverse_lds<M>(w, dw, L + S::c_s1)) st_contact = 0;
            DWBC_SYNC();
            LANES {
                if (k > 0) {
#pragma unroll
                    for (int i = 0; i < M; i++) LV(w)[i] -= ialpha * LV(pc)[i];
                }
            }
            // One Newton step on the result, X <- X - X (W X - I) (on two contacts, where X = W^+ and W X is a projector: the Ben-Israel
            // step, X (W X - I) = X W X - X).  The sweep eliminates without pivoting, and what it leaves in |W X W - W| grows with the
            // condition of W + alpha P: 1e-9 on the 43-dof model against 1e-11 of the restatement's orthogonal decomposition (host
            // emulation); the step brings it below the restatement's on every model.  W (staged ahead of the sweep), then X in its place, are
            // read back as uniform rows against the lane's own column.
            {
                constexpr int RS = S::w_rs;
                real_t *Ws = L + S::c_Ws;
                PLA(real_t, e, M);
                LANES {
                    DWBC_LANE_OPAQUE(le);
                    lds_rows_dot<M, M, RS, 1, 0, true>(Ws, LV(w), LV(e));  // e = W x_lane
#pragma unroll
                    for (int i = 0; i < M; i++) LV(e)[i] -= (i == le) ? real_t(1.0) : real_t(0.0);
                }
                DWBC_SYNC();
                LANES {
                    if (lane < M) {
#pragma unroll
                        for (int i = 0; i < M; i++) Ws[i * RS + lane] = LV(w)[i];
                    }
                }
                DWBC_SYNC();
                LANES {
                    lds_rows_dot<M, M, RS, 1, 1, true>(Ws, LV(e), LV(w));  // x_lane -= X e
                }
            }
            LANES {
                if (lane < M) {
#pragma unroll
                    for (int i = 0; i < M; i++) o_Wi[i * M + lane] = LV(w)[i];
                }
            }
        }
    }

    // ================= a failed instance: what was written goes back to zero =================
    if (!st_contact) {
        auto zero = [&](unsigned bit, io_t *p, int cnt) {
            if (mask & bit)
                for (int idx = th.tid; idx < cnt; idx += NT) p[idx] = real_t(0.0);
        };
        zero(kCsJC, o_JC, C * N);
        zero(kCsLambda, o_Lam, C * C);
        zero(kCsJCInvT, o_JbT, C * N);
        zero(kCsNC, o_NC, N * N);
        zero(kCsAInvNC, o_AiNc, N * N);
        zero(kCsW, o_W, M * M);
        zero(kCsWInv, o_Wi, M * M);
        zero(kCsNwJw, o_Nw, M * 6);
        zero(kCsPos, o_pos, kMaxActiveContacts * 3);
        zero(kCsRot, o_rot, kMaxActiveContacts * 9);
    }
    if (th.tid == 0) cio.status[inst] = st_contact ? 1 : 0;
}

}  // namespace dwbc
