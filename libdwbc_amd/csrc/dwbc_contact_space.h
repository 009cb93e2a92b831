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
// Everything behind stage 0 is dwbc_contact_space_body.inc: the task-space kernel (dwbc_task_space.h) runs the same text ahead of its levels.
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
    const real_t *body = DWBC_BODY(io, inst, nb);
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

#include "dwbc_contact_space_body.inc"

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
