// dwbc_dynamics.h -- the dynamics half of RobotData::UpdateKinematics (reference src/dwbc.cpp:279-371) in a launch of its own, one
// wavefront per instance: what a caller reads off RobotData after UpdateKinematics --
//   A_ (dwbc.cpp:305)   A_inv_ (:307)   B_ = C qdot + g (:343-344)   G_ (:358)   CMM_ (:329-336)   com_pos (:320-326)
// -- written to buffers of their own, selected by a mask.  It is stage 0 of the one-wave kernels and nothing behind it:
//   stage 0 (dwbc_cycle2_stage0.inc up to the column-per-lane load, shared text)   kinematics, CRBA, A and G_
//   centroidal block (the arithmetic of dump_centroidal, dwbc_cycle.h)               CMM_, com_pos from the six base rows of A
//   A^-1 (sweep_inverse_tree, dwbc_cycle2.h)                                        tree-sparse on a constant tree, dense leaves-first otherwise;
//                                                                                   written transposed (see below)
//   B_ (velocity_rnea, dwbc_velocity.h)                                             recursive Newton-Euler at zero acceleration
// Each of the last three sits behind a wave-uniform branch on the mask (a kernel argument): without DWBC_DYN_A_INV there is no sweep,
// without DWBC_DYN_B or without a qdot no RNEA (B_(q, 0) = G_: a copy), without DWBC_DYN_CMM / DWBC_DYN_COM no centroidal block.
// No contact, no task, no torque limit and no QP: of BatchIO it reads q, qdot, body and topo, of Setup the tree.
#pragma once
#include "dwbc_cycle2.h"
#include "dwbc_velocity.h"

namespace dwbc {

// bits of DynIO::mask: 1u << dwbc_dynamics_output (include/dwbc_batch.h; dwbc_capi.hip asserts the two agree)
enum : unsigned { kDynA = 1u << 0, kDynAInv = 1u << 1, kDynB = 1u << 2, kDynG = 1u << 3, kDynCmm = 1u << 4, kDynCom = 1u << 5 };

// device pointers of a dynamics launch, batch-major; the kernel's own argument struct beside BatchIO (whose layout is pack ABI and stays).
// A pointer whose bit is clear is never dereferenced.
struct DynIO {
    unsigned mask;
    io_t *A;      // B x N x N   A_
    io_t *A_inv;  // B x N x N   A_inv_
    io_t *Bv;     // B x N       B_ (without BatchIO::qdot: G_ to the bit)
    io_t *G;      // B x N       G_
    io_t *CMM;    // B x 6 x N   CMM_
    io_t *com;    // B x 3       com_pos
    int *status;  // B           always written: 0 only if A_inv_ was asked for and the sweep met a bad pivot (every asked-for output of
                  //             the instance is then zero)
};

// LDS map.  The names are the ones the stage-0 text and velocity_rnea address; nothing of the contact or task stages has a place.
// Life times (region : kinematics + CRBA | centroidal block, sweep | RNEA):
//   q, G   : q, G_ ............................................. G_ (copied into B_ without a qdot)
//   Bq     : .                          | .                    | B_
//   Rw pw  : link rotations and positions ...................... (RNEA: body inertias to the world frame)
//   aw     : world joint axes           | .                    | .
//   k_S    : (zeros of the text's head), motion axes S ......... S
//   k_F    : F = Ic S                   | .                    | c_j, then the body forces
//   X      : k_Iw k_Ic (k_Rl, k_anc over them), then the staged packed A | A (base rows: com_pos) | bias accelerations (k_Iw), velocities (k_Rl)
//   (X .. total, behind the sweep: rows of A_inv_ on their way out; the 64 doubles behind X round that staging up)
// k_Rl sits 6 NB behind k_Iw, not 3 NB as on the compact maps of the cycle: velocity_rnea keeps the link velocities in k_Rl and the bias
// accelerations in k_Iw, 6 NB doubles each, at the same time.  The text's ping-pong partner of pw (3 NB at k_Iw) and the local rotations
// (9 NB at k_Rl) still end below the ancestor indices at the tail of k_Ic.
// Bytes (N / NB: total_bytes):  23 / 18: 8 336    37 / 32: 14 448    39 / 34: 15 536    43 / 38: 17 824    50 / 45: 22 144
template <int N, int NB>
struct LdsDyn {
    static constexpr bool compact = true;  // the packed staging of A
    static constexpr int M = N - 6;
    static constexpr int max2(int a, int b) { return a > b ? a : b; }
    static constexpr int ev(int a) { return (a + 1) & ~1; }
    static constexpr int q = 0;                         // N + 1
    static constexpr int G = q + ev(N + 1);             // N
    static constexpr int Bq = G + ev(N);                // N
    static constexpr int Rw = Bq + ev(N);               // NB x 9
    static constexpr int pw = Rw + NB * 9;              // NB x 3
    static constexpr int aw = pw + NB * 3;              // NB x 3
    static constexpr int k_S = ev(aw + NB * 3);         // N x 6
    static constexpr int k_F = k_S + N * 6;             // N x 6
    static constexpr int tg = k_S;                      // the 3 M doubles the text clears at its head: over S and F, which are written later
    static_assert(tg + 3 * M <= k_F + N * 6, "the cleared head lies inside S and F");
    static constexpr int X = k_F + N * 6;
    static constexpr int k_Iw = X;                      // NB x 10 (first the ping-pong partner of pw)
    static constexpr int k_Ic = k_Iw + NB * 10;         // NB x 10
    static constexpr int k_Rl = k_Iw + NB * 6;          // NB x 9, dead before Iw and Ic are written
    static constexpr int k_anc = k_Ic + NB * 10 - 2 * NB;
    static_assert(k_Iw + NB * 3 <= k_Rl && k_Rl + NB * 9 <= k_anc, "ping-pong buffers and ancestor indices of the world transforms");
    static_assert(k_Iw + NB * 6 <= k_Rl && k_Rl + NB * 6 <= k_Ic + NB * 10, "bias accelerations and link velocities of velocity_rnea");
    static constexpr bool a_overlay = false, a_packed = true;
    static constexpr int k_A = X;                       // N (N + 1) / 2, written after Ic has been consumed
    static constexpr int total = ev(X + max2(N * (N + 1) / 2, NB * 20)) + 64;
    static constexpr int T_rows = (total - X) / N;      // rows of A_inv_ staged at a time over X .. total for the row-major write (the staged A is dead)
    static_assert(T_rows >= 8, "the transposed write of A_inv_ takes a handful of rounds at most");
    static constexpr int total_bytes = total * (int)sizeof(real_t);
    // named by the shared text in branches that are dead here (EXTRAS = false, no dump record)
    static constexpr int comp = 0, Jcm = 0;
};

template <int N, int NB, int NT, class Topo>
DWBC_DEV void dynamics_instance(Thr th, const Setup &su, const BatchIO &io, const DynIO &dio, int inst, real_t *L) {
    using S = LdsDyn<N, NB>;
    constexpr bool kExtras = false;
    constexpr int M = S::M;
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
    const unsigned mask = dio.mask;

    PLA(real_t, s, N);  // column `lane` of A -> A^-1
    PL(real_t, dg);     // its diagonal element

#define DWBC_STAGE0_FRONT_ONLY
#include "dwbc_cycle2_stage0.inc"
#undef DWBC_STAGE0_FRONT_ONLY

    // ================= A_ and the centroidal block: from the columns in registers, before the sweep turns them into A^-1 =================
    if (mask & kDynA) {
        io_t *Ao = dio.A + (size_t)inst * N * N;
        LANES {
            if (lane < N) {
#pragma unroll
                for (int i = 0; i < N; i++) Ao[i * N + lane] = LV(s)[i];
            }
        }
    }
    if (mask & (kDynCmm | kDynCom)) {
        // dump_centroidal (dwbc_cycle.h) on the packed staging: com_from_pelv from skm = R0 A[3:6, 0:3] / m, CMM_ = cm_rot6 A[0:6, :]
        const real_t *A = L + S::k_A, *R0 = L + S::Rw, *q0 = L + S::q;
        const real_t mt = A[0];  // A(0, 0) = total mass
        real_t c[3];
        const int ra[3] = {2, 0, 1}, cb[3] = {1, 2, 0};
        for (int e = 0; e < 3; e++) {
            real_t acc = real_t(0.0);
            for (int b = 0; b < 3; b++) acc += R0[ra[e] * 3 + b] * A[(3 + b) * (4 + b) / 2 + cb[e]];  // (3 + b, cb) of the lower triangle
            c[e] = acc / mt;
        }
        if ((mask & kDynCom) && th.tid == 0) {
            io_t *co = dio.com + (size_t)inst * 3;
            for (int a = 0; a < 3; a++) co[a] = c[a] + q0[a];
        }
        if (mask & kDynCmm) {
            // skew(c)^T rows: [0 c2 -c1; -c2 0 c0; c1 -c0 0]
            const real_t St[9] = {real_t(0.0), c[2], -c[1], -c[2], real_t(0.0), c[0], c[1], -c[0], real_t(0.0)};
            io_t *Co = dio.CMM + (size_t)inst * 6 * N;
            LANES {
                if (lane < N) {
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        Co[a * N + lane] = LV(s)[a];
                        real_t acc = real_t(0.0);
#pragma unroll
                        for (int b = 0; b < 3; b++) acc += St[a * 3 + b] * LV(s)[b] + R0[a * 3 + b] * LV(s)[3 + b];
                        Co[(3 + a) * N + lane] = acc;
                    }
                }
            }
        }
    }

    // ================= A_inv_ (dwbc.cpp:307): the LDS-fed sweep of the compact lean builds =================
    int ok = 1;
    if (mask & kDynAInv) {
        // The register sweep (pivot column by v_readlane), not the LDS-fed one of the compact lean builds: that one carries the diagonal
        // shifted by two, which costs a pivot of 1e-3 kg m^2 three digits -- fine for the cycle (A_inv_ 1.5e-10 off the restatement, bar
        // 1e-8), but max|A A_inv - I| comes out at 2e-13 .. 4.5e-13 on an MI355X where this sweep stays at 1e-13, and a caller of this
        // launch reads A_inv_ itself.  It is also the sweep of the extras builds, so A_inv_ here is the dump record's, transposed.
        using SweepTopo = typename std::conditional<kTree, Topo, TopoDense<N>>::type;
        if (!sweep_inverse_tree<SweepTopo, N>(s, dg)) ok = 0;
        DWBC_SYNC();
        // The sweep works on columns, and its result X is a tighter left inverse than right inverse (host emulation, TOCABI: max|X A - I|
        // 5e-14 .. 1.2e-13, max|A X - I| 6e-14 .. 9.6e-13; the restatement's LLT inverse: 1e-14 .. 3.5e-14 either way).  A_inv_ is symmetric,
        // so X^T is written: A X^T - I = (X A - I)^T.  Lane r holds row r of X^T; S::T_rows of them at a time go through the dead staging
        // of A, so that the global stores are rows written by consecutive lanes.
        io_t *Io = dio.A_inv + (size_t)inst * N * N;
        real_t *T = L + S::X;
        for (int r0 = 0; r0 < N; r0 += S::T_rows) {
            LANES {
                if (lane >= r0 && lane < r0 + S::T_rows && lane < N) {
#pragma unroll
                    for (int c = 0; c < N; c++) T[(lane - r0) * N + c] = ok ? LV(s)[c] : real_t(0.0);
                }
            }
            DWBC_SYNC();
            const int cnt = (N - r0 < S::T_rows ? N - r0 : S::T_rows) * N;
            for (int idx = th.tid; idx < cnt; idx += NT) Io[r0 * N + idx] = T[idx];
            DWBC_SYNC();
        }
    }

    // ================= B_ (dwbc.cpp:343-344) and G_ =================
    if (mask & kDynB) {
        if (io.qdot != nullptr) {
            velocity_rnea<S, N, NB, NT>(th, su, io.qdot + (size_t)inst * N, body, topo, L, L + S::Bq, nullptr, nullptr);
        } else {
            DWBC_SYNC();
            for (int j = th.tid; j < N; j += NT) L[S::Bq + j] = L[S::G + j];
            DWBC_SYNC();
        }
        io_t *Bo = dio.Bv + (size_t)inst * N;
        for (int j = th.tid; j < N; j += NT) Bo[j] = ok ? L[S::Bq + j] : real_t(0.0);
    }
    if (mask & kDynG) {
        io_t *Go = dio.G + (size_t)inst * N;
        for (int j = th.tid; j < N; j += NT) Go[j] = ok ? L[S::G + j] : real_t(0.0);
    }
    if (!ok) {  // a bad pivot: what was written before the sweep goes back to zero
        if (mask & kDynA) {
            io_t *Ao = dio.A + (size_t)inst * N * N;
            for (int idx = th.tid; idx < N * N; idx += NT) Ao[idx] = real_t(0.0);
        }
        if (mask & kDynCmm) {
            io_t *Co = dio.CMM + (size_t)inst * 6 * N;
            for (int idx = th.tid; idx < 6 * N; idx += NT) Co[idx] = real_t(0.0);
        }
        if ((mask & kDynCom) && th.tid == 0) {
            io_t *co = dio.com + (size_t)inst * 3;
            for (int a = 0; a < 3; a++) co[a] = real_t(0.0);
        }
    }
    if (th.tid == 0) dio.status[inst] = ok;
    (void)st_contact;
}

}  // namespace dwbc
