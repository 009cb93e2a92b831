// dwbc_link_query.h -- RobotData::UpdateKinematics as a call of its own (reference include/dwbc.h, src/dwbc.cpp:279-371), for what a
// caller reads between it and SetTaskSpace: link_[i].xpos / rotm / v / w / jac_ of a handful of links and com_pos, one wavefront per
// instance.  The reference's own harnesses rotate a pelvis-frame f* by link_[0].rotm (tests/sp_test/regulation_test.cpp:97-98), take a
// hand position relative to the pelvis (redu_dyn_test.cpp:372) and build TASK_CUSTOM levels from link Jacobians (include/dwbc.h:333)
// before they set a single f*.  The kernel is the front of stage 0 of the fused cycle and nothing behind it:
//   world transforms of all bodies, world joint axes                    (Link::UpdatePos, src/link.cpp:76-84)
//   per queried (link, local point): position, rotation, [v; w] of the point, optionally its 6 x N Jacobian (src/link.cpp:85-119)
//   the synthetic COM link (link == nb) if an entry asks for it: com_pos, pelvis rotation, jac_com_ = SI_body^-1 CMM_ and jac_com_ qdot
//   (src/dwbc.cpp:318-367) from the six base rows of A alone -- composite inertias, S and F; no CRBA beyond those rows
// No mass-matrix inverse, no contact stage, no QP, no output of the cycle.
//
// World transforms: the depth rounds of dwbc_cycle_gc.h rather than the pointer jumping of dwbc_cycle2_stage0.inc.  They form every
// product in the order of the restatement (R_parent (R_T R_joint), oracle/dwbc_np.py: forward_kinematics), need no second transform
// buffer and no ancestor table, and read the tree's depth at run time, so any tree of the row's size is served by one instantiation.
// The price is `maxdepth` dependent rounds (TOCABI: 11) of one 3 x 3 product instead of ceil(log2(maxdepth + 1)); against the Jacobian
// stores of a query (6 N doubles per entry) that is not what bounds the kernel (link query).
//
// Velocities: the walk of velocity_rnea's first loop (dwbc_velocity.h:35-49) -- the base dofs, then the joints on the path from the link
// to the root -- done per queried entry about the query point itself instead of per body about the pelvis origin: no body-velocity
// table in LDS, and [v; w] is the product of the entry's Jacobian with qdot term by term.  Without qdot (BatchIO::qdot == nullptr: the
// state was set without one) every velocity is zero, as task_reference (dwbc_fstar.h) treats a missing qdot.
#pragma once
#include "dwbc_cycle.h"

namespace dwbc {

constexpr int kMaxLinkQuery = 16;

// what a query launch reads and writes beyond BatchIO::q / qdot / body / topo (BatchIO's layout is part of the kernel-pack ABI and stays)
struct LinkQueryIO {
    int n;             // entries, 1 .. kMaxLinkQuery
    int nb, maxdepth;  // bodies and depth of the model's tree
    int want_jac;      // jac is written
    int has_com;       // some entry is the synthetic COM link (link == nb)
    int link[kMaxLinkQuery];
    double point[kMaxLinkQuery][3];  // in the link's frame (zero for the COM link)
    io_t *pos;  // B x n x 3
    io_t *rot;  // B x n x 3 x 3, row-major
    io_t *vel;  // B x n x 6, [v of the point; w]
    io_t *jac;  // B x n x 6 x N, rows [linear; angular] (point_jacobian's convention); nullptr unless want_jac
};

// LDS map of this kernel alone (reals).  Life times (block : transforms | COM block | outputs):
//   q Rw pw aw : ........................................................
//   Pq         : .                | .                      | world points of the entries
//   U          : local transforms | body, then composite inertias | .
//   Sm         : .                | S .................... | .
//   FJ         : .                | F, then jac_com_ and com_pos ......
//   A6         : .                | A[:6, :]               | .
// TOCABI: 13 152 B -- twelve workgroups per CU by LDS (160 KiB), three waves per SIMD.
constexpr int lq_even(int x) { return (x + 1) & ~1; }  // blocks start on 16-byte boundaries
template <int N, int NB>
struct LdsLq {
    static constexpr int q = 0;                                  // N + 1
    static constexpr int Rw = q + lq_even(N + 1);                   // NB x 9
    static constexpr int pw = Rw + lq_even(NB * 9);                 // NB x 3
    static constexpr int aw = pw + lq_even(NB * 3);                 // NB x 3
    static constexpr int Pq = aw + lq_even(NB * 3);                 // kMaxLinkQuery x 3
    static constexpr int U = Pq + kMaxLinkQuery * 3;             // NB x 10: Rl (NB x 9), then Iw -> Ic in place
    static constexpr int Sm = U + NB * 10;                       // N x 6
    static constexpr int FJ = Sm + N * 6;                        // N x 6 (F), then 6 x N + 3 (com_jacobian's record)
    static constexpr int A6 = FJ + lq_even(6 * N + 3);              // 6 x N
    static constexpr int total = A6 + 6 * N;
    static constexpr int total_bytes = total * (int)sizeof(real_t);
};

template <int N, int NB, int NT>
DWBC_DEV void link_query_instance(Thr th, const BatchIO &io, const LinkQueryIO &lq, int inst, real_t *L) {
    using S = LdsLq<N, NB>;
    static_assert(NB <= 64 && N <= 64, "one body and one dof per lane");
    DWBC_LANE_DECL;
    const int nb = lq.nb, ne = lq.n;
    const real_t *body = DWBC_BODY(io, inst, nb);
    const int *topo = io.topo;  // parent[nb] depth[nb] subtree[nb]
    const io_t *qin = io.q + (size_t)inst * (N + 1);
    const io_t *qd = io.qdot ? io.qdot + (size_t)inst * N : nullptr;
    real_t *Rw = L + S::Rw, *pw = L + S::pw, *aw = L + S::aw, *Pq = L + S::Pq;
    const real_t *q = L + S::q;

    for (int i = th.tid; i < N + 1; i += NT) L[S::q + i] = (real_t)qin[i];
    DWBC_SYNC();
    // ================= world transforms (Link::UpdatePos) =================
    {
        real_t *Rl = L + S::U;
        // local joint transforms R_T * Rot(axis, q_i)
        for (int i = th.tid; i < nb; i += NT) {
            const real_t *bd = body + i * kBodyStride;
            if (i == 0) {
                const real_t x = q[3], y = q[4], z = q[5], w = q[N];
                real_t *R = Rw;
                R[0] = 1 - 2 * y * y - 2 * z * z; R[1] = 2 * x * y - 2 * w * z; R[2] = 2 * x * z + 2 * w * y;
                R[3] = 2 * x * y + 2 * w * z; R[4] = 1 - 2 * x * x - 2 * z * z; R[5] = 2 * y * z - 2 * w * x;
                R[6] = 2 * x * z - 2 * w * y; R[7] = 2 * y * z + 2 * w * x; R[8] = 1 - 2 * x * x - 2 * y * y;
                pw[0] = q[0]; pw[1] = q[1]; pw[2] = q[2];
            } else {
                const real_t ax = bd[BF_AXIS], ay = bd[BF_AXIS + 1], az = bd[BF_AXIS + 2];
                real_t sn, cs;
                sincos_r(q[6 + i - 1], &sn, &cs);
                const real_t c1 = real_t(1.0) - cs;
                real_t Rj[9];
                Rj[0] = cs + ax * ax * c1; Rj[1] = ax * ay * c1 - az * sn; Rj[2] = ax * az * c1 + ay * sn;
                Rj[3] = ay * ax * c1 + az * sn; Rj[4] = cs + ay * ay * c1; Rj[5] = ay * az * c1 - ax * sn;
                Rj[6] = az * ax * c1 - ay * sn; Rj[7] = az * ay * c1 + ax * sn; Rj[8] = cs + az * az * c1;
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b < 3; b++)
                        Rl[i * 9 + a * 3 + b] = bd[BF_RT + a * 3] * Rj[b] + bd[BF_RT + a * 3 + 1] * Rj[3 + b] + bd[BF_RT + a * 3 + 2] * Rj[6 + b];
            }
        }
        for (int d = 1; d <= lq.maxdepth; d++) {
            DWBC_SYNC();
            for (int i = th.tid; i < nb; i += NT) {
                if (topo[nb + i] != d) continue;
                const int par = topo[i];
                const real_t *bd = body + i * kBodyStride;
                const real_t *Rp = Rw + par * 9;
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++)
                        Rw[i * 9 + a * 3 + b] = Rp[a * 3] * Rl[i * 9 + b] + Rp[a * 3 + 1] * Rl[i * 9 + 3 + b] + Rp[a * 3 + 2] * Rl[i * 9 + 6 + b];
                    pw[i * 3 + a] = pw[par * 3 + a] + Rp[a * 3] * bd[BF_PT] + Rp[a * 3 + 1] * bd[BF_PT + 1] + Rp[a * 3 + 2] * bd[BF_PT + 2];
                }
            }
        }
        DWBC_SYNC();
        for (int i = th.tid; i < nb; i += NT) {  // world joint axes
            const real_t *bd = body + i * kBodyStride;
            const real_t *R = Rw + i * 9;
            for (int a = 0; a < 3; a++) aw[i * 3 + a] = R[a * 3] * bd[BF_AXIS] + R[a * 3 + 1] * bd[BF_AXIS + 1] + R[a * 3 + 2] * bd[BF_AXIS + 2];
        }
        DWBC_SYNC();
    }

    // ================= the synthetic COM link (src/dwbc.cpp:318-367): only if an entry asks for it =================
    real_t *Jcm = L + S::FJ;  // 6 x N [linear; angular], then com_pos (com_jacobian, dwbc_cycle.h)
    real_t vcom[6] = {real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0), real_t(0.0)};
    if (lq.has_com) {
        // world-frame spatial inertia of each body about O = pelvis origin, as stage 0 of the cycle forms it
        real_t *Iw = L + S::U;  // (the local transforms are dead)
        for (int i = th.tid; i < nb; i += NT) {
            const real_t *bd = body + i * kBodyStride;
            const real_t *R = Rw + i * 9;
            const real_t m = bd[BF_MASS];
            real_t r[3];
            for (int a = 0; a < 3; a++)
                r[a] = pw[i * 3 + a] + R[a * 3] * bd[BF_COM] + R[a * 3 + 1] * bd[BF_COM + 1] + R[a * 3 + 2] * bd[BF_COM + 2] - pw[a];
            const real_t Ic[9] = {bd[BF_ICOM], bd[BF_ICOM + 1], bd[BF_ICOM + 2], bd[BF_ICOM + 1], bd[BF_ICOM + 3],
                                  bd[BF_ICOM + 4], bd[BF_ICOM + 2], bd[BF_ICOM + 4], bd[BF_ICOM + 5]};
            real_t Tm[9];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) Tm[a * 3 + b] = R[a * 3] * Ic[b] + R[a * 3 + 1] * Ic[3 + b] + R[a * 3 + 2] * Ic[6 + b];
            const real_t rr2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
            real_t *o = Iw + i * 10;
            o[0] = m;
            o[1] = m * r[0]; o[2] = m * r[1]; o[3] = m * r[2];
            int c = 4;
            for (int a = 0; a < 3; a++)
                for (int b = a; b < 3; b++) {
                    real_t v = Tm[a * 3] * R[b * 3] + Tm[a * 3 + 1] * R[b * 3 + 1] + Tm[a * 3 + 2] * R[b * 3 + 2];
                    v += m * ((a == b ? rr2 : real_t(0.0)) - r[a] * r[b]);
                    o[c++] = v;
                }
        }
        DWBC_SYNC();
        // composite inertia of the subtree [b, b + len_b) (bodies are numbered depth first): inclusive prefix sums over the body order in
        // registers, Ic[b] = P[b + len_b - 1] - P[b - 1] (dwbc_cycle_gc.h), written back over the body inertias -- every lane has read its own
        {
            real_t *Icm = Iw;
            PLA(real_t, pf, 10);
            PL(int, len);
            LANES {
                const int bi = lane < nb ? lane : 0;
                LV(len) = lane < nb ? topo[2 * nb + bi] : 1;
#pragma unroll
                for (int c = 0; c < 10; c++) {
                    const real_t v_ = Iw[bi * 10 + c];
                    LV(pf)[c] = lane < nb ? v_ : real_t(0.0);
                }
            }
            DWBC_SYNC();
#pragma unroll
            for (int c = 0; c < 10; c++) WAVE_PREFIX_A(pf, c);
            LANES {
                int e_ = lane + LV(len) - 1;
                e_ = e_ < 63 ? e_ : 63;
                const int s_ = lane > 0 ? lane - 1 : 0;
#pragma unroll
                for (int c = 0; c < 10; c++) {
                    const real_t hi_ = SHFLA(pf, c, e_), lo_ = SHFLA(pf, c, s_);
                    if (lane < nb) Icm[lane * 10 + c] = hi_ - (lane > 0 ? lo_ : real_t(0.0));
                }
            }
        }
        // motion axes S_j = [omega; v_O] about O and F_j = Ic_body(j) S_j
        real_t *Sm = L + S::Sm, *Fm = L + S::FJ, *A6 = L + S::A6;
        const real_t *Icm = L + S::U;
        for (int j = th.tid; j < N; j += NT) {
            real_t w[3] = {0, 0, 0}, v[3] = {0, 0, 0};
            if (j < 3) {
                v[j] = real_t(1.0);
            } else if (j < 6) {
                for (int a = 0; a < 3; a++) w[a] = Rw[a * 3 + (j - 3)];
            } else {
                const int b = j - 5;
                for (int a = 0; a < 3; a++) w[a] = aw[b * 3 + a];
                const real_t d0 = pw[b * 3] - pw[0], d1 = pw[b * 3 + 1] - pw[1], d2 = pw[b * 3 + 2] - pw[2];
                v[0] = d1 * w[2] - d2 * w[1];
                v[1] = d2 * w[0] - d0 * w[2];
                v[2] = d0 * w[1] - d1 * w[0];
            }
            for (int a = 0; a < 3; a++) { Sm[j * 6 + a] = w[a]; Sm[j * 6 + 3 + a] = v[a]; }
        }
        DWBC_SYNC();
        for (int j = th.tid; j < N; j += NT) {
            const int b = j < 6 ? 0 : j - 5;
            const real_t *I = Icm + b * 10;
            const real_t *s = Sm + j * 6;
            const real_t m = I[0], h0 = I[1], h1 = I[2], h2 = I[3];
            const real_t w0 = s[0], w1 = s[1], w2 = s[2], v0 = s[3], v1 = s[4], v2 = s[5];
            // L = I w + h x v ; p = m v + w x h
            Fm[j * 6 + 0] = I[4] * w0 + I[5] * w1 + I[6] * w2 + (h1 * v2 - h2 * v1);
            Fm[j * 6 + 1] = I[5] * w0 + I[7] * w1 + I[8] * w2 + (h2 * v0 - h0 * v2);
            Fm[j * 6 + 2] = I[6] * w0 + I[8] * w1 + I[9] * w2 + (h0 * v1 - h1 * v0);
            Fm[j * 6 + 3] = m * v0 + (w1 * h2 - w2 * h1);
            Fm[j * 6 + 4] = m * v1 + (w2 * h0 - w0 * h2);
            Fm[j * 6 + 5] = m * v2 + (w0 * h1 - w1 * h0);
        }
        DWBC_SYNC();
        // the six base rows of A: every base dof lies on the path of every dof, A[r][j] = S_r . F_j (r <= j; the cycle's CRBA mirrors the rest)
        for (int j = th.tid; j < N; j += NT) {
            for (int r = 0; r < 6; r++) {
                const real_t *s = Sm + (r < j ? r : j) * 6, *f = Fm + (r < j ? j : r) * 6;
                A6[r * N + j] = s[0] * f[0] + s[1] * f[1] + s[2] * f[2] + s[3] * f[3] + s[4] * f[4] + s[5] * f[5];
            }
        }
        DWBC_SYNC();
        com_jacobian<N, NT>(th, A6, N, Rw, q, Jcm);  // over F, which is dead
        DWBC_SYNC();
        if (qd) {  // link_.back().v / .w = jac_com_ qdot (src/dwbc.cpp:360-367): one dof per lane, summed over the wave
            for (int r = 0; r < 6; r++) {
                PL(real_t, t);
                LANES {
                    const int j = lane < N ? lane : 0;
                    const real_t v_ = Jcm[r * N + j] * (real_t)qd[j];
                    LV(t) = lane < N ? v_ : real_t(0.0);
                }
                WAVE_SUM(t, vcom[r]);
            }
        }
    }

    // ================= the queried entries =================
    for (int e = th.tid; e < ne; e += NT) {
        const int link = lq.link[e];
        const bool is_com = link == nb;
        const int l = is_com ? 0 : link;  // rotm of the COM link is the pelvis rotation (src/dwbc.cpp:326)
        const real_t *R = Rw + l * 9;
        real_t P[3], v[3] = {0, 0, 0}, w[3] = {0, 0, 0};
        for (int a = 0; a < 3; a++)
            P[a] = is_com ? Jcm[6 * N + a]
                          : pw[l * 3 + a] + R[a * 3] * (real_t)lq.point[e][0] + R[a * 3 + 1] * (real_t)lq.point[e][1] + R[a * 3 + 2] * (real_t)lq.point[e][2];
        if (is_com) {
            for (int a = 0; a < 3; a++) { v[a] = vcom[a]; w[a] = vcom[3 + a]; }
        } else if (qd) {
            // [v; w] = J qdot, column by column of point_jacobian: the base, then the joints on the path to the root
            for (int a = 0; a < 3; a++) v[a] = (real_t)qd[a];
            for (int k = 0; k < 3; k++) {
                const real_t qk = (real_t)qd[3 + k];
                const real_t a0 = Rw[k], a1 = Rw[3 + k], a2 = Rw[6 + k];
                const real_t d0 = P[0] - pw[0], d1 = P[1] - pw[1], d2 = P[2] - pw[2];
                v[0] += (a1 * d2 - a2 * d1) * qk; v[1] += (a2 * d0 - a0 * d2) * qk; v[2] += (a0 * d1 - a1 * d0) * qk;
                w[0] += a0 * qk; w[1] += a1 * qk; w[2] += a2 * qk;
            }
            for (int c = l; c > 0; c = topo[c]) {
                const real_t qk = (real_t)qd[c + 5];
                const real_t a0 = aw[c * 3], a1 = aw[c * 3 + 1], a2 = aw[c * 3 + 2];
                const real_t d0 = P[0] - pw[c * 3], d1 = P[1] - pw[c * 3 + 1], d2 = P[2] - pw[c * 3 + 2];
                v[0] += (a1 * d2 - a2 * d1) * qk; v[1] += (a2 * d0 - a0 * d2) * qk; v[2] += (a0 * d1 - a1 * d0) * qk;
                w[0] += a0 * qk; w[1] += a1 * qk; w[2] += a2 * qk;
            }
        }
        const size_t o = (size_t)inst * ne + e;
        for (int a = 0; a < 3; a++) {
            Pq[e * 3 + a] = P[a];
            lq.pos[o * 3 + a] = P[a];
            lq.vel[o * 6 + a] = v[a];
            lq.vel[o * 6 + 3 + a] = w[a];
        }
        for (int a = 0; a < 9; a++) lq.rot[o * 9 + a] = R[a];
    }
    if (!lq.want_jac) return;
    DWBC_SYNC();
    for (int e = 0; e < ne; e++) {  // one row of 6 x N per entry, each row stored by N consecutive lanes
        io_t *J = lq.jac + ((size_t)inst * ne + e) * 6 * N;
        const int link = lq.link[e];
        if (link == nb) {
            for (int idx = th.tid; idx < 6 * N; idx += NT) J[idx] = Jcm[idx];
        } else {
            point_jacobian<N, NB, NT>(th, L + S::Rw, pw, aw, topo, nb, link, Pq + e * 3, J, N, 0, 6, 0);
        }
    }
}

}  // namespace dwbc
