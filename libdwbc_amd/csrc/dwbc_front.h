// dwbc_front.h -- the kinematics and CRBA front end (RobotData::UpdateKinematics, reference src/dwbc.cpp:279-371, Link::UpdatePos,
// src/link.cpp:76-84): joint rotations, world transforms, world joint axes, world-frame body inertias, composite inertias, motion axes
// S, forces F = Ic S, the packed CRBA pairs of the mass matrix and its column-per-lane load.  Called by the two-wave kernel
// (dwbc_cycle2p.h) and the general-contact kernel (dwbc_cycle_gc.h).  Stage 0 of the one-wave kernels (dwbc_cycle2_stage0.inc) and
// the link query (dwbc_link_query.h) still hold the same blocks as text: the optimiser meets an inlined function in another order
// than the text, and on these functions the register-capped extras builds, the reduced builds and the redistribution kernel
// changed their register and spill counts, and the link query its results in the last bit (other fused multiply-adds).  Those two
// files wait for a form that leaves them alone (profiles/front_end_codeobj.txt).  Included by dwbc_cycle.h, behind the macros and
// types it uses.
//
// The functions take explicit pointers (each caller passes its own LDS blocks), are force-inlined, and carry no stage stamps.  None
// of them ends with a DWBC_SYNC(): the caller places the one that separates a function's stores from the next reader, and the
// workgroup barriers of the two-wave kernel.  Those with a DWBC_SYNC() inside say so.
//
// Two world-transform routines exist because the kernels differ in arithmetic order and buffers, and each keeps its own:
//   world_transforms_jump:  pointer jumping, ceil(log2(depth + 1)) rounds, a second transform buffer and an ancestor table
//   world_transforms_depth: one round per tree depth in the order of the restatement R_parent (R_T R_joint), no extra buffer
// The composite inertias of both callers are composite_inertias_scan (stage 0 keeps its window sums through LDS).
#pragma once

namespace dwbc {

// base quaternion -> Rw[0], base position -> pw[0]; local joint transforms R_T * Rot(axis, q_i) -> Rl[i], i >= 1
template <int N, int NT>
DWBC_DEV void joint_transforms(Thr th, const real_t *q, const real_t *body, int nb, real_t *Rw, real_t *pw, real_t *Rl) {
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
}

// rounds of pointer jumping that cover a tree of depth `maxdepth`
DWBC_DEV constexpr int jump_rounds(int maxdepth) {
    int rounds = 0;
    while ((1 << rounds) < maxdepth + 1) rounds++;
    return rounds;
}

// world transforms by pointer jumping: T_i <- T_anc(i) o T_i, anc(i) <- anc(anc(i)); `rounds` rounds of one 3x3 product per body
// instead of `depth` dependent rounds.  Buffer 0 = (Rw, pw), buffer 1 = (Rl, p_alt); ancestor indices ride along as reals in
// anc (2 x NB).  (T_a o T_i: R = R_a R_i, p = p_a + R_a p_i.)  Begins with a DWBC_SYNC() and has one before every round.
template <int NB, int NT>
DWBC_DEV void world_transforms_jump(Thr th, const real_t *body, const int *topo, int nb, int rounds, real_t *Rw, real_t *pw, real_t *Rl,
                                    real_t *p_alt, real_t *anc) {
    const bool odd = rounds & 1;  // start in the buffer that makes the last round land in (Rw, pw)
    real_t *Rc = odd ? Rl : Rw, *Rn = odd ? Rw : Rl;
    real_t *pc = odd ? p_alt : pw, *pn = odd ? pw : p_alt;
    real_t *ac = anc, *an_ = anc + NB;
    DWBC_SYNC();
    for (int i = th.tid; i < nb; i += NT) {
        const real_t *bd = body + i * kBodyStride;
        real_t Ri[9], pi[3];
        for (int a = 0; a < 9; a++) Ri[a] = (i == 0) ? Rw[a] : Rl[i * 9 + a];
        for (int a = 0; a < 3; a++) pi[a] = (i == 0) ? pw[a] : bd[BF_PT + a];
        const real_t an = (i == 0) ? -real_t(1.0) : (real_t)topo[i];
        for (int a = 0; a < 9; a++) Rc[i * 9 + a] = Ri[a];
        for (int a = 0; a < 3; a++) pc[i * 3 + a] = pi[a];
        ac[i] = an;
    }
    for (int r = 0; r < rounds; r++) {
        DWBC_SYNC();
        for (int i = th.tid; i < nb; i += NT) {
            // all loads first (the compiler cannot reorder LDS loads across the stores below: same base pointer)
            const int an = (int)ac[i];
            const int aa = an < 0 ? 0 : an;
            real_t Ri[9], pi[3], Ra[9], pa[3];
            for (int a = 0; a < 9; a++) { Ri[a] = Rc[i * 9 + a]; Ra[a] = Rc[aa * 9 + a]; }
            for (int a = 0; a < 3; a++) { pi[a] = pc[i * 3 + a]; pa[a] = pc[aa * 3 + a]; }
            const real_t a2 = ac[aa];
            real_t Ro[9], po[3];
            for (int a = 0; a < 3; a++) {
                for (int c = 0; c < 3; c++) Ro[a * 3 + c] = Ra[a * 3] * Ri[c] + Ra[a * 3 + 1] * Ri[3 + c] + Ra[a * 3 + 2] * Ri[6 + c];
                po[a] = pa[a] + Ra[a * 3] * pi[0] + Ra[a * 3 + 1] * pi[1] + Ra[a * 3 + 2] * pi[2];
            }
            for (int a = 0; a < 9; a++) Rn[i * 9 + a] = an < 0 ? Ri[a] : Ro[a];
            for (int a = 0; a < 3; a++) pn[i * 3 + a] = an < 0 ? pi[a] : po[a];
            an_[i] = an < 0 ? -real_t(1.0) : a2;
        }
        { real_t *t_ = Rc; Rc = Rn; Rn = t_; t_ = pc; pc = pn; pn = t_; t_ = ac; ac = an_; an_ = t_; }
    }
}

// world transforms by depth rounds: bodies of depth d take R_parent (R_T R_joint) once the round of depth d - 1 is through; a
// DWBC_SYNC() before every round
template <int NT>
DWBC_DEV void world_transforms_depth(Thr th, const real_t *body, const int *topo, int nb, int maxdepth, real_t *Rw, real_t *pw,
                                     const real_t *Rl) {
    for (int d = 1; d <= maxdepth; d++) {
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
}

DWBC_DEV void world_axis(const real_t *bd, const real_t *R, real_t *aw, int i) {
    for (int a = 0; a < 3; a++) aw[i * 3 + a] = R[a * 3] * bd[BF_AXIS] + R[a * 3 + 1] * bd[BF_AXIS + 1] + R[a * 3 + 2] * bd[BF_AXIS + 2];
}

// world joint axes, in a loop of their own
template <int NT>
DWBC_DEV void world_axes(Thr th, const real_t *body, int nb, const real_t *Rw, real_t *aw) {
    for (int i = th.tid; i < nb; i += NT) world_axis(body + i * kBodyStride, Rw + i * 9, aw, i);
}

// world-frame spatial inertia of each body about O = pelvis origin, ten components per body [m | m r | I_O upper triangle];
// WITH_AXES: the world joint axes into aw in the same loop (aw is not used otherwise)
template <int NT, bool WITH_AXES>
DWBC_DEV void world_inertias(Thr th, const real_t *body, int nb, const real_t *Rw, const real_t *pw, real_t *Iw, real_t *aw = nullptr) {
    for (int i = th.tid; i < nb; i += NT) {
        const real_t *bd = body + i * kBodyStride;
        const real_t *R = Rw + i * 9;
        if constexpr (WITH_AXES) world_axis(bd, R, aw, i);
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
}

// components [C0, C1) of the composite inertia of the subtree [b, b + len_b) (bodies are numbered depth first): inclusive prefix sums
// over the body order in registers (DPP), Ic[b] = P[b + len_b - 1] - P[b - 1].  Everything is expressed about the pelvis origin, where
// the smallest subtree (a wrist link, m r^2 ~ 0.1) is within 1e3 of the total: the difference keeps 13 digits.  One body per lane.
template <int C0, int C1>
DWBC_DEV void composite_inertias_scan(const int *topo, int nb, const real_t *Iw, real_t *Icm) {
    constexpr int NCP = C1 - C0;
    DWBC_LANE_DECL;
    PLA(real_t, pf, NCP);
    PL(int, len);
    LANES {
        const int bi = lane < nb ? lane : 0;
        LV(len) = lane < nb ? topo[2 * nb + bi] : 1;
#pragma unroll
        for (int c = 0; c < NCP; c++) {
            const real_t v_ = Iw[bi * 10 + C0 + c];
            LV(pf)[c] = lane < nb ? v_ : real_t(0.0);
        }
    }
#pragma unroll
    for (int c = 0; c < NCP; c++) WAVE_PREFIX_A(pf, c);
    LANES {
        int e_ = lane + LV(len) - 1;
        e_ = e_ < 63 ? e_ : 63;
        const int s_ = lane > 0 ? lane - 1 : 0;
#pragma unroll
        for (int c = 0; c < NCP; c++) {
            const real_t hi_ = SHFLA(pf, c, e_), lo_ = SHFLA(pf, c, s_);
            if (lane < nb) Icm[lane * 10 + C0 + c] = hi_ - (lane > 0 ? lo_ : real_t(0.0));
        }
    }
}

// ---- Forms of the two-wave kernel (dwbc_cycle2p.h), where a wave has one body per lane (64 >= nb): the lane's record of the body
// table and its topo words are requested at the top of the kernel (lane_record_fetch and the topo words beside it) and taken from registers here, so that no
// routine of the front end waits out a trip to global memory of its own.  The expressions are those of the forms above, in the same
// order.  Lanes >= nb hold the record of body 0 and store nothing.  The forms above are left as they are: the general-contact
// kernel calls them.

// fields [F0, F1) of the lane's record: loads only, no wait
template <int NB, int F0, int F1>
DWBC_DEV void lane_record_fetch(const real_t *body, PLA_REF(real_t, rec, kBodyStride)) {
    DWBC_LANE_DECL;
    LANES {
        const int bi = lane < NB ? lane : 0;
#pragma unroll
        for (int a = F0; a < F1; a++) LV(rec)[a] = body[bi * kBodyStride + a];
    }
}

// joint_transforms and the start of world_transforms_jump in one: the lane's local transform (body 0: the base pose), its constant
// offset p_T and its parent as the first ancestor go straight into the buffer the first jump round reads, and stay in (Ri, pi, an).
// qb: q[0..5] and q[N]; qj: the joint angle of the lane's body.
template <int NB>
DWBC_DEV void joint_transforms_lane(const real_t (&qb)[7], PL_REF(real_t, qj), PLA_REF(real_t, rec, kBodyStride), PL_REF(int, par), int rounds,
                                    real_t *Rw, real_t *pw, real_t *Rl, real_t *p_alt, real_t *anc, PLA_REF(real_t, Ri, 9),
                                    PLA_REF(real_t, pi, 3), PL_REF(real_t, an)) {
    const bool odd = rounds & 1;
    real_t *Rc = odd ? Rl : Rw, *pc = odd ? p_alt : pw;
    DWBC_LANE_DECL;
    LANES {
        const int i = lane;
        const real_t *bd = LV(rec);
        if (i == 0) {
            const real_t x = qb[3], y = qb[4], z = qb[5], w = qb[6];
            real_t *R = LV(Ri);
#if defined(DWBC_HOST_EMU)
            R[0] = 1 - 2 * y * y - 2 * z * z; R[1] = 2 * x * y - 2 * w * z; R[2] = 2 * x * z + 2 * w * y;
            R[3] = 2 * x * y + 2 * w * z; R[4] = 1 - 2 * x * x - 2 * z * z; R[5] = 2 * y * z - 2 * w * x;
            R[6] = 2 * x * z - 2 * w * y; R[7] = 2 * y * z + 2 * w * x; R[8] = 1 - 2 * x * x - 2 * y * y;
#else
            // The same nine expressions with the fused multiply-adds written out as the compiler forms them in joint_transforms: each
            // entry is a sum of two products of which either may be the fused one, and left to itself the compiler fuses the other one
            // here (its choice follows the order it meets the stores in), which moves a tilted base rotation in the last bit.
            const auto fm = [](real_t a, real_t b, real_t c) {
                if constexpr (sizeof(real_t) == 8) return (real_t)__builtin_fma(a, b, c);
                else return (real_t)__builtin_fmaf(a, b, c);
            };
            const real_t x2 = x + x, y2 = y + y, z2 = z + z, w2 = w + w;
            const real_t zw = z * w2, yw = y * w2, xw = x * w2;
            const real_t oy = fm(-y, y2, real_t(1.0)), ox = fm(-x, x2, real_t(1.0));
            R[0] = fm(-z, z2, oy); R[1] = fm(x2, y, -zw); R[2] = fm(x2, z, yw);
            R[3] = fm(x2, y, zw); R[4] = fm(-z, z2, ox); R[5] = fm(y2, z, -xw);
            R[6] = fm(x2, z, -yw); R[7] = fm(y2, z, xw); R[8] = fm(-y, y2, ox);
#endif
            LV(pi)[0] = qb[0]; LV(pi)[1] = qb[1]; LV(pi)[2] = qb[2];
            LV(an) = -real_t(1.0);
        } else {
            const real_t ax = bd[BF_AXIS], ay = bd[BF_AXIS + 1], az = bd[BF_AXIS + 2];
            real_t sn, cs;
            sincos_r(LV(qj), &sn, &cs);
            const real_t c1 = real_t(1.0) - cs;
            real_t Rj[9];
            Rj[0] = cs + ax * ax * c1; Rj[1] = ax * ay * c1 - az * sn; Rj[2] = ax * az * c1 + ay * sn;
            Rj[3] = ay * ax * c1 + az * sn; Rj[4] = cs + ay * ay * c1; Rj[5] = ay * az * c1 - ax * sn;
            Rj[6] = az * ax * c1 - ay * sn; Rj[7] = az * ay * c1 + ax * sn; Rj[8] = cs + az * az * c1;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++)
                    LV(Ri)[a * 3 + b] = bd[BF_RT + a * 3] * Rj[b] + bd[BF_RT + a * 3 + 1] * Rj[3 + b] + bd[BF_RT + a * 3 + 2] * Rj[6 + b];
            for (int a = 0; a < 3; a++) LV(pi)[a] = bd[BF_PT + a];
            LV(an) = (real_t)LV(par);
        }
        if (i < NB) {
            for (int a = 0; a < 9; a++) Rc[i * 9 + a] = LV(Ri)[a];
            for (int a = 0; a < 3; a++) pc[i * 3 + a] = LV(pi)[a];
            anc[i] = LV(an);
        }
    }
}

// the rounds of world_transforms_jump on the buffers joint_transforms_lane filled: a lane keeps its own transform and ancestor in
// registers and reads the ancestor's only.  A DWBC_SYNC() before every round; on return (Ri, pi) is the lane's world transform, as
// stored in (Rw, pw).
template <int NB>
DWBC_DEV void world_transforms_jump_lane(int rounds, real_t *Rw, real_t *pw, real_t *Rl, real_t *p_alt, real_t *anc, PLA_REF(real_t, Ri, 9),
                                         PLA_REF(real_t, pi, 3), PL_REF(real_t, an)) {
    const bool odd = rounds & 1;  // start in the buffer that makes the last round land in (Rw, pw)
    real_t *Rc = odd ? Rl : Rw, *Rn = odd ? Rw : Rl;
    real_t *pc = odd ? p_alt : pw, *pn = odd ? pw : p_alt;
    real_t *ac = anc, *an_ = anc + NB;
    DWBC_LANE_DECL;
    for (int r = 0; r < rounds; r++) {
        DWBC_SYNC();
        LANES {
            const int i = lane;
            if (i < NB) {
                const int ai = (int)LV(an);
                const int aa = ai < 0 ? 0 : ai;
                real_t Ra[9], pa[3];
                for (int a = 0; a < 9; a++) Ra[a] = Rc[aa * 9 + a];
                for (int a = 0; a < 3; a++) pa[a] = pc[aa * 3 + a];
                const real_t a2 = ac[aa];
                real_t Ro[9], po[3];
                for (int a = 0; a < 3; a++) {
                    for (int c = 0; c < 3; c++)
                        Ro[a * 3 + c] = Ra[a * 3] * LV(Ri)[c] + Ra[a * 3 + 1] * LV(Ri)[3 + c] + Ra[a * 3 + 2] * LV(Ri)[6 + c];
                    po[a] = pa[a] + Ra[a * 3] * LV(pi)[0] + Ra[a * 3 + 1] * LV(pi)[1] + Ra[a * 3 + 2] * LV(pi)[2];
                }
                for (int a = 0; a < 9; a++) LV(Ri)[a] = ai < 0 ? LV(Ri)[a] : Ro[a];
                for (int a = 0; a < 3; a++) LV(pi)[a] = ai < 0 ? LV(pi)[a] : po[a];
                LV(an) = ai < 0 ? -real_t(1.0) : a2;
                for (int a = 0; a < 9; a++) Rn[i * 9 + a] = LV(Ri)[a];
                for (int a = 0; a < 3; a++) pn[i * 3 + a] = LV(pi)[a];
                an_[i] = LV(an);
            }
        }
        { real_t *t_ = Rc; Rc = Rn; Rn = t_; t_ = pc; pc = pn; pn = t_; t_ = ac; ac = an_; an_ = t_; }
    }
}

// world joint axes from the lane's world rotation in registers
template <int NB>
DWBC_DEV void world_axes_lane(PLA_REF(real_t, rec, kBodyStride), PLA_REF(real_t, Ri, 9), real_t *aw) {
    DWBC_LANE_DECL;
    LANES {
        if (lane < NB) world_axis(LV(rec), LV(Ri), aw, lane);
    }
}

// world_inertias<NT, false> with the lane's mass, COM and inertia from its record
template <int NB>
DWBC_DEV void world_inertias_lane(PLA_REF(real_t, rec, kBodyStride), const real_t *Rw, const real_t *pw, real_t *Iw) {
    DWBC_LANE_DECL;
    LANES {
        const int i = lane;
        if (i < NB) {
            const real_t *bd = LV(rec);
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
    }
}

// composite_inertias_scan with the length of the lane's subtree from its register
template <int C0, int C1>
DWBC_DEV void composite_inertias_scan_lane(PL_REF(int, len), int nb, const real_t *Iw, real_t *Icm) {
    constexpr int NCP = C1 - C0;
    DWBC_LANE_DECL;
    PLA(real_t, pf, NCP);
    LANES {
        const int bi = lane < nb ? lane : 0;
#pragma unroll
        for (int c = 0; c < NCP; c++) {
            const real_t v_ = Iw[bi * 10 + C0 + c];
            LV(pf)[c] = lane < nb ? v_ : real_t(0.0);
        }
    }
#pragma unroll
    for (int c = 0; c < NCP; c++) WAVE_PREFIX_A(pf, c);
    LANES {
        int e_ = lane + (lane < nb ? LV(len) : 1) - 1;
        e_ = e_ < 63 ? e_ : 63;
        const int s_ = lane > 0 ? lane - 1 : 0;
#pragma unroll
        for (int c = 0; c < NCP; c++) {
            const real_t hi_ = SHFLA(pf, c, e_), lo_ = SHFLA(pf, c, s_);
            if (lane < nb) Icm[lane * 10 + C0 + c] = hi_ - (lane > 0 ? lo_ : real_t(0.0));
        }
    }
}

// motion axes S_j = [omega; v_O] about O = pelvis origin (N x 6): base translations, base rotations, then joint j on body j - 5
template <int N, int NT>
DWBC_DEV void motion_axes(Thr th, const real_t *Rw, const real_t *pw, const real_t *aw, real_t *Sm) {
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
}

// F_j = Ic_body(j) S_j (N x 6): L = I w + h x v ; p = m v + w x h
template <int N, int NT>
DWBC_DEV void body_forces(Thr th, const real_t *Icm, const real_t *Sm, real_t *Fm) {
    for (int j = th.tid; j < N; j += NT) {
        const int b = j < 6 ? 0 : j - 5;
        const real_t *I = Icm + b * 10;
        const real_t *sv = Sm + j * 6;
        const real_t m = I[0], h0 = I[1], h1 = I[2], h2 = I[3];
        const real_t w0 = sv[0], w1 = sv[1], w2 = sv[2], v0 = sv[3], v1 = sv[4], v2 = sv[5];
        Fm[j * 6 + 0] = I[4] * w0 + I[5] * w1 + I[6] * w2 + (h1 * v2 - h2 * v1);
        Fm[j * 6 + 1] = I[5] * w0 + I[7] * w1 + I[8] * w2 + (h2 * v0 - h0 * v2);
        Fm[j * 6 + 2] = I[6] * w0 + I[8] * w1 + I[9] * w2 + (h0 * v1 - h1 * v0);
        Fm[j * 6 + 3] = m * v0 + (w1 * h2 - w2 * h1);
        Fm[j * 6 + 4] = m * v1 + (w2 * h0 - w0 * h2);
        Fm[j * 6 + 5] = m * v2 + (w0 * h1 - w1 * h0);
    }
}

// coupled dof pairs (j << 8 | k, k on the path from j to the root) of the mass matrix (Model::topo_table), npair = topo[3 nb] of them
// behind the count: a thread's share into registers.  Fetched early, so that the kinematics cover the latency, and used by
// crba_pairs_fill.
template <int N, int NT>
constexpr int kCrbaPairRounds = (N * (N + 1) / 2 + NT - 1) / NT;  // a chain is the worst case; TOCABI: 396 pairs, 7 rounds
template <int N, int NT>
DWBC_DEV void crba_pairs_fetch(Thr th, const int *topo, int nb, int npair, int (&pairw)[kCrbaPairRounds<N, NT>]) {
#pragma unroll
    for (int r = 0; r < kCrbaPairRounds<N, NT>; r++) pairw[r] = (r * NT + th.tid < npair) ? topo[3 * nb + 1 + r * NT + th.tid] : 0;
}

// A[j][k] = S_k . F_j for k on the path from j to the root (CRBA, [ext] RBDL CompositeRigidBodyAlgorithm) into the zeroed A:
// lower triangle, row-packed, (i, j <= i) at i (i + 1) / 2 + j
template <int N, int NT>
DWBC_DEV void crba_pairs_fill(Thr th, int npair, const int (&pairw)[kCrbaPairRounds<N, NT>], const real_t *Sm, const real_t *Fm, real_t *A) {
#pragma unroll
    for (int r = 0; r < kCrbaPairRounds<N, NT>; r++) {
        if (r * NT + th.tid < npair) {
            const int j = pairw[r] >> 8, kk = pairw[r] & 255;  // kk <= j
            const real_t *f = Fm + j * 6, *sv = Sm + kk * 6;
            const real_t v = sv[0] * f[0] + sv[1] * f[1] + sv[2] * f[2] + sv[3] * f[3] + sv[4] * f[4] + sv[5] * f[5];
            A[j * (j + 1) / 2 + kk] = v;
        }
    }
}

// the staged (row-packed) mass matrix column per lane into registers, its diagonal, and G_ = -J_com_lin^T m g = 9.81 * A[2,:] (dwbc.cpp:358)
template <int N>
DWBC_DEV void load_mass_columns(const real_t *A, PLA_REF(real_t, s, N), PL_REF(real_t, dg), real_t *G) {
    DWBC_LANE_DECL;
    LANES {
        const int col = lane < N ? lane : 0;
        const int cbase = col * (col + 1) / 2;
#pragma unroll
        for (int i = 0; i < N; i++) LV(s)[i] = (lane < N) ? A[i >= col ? i * (i + 1) / 2 + col : cbase + i] : real_t(0.0);
        LV(dg) = (lane < N) ? A[cbase + col] : real_t(1.0);
        if (lane < N) G[lane] = kGrav * A[col >= 2 ? cbase + 2 : 3 + col];  // A[2][col] (row 2 starts at 3)
    }
}

}  // namespace dwbc
