// dwbc_cycle2_stage0.inc -- textual part of the fused cycle shared by cycle_instance_v2 (dwbc_cycle2.h) and
// cycle_instance_reduced (dwbc_reduced.h): kinematics, CRBA, column-per-lane load of A and the A^-1 sweep.
// Expects in scope: S (LDS map), N, NB, NT, th, su, io, L, body, topo, nb, qin, dump, dl, diag, s, dg.
// Defines: st_contact.  With DWBC_STAGE0_FRONT_ONLY defined the text ends behind the column-per-lane load (dwbc_dynamics.h).
    // ================= stage 0: kinematics and CRBA (src/dwbc.cpp:279-371) =================
    for (int i = th.tid; i < N + 1; i += NT) L[S::q + i] = (real_t)qin[i];
    for (int i = th.tid; i < 3 * M; i += NT) L[S::tg + i] = real_t(0.0);
    DWBC_SYNC();
    DWBC_FSTAMP(32);
    // coupled dof pairs of the mass matrix for the CRBA below (Model::topo_table): fetched here, behind the fence, so that the
    // joint rotations below cover the latency; used after the kinematics
    constexpr int kPairRounds = (N * (N + 1) / 2 + NT - 1) / NT;  // a chain is the worst case; TOCABI: 396 pairs, 7 rounds
    const int npair = topo[3 * nb];
    int pairw[kPairRounds];
#pragma unroll
    for (int r = 0; r < kPairRounds; r++) pairw[r] = (r * NT + th.tid < npair) ? topo[3 * nb + 1 + r * NT + th.tid] : 0;
    {
        real_t *Rw = L + S::Rw, *pw = L + S::pw, *aw = L + S::aw, *Rl = L + S::k_Rl;
        const real_t *q = L + S::q;
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
        DWBC_FSTAMP(33);
        // world transforms by pointer jumping: T_i <- T_anc(i) o T_i, anc(i) <- anc(anc(i)); ceil(log2(depth+1)) rounds of
        // one 3x3 product per body instead of `depth` dependent rounds.  Buffer 0 = (Rw, pw), buffer 1 = (k_Rl, k_Iw);
        // ancestor indices ride along as doubles in k_Ic.  (T_a o T_i: R = R_a R_i, p = p_a + R_a p_i.)
        {
            int rounds = 0;
            if constexpr (kTree) {
                constexpr int md = std::conditional<kTree, Topo, TopoTocabi>::type::maxdepth;
                while ((1 << rounds) < md + 1) rounds++;
            } else {
                while ((1 << rounds) < su.maxdepth + 1) rounds++;
            }
            const bool odd = rounds & 1;  // start in the buffer that makes the last round land in (Rw, pw)
            real_t *Rc = odd ? Rl : Rw, *Rn = odd ? Rw : Rl;
            real_t *pc = odd ? L + S::k_Iw : pw, *pn = odd ? pw : L + S::k_Iw;
            real_t *ac = L + S::k_anc, *an_ = L + S::k_anc + NB;
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
        DWBC_SYNC();
        real_t *Iw = L + S::k_Iw;
        DWBC_FSTAMP(34);
        for (int i = th.tid; i < nb; i += NT) {
            const real_t *bd = body + i * kBodyStride;
            const real_t *R = Rw + i * 9;
            for (int a = 0; a < 3; a++) aw[i * 3 + a] = R[a * 3] * bd[BF_AXIS] + R[a * 3 + 1] * bd[BF_AXIS + 1] + R[a * 3 + 2] * bd[BF_AXIS + 2];
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
        DWBC_FSTAMP(35);
        // composite inertia of the subtree [i, i + len_i) (bodies are numbered depth first).  Window sums of length 2^k
        // by doubling, S_{k+1}[i] = S_k[i] + S_k[i + 2^k] (ping-pong Iw <-> k_Ic); the subtree sum picks S_k at the set bits
        // of len_i, so no differences of large prefix sums are taken.  Lane i owns body i: its 10 window sums and its
        // accumulator stay in registers, every round is one batch of independent LDS loads.
        real_t *Icm = L + S::k_Ic;
        {
            real_t *Sc = Iw, *Sn = Icm;
            PLA(real_t, sk, 10);
            PLA(real_t, acc, 10);
            PL(int, len);
            LANES {
                const int bi = lane < nb ? lane : 0;
                LV(len) = lane < nb ? topo[2 * nb + bi] : 0;
#pragma unroll
                for (int c = 0; c < 10; c++) { LV(sk)[c] = Sc[bi * 10 + c]; LV(acc)[c] = real_t(0.0); }
            }
            for (int kbit = 0, off = 1; off <= nb; kbit++, off <<= 1) {  // <=: a root subtree of exactly 2^k bodies takes its sum at off = nb
                LANES {
                    const bool take = (LV(len) >> kbit) & 1;
                    int pos = lane + (LV(len) & (off - 1));
                    pos = (take && pos < nb) ? pos : 0;
                    const bool nbr = lane + off < nb;
                    const int pn = nbr ? lane + off : 0;
                    real_t a_[10], b_[10];
#pragma unroll
                    for (int c = 0; c < 10; c++) { a_[c] = Sc[pos * 10 + c]; b_[c] = Sc[pn * 10 + c]; }
#pragma unroll
                    for (int c = 0; c < 10; c++) {
                        LV(acc)[c] += take ? a_[c] : real_t(0.0);
                        LV(sk)[c] += nbr ? b_[c] : real_t(0.0);
                        if (lane < nb) Sn[lane * 10 + c] = LV(sk)[c];
                    }
                }
                DWBC_SYNC();
                { real_t *t_ = Sc; Sc = Sn; Sn = t_; }
            }
            LANES {
                if (lane < nb) {
#pragma unroll
                    for (int c = 0; c < 10; c++) Icm[lane * 10 + c] = LV(acc)[c];
                }
            }
            DWBC_SYNC();
        }
        DWBC_FSTAMP(36);
        real_t *Sm = L + S::k_S, *Fm = L + S::k_F;
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
        DWBC_FSTAMP(37);
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
        DWBC_SYNC();
        DWBC_FSTAMP(38);
        // A[j][k] = S_k . F_j for k on the path from j to the root (CRBA, [ext] RBDL CompositeRigidBodyAlgorithm), staged
        // through LDS once and then loaded column-per-lane into registers
        real_t *A = L + S::k_A;
        constexpr bool kPacked = S::a_packed;  // lower triangle, row-packed: (i, j <= i) at i (i + 1) / 2 + j
        for (int idx = th.tid; idx < (kPacked ? N * (N + 1) / 2 : N * N); idx += NT) A[idx] = real_t(0.0);
        DWBC_SYNC();
        DWBC_FSTAMP(39);
#pragma unroll
        for (int r = 0; r < kPairRounds; r++) {
            if (r * NT + th.tid < npair) {
                const int j = pairw[r] >> 8, kk = pairw[r] & 255;  // kk <= j: a dof on the path from j to the root
                const real_t *f = Fm + j * 6, *sv = Sm + kk * 6;
                const real_t v = sv[0] * f[0] + sv[1] * f[1] + sv[2] * f[2] + sv[3] * f[3] + sv[4] * f[4] + sv[5] * f[5];
                if constexpr (kPacked) {
                    A[j * (j + 1) / 2 + kk] = v;
                } else {
                    A[j * N + kk] = v;
                    A[kk * N + j] = v;
                }
            }
        }
        DWBC_SYNC();
        DWBC_FSTAMP(40);
        LANES {
            const int col = lane < N ? lane : 0;
            if constexpr (kPacked) {
                const int cbase = col * (col + 1) / 2;
#pragma unroll
                for (int i = 0; i < N; i++) LV(s)[i] = (lane < N) ? A[i >= col ? i * (i + 1) / 2 + col : cbase + i] : real_t(0.0);
                LV(dg) = (lane < N) ? A[cbase + col] : real_t(1.0);
                if (lane < N) L[S::G + lane] = kGrav * A[col >= 2 ? cbase + 2 : 3 + col];  // A[2][col] (row 2 starts at 3)
            } else {
#pragma unroll
                for (int i = 0; i < N; i++) LV(s)[i] = (lane < N) ? A[i * N + col] : real_t(0.0);
                LV(dg) = (lane < N) ? A[col * N + col] : real_t(1.0);
                if (lane < N) L[S::G + lane] = kGrav * A[2 * N + col];  // G_ = -J_com_lin^T m g = 9.81 * A[2,:] (dwbc.cpp:358)
            }
        }
        DWBC_FSTAMP(41);
        if (dump) {
            LANES {
                if (lane < N) {
#pragma unroll
                    for (int i = 0; i < N; i++) dump[dl.A + i * N + lane] = LV(s)[i];
                }
            }
            for (int idx = th.tid; idx < nb * 9; idx += NT) dump[dl.link_R + idx] = Rw[idx];
            for (int idx = th.tid; idx < nb * 3; idx += NT) dump[dl.link_p + idx] = pw[idx];
            dump_centroidal<N, NT>(th, A, N, Rw, L + S::q, A[0], dump, dl);  // A(0,0) = total mass
        }
        if (kExtras && !io.hqp && th.tid == 0) {  // com_pos for the closed-form redistribution (dwbc.cpp:320-324): R0 A[3:6,0:3] / m unskewed
            const int ra[3] = {2, 0, 1}, cb[3] = {1, 2, 0};
            for (int e = 0; e < 3; e++) {
                real_t acc = real_t(0.0);
                for (int b = 0; b < 3; b++) acc += Rw[ra[e] * 3 + b] * A[(3 + b) * N + cb[e]];
                L[S::comp + e] = acc / A[0] + L[S::q + e];
            }
        }
        if (kExtras && su.has_com_task) {  // Jacobian of the COM link for COM task levels (the staged A is still intact in rows 0..5)
            DWBC_SYNC();
            com_jacobian<N, NT>(th, A, N, Rw, L + S::q, L + S::Jcm);
            DWBC_SYNC();
        }
    }
    DWBC_STAMP(0);  // kinematics + CRBA done
    int st_contact = 1;
#ifndef DWBC_STAGE0_FRONT_ONLY  // (dwbc_dynamics.h ends the text here: its A^-1 sweep is optional, and it stages no task reference)
    // A_inv (dwbc.cpp:307)
    if constexpr (std::is_same<Topo, TopoGeneric>::value) {
        // beyond 40 columns the runtime-pivot sweep would pick the lane's own pivot-row element from six candidate registers, which
        // the compiler turns into ONE load through a selected address -- and the whole column array then lives in scratch (4 x
        // slower at 43 dof).  Compile-time pivots (the dense "tree") keep every index static.
        // compact lean build (the redistribution kernel on any tree): leaves-first pivots fed through LDS, the dense form of the sweep the
        // constant-tree build of that kernel runs.  In this order the entries outside a tree's pattern stay exact zeros, so on a model
        // whose tree the constant-tree build knows the two builds compute the same A^-1 to the bit, where the ascending runtime pivots
        // below eliminate in another order (1e-16 apart in A^-1, which an ill-conditioned redistribution QP shows as 5e-9 Nm)
        if constexpr (S::compact && !kExtras && sizeof(real_t) == 8) {
            DWBC_SYNC();
            if (!sweep_inverse_tree_lds<TopoDense<N>, N>(s, dg, L + S::c_s1)) st_contact = 0;
            DWBC_SYNC();
        } else if constexpr (N > 40) {
            if (!sweep_inverse_tree<TopoDense<N>, N>(s, dg)) st_contact = 0;
        } else {
            if (!sweep_inverse_rl<N>(s, dg)) st_contact = 0;
        }
    } else {  // the launcher picks this instantiation only for a model whose parent table equals Topo's (Setup::topo_kind)
        // compact lean build: the pivot column through LDS (sweep_inverse_tree_lds: 2.3 k v_readlane / s_nop fewer per instance -- VALU
        // issue slots, which is what bounds this kernel at two waves per SIMD); the staged mass matrix under the column is dead
        // once the columns are in registers
#ifndef DWBC_COMPACT_REG_SWEEP
        if constexpr (S::compact && !kExtras && sizeof(real_t) == 8) {
            DWBC_SYNC();
            if (!sweep_inverse_tree_lds<Topo, N>(s, dg, L + S::c_s1)) st_contact = 0;
            DWBC_SYNC();
        } else
#endif
        if (!sweep_inverse_tree<Topo, N>(s, dg)) st_contact = 0;
    }
    if (dump) {
        LANES {
            if (lane < N) {
#pragma unroll
                for (int i = 0; i < N; i++) dump[dl.A_inv + i * N + lane] = LV(s)[i];
            }
        }
        for (int j = th.tid; j < N; j += NT) dump[dl.G + j] = L[S::G + j];
    }
    {
        // velocity-dependent UpdateKinematics outputs (dwbc_velocity.h; B_ and link velocities go to the dump record only)
        // and the task reference f* (dwbc_fstar.h)
        const bool want_traj = kExtras && io.traj != nullptr && su.n_traj > 0;
        const bool vel = kExtras && io.qdot != nullptr && (dump != nullptr || want_traj);
        if (vel)
            velocity_rnea<S, N, NB, NT>(th, su, io.qdot + (size_t)inst * N, body, topo, L, dump ? dump + dl.B : nullptr,
                                        dump ? dump + dl.link_v : nullptr, dump ? dump + dl.link_w : nullptr);
        task_reference<S, N, NB, NT, kExtras>(th, su, io, inst, body, L, vel ? L + S::k_Rl : nullptr);
    }
    DWBC_STAMP(1);  // A_inv done
#endif
