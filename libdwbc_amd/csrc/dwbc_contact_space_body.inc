// dwbc_contact_space_body.inc -- the contact stage of contact_space_instance (dwbc_contact_space.h) behind stage 0, as shared text: the
// contact-space kernel includes it with the mask of its request, the task-space kernel (dwbc_task_space.h) with the bits of what its levels
// need.  The including function provides th, su, io, inst, L, topo, nb, kTree, the map S (LdsCs or a map derived from it), M, C, the register
// columns s / dg as stage 0 left them, st_contact, `mask` and the output pointers o_JC .. o_rot (one whose bit is clear is never read).
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

#ifdef DWBC_CS_BEFORE_W_INV
        DWBC_CS_BEFORE_W_INV  // (dwbc_task_space.h: what its levels need of the columns A^-1 N_c, which die in the sweep below)
#endif
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
