// dwbc_cycle2_stage1.inc -- textual part of the fused cycle shared by cycle_instance_v2 (dwbc_cycle2.h) and
// cycle_instance_reduced (dwbc_reduced.h): active contacts, J_C, Y = J_C A^-1, Lambda_c, J̄_c^T, s <- A^-1 N_c,
// the gravity pre-vector and P_C.  Expects the scope of stage 0 plus M, C.
// Defines: fl, act_c, nc, too_many, cd, k, JCt, Yt, Lam, JbT, cm0, cm1.
    // ================= stage 1: contacts (dwbc.h:432-474, dwbc.cpp:433-478, wbd.cpp:108-143) =================
    const unsigned char *fl = io.flags + (size_t)inst * su.n_contacts;
    int act_c[kMaxActiveContacts] = {0, 0};
    int nc = 0, nflag = 0;
    for (int i = 0; i < su.n_contacts; i++) {
        if (fl[i] && nc < kMaxActiveContacts) act_c[nc++] = i;
        nflag += fl[i] ? 1 : 0;
    }
    // more simultaneous contacts than the kernel stacks (the reference stacks any number, dwbc.cpp:445-453): never solved with a
    // subset -- the instance fails (status 0, zero torques and wrench); dwbc_batch_set_contact refuses such flags on the host
    const bool too_many = nflag > kMaxActiveContacts;
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
    if constexpr (S::compact) {
        // the link rotations (in the U region) die here: keep the pelvis rotation for the base columns of the point Jacobians and
        // take the world points of the task links now (dwbc.cpp:700-712: link position + R * local point)
        for (int r = th.tid; r < 9; r += NT) L[S::Rw0 + r] = L[S::Rw + r];
        for (int idx = th.tid; idx < su.n_levels * kMaxTaskLinks * 3; idx += NT) {
            const int lv = idx / (kMaxTaskLinks * 3), li = (idx / 3) % kMaxTaskLinks, a = idx % 3;
            if (li < su.t_nlinks[lv]) {
                const int mode = su.t_mode[lv][li], link = su.t_link[lv][li];
                real_t pl[3] = {0, 0, 0};
                if ((mode == TASK_LINK_6D_COM_FRAME || mode == TASK_LINK_POSITION_COM_FRAME) && link < nb)
                    for (int b = 0; b < 3; b++) pl[b] = body[link * kBodyStride + BF_COM + b];
                else if (mode == TASK_LINK_6D_CUSTOM_FRAME || mode == TASK_LINK_POSITION_CUSTOM_FRAME)
                    for (int b = 0; b < 3; b++) pl[b] = su.t_point[lv][li][b];
                const real_t *R = L + S::Rw + (link < nb ? link : 0) * 9;
                L[S::Pt + idx] = L[S::pw + (link < nb ? link : 0) * 3 + a] + R[a * 3] * pl[0] + R[a * 3 + 1] * pl[1] + R[a * 3 + 2] * pl[2];
            }
        }
    }
    DWBC_SYNC();
    // J_C and Y = J_C A^-1 are kept TRANSPOSED in LDS (N x C): all C contact rows of one column are 96 contiguous bytes,
    // so "own column . all rows" products fetch them with broadcast b128 reads and run C independent FMA chains
    real_t *JCt = L + S::c_JC, *Yt = L + S::c_Y, *Lam = L + S::c_Lam, *JbT = L + S::JbT;
    DWBC_FSTAMP(0);
    for (int idx = th.tid; idx < C * N; idx += NT) { JCt[idx] = real_t(0.0); Yt[idx] = real_t(0.0); JbT[idx] = real_t(0.0); }  // (the staged A is dead)
    DWBC_SYNC();
    for (int a = 0; a < nc; a++)
        point_jacobian<N, NB, NT>(th, L + S::Rw0, L + S::pw, L + S::aw, topo, nb, su.c_link[act_c[a]], L + S::Pc + a * 3, JCt, 1, 6 * a, 6, 0, C);
    DWBC_SYNC();
    DWBC_FSTAMP(1);  // J_C built
    if constexpr (S::compact) {
        // compact map: Jbar^T will be written over J_C, so its only later reader -- the internal-wrench basis Vb of the NwJw block
        // (dwbc_cycle2.h) -- is formed here
        if (k > 0) internal_wrench_basis<N, NT>(th, L + S::Pc, JCt, L + S::c_Vb);
        DWBC_SYNC();
    }
    // Y[:, lane] = J_C * (lane's column of A^-1).  Column i of J_C is zero unless dof i lies between the contact link and
    // the base (su.c_dofmask): uniform branches skip the zero columns, per contact.
    const unsigned long long cm0 = nc > 0 ? su.c_dofmask[act_c[0]] : 0ull, cm1 = nc > 1 ? su.c_dofmask[act_c[1]] : 0ull;
    static_assert(C == 12, "two 6D contacts");
    LANES {
        real_t yc[C];
#pragma unroll
        for (int p = 0; p < C; p++) yc[p] = real_t(0.0);
#pragma unroll
        for (int ib = 0; ib < N; ib += 3) {  // one uniform branch per 3 columns and contact (a branch costs ~40 cycles)
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
    DWBC_FSTAMP(2);  // Y
    // Lambda_c lives in a C x C block with row stride C whatever cd is, zero outside cd x cd: the products below run
    // over all C x C entries without per-element guards (the rows of Y / J_C beyond cd are zero as well)
    contact_gram<N, C, NT, S::c_s2>(th, Yt, JCt, cd, L);  // J A^-1 J^T = Y J_C^T (one matrix-core tile on the fp64 device: dwbc_cycle2.h)
    if (cd > 0) {
        if (!spd_inverse_small(L + S::c_s2, C, cd, Lam, C, L + S::c_s1)) st_contact = 0;  // Lambda_c (wbd.cpp:115)
    }
    DWBC_SYNC();
    DWBC_FSTAMP(3);  // Lambda_c
    // J̄^T = Lambda J A^-1 (wbd.cpp:116), then A^-1 N_c = A^-1 - Y^T J̄^T (wbd.cpp:117-118, N_c never materialised)
    LANES {
        real_t yc[C], jb[C];
        const int col = lane < N ? lane : 0;
#pragma unroll
        for (int p = 0; p < C; p++) yc[p] = Yt[col * C + p];
        lds_rows_dot<C, C, C, 4, 0, S::batch_reads && S::c_Lam % 2 == 0>(Lam, yc, jb);  // column `lane` of Jbar^T = Lambda_c Y
#pragma unroll
        for (int p = 0; p < C; p++)
            if (lane < N) JbT[p * N + lane] = jb[p];
        real_t dsub = real_t(0.0);
#pragma unroll
        for (int p = 0; p < C; p++) dsub += yc[p] * jb[p];
        LV(dg) -= dsub;
        lds_rows_dot<N, C, C, 2, 1, S::batch_reads && S::c_Y % 2 == 0>(Yt, jb, LV(s));  // s[i] -= Y^T[i, :] . Jbar^T[:, lane]  (reads batched by hand, two rows at a time: the register-capped builds have no room for more)
    }
    DWBC_SYNC();
    if (dump) {
        for (int idx = th.tid; idx < cd * N; idx += NT) { dump[dl.J_C + idx] = JCt[(idx % N) * C + idx / N]; dump[dl.J_C_INV_T + idx] = JbT[idx]; }
        for (int idx = th.tid; idx < cd * cd; idx += NT) dump[dl.Lambda_c + idx] = Lam[(idx / cd) * C + idx % cd];
        LANES {
            if (lane < N) {
#pragma unroll
                for (int i = 0; i < N; i++) dump[dl.A_inv_N_C + i * N + lane] = LV(s)[i];
            }
        }
    }
    DWBC_FSTAMP(5);  // AiNc
    // gravity pre-vector (A^-1 N_c G) and P_C = J̄^T G  (wbd.cpp:186-192)
    LANES {
        real_t gv1[1];
        lds_rows_dot<1, N, 2 * ((N + 1) / 2), 1, 0, S::batch_reads && S::G % 2 == 0>(L + S::G, LV(s), gv1);
        if (lane < N) L[S::c_vec + lane] = gv1[0];
    }
    mv_n<NT>(th, L + S::PC, JbT, N, L + S::G, cd, N);
    DWBC_STAMP(2);  // J_C, Lambda_c, J̄, A^-1 N_c done
    DWBC_FSTAMP(6);  // vec, PC
