// dwbc_task_space_level_front.inc -- one task level ahead of the W^+ sweep, as shared text: J_task, T1 = J_task (A^-1 N_c) one column per lane,
// Lambda^-1 = T1 J_task^T and Lambda_task (wbd.cpp:210).  The task-space kernel (dwbc_task_space.h) includes it once per level, the
// single-level task-QP kernel (dwbc_task_qp.h) for its one level.  The including scope provides th, su, the map S, L, N, NB, NT, T, topo, nb,
// the register columns s, `want` with put_j_task, Jt, st_task, the level lv and ls, the index of the level's blocks in the map (T1, Lt, G, Pt).
    const int t = su.t_dof[lv];
    const unsigned long long tm = su.t_dofmask[lv];
    real_t *T1 = L + S::e_T1 + ls * T * N, *Lt = L + S::e_Lt + ls * T * T;
    task_jacobian_rows<N, NB, NT>(th, su, lv, L + S::Rw0, L + S::pw, L + S::aw, topo, nb, L + S::e_Pt + ls * kMaxTaskLinks * 3, L + S::e_Jcm, Jt);
    if (want & kTsJTask) put_j_task(lv);
    LANES {  // T1[:, lane] = J_task (lane's column of A^-1 N_c)
        real_t tc_[T];
#pragma unroll
        for (int r = 0; r < T; r++) tc_[r] = real_t(0.0);
#pragma unroll
        for (int ib = 0; ib < N; ib += 3) {  // one uniform branch per 3 columns, as in the cycle: the zero columns of J_task are skipped
            if ((tm >> ib) & 7) {
#pragma unroll
                for (int i = ib; i < ib + 3 && i < N; i++)
#pragma unroll
                    for (int r = 0; r < T; r++) tc_[r] += Jt[i * T + r] * LV(s)[i];
            }
        }
        if (lane < N) {
#pragma unroll
            for (int r = 0; r < T; r++) T1[r * N + lane] = tc_[r];
        }
    }
    DWBC_SYNC();
    real_t *Gl = L + S::e_G + ls * T * T;
    mm_nn<NT>(th, Gl, t, T1, N, Jt, T, t, N, t);  // Lambda^-1 = J_task A^-1 N_c J_task^T, kept for the level's J_kt
    if (!spd_inverse_small(Gl, t, t, Lt, t, L + S::c_s1)) st_task = 0;
    newton_step_small<NT>(th, Gl, Lt, t, L + S::e_Pi, L + S::e_cod);
