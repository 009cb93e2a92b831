// dwbc_task_space_level_back.inc -- one task level behind the W^+ sweep, as shared text: Q = (Lambda T1)[:, 6:], Q W^+, J_kt = (Q W^+)^T
// pinv(Q W^+ Q^T) (wbd.cpp:212-214, CalculateJKT) and X = J_kt Lambda with its step on the right inverse.  Included inside a loop or a
// do { } while (0): a rejected t x t block leaves through `break` with st_task = 0.  The including scope provides th, su, the map S, L, N, NT, T,
// M, t, T1, Lt, Wp, Q, QW, Jk, Pi, s2, cod, st_task and ls, the index of the level's blocks in the map; it is left with X (M x t, over Q) and
// U (over QW, free).
    for (int idx = th.tid; idx < t * M; idx += NT) {  // Q = (Lambda T1)[:, 6:]
        const int i = idx / M, j = idx - i * M;
        real_t acc = real_t(0.0);
        for (int p = 0; p < t; p++) acc += Lt[i * t + p] * T1[p * N + 6 + j];
        Q[idx] = acc;
    }
    DWBC_SYNC();
    mm_nn<NT>(th, QW, M, Q, M, Wp, M, t, M, M);  // Q W^+
    DWBC_SYNC();
    mm_nt<NT>(th, s2, t, QW, M, Q, M, t, M, t);  // Q W^+ Q^T
    real_t pr_ = real_t(1.0);
    bool truncated = false;
    int cond = spd_inverse_small(s2, t, t, Pi, t, L + S::c_s1, &pr_);  // PinvCODWB, full-rank case: the SPD inverse
    if (cond) newton_step_small<NT>(th, s2, Pi, t, cod, cod + T * T);
    DWBC_SYNC();
    if (!cond || pr_ < kCodCheck) {  // as the cycle: the rank decision of the reference's complete orthogonal decomposition
        const int rk = pinv_cod_small<NT>(th, s2, t, kCodThreshold, Pi, cod, cod + T * T, cod + 2 * T * T, cod + 3 * T * T);
        if (rk < t) { cond = 1; truncated = true; }
    }
    if (!cond) { st_task = 0; break; }
    DWBC_SYNC();
    for (int idx = th.tid; idx < M * t; idx += NT) {  // J_kt = W^+ Q^T pinv(.) = (Q W^+)^T pinv(.), M x t
        const int i = idx / t, j = idx - i * t;
        real_t acc = real_t(0.0);
        for (int r = 0; r < t; r++) acc += QW[r * M + i] * Pi[r * t + j];
        Jk[idx] = acc;
    }
    DWBC_SYNC();
    // A caller multiplies J_kt Lambda back onto Y = T1[:, 6:] (Y X = I makes I - X Y the level's projector): one step on the right
    // inverse, X <- X - X (Y X - I), takes out what the m-long sums of Q W^+ and Q W^+ Q^T left in Y X - I (2 - 3e-13 in host emulation,
    // five times the restatement's; behind the step, its level).  J_kt = X Lambda^-1 keeps the column space of W^+ Q^T.
    real_t *X = Q, *U = QW;  // both dead behind J_kt
    mm_nn<NT>(th, X, t, Jk, t, Lt, t, M, t, t);  // X = J_kt Lambda, M x t
    DWBC_SYNC();
    if (!truncated) {  // (a truncated pseudo-inverse has Y X != I by design)
    for (int idx = th.tid; idx < t * t; idx += NT) {  // E = Y X - I
        const int i = idx / t, j = idx - i * t;
        real_t acc = (i == j) ? real_t(-1.0) : real_t(0.0);
        for (int c = 0; c < M; c++) acc += T1[i * N + 6 + c] * X[c * t + j];
        s2[idx] = acc;
    }
    DWBC_SYNC();
    for (int i = th.tid; i < M; i += NT) {  // row i of X - X E, in place: the row is read before it is written
        real_t xr[T], xn[T];
        for (int j = 0; j < t; j++) xr[j] = X[i * t + j];
        for (int j = 0; j < t; j++) {
            real_t acc = xr[j];
            for (int r = 0; r < t; r++) acc -= xr[r] * s2[r * t + j];
            xn[j] = acc;
        }
        for (int j = 0; j < t; j++) X[i * t + j] = xn[j];
    }
    DWBC_SYNC();
    mm_nn<NT>(th, Jk, t, X, t, L + S::e_G + ls * T * T, t, M, t, t);  // J_kt = X Lambda^-1
    DWBC_SYNC();
    }
