// eskf_tick_body.inc -- the body of the error-state filter's tick kernels, included by eskf_kernel.hip once per kernel: in eskf_tick_kernel<UPDATE>
// (predict only, or predict followed by update) and, with ESKF_TICK_MASKED defined, in eskf_tick_masked_kernel, where UPDATE is true and filter
// b runs the update tick where fix[b] != 0 and the predict-only tick where it is 0: a filter without a fix leaves the elimination with
// ok = false, the path a failed pivot takes, which leaves state and covariance at the prediction (the second eskf_mirror is idempotent on the
// exactly symmetric P_pred) and uses nothing that was made from gps_p, gps_v, q_meas or thrust.  ok is uniform over the filter's 32 lanes;
// lane 0 reads fix again for the status.  Text, not a function: inlining one shared function into the two existing kernels kept their
// instructions but renamed their registers (profiles/eskf_rates_isa.txt); included as text they compile to the code they always did.
// In scope: EskfArgs A; bool UPDATE; masked: const int* fix.
    __shared__ double sm[kEskfFilters * kEskfLds];
    const EskfConst& c = *A.c;
    const int f = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int inst0 = blockIdx.x * kEskfFilters + f;
    const bool live = inst0 < A.B;
    const int inst = live ? inst0 : A.B - 1;       // a dead half-wave repeats the last filter and writes nothing
    const int i = l < SN ? l : SN - 1;             // lanes 21..31 repeat row 20: the same values to the same LDS addresses
    double* Pm = sm + f * kEskfLds;
    double* U = Pm + SN * SN;
    double* dxs = U + SY * SY;
    double* xs = dxs + SN;
    double* ys = xs + SX;
    const double dt = c.dt;

    // ---- P -> LDS, 32 lanes wide; the nominal state and the IMU sample into every lane
    double* pg = A.P + (size_t)inst * (SN * SN);
#pragma unroll
    for (int m = 0; m < (SN * SN + 31) / 32; m++) {
        const int e = m * 32 + l;
        if (e < SN * SN) Pm[e] = pg[e];
    }
    double x[SX], a[3], w[3];
    {
        const double* xg = A.x + (size_t)inst * SX;
#pragma unroll
        for (int j = 0; j < SX; j++) x[j] = xg[j];
        const double* ig = A.imu + (size_t)inst * 6;
#pragma unroll
        for (int k = 0; k < 3; k++) { a[k] = ig[k] - x[13 + k]; w[k] = ig[3 + k] - x[10 + k]; }
    }
    __syncthreads();
    double row[SN];
#pragma unroll
    for (int j = 0; j < SN; j++) row[j] = Pm[i * SN + j];

    // ---- predict: the nominal state (Eskf.cpp:109-133) ...
    double q[4], M1[9], M2[9], E[9];
    {
        double q0[4], R[9], qe[4];
        q_unit(&x[6], q0);
        q_rot(q0, R);
        const double Ra[3] = {R[0] * a[0] + R[1] * a[1] + R[2] * a[2], R[3] * a[0] + R[4] * a[1] + R[5] * a[2], R[6] * a[0] + R[7] * a[1] + R[8] * a[2]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double g = x[16 + k];
            x[k] = x[k] + x[3 + k] * dt + 0.5 * Ra[k] * dt * dt + 0.5 * g * dt * dt;
            x[3 + k] = x[3 + k] + Ra[k] * dt + g * dt;
        }
        q_exp(w[0] * dt, w[1] * dt, w[2] * dt, qe);
        q_mul_unit(q0, qe, q);
        // ... and the blocks of F (:150-157), from the NEW attitude
        q_rot(q, R);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            M1[r * 3 + 0] = -(R[r * 3 + 1] * a[2] - R[r * 3 + 2] * a[1]) * dt;
            M1[r * 3 + 1] = -(R[r * 3 + 2] * a[0] - R[r * 3 + 0] * a[2]) * dt;
            M1[r * 3 + 2] = -(R[r * 3 + 0] * a[1] - R[r * 3 + 1] * a[0]) * dt;
#pragma unroll
            for (int k = 0; k < 3; k++) M2[r * 3 + k] = -R[r * 3 + k] * dt;
        }
        q_exp(-(w[0] * dt), -(w[1] * dt), -(w[2] * dt), qe);
        q_rot(qe, E);
    }
    // ---- B = P F': columns 0..8 of the lane's own row
    {
        double t0[3], t1[3], t2[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            t0[r] = fma(dt, row[3 + r], row[r]);
            double s = fma(dt, row[15 + r], row[3 + r]), e = -dt * row[9 + r];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s = fma(M1[r * 3 + k], row[6 + k], s);
                s = fma(M2[r * 3 + k], row[12 + k], s);
                e = fma(E[r * 3 + k], row[6 + k], e);
            }
            t1[r] = s; t2[r] = e;
        }
#pragma unroll
        for (int r = 0; r < 3; r++) { row[r] = t0[r]; row[3 + r] = t1[r]; row[6 + r] = t2[r]; }
    }
    __syncthreads();   // every lane has its row of P out of LDS
#pragma unroll
    for (int j = 0; j < SN; j++) Pm[i * SN + j] = row[j];      // (lanes 21..31: what lane 20 writes)
    __syncthreads();
    // ---- P_pred = F B + diag(Q): rows 0..8; the coefficients of the lane's row of F are selected, not indexed
    if (i < 9) {
        const int grp = i / 3, r = i - 3 * grp;
        double ca[3], cb[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double m1 = r == 0 ? M1[k] : (r == 1 ? M1[3 + k] : M1[6 + k]);
            const double m2 = r == 0 ? M2[k] : (r == 1 ? M2[3 + k] : M2[6 + k]);
            const double ee = r == 0 ? E[k] : (r == 1 ? E[3 + k] : E[6 + k]);
            ca[k] = grp == 1 ? m1 : (grp == 2 ? ee : 0.0);
            cb[k] = grp == 1 ? m2 : 0.0;
        }
        const double d = grp == 2 ? -dt : dt;
        const int rd = grp == 0 ? 3 + r : (grp == 1 ? 15 + r : 9 + r);
#pragma unroll
        for (int j = 0; j < SN; j++) {
            double s = grp == 2 ? 0.0 : row[j];
            s = fma(d, Pm[rd * SN + j], s);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s = fma(ca[k], Pm[(6 + k) * SN + j], s);
                s = fma(cb[k], Pm[(12 + k) * SN + j], s);
            }
            row[j] = s;
        }
    }
    {
        const double qi = c.Q[i];
#pragma unroll
        for (int j = 0; j < SN; j++) row[j] += (j == i) ? qi : 0.0;
    }
    eskf_mirror(Pm, row, i);
#pragma unroll
    for (int k = 0; k < 4; k++) x[6 + k] = q[k];

    bool ok = true;
    if constexpr (UPDATE) {
        // ---- innovation (:203-272), every lane
        {
            double y[SY], qm[4], R[9], Rm[9];
            q_unit(A.qm + (size_t)inst * 4, qm);
            q_rot(q, R);
            q_rot(qm, Rm);
            const double* gp = A.gps_p + (size_t)inst * 3;
            const double* gv = A.gps_v + (size_t)inst * 3;
            const double* tg = A.thrust + (size_t)inst * 6;
            double th[6];
#pragma unroll
            for (int k = 0; k < 6; k++) th[k] = tg[k];
            const double qc[4] = {q[0], -q[1], -q[2], -q[3]};
            double dq[4], att[3];
            q_mul_unit(qc, qm, dq);
            q_log(dq, att);
            const double mrb[3] = {c.mass * a[0] + c.mzg * w[1], c.mass * a[1] - c.mzg * w[0], c.mass * a[2]};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                y[k] = gp[k] - x[k];
                y[3 + k] = gv[k] - x[3 + k];
                y[6 + k] = att[k];
                const double vB = R[k] * x[3] + R[3 + k] * x[4] + R[6 + k] * x[5];          // R' v
                const double gB = -c.g * Rm[6 + k];                                        // R(q_meas)' (0, 0, -g)
                const double ma = c.am[k] * (a[k] + gB);
                const double d3 = (-c.Dl[k] - c.Dnl[k] * fabs(vB)) * vB;
                const double g3 = -c.wb * R[6 + k];   // (m g - b) [sin th, -cos th sin ph, -cos th cos ph] = -(m g - b) (row 2 of R)
                double tau = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) tau += c.K3[k * 6 + m] * th[m];
                y[9 + k] = tau - (mrb[k] - x[19 + k] + ma + d3 + g3);
            }
            // the predicted state and the innovation wait in LDS (every lane of the filter writes the same values) while the registers hold
            // the rows of S and of the gain
#pragma unroll
            for (int j = 0; j < SX; j++) xs[j] = x[j];
#pragma unroll
            for (int b = 0; b < SY; b++) ys[b] = y[b];
        }
        // ---- S = H P H' + diag(R12): lane a < 12 gathers row a; elimination without row exchanges, the pivot row through LDS
        double ipk[SY];
        {
            const int as = l < SY ? l : SY - 1;      // lanes 12..31 repeat row 11: the same values to the same addresses
            const int ha = eskf_hsel(as);
            const double sa = eskf_hsgn(as), r12 = c.R12[as];
            double srow[SY];
#pragma unroll
            for (int b = 0; b < SY; b++) srow[b] = (sa * eskf_hsgn(b)) * Pm[ha * SN + eskf_hsel(b)] + ((b == as) ? r12 : 0.0);
            // step k: every lane puts its row as it stands into LDS (rows <= k are final: the factor), the pivot row comes back to all, rows
            // below it are updated -- selected, not branched: straight-line code between the barriers
#pragma unroll
            for (int k = 0; k < SY; k++) {
#pragma unroll
                for (int j = k; j < SY; j++) U[as * SY + j] = srow[j];
                __syncthreads();
                const double pk = U[k * SY + k];
                ok = ok && (pk > 0.0) && (pk < 1e300);
                ipk[k] = 1.0 / pk;
                const double fk = srow[k] * ipk[k];
#pragma unroll
                for (int j = k + 1; j < SY; j++) {
                    const double t = fma(-fk, U[k * SY + j], srow[j]);
                    srow[j] = (as > k) ? t : srow[j];
                }
            }
        }
        // ---- row i of the gain: S z = (P H')[i,:]', two substitutions; dx_i; row i of P - Kal (P H')'
#ifdef ESKF_TICK_MASKED
        ok = ok && fix[inst] != 0;   // (read here, behind the elimination, where no register is short)
#endif
        double dxi = 0.0;
        if (ok) {
            double z[SY], t[SY];
#pragma unroll
            for (int b = 0; b < SY; b++) {
                double s = eskf_hsgn(b) * row[eskf_hsel(b)];
#pragma unroll
                for (int k = 0; k < b; k++) s = fma(-U[k * SY + b], t[k], s);
                z[b] = s; t[b] = s * ipk[b];
            }
#pragma unroll
            for (int b = SY - 1; b >= 0; b--) {
                double s = z[b];
#pragma unroll
                for (int j = b + 1; j < SY; j++) s = fma(-U[b * SY + j], z[j], s);
                z[b] = s * ipk[b];
            }
#pragma unroll
            for (int b = 0; b < SY; b++) dxi = fma(z[b], ys[b], dxi);
#pragma unroll
            for (int b = 0; b < SY; b++) {
                const double zb = -eskf_hsgn(b) * z[b];
#pragma unroll
                for (int j = 0; j < SN; j++) row[j] = fma(zb, Pm[eskf_hsel(b) * SN + j], row[j]);
            }
        }
        dxs[i] = dxi;
        eskf_mirror(Pm, row, i);   // (its first barrier also puts dxs in front of the reads below)
        // ---- inject (:320-332)
#pragma unroll
        for (int j = 0; j < SX; j++) x[j] = xs[j];
        if (ok) {
            const double q[4] = {x[6], x[7], x[8], x[9]};
            double dx[SN];
#pragma unroll
            for (int j = 0; j < SN; j++) dx[j] = dxs[j];
            double qe[4], qn[4];
            q_exp(dx[6], dx[7], dx[8], qe);
            q_mul_unit(q, qe, qn);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                x[k] += dx[k];
                x[3 + k] += c.vel_inject * dx[3 + k];
                x[19 + k] += dx[18 + k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) x[6 + k] = qn[k];
            if (c.inject) {
#pragma unroll
                for (int k = 0; k < 9; k++) x[10 + k] += dx[9 + k];
            }
        }
    }
    // ---- out: P 32 lanes wide out of LDS, the state and the outputs by lane 0
    if (live) {
#pragma unroll
        for (int m = 0; m < (SN * SN + 31) / 32; m++) {
            const int e = m * 32 + l;
            if (e < SN * SN) pg[e] = Pm[e];
        }
        if (l == 0) {
            double* xg = A.x + (size_t)inst * SX;
            bool fin = true;
#pragma unroll
            for (int j = 0; j < SX; j++) { xg[j] = x[j]; fin = fin && (fabs(x[j]) < 1e300); }
            const double qf[4] = {x[6], x[7], x[8], x[9]};
            double R[9];
            q_rot(qf, R);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                A.xi[(size_t)inst * 3 + k] = x[19 + k];
                A.xw[(size_t)inst * 3 + k] = R[k * 3] * x[19] + R[k * 3 + 1] * x[20] + R[k * 3 + 2] * x[21];
            }
            double* mp = A.mp + (size_t)inst * 4;
            mp[0] = x[19] * c.inv_cc; mp[1] = x[20] * c.inv_cc; mp[2] = x[21] * c.inv_rc; mp[3] = 0.0;
#ifdef ESKF_TICK_MASKED
            A.status[inst] = (fix[inst] != 0 && !ok) ? 1 : (fin ? 0 : 2);
#else
            A.status[inst] = !ok ? 1 : (fin ? 0 : 2);
#endif
        }
    }
