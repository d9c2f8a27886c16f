// The bodies of k_bloch_train_run_gn (DESIGN 8ab) and k_bloch_train_run_sched_gn (DESIGN 8af), included twice by sim_dev.h: as they are,
// the component fits, and as ..._mag with TRAIN_MAG true, the magnitude fits of (|Mxy|, mz) (DESIGN 8ai).  The two passes differ in
// the two blocks that make a cotangent (lambda_N and ce_k) and in nothing else; with TRAIN_MAG the weights are two planes (xy, z),
// PE / PO apart, and rho and u are those of the primal echo, formed with k_bloch_train_run's statements, and of m_N.
// TRAIN_GN_BODY(name): the function's name in this pass; TRAIN_MAG: false or true.

// k_bloch_train_run_gn for the workgroup bk = (pulse, scale, chunk of 256 points, direction).
__device__ __forceinline__ void TRAIN_GN_BODY(bloch_train_run_gn_body)(
    const SimBlock bk, const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep,
    const int* __restrict__ gidx, const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses,
    const TrainPulseDev* __restrict__ trains, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0, int demod, int ebcast,
    int ndir, const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, long WT, long CK, double* ck,
    double* cw) {
    __shared__ double2 scs[256];
    __shared__ double srw[256];
    __shared__ int sgi[256];
    const int tid = threadIdx.x;
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain, dir = bk.pad;
    const double meq = Tr.meq;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;
    const long blk = (long)bk.scale * npair + pair;
    const long comb0 = (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    const double* wb = ws + Tr.w_off + comb0;
    // direction dir of the scale's first combination; a combination is ndir directions of TRAIN_ENT npair doubles
    const double* db = dws + (long)ndir * Tr.w_off + ((long)bk.scale * G * ndir + dir) * TRAIN_ENT * npair + (live ? pair : 0);
    const long gstr = (long)TRAIN_ENT * npair, dgstr = (long)ndir * gstr;
    double* cb = cw + (long)dir * WT + Tr.w_off + comb0;
    const long nch = (npair + 255) / 256;
    double* wck = ck + 2 * ((long)dir * CK + K.c_off + ((long)bk.scale * nch + bk.chunk) * K.ng * BLOCH_CK) + tid;
    const bool hoist = TGN_HOIST && G == 1;
    double m[3] = {0, 0, 1}, dm[3] = {0, 0, 0}, W[TRAIN_ENT], acc[TRAIN_ENT];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int e = 0; e < TRAIN_ENT; ++e) acc[e] = 0;
    if (hoist) {
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wb[e * npair];
    }
    auto stage = [&](int k0) {
        __syncthreads();
        const int cnt = min(256, ntr - k0);
        if (tid < cnt) {
            scs[tid] = rep[Tr.r_off + k0 + tid];
            sgi[tid] = gidx[Tr.r_off + k0 + tid];
            srw[tid] = rw ? rw[Tr.r_off + k0 + tid] : 1.0;
        }
        __syncthreads();
    };
    // (m_k, dm_k) -> (m_{k+1}, dm_{k+1}) from (u_k, du_k) (in v, dv), with the planes of the repetition in W[0 .. 11] and its tangent
    // planes at dg, as k_bloch_train_run_jvp steps them
    auto advance = [&](double c, double s, const double* dg, double v[3], double dv[3]) {
        double dW[12], n[3], dn[3];
#pragma unroll
        for (int e = 0; e < 12; ++e) dW[e] = dg[e * npair];
        train_affine_jvp(W, dW, dW + 9, meq, v, dv, dn);
        train_zm(c, s, dn);
        train_affine(W, W + 9, meq, v, n);
        train_zm(c, s, n);
        v[0] = n[0]; v[1] = n[1]; v[2] = n[2];
        dv[0] = dn[0]; dv[1] = dn[1]; dv[2] = dn[2];
    };
    for (int k0 = 0; k0 < ntr; k0 += 256) {                               // forwards: the checkpoints of m and dm
        stage(k0);
        const int cnt = min(256, ntr - k0);
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            if ((q & (TRV_T - 1)) == 0) {                                 // (m, dm) before repetition k0 + q
                double* w = wck + (long)((k0 + q) / TRV_T) * (2 * BLOCH_CK);
                w[0] = m[0]; w[256] = m[1]; w[512] = m[2];
                w[768] = dm[0]; w[1024] = dm[1]; w[1280] = dm[2];
            }
            if (!hoist) {
                const double* wg = wb + (long)sgi[q] * gstr;
#pragma unroll
                for (int e = 0; e < 12; ++e) W[e] = wg[e * npair];
            }
            train_zp(scs[q].x, scs[q].y, m);
            train_zp(scs[q].x, scs[q].y, dm);
            advance(scs[q].x, scs[q].y, db + (long)sgi[q] * dgstr, m, dm);
        }
    }
    double l[3] = {0, 0, 0};
    if (live && wf) {                                                     // lambda_N = wf dm_N
        const long o = P.o_off + blk;
        if (TRAIN_MAG) {                                                  // lambda_N = (w_xy (u . dm_xy) u, w_z dm_z), u of m_N
            const double wv[2] = {wf[o], wf[PO + o]};
            const BlochMagDir D = bloch_mag_dir(m[0], m[1]);
            bloch_mag_seed(D, wv, D.ux * dm[0] + D.uy * dm[1], dm[2], true, l);
        } else {
            l[0] = wf[o] * dm[0]; l[1] = wf[PO + o] * dm[1]; l[2] = wf[2 * PO + o] * dm[2];
        }
    }
    const long eo = ebcast ? P.o_off + blk : Tr.e_off + (long)bk.scale * ntr * npair + pair, kstr = ebcast ? 0 : npair;
    const double* wp = we ? we + eo : nullptr;
    const int klast = (ntr - 1) / 256 * 256;
    for (int k0 = klast; k0 >= 0; k0 -= 256) {                            // backwards, group by group
        if (k0 != klast) stage(k0);
        const int cnt = min(256, ntr - k0);
        if (!live) continue;
        for (int g0 = (cnt - 1) / TRV_T * TRV_T; g0 >= 0; g0 -= TRV_T) {
            const int ge = min(g0 + TRV_T, cnt);
            double us[TRV_T][3], dus[TRV_T][3], mm[3], dmm[3];            // (u, du) of repetition k0 + g0 + j
            const double* w = wck + (long)((k0 + g0) / TRV_T) * (2 * BLOCH_CK);
            mm[0] = w[0]; mm[1] = w[256]; mm[2] = w[512];
            dmm[0] = w[768]; dmm[1] = w[1024]; dmm[2] = w[1280];
#pragma unroll
            for (int j = 0; j < TRV_T; ++j) {
                if (g0 + j < ge) {
                    const double c = scs[g0 + j].x, s = scs[g0 + j].y;
                    train_zp(c, s, mm);
                    train_zp(c, s, dmm);
                    us[j][0] = mm[0]; us[j][1] = mm[1]; us[j][2] = mm[2];
                    dus[j][0] = dmm[0]; dus[j][1] = dmm[1]; dus[j][2] = dmm[2];
                    if (g0 + j + 1 < ge) {
                        if (!hoist) {
                            const double* wg = wb + (long)sgi[g0 + j] * gstr;
#pragma unroll
                            for (int e = 0; e < 12; ++e) W[e] = wg[e * npair];
                        }
                        advance(c, s, db + (long)sgi[g0 + j] * dgstr, mm, dmm);
                    }
                }
            }
#pragma unroll
            for (int j = TRV_T - 1; j >= 0; --j) {
                if (g0 + j < ge) {
                    const double c = scs[g0 + j].x, s = scs[g0 + j].y;
                    const long go = (long)sgi[g0 + j] * gstr;
                    if (!hoist) {
#pragma unroll
                        for (int e = 0; e < TRAIN_ENT; ++e) { W[e] = wb[go + e * npair]; acc[e] = 0; }
                    }
                    const double* u = us[j];
                    double a[3] = {l[0], l[1], l[2]};
                    train_zp(c, s, a);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        acc[i] += a[i] * u[0]; acc[3 + i] += a[i] * u[1]; acc[6 + i] += a[i] * u[2];
                        acc[9 + i] += meq * a[i];
                        l[i] = W[3 * i] * a[0] + W[3 * i + 1] * a[1] + W[3 * i + 2] * a[2];           // A' a
                    }
                    if (wp) {
                        const long ko = (long)(k0 + g0 + j) * kstr;
                        const double rk = srw[g0 + j];
                        const double* dk = db + (long)sgi[g0 + j] * dgstr + 12 * npair;
                        double dW[12], ae[3];
#pragma unroll
                        for (int e = 0; e < 12; ++e) dW[e] = dk[e * npair];
                        train_affine_jvp(W + 12, dW, dW + 9, meq, u, dus[j], ae);      // decho, as k_bloch_train_run_jvp forms it
                        if (!demod) train_zm(c, s, ae);
                        if (TRAIN_MAG) {                                  // ce_k = rw_k (w_xy (u . decho_xy) u, w_z decho_z)
                            double e[3], cs[3];
                            train_affine(W + 12, W + 21, meq, u, e);      // the primal echo, as k_bloch_train_run forms it
                            if (!demod) train_zm(c, s, e);
                            const double wv[2] = {wp[ko], wp[ko + PE]};
                            const BlochMagDir D = bloch_mag_dir(e[0], e[1]);
                            bloch_mag_seed(D, wv, D.ux * ae[0] + D.uy * ae[1], ae[2], true, cs);
#pragma unroll
                            for (int i = 0; i < 3; ++i) ae[i] = rk * cs[i];
                        } else {
#pragma unroll
                            for (int i = 0; i < 3; ++i) ae[i] = rk * (wp[ko + i * PE] * ae[i]);       // ce_k = rw_k w decho_k
                        }
                        if (!demod) train_zp(c, s, ae);
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            acc[12 + i] += ae[i] * u[0]; acc[15 + i] += ae[i] * u[1]; acc[18 + i] += ae[i] * u[2];
                            acc[21 + i] += meq * ae[i];
                            l[i] += W[12 + 3 * i] * ae[0] + W[13 + 3 * i] * ae[1] + W[14 + 3 * i] * ae[2];       // A_e' ae
                        }
                    }
                    train_zm(c, s, l);
                    if (!hoist) {                                         // the thread's own column of the repetition's gain
#pragma unroll
                        for (int e = 0; e < TRAIN_ENT; ++e) cb[go + e * npair] += acc[e];
                    }
                }
            }
        }
    }
    if (!live) return;
    if (hoist) {
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) cb[e * npair] = acc[e];
    }
}

// k_bloch_train_run_sched_gn for the workgroup bk = (pulse, scale, chunk of 256 points, direction).
__device__ __forceinline__ void TRAIN_GN_BODY(bloch_train_run_sched_gn_body)(
    const SimBlock bk, const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep,
    const int* __restrict__ gidx, const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses,
    const TrainPulseDev* __restrict__ trains, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const double* __restrict__ m0, const double* __restrict__ dgain, const double* __restrict__ dphi, int demod, int ebcast, int ndir,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, long CK, long NP, double* ck,
    double2* __restrict__ part) {
    __shared__ double2 scs[256];
    __shared__ double2 sdr[256];                                          // (dg_k, dp_k) of the workgroup's direction
    __shared__ double srw[256];
    __shared__ int sgi[256];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    static_assert(TRV_T == VJP_T, "a group of repetitions fills the tile's VJP_T x 2 rows");
    const int tid = threadIdx.x;
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain, dir = bk.pad;
    const double meq = Tr.meq;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;                                       // a thread past the end of the grid: the barriers only
    const long blk = (long)bk.scale * npair + pair;
    const long comb0 = (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    const double* wb = ws + Tr.w_off + comb0;
    const double* db = dws ? dws + Tr.w_off + comb0 : nullptr;
    const long gstr = (long)TRAIN_ENT * npair;
    const long nch = (npair + 255) / 256;
    double* wck = ck + 2 * ((long)dir * CK + K.c_off + ((long)bk.scale * nch + bk.chunk) * K.ng * BLOCH_CK) + tid;
    double2* wpart = part + (long)dir * NP + V.p_off + ((long)bk.scale * nch + bk.chunk) * ntr;
    const long sbase = (long)ndir * Tr.r_off + (long)dir * ntr;           // the direction's first repetition in dgain / dphi
    const int row = tid >> 4, ln = tid & 15;
    const bool hoist = TSGN_HOIST && G == 1;
    double m[3] = {0, 0, 1}, dm[3] = {0, 0, 0}, W[TRAIN_ENT], dW[TRAIN_ENT];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int e = 0; e < TRAIN_ENT; ++e) dW[e] = 0;
    if (hoist) {
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wb[e * npair];
        if (db) {
#pragma unroll
            for (int e = 0; e < TRAIN_ENT; ++e) dW[e] = db[e * npair];
        }
    }
    auto stage = [&](int k0) {
        __syncthreads();
        const int cnt = min(256, ntr - k0);
        if (tid < cnt) {
            const long o = sbase + k0 + tid;
            scs[tid] = rep[Tr.r_off + k0 + tid];
            sgi[tid] = gidx[Tr.r_off + k0 + tid];
            srw[tid] = rw ? rw[Tr.r_off + k0 + tid] : 1.0;
            sdr[tid] = make_double2(dgain ? dgain[o] : 0.0, dphi ? dphi[o] : 0.0);
        }
        __syncthreads();
    };
    // the state's half of the planes of the gain at go, and of their tangents, into W[0 .. 11] and dW[0 .. 11]
    auto load_state = [&](long go) {
        if (hoist) return;
#pragma unroll
        for (int e = 0; e < 12; ++e) W[e] = wb[go + e * npair];
        if (db) {
#pragma unroll
            for (int e = 0; e < 12; ++e) dW[e] = db[go + e * npair];
        }
    };
    // (m_k, dm_k) -> (m_{k+1}, dm_{k+1}) from (u_k, du_k) (in v, dv), as k_bloch_train_run_sched_jvp steps them
    auto advance = [&](double c, double s, double2 d, double v[3], double dv[3]) {
        double n[3], gn[3], dn[3];
        train_affine(W, W + 9, meq, v, n);
        train_affine(dW, dW + 9, meq, v, gn);                             // dA u + meq dB (zeros without the tangent planes)
        train_sj_map(W, gn, n, d.x, d.y, true, dv, dn);
        train_zm(c, s, dn);
        train_zm(c, s, n);
        v[0] = n[0]; v[1] = n[1]; v[2] = n[2];
        dv[0] = dn[0]; dv[1] = dn[1]; dv[2] = dn[2];
    };
    for (int k0 = 0; k0 < ntr; k0 += 256) {                               // forwards: the checkpoints of m and dm
        stage(k0);
        const int cnt = min(256, ntr - k0);
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            if ((q & (TRV_T - 1)) == 0) {                                 // (m, dm) before repetition k0 + q
                double* w = wck + (long)((k0 + q) / TRV_T) * (2 * BLOCH_CK);
                w[0] = m[0]; w[256] = m[1]; w[512] = m[2];
                w[768] = dm[0]; w[1024] = dm[1]; w[1280] = dm[2];
            }
            const double c = scs[q].x, s = scs[q].y;
            load_state((long)sgi[q] * gstr);
            train_zp(c, s, m);
            train_sj_in(c, s, sdr[q].y, m, dm);
            advance(c, s, sdr[q], m, dm);
        }
    }
    double l[3] = {0, 0, 0};
    if (live && wf) {                                                     // lambda_N = wf dm_N
        const long o = P.o_off + blk;
        if (TRAIN_MAG) {                                                  // lambda_N = (w_xy (u . dm_xy) u, w_z dm_z), u of m_N
            const double wv[2] = {wf[o], wf[PO + o]};
            const BlochMagDir D = bloch_mag_dir(m[0], m[1]);
            bloch_mag_seed(D, wv, D.ux * dm[0] + D.uy * dm[1], dm[2], true, l);
        } else {
            l[0] = wf[o] * dm[0]; l[1] = wf[PO + o] * dm[1]; l[2] = wf[2 * PO + o] * dm[2];
        }
    }
    const long eo = ebcast ? P.o_off + blk : Tr.e_off + (long)bk.scale * ntr * npair + pair, kstr = ebcast ? 0 : npair;
    const double* wp = we ? we + eo : nullptr;
    const int klast = (ntr - 1) / 256 * 256;
    for (int k0 = klast; k0 >= 0; k0 -= 256) {                            // backwards, group by group
        if (k0 != klast) stage(k0);                                       // the forward walk left the last tile staged
        const int cnt = min(256, ntr - k0);
        for (int g0 = (cnt - 1) / TRV_T * TRV_T; g0 >= 0; g0 -= TRV_T) {
            const int ge = min(g0 + TRV_T, cnt);
            if (live) {
                double us[TRV_T][3], dus[TRV_T][3], mm[3], dmm[3];        // (u, du) of repetition k0 + g0 + j
                const double* w = wck + (long)((k0 + g0) / TRV_T) * (2 * BLOCH_CK);
                mm[0] = w[0]; mm[1] = w[256]; mm[2] = w[512];
                dmm[0] = w[768]; dmm[1] = w[1024]; dmm[2] = w[1280];
#pragma unroll
                for (int j = 0; j < TRV_T; ++j) {
                    if (g0 + j < ge) {
                        const double c = scs[g0 + j].x, s = scs[g0 + j].y;
                        const double2 d = sdr[g0 + j];
                        train_zp(c, s, mm);
                        train_sj_in(c, s, d.y, mm, dmm);
                        us[j][0] = mm[0]; us[j][1] = mm[1]; us[j][2] = mm[2];
                        dus[j][0] = dmm[0]; dus[j][1] = dmm[1]; dus[j][2] = dmm[2];
                        if (g0 + j + 1 < ge) {
                            load_state((long)sgi[g0 + j] * gstr);
                            advance(c, s, d, mm, dmm);
                        }
                    }
                }
#pragma unroll
                for (int j = TRV_T - 1; j >= 0; --j) {
                    if (g0 + j < ge) {
                        const double c = scs[g0 + j].x, s = scs[g0 + j].y;
                        const long go = (long)sgi[g0 + j] * gstr;
                        const double* u = us[j];
                        double gg = 0, gp = 0, le[3] = {0, 0, 0};
                        if (wp) {                                         // the echo's half first: its planes are dead before the state's
                            const long ko = (long)(k0 + g0 + j) * kstr;
                            const double rk = srw[g0 + j];
                            const double2 d = sdr[g0 + j];
                            if (!hoist) {
#pragma unroll
                                for (int e = 12; e < TRAIN_ENT; ++e) W[e] = wb[go + e * npair];
                                if (db) {
#pragma unroll
                                    for (int e = 12; e < TRAIN_ENT; ++e) dW[e] = db[go + e * npair];
                                }
                            }
                            double ne[3], ge3[3], ae[3];
                            train_affine(W + 12, W + 21, meq, u, ne);
                            train_affine(dW + 12, dW + 21, meq, u, ge3);  // dA_e u + meq dB_e
                            train_sj_map(W + 12, ge3, ne, d.x, d.y, !demod, dus[j], ae);      // decho, as k_bloch_train_run_sched_jvp forms it
                            if (!demod) train_zm(c, s, ae);
                            if (TRAIN_MAG) {                              // ce_k = rw_k (w_xy (u . decho_xy) u, w_z decho_z)
                                double e[3] = {ne[0], ne[1], ne[2]}, cs[3];       // the primal echo, as k_bloch_train_run forms it
                                if (!demod) train_zm(c, s, e);
                                const double wv[2] = {wp[ko], wp[ko + PE]};
                                const BlochMagDir D = bloch_mag_dir(e[0], e[1]);
                                bloch_mag_seed(D, wv, D.ux * ae[0] + D.uy * ae[1], ae[2], true, cs);
#pragma unroll
                                for (int i = 0; i < 3; ++i) ae[i] = rk * cs[i];
                            } else {
#pragma unroll
                                for (int i = 0; i < 3; ++i) ae[i] = rk * (wp[ko + i * PE] * ae[i]);       // ce_k = rw_k w decho_k
                            }
                            if (!demod) train_zp(c, s, ae);
                            gg = train_sched_dot(ae, ge3);
                            gp = demod ? train_sched_dphi_demod(W + 12, ae, u) : train_sched_dphi(W + 12, ae, u, ne);
                            train_sg_back(W + 12, ae, le);                // A_e' ae
                        }
                        load_state(go);
                        double a[3] = {l[0], l[1], l[2]}, n[3], dn[3];
                        train_zp(c, s, a);
                        train_affine(W, W + 9, meq, u, n);
                        train_affine(dW, dW + 9, meq, u, dn);
                        gp += train_sched_dphi(W, a, u, n);
                        gg += train_sched_dot(a, dn);
                        train_sg_back(W, a, l);                           // A' a
                        l[0] += le[0]; l[1] += le[1]; l[2] += le[2];
                        train_zm(c, s, l);
                        red[(2 * j) * VJP_ROW + tid] = gg;
                        red[(2 * j + 1) * VJP_ROW + tid] = gp;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < TRV_T; ++j)
                    if (g0 + j < ge) { red[(2 * j) * VJP_ROW + tid] = 0.0; red[(2 * j + 1) * VJP_ROW + tid] = 0.0; }
            }
            __syncthreads();
            double sum = 0;                                               // row = 2 (repetition - g0) + (0: gain, 1: phase); rows past ge are not stored
            for (int k = 0; k < 16; ++k) sum += red[row * VJP_ROW + ln + 16 * k];
            for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
            if (ln == 0 && row < 2 * (ge - g0)) reinterpret_cast<double*>(wpart + k0 + g0)[row] = sum;
            __syncthreads();
        }
    }
}
