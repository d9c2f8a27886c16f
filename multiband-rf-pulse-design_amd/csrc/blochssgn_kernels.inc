// The three sweep kernels of blochssgn.hip (DESIGN 8u, 8v), included there twice: as they are, the component fits of (mx, my, mz),
// and as k_..._mag with BLOCH_SS_MAG true, the magnitude fits of (|Mxy|, mz) (DESIGN 8ah).  The two differ in the block that makes the
// cotangent c and in nothing else.  Plain kernels on both sides, not instances of a template or of an inlined body: either of those
// changed the schedule the compiler gives the component kernels.
// BLOCH_SS_KERNEL(name): the kernel's name in this pass; BLOCH_SS_MAG: false or true, whether this pass is the magnitude one.
// in, df, pos3, scales, pulses, blocks, vp, cks, part, ck, mx / my / mz: k_bloch_ss_vjp_batch's.  w, tg: three planes of O entries
// each (x, y, z), laid out as k_bloch_batch writes mx / my / mz in mode 1.  lp: a pulse's first loss partial, its workgroup (scale,
// chunk) at scale nch + chunk.
__global__ __launch_bounds__(256) void BLOCH_SS_KERNEL(k_bloch_ss_lsq_batch)(const double* __restrict__ in, const double* __restrict__ df,
                                                            const double* __restrict__ pos3, const double* __restrict__ scales,
                                                            const BlochPulseDev* __restrict__ pulses,
                                                            const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                            const BlochCkDev* __restrict__ cks, const long* __restrict__ lp,
                                                            const double* __restrict__ w, const double* __restrict__ tg, long O,
                                                            double2* __restrict__ part, double* ck, double* __restrict__ lpart,
                                                            double* __restrict__ mx, double* __restrict__ my,
                                                            double* __restrict__ mz) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ __align__(16) double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime;
    const BlochSsPoint G = bloch_ss_point(bk, P, df, pos3);
    const double px = G.px, py = G.py, pz = G.pz, dfv = G.dfv;
    const bool live = G.live;
    const long wg = (long)bk.scale * V.nch + bk.chunk;                   // the workgroup among its pulse's
    double* wck = ck + K.c_off + wg * K.ng * BLOCH_CK + tid;
    // a thread past the end of the grid sweeps the first point with a zero seed and contributes exact zeros
    double m[3], l[3];
    {
        double inv[9];
        bloch_ss_pass0(sst, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, inv, m);
        double wv[3] = {0, 0, 0}, tv[3] = {0, 0, 0};
        if (BLOCH_SS_MAG) {
            if (live) {
                wv[0] = w[G.o]; wv[1] = w[O + G.o];
                tv[0] = tg[G.o]; tv[1] = tg[O + G.o];
            }
            const BlochMagDir D = bloch_mag_dir(m[0], m[1]);              // of mode 1's own M
            const double r0 = D.rho - tv[0], r2 = m[2] - tv[1];
            double c[3];
            bloch_mag_seed(D, wv, r0, r2, live, c);
            for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c[0] + inv[3 * j + 1] * c[1] + inv[3 * j + 2] * c[2];      // lambda = inv' c
            red[tid] = live ? 0.5 * (wv[0] * (r0 * r0) + wv[1] * (r2 * r2)) : 0.0;      // the loss: row 0 of the tile
        } else {
            if (live) {
                wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o];
                tv[0] = tg[G.o]; tv[1] = tg[O + G.o]; tv[2] = tg[2 * O + G.o];
            }
            const double r0 = m[0] - tv[0], r1 = m[1] - tv[1], r2 = m[2] - tv[2];      // the residual of mode 1's own M
            const double c0 = live ? wv[0] * r0 : 0.0, c1 = live ? wv[1] * r1 : 0.0, c2 = live ? wv[2] * r2 : 0.0;
            for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c0 + inv[3 * j + 1] * c1 + inv[3 * j + 2] * c2;      // lambda = inv' c
            red[tid] = live ? 0.5 * (wv[0] * (r0 * r0) + wv[1] * (r1 * r1) + wv[2] * (r2 * r2)) : 0.0;      // the loss: row 0 of the tile
        }
    }
    if (live && mx) { mx[G.o] = m[0]; my[G.o] = m[1]; mz[G.o] = m[2]; }
    {
        __syncthreads();
        const int ln = tid & 15;
        double sum = 0;                                                   // every row of threads sums row 0; thread 0 stores
        for (int k = 0; k < 16; ++k) sum += red[ln + 16 * k];
        for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
        if (tid == 0) lpart[lp[bk.pulse] + wg] = sum;
        __syncthreads();
    }
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        if (t0 != tlast || t0 != 0) bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);      // pass 0 left the last tile staged
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int q = 0; q < cnt; ++q) {
            if ((q & (VJP_T - 1)) == 0) {                                 // m before sample t0 + q: the group's checkpoint
                double* c = wck + (long)((t0 + q) / VJP_T) * BLOCH_CK;
                c[0] = m[0]; c[256] = m[1]; c[512] = m[2];
            }
            const double* s = sst[q];
            bloch_fwd_step(s, bloch_rotz(s, px, py, pz, dfv), m);
        }
    }
    bloch_ss_reverse(sst, red, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, live, l, part + V.p_off + wg * V.n, wck);
}

// As k_bloch_ss_lsq_batch without targets; blocks: the forward table repeated per direction, the direction in SimBlock::pad; vp,
// cks: the descriptors of (pulse, direction) at pulse ndir + direction; v (interleaved): direction k of pulse p at ndir t_off + k
// ntime, as k_bloch_jvp_batch takes it; sinv: BLOCH_SSINV doubles per workgroup, written and read back coalesced by the same thread.
__global__ __launch_bounds__(256) void BLOCH_SS_KERNEL(k_bloch_ss_gn_batch)(const double* __restrict__ in, const double* __restrict__ df,
                                                           const double* __restrict__ pos3, const double* __restrict__ scales,
                                                           const BlochPulseDev* __restrict__ pulses,
                                                           const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                           const BlochCkDev* __restrict__ cks, const double* __restrict__ w, long O,
                                                           const double2* __restrict__ v, int ndir, double2* __restrict__ part,
                                                           double* ck, double* sinv) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ __align__(16) double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    static_assert(sizeof(double2) * BLOCH_CH <= sizeof(double) * 2 * VJP_T * VJP_ROW, "the direction row fits in the tile");
    double2* sdn = reinterpret_cast<double2*>(red);                   // (dnx, dny) of the staged rows: forward sweep only
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[(long)bk.pulse * ndir + bk.pad];
    const BlochCkDev K = cks[(long)bk.pulse * ndir + bk.pad];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime;
    const BlochSsPoint G = bloch_ss_point(bk, P, df, pos3);
    const double px = G.px, py = G.py, pz = G.pz, dfv = G.dfv;
    const bool live = G.live;
    const long wg = (long)bk.scale * V.nch + bk.chunk;
    const double2* vd = v + (long)ndir * P.t_off + (long)bk.pad * ntime;
    double* wck = ck + K.c_off + wg * K.ng * BLOCH_CK + tid;
    double* winv = sinv + (long)blockIdx.x * BLOCH_SSINV + tid;
    double m[3], dm[3] = {0, 0, 0};
    {
        double inv[9];
        bloch_ss_pass0(sst, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, inv, m);
        for (int e = 0; e < 9; ++e) winv[e * 256] = inv[e];               // read back by this thread alone
    }
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 s, as k_bloch_batch forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
            const double2 d = vd[t0 + tid];
            sdn[tid] = make_double2(((-(d.x * sc)) * gamma) * dt, ((d.y * sc) * gamma) * dt);      // as k_bloch_jvp_batch stages it
        }
        __syncthreads();
        for (int q = 0; q < cnt; ++q) {
            if ((q & (VJP_T - 1)) == 0) {                                 // m before sample t0 + q: the group's checkpoint
                double* c = wck + (long)((t0 + q) / VJP_T) * BLOCH_CK;
                c[0] = m[0]; c[256] = m[1]; c[512] = m[2];
            }
            const double* s = sst[q];
            const double rotz = bloch_rotz(s, px, py, pz, dfv);
            Rot3 R;
            BlochTrig tr;
            bloch_rotmat_trig<true>(s[0], s[1], rotz, R, tr);
            const double e1 = s[6], e2 = s[7];
            BlochJvpShared W;
            bloch_jvp_shared(s[0], s[1], rotz, tr, m, W);
            const double2 dn = sdn[q];
            const double nd = s[0] * dn.x + s[1] * dn.y;
            double o[3];
            rot_vec(R, dm, o);
            dm[0] = e2 * (o[0] + (nd * W.U[0] + dn.x * W.Vx[0] + dn.y * W.Vy[0]));
            dm[1] = e2 * (o[1] + (nd * W.U[1] + dn.x * W.Vx[1] + dn.y * W.Vy[1]));
            dm[2] = e1 * (o[2] + (nd * W.U[2] + dn.x * W.Vx[2] + dn.y * W.Vy[2]));
            rot_vec(R, m, o);
            m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = e1 * o[2] + (1 - e1);
        }
    }
    double l[3];
    {
        double inv[9], wv[3] = {0, 0, 0};
        for (int e = 0; e < 9; ++e) inv[e] = winv[e * 256];
        double c[3];
        if (BLOCH_SS_MAG) {
            if (live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; }
            double dM[3];
            for (int i = 0; i < 3; ++i) dM[i] = inv[i] * dm[0] + inv[3 + i] * dm[1] + inv[6 + i] * dm[2];      // dM = inv d
            const BlochMagDir D = bloch_mag_dir(wck[0], wck[256]);        // M: the first checkpoint, written by this thread
            bloch_mag_seed(D, wv, D.ux * dM[0] + D.uy * dM[1], dM[2], live, c);
        } else {
            if (live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o]; }
            for (int i = 0; i < 3; ++i) {
                const double d = inv[i] * dm[0] + inv[3 + i] * dm[1] + inv[6 + i] * dm[2];      // dM = inv d
                c[i] = live ? wv[i] * d : 0.0;
            }
        }
        for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c[0] + inv[3 * j + 1] * c[1] + inv[3 * j + 2] * c[2];      // lambda = inv' c
    }
    __syncthreads();                                                      // the direction row is read no more: the tile is free
    bloch_ss_reverse(sst, red, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, live, l, part + V.p_off + wg * V.n, wck);
}

// k_bloch_ss_gn_batch at ndir = 1 for the pulses that still run, pass 0 taken from k_bloch_ss_lm_prep's plane: the forward call's
// block table, the direction the device's p (laid out as b1 is).  The forward loop stages every tile itself, as the shipped one
// does; the loop, the cotangent and the reverse sweep are the shipped kernel's statements.
__global__ __launch_bounds__(256) void BLOCH_SS_KERNEL(k_bloch_ss_lm_sweep)(const double* __restrict__ in, const double* __restrict__ df,
                                                           const double* __restrict__ pos3, const double* __restrict__ scales,
                                                           const BlochPulseDev* __restrict__ pulses,
                                                           const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                           const BlochCkDev* __restrict__ cks, const double* __restrict__ w, long O,
                                                           const double2* __restrict__ v, const LmState* __restrict__ st,
                                                           double2* __restrict__ part, double* ck,
                                                           const double* __restrict__ plane) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ __align__(16) double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    static_assert(sizeof(double2) * BLOCH_CH <= sizeof(double) * 2 * VJP_T * VJP_ROW, "the direction row fits in the tile");
    double2* sdn = reinterpret_cast<double2*>(red);                   // (dnx, dny) of the staged rows: forward sweep only
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime;
    const BlochSsPoint G = bloch_ss_point(bk, P, df, pos3);
    const double px = G.px, py = G.py, pz = G.pz, dfv = G.dfv;
    const bool live = G.live;
    const long wg = (long)bk.scale * V.nch + bk.chunk;
    const double2* vd = v + P.t_off;
    double* wck = ck + K.c_off + wg * K.ng * BLOCH_CK + tid;
    const double* wpl = plane + (long)blockIdx.x * BLOCH_SSLM_PLANE + tid;
    double m[3], dm[3] = {0, 0, 0};
    for (int e = 0; e < 3; ++e) m[e] = wpl[(9 + e) * 256];               // M of pass 0, written by this thread of the prep launch
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 s, as k_bloch_batch forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
            const double2 d = vd[t0 + tid];
            sdn[tid] = make_double2(((-(d.x * sc)) * gamma) * dt, ((d.y * sc) * gamma) * dt);      // as k_bloch_jvp_batch stages it
        }
        __syncthreads();
        for (int q = 0; q < cnt; ++q) {
            if ((q & (VJP_T - 1)) == 0) {                                 // m before sample t0 + q: the group's checkpoint
                double* c = wck + (long)((t0 + q) / VJP_T) * BLOCH_CK;
                c[0] = m[0]; c[256] = m[1]; c[512] = m[2];
            }
            const double* s = sst[q];
            const double rotz = bloch_rotz(s, px, py, pz, dfv);
            Rot3 R;
            BlochTrig tr;
            bloch_rotmat_trig<true>(s[0], s[1], rotz, R, tr);
            const double e1 = s[6], e2 = s[7];
            BlochJvpShared W;
            bloch_jvp_shared(s[0], s[1], rotz, tr, m, W);
            const double2 dn = sdn[q];
            const double nd = s[0] * dn.x + s[1] * dn.y;
            double o[3];
            rot_vec(R, dm, o);
            dm[0] = e2 * (o[0] + (nd * W.U[0] + dn.x * W.Vx[0] + dn.y * W.Vy[0]));
            dm[1] = e2 * (o[1] + (nd * W.U[1] + dn.x * W.Vx[1] + dn.y * W.Vy[1]));
            dm[2] = e1 * (o[2] + (nd * W.U[2] + dn.x * W.Vx[2] + dn.y * W.Vy[2]));
            rot_vec(R, m, o);
            m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = e1 * o[2] + (1 - e1);
        }
    }
    double l[3];
    {
        double inv[9], wv[3] = {0, 0, 0};
        for (int e = 0; e < 9; ++e) inv[e] = wpl[e * 256];
        double c[3];
        if (BLOCH_SS_MAG) {
            if (live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; }
            double dM[3];
            for (int i = 0; i < 3; ++i) dM[i] = inv[i] * dm[0] + inv[3 + i] * dm[1] + inv[6 + i] * dm[2];      // dM = inv d
            const BlochMagDir D = bloch_mag_dir(wck[0], wck[256]);        // M: the first checkpoint, written by this thread
            bloch_mag_seed(D, wv, D.ux * dM[0] + D.uy * dM[1], dM[2], live, c);
        } else {
            if (live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o]; }
            for (int i = 0; i < 3; ++i) {
                const double d = inv[i] * dm[0] + inv[3 + i] * dm[1] + inv[6 + i] * dm[2];      // dM = inv d
                c[i] = live ? wv[i] * d : 0.0;
            }
        }
        for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c[0] + inv[3 * j + 1] * c[1] + inv[3 * j + 2] * c[2];      // lambda = inv' c
    }
    __syncthreads();                                                      // the direction row is read no more: the tile is free
    bloch_ss_reverse(sst, red, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, live, l, part + V.p_off + wg * V.n, wck);
}

