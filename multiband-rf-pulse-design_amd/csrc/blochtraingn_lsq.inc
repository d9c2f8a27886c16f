// k_bloch_train_run_lsq (DESIGN 8ab), included twice: by blochtraingn.hip as it is, the component fit, and by blochtrainmag.hip as
// k_bloch_train_run_lsq_mag with TRAIN_MAG true, the magnitude fit of (|Mxy|, mz) per echo and at the final state (DESIGN 8ai).  The
// two differ in the two blocks that make the residual, the cotangent and the loss; with TRAIN_MAG the weights and targets are two
// planes (xy, z), PE / PO apart.  Plain kernels on both sides, as in blochssgn_kernels.inc, and in two files: side by side in one,
// the component kernel got another LDS layout.
// TRAIN_LSQ_KERNEL(name): the kernel's name in this pass; TRAIN_MAG: false or true.
// blocks, ws, cw, cks, ck, gmx..: k_bloch_train_run_vjp's.  rw (null: ones): the repetitions' factors, laid out as rep.  we / te
// (null: no echo term): the echo weights and targets, three planes PE entries apart, pulse p from e_off (ebcast 0) or o_off
// (ebcast 1).  wf / tf (null: no final term): three planes PO apart, where the final planes lie.  lpart: one loss partial per
// workgroup, workgroup (scale, chunk) of pulse p at lp[p] + scale nch + chunk.
__global__ __launch_bounds__(256) void TRAIN_LSQ_KERNEL(k_bloch_train_run_lsq)(
    const double* __restrict__ ws, const double2* __restrict__ rep, const int* __restrict__ gidx, const double* __restrict__ rw,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const SimBlock* __restrict__ blocks,
    const BlochCkDev* __restrict__ cks, const long* __restrict__ lp, const double* __restrict__ m0, int demod, int ebcast,
    const double* __restrict__ we, const double* __restrict__ te, long PE, const double* __restrict__ wf,
    const double* __restrict__ tf, long PO, double* ck, double* cw, double* __restrict__ gmx, double* __restrict__ gmy,
    double* __restrict__ gmz, double* __restrict__ lpart) {
    __shared__ double2 scs[256];
    __shared__ double srw[256];
    __shared__ int sgi[256];
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain;
    const double meq = Tr.meq;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;                                       // a thread past the end of the grid contributes nothing
    const long blk = (long)bk.scale * npair + pair;
    const long comb0 = (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    const double* wb = ws + Tr.w_off + comb0;
    double* cb = cw + Tr.w_off + comb0;
    const long nch = (npair + 255) / 256;
    double* wck = ck + K.c_off + ((long)bk.scale * nch + bk.chunk) * K.ng * BLOCH_CK + tid;
    double m[3] = {0, 0, 1}, W[TRAIN_ENT], acc[TRAIN_ENT];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int e = 0; e < TRAIN_ENT; ++e) acc[e] = 0;
    if (G == 1) {                                                         // one distinct gain: the planes are loaded once
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
    // m_k -> m_{k+1} from u_k = Z(+phi_k) m_k (in v), with the planes of the repetition in W[0 .. 11]
    auto advance = [&](double c, double s, double v[3]) {
        double n[3];
        train_affine(W, W + 9, meq, v, n);
        train_zm(c, s, n);
        v[0] = n[0]; v[1] = n[1]; v[2] = n[2];
    };
    for (int k0 = 0; k0 < ntr; k0 += 256) {                               // forwards: the checkpoints
        stage(k0);
        const int cnt = min(256, ntr - k0);
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            if ((q & (TRV_T - 1)) == 0) {                                 // m before repetition k0 + q
                double* w = wck + (long)((k0 + q) / TRV_T) * BLOCH_CK;
                w[0] = m[0]; w[256] = m[1]; w[512] = m[2];
            }
            if (G != 1) {
                const double* wg = wb + (long)sgi[q] * TRAIN_ENT * npair;
#pragma unroll
                for (int e = 0; e < 12; ++e) W[e] = wg[e * npair];
            }
            train_zp(scs[q].x, scs[q].y, m);
            advance(scs[q].x, scs[q].y, m);
        }
    }
    double l[3] = {0, 0, 0}, ls = 0;
    if (live && wf) {                                                     // lambda_N = wf (m_N - tf), and the final loss
        const long o = P.o_off + blk;
        if (TRAIN_MAG) {                                                  // lambda_N = (w_xy (rho_N - tf_xy) u, w_z (m_Nz - tf_z))
            const double wv[2] = {wf[o], wf[PO + o]};
            const BlochMagDir D = bloch_mag_dir(m[0], m[1]);
            const double r0 = D.rho - tf[o], r2 = m[2] - tf[PO + o];
            bloch_mag_seed(D, wv, r0, r2, true, l);
            ls = 0.5 * (wv[0] * (r0 * r0) + wv[1] * (r2 * r2));
        } else {
            const double w0 = wf[o], w1 = wf[PO + o], w2 = wf[2 * PO + o];
            const double r0 = m[0] - tf[o], r1 = m[1] - tf[PO + o], r2 = m[2] - tf[2 * PO + o];
            l[0] = w0 * r0; l[1] = w1 * r1; l[2] = w2 * r2;
            ls = 0.5 * (w0 * (r0 * r0) + w1 * (r1 * r1) + w2 * (r2 * r2));
        }
    }
    // the weights and targets of repetition k at wp[k kstr], tp[k kstr]
    const long eo = ebcast ? P.o_off + blk : Tr.e_off + (long)bk.scale * ntr * npair + pair, kstr = ebcast ? 0 : npair;
    const double* wp = we ? we + eo : nullptr;
    const double* tp = we ? te + eo : nullptr;
    const int klast = (ntr - 1) / 256 * 256;
    for (int k0 = klast; k0 >= 0; k0 -= 256) {                            // backwards, group by group
        if (k0 != klast) stage(k0);                                       // the forward walk left the last tile staged
        const int cnt = min(256, ntr - k0);
        if (!live) continue;
        for (int g0 = (cnt - 1) / TRV_T * TRV_T; g0 >= 0; g0 -= TRV_T) {
            const int ge = min(g0 + TRV_T, cnt);
            double us[TRV_T][3], mm[3];                                   // us[j] = u of repetition k0 + g0 + j
            const double* w = wck + (long)((k0 + g0) / TRV_T) * BLOCH_CK;
            mm[0] = w[0]; mm[1] = w[256]; mm[2] = w[512];
#pragma unroll
            for (int j = 0; j < TRV_T; ++j) {
                if (g0 + j < ge) {
                    const double c = scs[g0 + j].x, s = scs[g0 + j].y;
                    train_zp(c, s, mm);
                    us[j][0] = mm[0]; us[j][1] = mm[1]; us[j][2] = mm[2];
                    if (g0 + j + 1 < ge) {
                        if (G != 1) {
                            const double* wg = wb + (long)sgi[g0 + j] * TRAIN_ENT * npair;
#pragma unroll
                            for (int e = 0; e < 12; ++e) W[e] = wg[e * npair];
                        }
                        advance(c, s, mm);
                    }
                }
            }
#pragma unroll
            for (int j = TRV_T - 1; j >= 0; --j) {
                if (g0 + j < ge) {
                    const double c = scs[g0 + j].x, s = scs[g0 + j].y;
                    const long go = (long)sgi[g0 + j] * TRAIN_ENT * npair;
                    if (G != 1) {
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
                        double e[3], ae[3];
                        train_affine(W + 12, W + 21, meq, u, e);          // the echo, as k_bloch_train_run forms it
                        if (!demod) train_zm(c, s, e);
                        double q2 = 0;
                        if (TRAIN_MAG) {                                  // ce_k = rw_k (w_xy (rho_k - t_xy) u, w_z (e_kz - t_z))
                            const double wv[2] = {wp[ko], wp[ko + PE]};
                            const BlochMagDir D = bloch_mag_dir(e[0], e[1]);
                            const double r0 = D.rho - tp[ko], r2 = e[2] - tp[ko + PE];
                            double cs[3];
                            bloch_mag_seed(D, wv, r0, r2, true, cs);
#pragma unroll
                            for (int i = 0; i < 3; ++i) ae[i] = rk * cs[i];
                            q2 = wv[0] * (r0 * r0) + wv[1] * (r2 * r2);
                        } else {
#pragma unroll
                            for (int i = 0; i < 3; ++i) {
                                const double wi = wp[ko + i * PE], r = e[i] - tp[ko + i * PE];
                                ae[i] = rk * (wi * r);                    // ce_k = rw_k w r
                                q2 += wi * (r * r);
                            }
                        }
                        ls += rk * (0.5 * q2);
                        if (!demod) train_zp(c, s, ae);
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            acc[12 + i] += ae[i] * u[0]; acc[15 + i] += ae[i] * u[1]; acc[18 + i] += ae[i] * u[2];
                            acc[21 + i] += meq * ae[i];
                            l[i] += W[12 + 3 * i] * ae[0] + W[13 + 3 * i] * ae[1] + W[14 + 3 * i] * ae[2];       // A_e' ae
                        }
                    }
                    train_zm(c, s, l);
                    if (G != 1) {                                         // the thread's own column of the repetition's gain
#pragma unroll
                        for (int e = 0; e < TRAIN_ENT; ++e) cb[go + e * npair] += acc[e];
                    }
                }
            }
        }
    }
    const double sum = lm_block_sum(live ? ls : 0.0, reinterpret_cast<double*>(scs));         // 256 doubles of the 512 of scs
    if (tid == 0) lpart[lp[bk.pulse] + (long)bk.scale * nch + bk.chunk] = sum;
    if (!live) return;
    if (G == 1) {
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) cb[e * npair] = acc[e];
    }
    if (gmx) { const long o = P.o_off + blk; gmx[o] = l[0]; gmy[o] = l[1]; gmz[o] = l[2]; }
}
