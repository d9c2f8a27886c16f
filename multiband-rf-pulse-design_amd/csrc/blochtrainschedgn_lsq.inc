// k_bloch_train_run_sched_lsq (DESIGN 8af), included twice: by blochtrainschedgn.hip as it is, the component fit, and by
// blochtrainmag.hip as k_bloch_train_run_sched_lsq_mag with TRAIN_MAG true, the magnitude fit of (|Mxy|, mz) per echo and at the final
// state (DESIGN 8ai).  The two differ in the two blocks that make the residual, the cotangent and the loss; with TRAIN_MAG the weights
// and targets are two planes (xy, z), PE / PO apart.  Plain kernels on both sides, as in blochssgn_kernels.inc, and in two files: side
// by side in one, the component kernel got another LDS layout.
// TRAIN_LSQ_KERNEL(name): the kernel's name in this pass; TRAIN_MAG: false or true.
// blocks, ws, dws (null: the gains' half of every partial is zero), rep, gidx, vp, cks, ck, part, gmx ..: k_bloch_train_run_sched's.
// rw (null: ones), we / te (null: no echo term), PE, wf / tf (null: no final term), PO, ebcast, lp, lpart: k_bloch_train_run_lsq's.
__global__ __launch_bounds__(256) void TRAIN_LSQ_KERNEL(k_bloch_train_run_sched_lsq)(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const long* __restrict__ lp, const double* __restrict__ m0, int demod, int ebcast, const double* __restrict__ we,
    const double* __restrict__ te, long PE, const double* __restrict__ wf, const double* __restrict__ tf, long PO, double* ck,
    double2* __restrict__ part, double* __restrict__ gmx, double* __restrict__ gmy, double* __restrict__ gmz,
    double* __restrict__ lpart) {
    __shared__ double2 scs[256];
    __shared__ double srw[256];
    __shared__ int sgi[256];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    static_assert(TRV_T == VJP_T, "a group of repetitions fills the tile's VJP_T x 2 rows");
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain;
    const double meq = Tr.meq;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;                                       // a thread past the end of the grid: the barriers only
    const long blk = (long)bk.scale * npair + pair;
    const long comb0 = (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    const double* wb = ws + Tr.w_off + comb0;
    const double* db = dws ? dws + Tr.w_off + comb0 : nullptr;
    const long nch = (npair + 255) / 256;
    double* wck = ck + K.c_off + ((long)bk.scale * nch + bk.chunk) * K.ng * BLOCH_CK + tid;
    double2* wpart = part + V.p_off + ((long)bk.scale * nch + bk.chunk) * ntr;
    const int row = tid >> 4, ln = tid & 15;                              // reduction: 16 lanes per row of the tile
    double m[3] = {0, 0, 1}, W[TRAIN_ENT], dW[TRAIN_ENT];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int e = 0; e < TRAIN_ENT; ++e) dW[e] = 0;
    if (G == 1) {                                                         // one distinct gain: the planes are loaded once
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
        for (int g0 = (cnt - 1) / TRV_T * TRV_T; g0 >= 0; g0 -= TRV_T) {
            const int ge = min(g0 + TRV_T, cnt);
            if (live) {
                double us[TRV_T][3], mm[3];                               // us[j] = u of repetition k0 + g0 + j
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
                            for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wb[go + e * npair];
                            if (db) {
#pragma unroll
                                for (int e = 0; e < TRAIN_ENT; ++e) dW[e] = db[go + e * npair];
                            }
                        }
                        const double* u = us[j];
                        double a[3] = {l[0], l[1], l[2]}, n[3], dn[3];
                        train_zp(c, s, a);
                        train_affine(W, W + 9, meq, u, n);
                        train_affine(dW, dW + 9, meq, u, dn);
                        double gp = train_sched_dphi(W, a, u, n), gg = train_sched_dot(a, dn);
                        train_sg_back(W, a, l);                           // A' a
                        if (wp) {
                            const long ko = (long)(k0 + g0 + j) * kstr;
                            const double rk = srw[g0 + j];
                            double e[3], ae[3], le[3];
                            train_affine(W + 12, W + 21, meq, u, n);      // ne, and the echo as k_bloch_train_run forms it
                            e[0] = n[0]; e[1] = n[1]; e[2] = n[2];
                            if (!demod) train_zm(c, s, e);
                            double q2 = 0;
                            if (TRAIN_MAG) {                              // ce_k = rw_k (w_xy (rho_k - t_xy) u, w_z (e_kz - t_z))
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
                                    ae[i] = rk * (wi * r);                // ce_k = rw_k w r
                                    q2 += wi * (r * r);
                                }
                            }
                            ls += rk * (0.5 * q2);
                            if (!demod) train_zp(c, s, ae);
                            train_affine(dW + 12, dW + 21, meq, u, dn);
                            gg += train_sched_dot(ae, dn);
                            gp += demod ? train_sched_dphi_demod(W + 12, ae, u) : train_sched_dphi(W + 12, ae, u, n);
                            train_sg_back(W + 12, ae, le);                // A_e' ae
                            l[0] += le[0]; l[1] += le[1]; l[2] += le[2];
                        }
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
    const double sum = lm_block_sum(live ? ls : 0.0, red);                // 256 doubles of the tile, free after the last group
    if (tid == 0) lpart[lp[bk.pulse] + (long)bk.scale * nch + bk.chunk] = sum;
    if (live && gmx) { const long o = P.o_off + blk; gmx[o] = l[0]; gmy[o] = l[1]; gmz[o] = l[2]; }
}
