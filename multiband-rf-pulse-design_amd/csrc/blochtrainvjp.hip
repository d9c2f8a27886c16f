// Adjoint of the pulse train: the vector-Jacobian product of bloch_train_batch's echoes and final state with respect to
// the period's b1 samples and to the initial magnetisation.  Per point, in blochtrain.hip's notation, with g the gain index of
// repetition k,
//     u_k = Z(+phi_k) m_k,   echo_k = Z(-phi_k) (A_e^g u_k + meq B_e^g)   (demod: without the leading Z),
//     m_{k+1} = Z(-phi_k) (A^g u_k + meq B^g)
// and the loss is L = sum_k <ce_k, echo_k> + <cf, m_N>.  The adjoint goes through the two stages of the forward call in reverse:
//   k_bloch_train_run_vjp:  lambda_N = cf; for k = N - 1 .. 0, a = Z(+phi_k) lambda_{k+1}, ae = Z(+phi_k) ce_k (demod: ce_k),
//                           Abar^g += a u_k', Bbar^g += meq a, Abar_e^g += ae u_k', Bbar_e^g += meq ae,
//                           lambda_k = Z(-phi_k) (A^g' a + A_e^g' ae);  lambda_0 = dL / dm0.
//                           The states m_k are checkpointed before every TRV_T-th repetition on the way forwards and stepped
//                           forwards again, group by group, on the way back (the step is a contraction: nothing is inverted).
//   k_bloch_train_prop_vjp: the four columns of X = [A | B] each obey the simulator's own sample recursion (columns 0..2 from e_j
//                           without the recovery term, column 3 from 0 with it), so each is swept by k_bloch_vjp_batch's scheme
//                           (blochgrad.hip) with the column of [Abar | Bbar] as its final cotangent and the column of
//                           [Abar_e | Bbar_e] added at the state after `echo` samples.  Wave w of a workgroup owns column w, lane
//                           l the point: 64 points per workgroup, the recovery switch uniform over a wavefront.
//   k_bloch_train_vjp_fold: chunks, then combinations (times scale x gain) in index order, times -+(gamma dt_t).
// The propagators' planes come from the shipped k_bloch_train_prop.  No atomics: a thread is the only writer of its column of the
// cotangent planes, and the 256 contributions to a sample go through the VJP_T x VJP_ROW tile in a fixed order.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// blocks: the forward table (pulse, scale, chunk of 256 points).  ws: the propagators' planes; cw: their cotangents, the same layout,
// zero on entry.  cex.. (null: no echo cotangents) lie where the echoes do, cfx.. (null: none) and gmx.. (null: not wanted) where
// the final planes do.  ck: the checkpoints, BlochCkDev's layout with groups of TRV_T repetitions.
__global__ __launch_bounds__(256) void k_bloch_train_run_vjp(
    const double* __restrict__ ws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const SimBlock* __restrict__ blocks,
    const BlochCkDev* __restrict__ cks, const double* __restrict__ m0, int demod, const double* __restrict__ cex,
    const double* __restrict__ cey, const double* __restrict__ cez, const double* __restrict__ cfx, const double* __restrict__ cfy,
    const double* __restrict__ cfz, double* ck, double* cw, double* __restrict__ gmx, double* __restrict__ gmy,
    double* __restrict__ gmz) {
    __shared__ double2 scs[256];
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
        if (tid < cnt) { scs[tid] = rep[Tr.r_off + k0 + tid]; sgi[tid] = gidx[Tr.r_off + k0 + tid]; }
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
    double l[3] = {0, 0, 0};
    if (live && cfx) { const long o = P.o_off + blk; l[0] = cfx[o]; l[1] = cfy[o]; l[2] = cfz[o]; }
    const double* ce = cex ? cex + Tr.e_off + (long)bk.scale * ntr * npair + pair : nullptr;
    const long dy = cey - cex, dz = cez - cex;                            // the three planes are laid out alike
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
                    if (ce) {
                        const double* cp = ce + (long)(k0 + g0 + j) * npair;
                        double ae[3] = {cp[0], cp[dy], cp[dz]};
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
    if (!live) return;
    if (G == 1) {
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) cb[e * npair] = acc[e];
    }
    if (gmx) { const long o = P.o_off + blk; gmx[o] = l[0]; gmy[o] = l[1]; gmz[o] = l[2]; }
}

// blocks: (pulse, combination, chunk of 64 points), k_bloch_train_prop's order.  cw: the cotangents of the planes from the run
// adjoint.  part: one double2 (sum of dL / d rotx, sum of dL / d roty) per (workgroup, sample), VjpPulseDev's layout with the
// combinations in place of the scales and nch = chunks of 64 points.  ck: the checkpoints, BlochCkDev's layout.
__global__ __launch_bounds__(256) void k_bloch_train_prop_vjp(const double* __restrict__ in, const double* __restrict__ df,
                                                              const double* __restrict__ pos3, const double* __restrict__ amp,
                                                              const BlochPulseDev* __restrict__ pulses,
                                                              const TrainPulseDev* __restrict__ trains,
                                                              const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                              const BlochCkDev* __restrict__ cks, const double* __restrict__ cw,
                                                              double2* __restrict__ part, double* ck) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    const SimBlock bk = blocks[blockIdx.x];
    const TrainPropVjpThread C = bloch_train_prop_vjp_thread(bk, df, pos3, amp, pulses, trains, vp, cks, part, ck);
    double l[3] = {0, 0, 0}, le[3] = {0, 0, 0};
    bloch_train_prop_vjp_seed(C, bk, cw, l, le);
    bloch_train_prop_vjp_forward(C, sst, in);
    bloch_train_prop_vjp_backward(C, sst, red, in, l, le);
}

// grad[t_off + t] = (-(gamma dt_t) X, +(gamma dt_t) Y), (X, Y) = sum_c amp_c (sum over chunks of part(c, chunk, t)), chunks then
// the pulse's combinations in index order; one thread per sample, one workgroup per (pulse, 256 samples) from its own table.
__global__ __launch_bounds__(256) void k_bloch_train_vjp_fold(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                              const SimBlock* __restrict__ blocks, const double* __restrict__ amp,
                                                              const TrainPulseDev* __restrict__ trains, int nscale,
                                                              const double* __restrict__ in, const BlochPulseDev* __restrict__ pulses,
                                                              double2* __restrict__ grad) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const int t = bk.chunk * 256 + threadIdx.x;
    if (t >= V.n) return;
    const double2 g = abr_vjp_fold_sum(part, V, amp + Tr.a_off, nscale * Tr.ngain, t);
    const double f = pulses[bk.pulse].gamma * in[BLOCH_IN * (V.r_off + t) + 8];
    grad[V.r_off + t] = make_double2(-(f * g.x), f * g.y);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_vjp_batch (arguments checked by api.cpp): the forward train's staging (bloch_stage, train_stage)
// plus the cotangents, the partial and checkpoint descriptors and the tables of the period adjoint and of the fold; one upload,
// four launches, one download.  The output region is the gradient (T double2), dL / d m0 (3 O doubles), then what stays on the
// device: the propagators' planes, their cotangents, the partials and the two kernels' checkpoints.
TrainVjpSections train_vjp_stage(TrainStaged& Ts, int npulse, const long* toff, int nscale, const int* ntr) {
    BlochStaged& B = Ts.B;
    Staging& S = B.S;
    TrainVjpSections V;
    std::vector<VjpPulseDev> vp(npulse);
    std::vector<BlochCkDev> ckr(npulse), ckp(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int n = B.ntime[p], nch = int((B.npair[p] + 255) / 256), nch64 = int((B.npair[p] + 63) / 64);
        const int ngr = (ntr[p] + TRV_T - 1) / TRV_T, ngp = (n + VJP_T - 1) / VJP_T;
        const long ncomb = (long)nscale * Ts.tr[p].ngain;
        vp[p] = VjpPulseDev{toff[p], V.npart, n, nch64};
        ckr[p] = BlochCkDev{V.nckr, ngr, 0};
        ckp[p] = BlochCkDev{V.nckp, ngp, 0};
        V.npart += ncomb * nch64 * n;
        V.nckr += (long)nscale * nch * ngr * BLOCH_CK;
        V.nckp += ncomb * nch64 * ngp * BLOCH_CK;
        V.nwg += ncomb * nch64;
        V.nfold += (n + 255) / 256;
    }
    V.o_vp = S.add(npulse * sizeof(VjpPulseDev));
    V.o_ckr = S.add(npulse * sizeof(BlochCkDev));
    V.o_ckp = S.add(npulse * sizeof(BlochCkDev));
    V.o_vb = S.add(V.nwg * sizeof(SimBlock));
    V.o_fb = S.add(V.nfold * sizeof(SimBlock));
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(V.o_vp));
    std::copy(ckr.begin(), ckr.end(), S.at<BlochCkDev>(V.o_ckr));
    std::copy(ckp.begin(), ckp.end(), S.at<BlochCkDev>(V.o_ckp));
    // the period adjoint's table: k_bloch_train_prop's order (the longest periods first) with chunks of 64 points
    const SimBlock* fb = S.at<SimBlock>(S.o_bk);
    SimBlock* vb = S.at<SimBlock>(V.o_vb);
    for (long w = 0; w < S.nblk; ++w) {
        if (fb[w].scale != 0 || fb[w].chunk != 0) continue;               // the first workgroup of each pulse, in launch order
        const int p = fb[w].pulse;
        const int ncomb = nscale * Ts.tr[p].ngain;
        for (int c = 0; c < ncomb; ++c)
            for (int k = 0; k < vp[p].nch; ++k) *vb++ = SimBlock{p, c, k, 0};
    }
    SimBlock* ob = S.at<SimBlock>(V.o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int k = 0; k < (B.ntime[p] + 255) / 256; ++k) *ob++ = SimBlock{p, 0, k, 0};
    return V;
}

void train_launch_prop_vjp(TrainStaged& Ts, const TrainVjpSections& V, hipStream_t st, const double* cw, double2* part, double* ck,
                           const double* in) {
    Staging& S = Ts.B.S;
    hipLaunchKernelGGL(k_bloch_train_prop_vjp, dim3((unsigned)V.nwg), dim3(256), 0, st, in ? in : S.dev<const double>(Ts.B.o_in),
                       S.dev<const double>(Ts.B.o_df), S.dev<const double>(Ts.B.o_pos), S.dev<const double>(Ts.o_amp),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(V.o_vb),
                       S.dev<const VjpPulseDev>(V.o_vp), S.dev<const BlochCkDev>(V.o_ckp), cw, part, ck);
}

void train_launch_run_vjp(TrainStaged& Ts, const TrainVjpSections& V, hipStream_t st, const double* ws, int demod, const double* ce,
                          const double* cf, double* ck, double* cw, double* gm) {
    Staging& S = Ts.B.S;
    const long O = Ts.B.O, E = Ts.E;
    hipLaunchKernelGGL(k_bloch_train_run_vjp, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, S.dev<const double2>(Ts.o_rep),
                       S.dev<const int>(Ts.o_gi), S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const BlochCkDev>(V.o_ckr), S.dev<const double>(Ts.B.o_m0), demod, ce,
                       ce ? ce + E : nullptr, ce ? ce + 2 * E : nullptr, cf, cf ? cf + O : nullptr, cf ? cf + 2 * O : nullptr, ck, cw,
                       gm, gm ? gm + O : nullptr, gm ? gm + 2 * O : nullptr);
}

void bloch_train_vjp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                               int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                               const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                               const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                               const double* m0x, const double* m0y, const double* m0z, const double* cex, const double* cey,
                               const double* cez, const double* cfx, const double* cfy, const double* cfz, double* g_re, double* g_im,
                               double* gmx, double* gmy, double* gmz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    Staging& S = B.S;
    const long O = B.O, T = toff[npulse], E = Ts.E;
    const size_t o_ce = S.add(cex ? (size_t)E * 24 : 0), o_cf = S.add(cfx ? (size_t)O * 24 : 0);
    if (cex) {
        double* c = S.at<double>(o_ce);
        std::copy(cex, cex + E, c);
        std::copy(cey, cey + E, c + E);
        std::copy(cez, cez + E, c + 2 * E);
    }
    if (cfx) {
        double* c = S.at<double>(o_cf);
        std::copy(cfx, cfx + O, c);
        std::copy(cfy, cfy + O, c + O);
        std::copy(cfz, cfz + O, c + 2 * O);
    }
    const TrainVjpSections V = train_vjp_stage(Ts, npulse, toff, nscale, ntr);
    const long npart = V.npart, nckr = V.nckr, nckp = V.nckp;
    const size_t O3 = ((size_t)O * 3 + 1) & ~size_t(1);          // an even count: the partials after it stay 16-byte aligned
    const size_t W = (size_t)Ts.W;
    S.upload(((size_t)T * 2 + O3 + 2 * W + (size_t)npart * 2 + (size_t)nckr + (size_t)nckp) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* gm = reinterpret_cast<double*>(grad + T);
    double* ws = gm + O3;
    double* cw = ws + W;
    double2* part = reinterpret_cast<double2*>(cw + W);
    double* ck1 = reinterpret_cast<double*>(part + npart);
    double* ck2 = ck1 + nckr;
    MBFIR_HIP(hipMemsetAsync(cw, 0, W * 8, st));                 // upload does not zero the output region
    train_launch_prop(Ts, st, ws);
    const double* ced = cex ? S.dev<const double>(o_ce) : nullptr;
    const double* cfd = cfx ? S.dev<const double>(o_cf) : nullptr;
    const bool want_m0 = gmx != nullptr;
    train_launch_run_vjp(Ts, V, st, ws, demod, ced, cfd, ck1, cw, want_m0 ? gm : nullptr);
    train_launch_prop_vjp(Ts, V, st, cw, part, ck2);
    hipLaunchKernelGGL(k_bloch_train_vjp_fold, dim3((unsigned)V.nfold), dim3(256), 0, st, part, S.dev<const VjpPulseDev>(V.o_vp),
                       S.dev<const SimBlock>(V.o_fb), S.dev<const double>(Ts.o_amp), S.dev<const TrainPulseDev>(Ts.o_tr), nscale,
                       S.dev<const double>(B.o_in), S.dev<const BlochPulseDev>(S.o_pd), grad);
    std::vector<double> h((size_t)T * 2 + (want_m0 ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), g_re, g_im);
    if (want_m0) {
        const double* hm = h.data() + 2 * T;
        std::copy(hm, hm + O, gmx);
        std::copy(hm + O, hm + 2 * O, gmy);
        std::copy(hm + 2 * O, hm + 3 * O, gmz);
    }
}

}  // namespace mbfir
