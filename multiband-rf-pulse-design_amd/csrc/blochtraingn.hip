// Fused least-squares and Gauss-Newton products of the pulse train.  In blochtrainvjp.hip's notation, per pulse,
//     L = 1/2 sum_s sum_k rw_k sum_points sum_c w_c (echo_{k,c} - t_c)^2 + 1/2 sum_s sum_points sum_c wf_c (m_{N,c} - tf_c)^2
// lsq returns L, g = dL / d Re b1 + i dL / d Im b1 and, on request, dL / dm0; gn returns H v = J' W J v for directions v of the
// period's b1, J the Jacobian of (echoes, final state) in b1 and W the weights, rw included.  Everything between the echoes (or
// their tangents) and the cotangents is pointwise and the thread that owns the point holds every operand, so neither is ever
// written: the run adjoint of 8z forms its own cotangents on the way back.
//   k_bloch_train_run_lsq: k_bloch_train_run_vjp's walk.  The forward walk writes the checkpoints only; at its end m_N has
//                          bloch_train_batch's bits, lambda_N = wf (m_N - tf).  On the way back the echo of repetition k is formed
//                          from the recomputed u_k with k_bloch_train_run's statements, r = echo - t, ce_k = rw_k w r, and the
//                          adjoint's accumulation follows.  The loss is summed per thread in the walk's order, per workgroup by a
//                          fixed tree (lm_block_sum) to one partial.
//   k_bloch_train_run_gn:  the same walk on the forward table times the directions, carrying (m, dm) with the tangent planes of
//                          the shipped k_bloch_train_prop_jvp; ce_k = rw_k w decho_k, lambda_N = wf dm_N.
//   k_bloch_train_gn_fold: k_bloch_train_vjp_fold per (pulse, direction), and the loss partials of a pulse in index order.
// The propagators' planes come from the shipped k_bloch_train_prop, the period's adjoint is the shipped k_bloch_train_prop_vjp,
// launched once per direction on that direction's cotangent planes and partials with one checkpoint region (launches on one stream
// are ordered).  No atomics.  Echo weights and targets lie as the echoes do (ebcast = 0) or as the final planes do, used at every
// repetition (ebcast = 1): then nothing echo-sized crosses the bus in either direction.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// k_bloch_train_run_gn's body and its switch TGN_HOIST are in sim_dev.h (bloch_train_run_gn_body), shared with the device
// Levenberg-Marquardt step (blochtrainlm.hip).

// blocks, ws, cw, cks, ck, gmx..: k_bloch_train_run_vjp's.  rw (null: ones): the repetitions' factors, laid out as rep.  we / te
// (null: no echo term): the echo weights and targets, three planes PE entries apart, pulse p from e_off (ebcast 0) or o_off
// (ebcast 1).  wf / tf (null: no final term): three planes PO apart, where the final planes lie.  lpart: one loss partial per
// workgroup, workgroup (scale, chunk) of pulse p at lp[p] + scale nch + chunk.
__global__ __launch_bounds__(256) void k_bloch_train_run_lsq(
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
        const double w0 = wf[o], w1 = wf[PO + o], w2 = wf[2 * PO + o];
        const double r0 = m[0] - tf[o], r1 = m[1] - tf[PO + o], r2 = m[2] - tf[2 * PO + o];
        l[0] = w0 * r0; l[1] = w1 * r1; l[2] = w2 * r2;
        ls = 0.5 * (w0 * (r0 * r0) + w1 * (r1 * r1) + w2 * (r2 * r2));
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
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const double wi = wp[ko + i * PE], r = e[i] - tp[ko + i * PE];
                            ae[i] = rk * (wi * r);                        // ce_k = rw_k w r
                            q2 += wi * (r * r);
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

// blocks: the forward table times the directions (pad).  dws: the tangent planes of k_bloch_train_prop_jvp, ndir directions.  cw:
// direction d's cotangent planes from d WT; ck: direction d's checkpoints from 2 d CK, a group 2 x 3 x 256 doubles (m, then dm).
// we / wf as k_bloch_train_run_lsq's.
__global__ __launch_bounds__(256) void k_bloch_train_run_gn(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0, int demod, int ebcast,
    int ndir, const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, long WT, long CK, double* ck,
    double* cw) {
    bloch_train_run_gn_body(blocks[blockIdx.x], ws, dws, rep, gidx, rw, pulses, trains, cks, m0, demod, ebcast, ndir, we, PE, wf, PO, WT, CK, ck,
                            cw);
}

// out[ndir r_off + d n + t] = k_bloch_train_vjp_fold's value from direction d's partials (part + d NP): one thread per sample, one
// workgroup per (pulse, direction, 256 samples) from its own table (SimBlock: pulse, direction, chunk of samples).  lsq (loss not
// null, ndir = 1): the first thread of a pulse's first workgroup also sums the pulse's nscale nch loss partials in index order.
__global__ __launch_bounds__(256) void k_bloch_train_gn_fold(const double2* __restrict__ part, long NP,
                                                             const VjpPulseDev* __restrict__ vp, const SimBlock* __restrict__ blocks,
                                                             const double* __restrict__ amp, const TrainPulseDev* __restrict__ trains,
                                                             int nscale, int ndir, const double* __restrict__ in,
                                                             const BlochPulseDev* __restrict__ pulses, double2* __restrict__ out,
                                                             const double* __restrict__ lpart, const long* __restrict__ lp,
                                                             double* __restrict__ loss) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const BlochPulseDev P = pulses[bk.pulse];
    const int t = bk.chunk * 256 + threadIdx.x;
    if (t >= V.n) return;
    const double2 g = abr_vjp_fold_sum(part + (long)bk.scale * NP, V, amp + Tr.a_off, nscale * Tr.ngain, t);
    const double f = P.gamma * in[BLOCH_IN * (V.r_off + t) + 8];
    out[(long)ndir * V.r_off + (long)bk.scale * V.n + t] = make_double2(-(f * g.x), f * g.y);
    if (loss && t == 0) {
        const double* q = lpart + lp[bk.pulse];
        const long nw = (long)nscale * (((long)P.nf * P.npos + 255) / 256);
        double s = 0;
        for (long k = 0; k < nw; ++k) s += q[k];
        loss[bk.pulse] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_lsq_batch and mbfir_bloch_train_gn_batch (arguments checked by api.cpp): the forward train's staging
// (bloch_stage, train_stage), the adjoint's tables (train_vjp_stage), the weights and targets, and for gn the directions and the
// tangent's table; one upload, the launches, one download.  The output region is what comes down (the gradient or the products, the
// loss, dL / dm0), then what stays on the device: the planes, their tangents (gn), their cotangents per direction, the partials
// per direction, the loss partials and the checkpoints.
namespace {

size_t add_triple(Staging& S, const double* x, const double* y, const double* z, long n) {
    const size_t o = S.add(x ? (size_t)n * 24 : 0);
    if (x) {
        double* d = S.at<double>(o);
        std::copy(x, x + n, d);
        std::copy(y, y + n, d + n);
        std::copy(z, z + n, d + 2 * n);
    }
    return o;
}

}  // namespace

// The sections after train_stage: t* null for gn.
void train_gn_stage(TrainGnCall& Cl, int npulse, const long* toff, int nscale, const int* ntr, const long* roff, int ebcast, int ndir,
                    const double* const w[3], const double* const t[3], const double* rw, const double* const wf[3],
                    const double* const tf[3]) {
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    Staging& S = B.S;
    Cl.V = train_vjp_stage(Ts, npulse, toff, nscale, ntr);
    Cl.PE = ebcast ? B.O : Ts.E;
    Cl.o_we = add_triple(S, w[0], w[1], w[2], Cl.PE);
    Cl.o_te = add_triple(S, t[0], t[1], t[2], Cl.PE);
    Cl.o_wf = add_triple(S, wf[0], wf[1], wf[2], B.O);
    Cl.o_tf = add_triple(S, tf[0], tf[1], tf[2], B.O);
    Cl.o_rw = S.add(rw ? (size_t)roff[npulse] * 8 : 0);
    if (rw) std::copy(rw, rw + roff[npulse], S.at<double>(Cl.o_rw));
    std::vector<long> lp(npulse);
    for (int p = 0; p < npulse; ++p) {
        lp[p] = Cl.nlp;
        Cl.nlp += (long)nscale * ((B.npair[p] + 255) / 256);
        Cl.ngf += (long)ndir * ((B.ntime[p] + 255) / 256);
    }
    Cl.o_lp = S.add(npulse * sizeof(long));
    std::copy(lp.begin(), lp.end(), S.at<long>(Cl.o_lp));
    Cl.o_gf = S.add(Cl.ngf * sizeof(SimBlock));
    SimBlock* gf = S.at<SimBlock>(Cl.o_gf);
    for (int p = 0; p < npulse; ++p)
        for (int d = 0; d < ndir; ++d)
            for (int k = 0; k < (B.ntime[p] + 255) / 256; ++k) *gf++ = SimBlock{p, d, k, 0};
}

// k_bloch_train_run_lsq on the staged sections of Cl with the planes ws, and k_bloch_train_gn_fold at one direction with the loss sum,
// on the input rows `in` (null: the staged ones): the launches of bloch_train_lsq_batch_run, which the device step's trial repeats.
void train_launch_run_lsq(TrainGnCall& Cl, hipStream_t st, int demod, int ebcast, bool echo, bool rep, bool fin, const double* ws,
                          double* ck, double* cw, double* gm, double* lpart) {
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    Staging& S = B.S;
    const TrainVjpSections& V = Cl.V;
    const long O = B.O;
    hipLaunchKernelGGL(k_bloch_train_run_lsq, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, S.dev<const double2>(Ts.o_rep),
                       S.dev<const int>(Ts.o_gi), rep ? S.dev<const double>(Cl.o_rw) : nullptr, S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(S.o_bk), S.dev<const BlochCkDev>(V.o_ckr),
                       S.dev<const long>(Cl.o_lp), S.dev<const double>(B.o_m0), demod, ebcast,
                       echo ? S.dev<const double>(Cl.o_we) : nullptr, echo ? S.dev<const double>(Cl.o_te) : nullptr, Cl.PE,
                       fin ? S.dev<const double>(Cl.o_wf) : nullptr, fin ? S.dev<const double>(Cl.o_tf) : nullptr, O, ck, cw,
                       gm, gm ? gm + O : nullptr, gm ? gm + 2 * O : nullptr, lpart);
}
void train_launch_lsq_fold(TrainGnCall& Cl, hipStream_t st, int nscale, const double2* part, const double* in, double2* grad,
                           const double* lpart, double* loss) {
    TrainStaged& Ts = Cl.Ts;
    Staging& S = Ts.B.S;
    const TrainVjpSections& V = Cl.V;
    hipLaunchKernelGGL(k_bloch_train_gn_fold, dim3((unsigned)Cl.ngf), dim3(256), 0, st, part, V.npart,
                       S.dev<const VjpPulseDev>(V.o_vp), S.dev<const SimBlock>(Cl.o_gf), S.dev<const double>(Ts.o_amp),
                       S.dev<const TrainPulseDev>(Ts.o_tr), nscale, 1, in ? in : S.dev<const double>(Ts.B.o_in),
                       S.dev<const BlochPulseDev>(S.o_pd), grad, lpart, S.dev<const long>(Cl.o_lp), loss);
}

void bloch_train_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                               int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                               const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                               const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                               const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* const w[3],
                               const double* const t[3], const double* rw, const double* const wf[3], const double* const tf[3],
                               double* loss, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainGnCall Cl;
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    train_gn_stage(Cl, npulse, toff, nscale, ntr, roff, ebcast, 1, w, t, rw, wf, tf);
    Staging& S = B.S;
    const TrainVjpSections& V = Cl.V;
    const long O = B.O, T = toff[npulse];
    const bool want_m0 = gmx != nullptr;
    const size_t NL = ((size_t)npulse + 1) & ~size_t(1), O3 = want_m0 ? ((size_t)O * 3 + 1) & ~size_t(1) : 0;      // 16-byte alignment
    const size_t W = (size_t)Ts.W, LP = ((size_t)Cl.nlp + 1) & ~size_t(1);
    S.upload(((size_t)T * 2 + NL + O3 + 2 * W + (size_t)V.npart * 2 + LP + (size_t)V.nckr + (size_t)V.nckp) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* dloss = reinterpret_cast<double*>(grad + T);
    double* gm = dloss + NL;
    double* ws = gm + O3;
    double* cw = ws + W;
    double2* part = reinterpret_cast<double2*>(cw + W);
    double* lpart = reinterpret_cast<double*>(part + V.npart);
    double* ck1 = lpart + LP;
    double* ck2 = ck1 + V.nckr;
    MBFIR_HIP(hipMemsetAsync(cw, 0, W * 8, st));                 // upload does not zero the output region
    train_launch_prop(Ts, st, ws);
    train_launch_run_lsq(Cl, st, demod, ebcast, w[0] != nullptr, rw != nullptr, wf[0] != nullptr, ws, ck1, cw, want_m0 ? gm : nullptr,
                         lpart);
    train_launch_prop_vjp(Ts, V, st, cw, part, ck2);
    train_launch_lsq_fold(Cl, st, nscale, part, nullptr, grad, lpart, dloss);
    std::vector<double> h((size_t)T * 2 + NL + O3);
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), g_re, g_im);
    std::copy(h.data() + 2 * T, h.data() + 2 * T + npulse, loss);
    if (want_m0) {
        const double* hm = h.data() + 2 * T + NL;
        std::copy(hm, hm + O, gmx);
        std::copy(hm + O, hm + 2 * O, gmy);
        std::copy(hm + 2 * O, hm + 3 * O, gmz);
    }
}

void bloch_train_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                              const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                              const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                              int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                              const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                              const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                              const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* const w[3],
                              const double* rw, const double* const wf[3], int ndir, const double* v_re, const double* v_im,
                              double* h_re, double* h_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainGnCall Cl;
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    const double* const none[3] = {nullptr, nullptr, nullptr};
    train_gn_stage(Cl, npulse, toff, nscale, ntr, roff, ebcast, ndir, w, none, rw, wf, none);
    Staging& S = B.S;
    const TrainVjpSections& V = Cl.V;
    const long O = B.O;
    const size_t NV = (size_t)ndir * toff[npulse], W = (size_t)Ts.W, K = (size_t)ndir;
    const size_t o_v = S.add(NV * 16), o_jb = sim_group_table(S, ndir);
    pack_cplx(NV, v_re, v_im, S.at<double2>(o_v));
    long nwq = 0;
    const size_t o_qb = train_jvp_table(Ts, nscale, ndir, nwq);
    S.upload((NV * 2 + W + 2 * K * W + K * (size_t)V.npart * 2 + 2 * K * (size_t)V.nckr + (size_t)V.nckp) * 8, st);
    double2* out = S.dev<double2>(S.o_out);
    double* ws = reinterpret_cast<double*>(out + NV);
    double* dws = ws + W;
    double* cw = dws + K * W;
    double2* part = reinterpret_cast<double2*>(cw + K * W);
    double* ck1 = reinterpret_cast<double*>(part + K * (size_t)V.npart);
    double* ck2 = ck1 + 2 * K * (size_t)V.nckr;
    MBFIR_HIP(hipMemsetAsync(cw, 0, K * W * 8, st));             // upload does not zero the output region
    train_launch_prop(Ts, st, ws);
    train_launch_prop_jvp(Ts, st, o_qb, nwq, o_v, ndir, dws);
    hipLaunchKernelGGL(k_bloch_train_run_gn, dim3((unsigned)(S.nblk * ndir)), dim3(256), 0, st, ws, dws,
                       S.dev<const double2>(Ts.o_rep), S.dev<const int>(Ts.o_gi), rw ? S.dev<const double>(Cl.o_rw) : nullptr,
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(o_jb),
                       S.dev<const BlochCkDev>(V.o_ckr), S.dev<const double>(B.o_m0), demod, ebcast, ndir,
                       w[0] ? S.dev<const double>(Cl.o_we) : nullptr, Cl.PE, wf[0] ? S.dev<const double>(Cl.o_wf) : nullptr, O,
                       (long)W, V.nckr, ck1, cw);
    for (int d = 0; d < ndir; ++d) train_launch_prop_vjp(Ts, V, st, cw + d * W, part + (size_t)d * V.npart, ck2);
    hipLaunchKernelGGL(k_bloch_train_gn_fold, dim3((unsigned)Cl.ngf), dim3(256), 0, st, part, V.npart,
                       S.dev<const VjpPulseDev>(V.o_vp), S.dev<const SimBlock>(Cl.o_gf), S.dev<const double>(Ts.o_amp),
                       S.dev<const TrainPulseDev>(Ts.o_tr), nscale, ndir, S.dev<const double>(B.o_in),
                       S.dev<const BlochPulseDev>(S.o_pd), out, nullptr, S.dev<const long>(Cl.o_lp), nullptr);
    std::vector<double> h(NV * 2);
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(NV, reinterpret_cast<const double2*>(h.data()), h_re, h_im);
}

}  // namespace mbfir
