// Adjoint of the pulse train in its schedule: the vector-Jacobian product of bloch_train_batch's echoes and final state
// with respect to the gain and the RF phase of every repetition.  In blochtrainvjp.hip's notation, per point and scale, with g the
// gain index of repetition k, u_k = Z(+phi_k) m_k, a_k = Z(+phi_k) lambda_{k+1}, ae_k = Z(+phi_k) ce_k (demod: ce_k), J v = (-v_y,
// v_x, 0) the generator of Z, and (dA, dB, dA_e, dB_e) the derivative of the gain's planes in the gain:
//     dL / dgains[k]  = a_k . (dA u_k + meq dB) + ae_k . (dA_e u_k + meq dB_e)
//     dL / dphases[k] = a_k . (A J u_k - J n_k) + ae_k . (A_e J u_k - (demod ? 0 : J ne_k)),   n_k = A u_k + meq B, ne_k = A_e u_k + meq B_e
// both summed over the scales and the points.  J commutes with Z and Z(-phi) is Z(+phi)', so a_k . J n_k is lambda_{k+1} . J m_{k+1}
// and ae_k . J ne_k is ce_k . J echo_k: the phase enters through the two z-rotations of a repetition only, the gain through the
// amplitude of its 24 propagator entries only, and neither needs a reverse sweep over the period's samples.
//   k_bloch_train_prop_dgain: the tangent of the period along its own b1 row times the scale: d amplitude / d gain = scale, so the
//                             direction is dn_t = (((-(Re b1_t scale)) gamma) dt_t, ((Im b1_t scale) gamma) dt_t) about the primal
//                             axis at scale x gain.  A gain of 0 is an ordinary primal; nothing is divided by the gain.
//                             k_bloch_train_prop_jvp's thread layout (wave w owns column w of [A | B], lane l the point) and
//                             per-sample arithmetic (bloch_jvp_shared) with one direction, staged from the sample rows themselves.
//   k_bloch_train_run_sched:  k_bloch_train_run_vjp's table, forward walk with a checkpoint every TRV_T repetitions and statements
//                             for u, a, ae and lambda (dL / dm0 keeps that kernel's bits); the two contractions in place of the
//                             planes' cotangents.  The 256 points' contributions to a group of TRV_T repetitions go through the
//                             VJP_T x 2 rows of the rf adjoint's tile in a fixed order: one double2 partial per (scale, chunk,
//                             repetition), no atomics.
//   k_bloch_train_sched_fold: one thread per repetition sums the chunks, then the scales, in index order.
// The primal planes come from the shipped k_bloch_train_prop.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// blocks: (pulse, combination, chunk of 64 points), k_bloch_train_prop_jvp's table with one direction group.  scales: the call's
// scales; amp: scale x gain per combination.  dws receives the tangent planes, laid out as k_bloch_train_prop lays out the primal.
__global__ __launch_bounds__(256) void k_bloch_train_prop_dgain(const double* __restrict__ in, const double* __restrict__ df,
                                                                const double* __restrict__ pos3, const double* __restrict__ amp,
                                                                const double* __restrict__ scales,
                                                                const BlochPulseDev* __restrict__ pulses,
                                                                const TrainPulseDev* __restrict__ trains,
                                                                const SimBlock* __restrict__ blocks, double* __restrict__ dws) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double2 sdn[BLOCH_CH];
    const int tid = threadIdx.x, col = tid >> 6, lane = tid & 63;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const double sc = amp[Tr.a_off + bk.scale], dsc = scales[bk.scale / Tr.ngain], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos, echo = Tr.echo;
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 64 + lane;
    const bool live = pair < npair;
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const bool rec = col == 3;                                            // uniform over the wavefront
    const int ent = rec ? 9 : 3 * col;                                    // the column's first entry among A (9), B (3)
    double* w = dws + Tr.w_off + (long)bk.scale * TRAIN_ENT * npair + (long)ent * npair + (live ? pair : 0);
    double m[3] = {col == 0 ? 1.0 : 0.0, col == 1 ? 1.0 : 0.0, col == 2 ? 1.0 : 0.0}, dm[3] = {0, 0, 0};
    if (echo == 0 && live) {                                              // (A_e, B_e) = (I, 0) has no tangent
        double* o = w + 12 * npair;
        o[0] = 0; o[npair] = 0; o[2 * npair] = 0;
    }
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 amp, as k_bloch_train_prop forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
            sdn[tid] = make_double2(((-(s[0] * dsc)) * gamma) * dt, ((s[1] * dsc) * gamma) * dt);      // d (rotx, roty) / d gain
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
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
            m[0] = e2 * o[0]; m[1] = e2 * o[1];
            if (rec) m[2] = e1 * o[2] + (1 - e1); else m[2] = e1 * o[2];
            if (t0 + q + 1 == echo) {                                     // uniform over the workgroup: (dA_e, dB_e)
                double* oe = w + 12 * npair;
                oe[0] = dm[0]; oe[npair] = dm[1]; oe[2 * npair] = dm[2];
            }
        }
    }
    if (!live) return;
    w[0] = dm[0]; w[npair] = dm[1]; w[2 * npair] = dm[2];
}

// train_sched_dphi, train_sched_dphi_demod and train_sched_dot, a repetition's shares of the two contractions, are in sim_dev.h,
// shared with the fused products of the schedule (blochtrainschedgn.hip).

// blocks: the forward table (pulse, scale, chunk of 256 points).  ws: the propagators' planes; dws: their tangents in the gain (null:
// the gains' gradient is not wanted and its half of every partial is zero).  cex.. / cfx.. / gmx.. / ck: k_bloch_train_run_vjp's.
// part: one double2 (dL / dgain, dL / dphi) per (scale, chunk, repetition), VjpPulseDev's layout with the repetitions in place of
// the samples and nch = chunks of 256 points.
__global__ __launch_bounds__(256) void k_bloch_train_run_sched(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const SimBlock* __restrict__ blocks,
    const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0, int demod,
    const double* __restrict__ cex, const double* __restrict__ cey, const double* __restrict__ cez, const double* __restrict__ cfx,
    const double* __restrict__ cfy, const double* __restrict__ cfz, double* ck, double2* __restrict__ part, double* __restrict__ gmx,
    double* __restrict__ gmy, double* __restrict__ gmz) {
    __shared__ double2 scs[256];
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
    const bool live = pair < npair;                                       // a thread past the end of the grid contributes zeros
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
#pragma unroll
                        for (int i = 0; i < 3; ++i) l[i] = W[3 * i] * a[0] + W[3 * i + 1] * a[1] + W[3 * i + 2] * a[2];          // A' a
                        if (ce) {
                            const double* cp = ce + (long)(k0 + g0 + j) * npair;
                            double ae[3] = {cp[0], cp[dy], cp[dz]};
                            if (!demod) train_zp(c, s, ae);
                            train_affine(dW + 12, dW + 21, meq, u, dn);
                            gg += train_sched_dot(ae, dn);
                            if (demod) {
                                gp += train_sched_dphi_demod(W + 12, ae, u);
                            } else {
                                train_affine(W + 12, W + 21, meq, u, n);
                                gp += train_sched_dphi(W + 12, ae, u, n);
                            }
#pragma unroll
                            for (int i = 0; i < 3; ++i)
                                l[i] += W[12 + 3 * i] * ae[0] + W[13 + 3 * i] * ae[1] + W[14 + 3 * i] * ae[2];                   // A_e' ae
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
    if (live && gmx) { const long o = P.o_off + blk; gmx[o] = l[0]; gmy[o] = l[1]; gmz[o] = l[2]; }
}

// out[r_off + k] = sum over the scales of (sum over the chunks of part(scale, chunk, k)), chunks then scales in index order; one
// thread per repetition, one workgroup per (pulse, 256 repetitions) from its own table.
__global__ __launch_bounds__(256) void k_bloch_train_sched_fold(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                                const SimBlock* __restrict__ blocks, int nscale,
                                                                double2* __restrict__ out) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int k = bk.chunk * 256 + threadIdx.x;
    if (k >= V.n) return;
    double2 g = make_double2(0, 0);
    for (int s = 0; s < nscale; ++s) {
        double2 t = make_double2(0, 0);
        const double2* rw = part + V.p_off + (long)s * V.nch * V.n + k;
        for (int c = 0; c < V.nch; ++c) {
            const double2 v = rw[(long)c * V.n];
            t.x += v.x; t.y += v.y;
        }
        g.x += t.x; g.y += t.y;
    }
    out[V.r_off + k] = g;
}

void train_launch_prop_dgain(TrainStaged& Ts, hipStream_t st, size_t o_qb, long nwg, double* dws) {
    Staging& S = Ts.B.S;
    hipLaunchKernelGGL(k_bloch_train_prop_dgain, dim3((unsigned)nwg), dim3(256), 0, st, S.dev<const double>(Ts.B.o_in),
                       S.dev<const double>(Ts.B.o_df), S.dev<const double>(Ts.B.o_pos), S.dev<const double>(Ts.o_amp),
                       S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr),
                       S.dev<const SimBlock>(o_qb), dws);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_vjp_sched_batch (arguments checked by api.cpp): the forward train's staging (bloch_stage,
// train_stage) plus the cotangents, the partial and checkpoint descriptors and the tables of the period's tangent and of the fold;
// one upload, three launches and the fold (the period's tangent is skipped when ggain is null), one download.  The output region is
// the gradients (R double2), dL / d m0 (3 O doubles), then what stays on the device: the partials, the primal planes, their tangents
// and the checkpoints.
void bloch_train_vjp_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, const double* cex, const double* cey, const double* cez, const double* cfx,
                                     const double* cfy, const double* cfz, double* ggain, double* gphi, double* gmx, double* gmy,
                                     double* gmz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    Staging& S = B.S;
    const long O = B.O, R = roff[npulse], E = Ts.E;
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
    // the partials' and checkpoints' descriptors and the fold's table: one workgroup per (pulse, 256 repetitions)
    std::vector<VjpPulseDev> vp(npulse);
    std::vector<BlochCkDev> ckr(npulse);
    long npart = 0, nck = 0, nfold = 0;
    for (int p = 0; p < npulse; ++p) {
        const int nch = int((B.npair[p] + 255) / 256), ngr = (ntr[p] + TRV_T - 1) / TRV_T;
        vp[p] = VjpPulseDev{roff[p], npart, ntr[p], nch};
        ckr[p] = BlochCkDev{nck, ngr, 0};
        npart += (long)nscale * nch * ntr[p];
        nck += (long)nscale * nch * ngr * BLOCH_CK;
        nfold += (ntr[p] + 255) / 256;
    }
    const size_t o_vp = S.add(npulse * sizeof(VjpPulseDev)), o_ck = S.add(npulse * sizeof(BlochCkDev));
    const size_t o_fb = S.add(nfold * sizeof(SimBlock));
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(o_vp));
    std::copy(ckr.begin(), ckr.end(), S.at<BlochCkDev>(o_ck));
    SimBlock* ob = S.at<SimBlock>(o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int k = 0; k < (ntr[p] + 255) / 256; ++k) *ob++ = SimBlock{p, 0, k, 0};
    const bool want_g = ggain != nullptr, want_m0 = gmx != nullptr;
    long nwg = 0;                                                         // workgroups of the period's tangent
    const size_t o_qb = want_g ? train_jvp_table(Ts, nscale, 1, nwg) : 0;
    const size_t O3 = ((size_t)O * 3 + 1) & ~size_t(1);          // an even count: the partials after it stay 16-byte aligned
    const size_t W = (size_t)Ts.W;
    S.upload(((size_t)R * 2 + O3 + (size_t)npart * 2 + W + (want_g ? W : 0) + (size_t)nck) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* gm = reinterpret_cast<double*>(grad + R);
    double2* part = reinterpret_cast<double2*>(gm + O3);
    double* ws = reinterpret_cast<double*>(part + npart);
    double* dws = want_g ? ws + W : nullptr;
    double* ck = ws + W + (want_g ? W : 0);
    train_launch_prop(Ts, st, ws);
    if (want_g) train_launch_prop_dgain(Ts, st, o_qb, nwg, dws);
    const double* ced = cex ? S.dev<const double>(o_ce) : nullptr;
    const double* cfd = cfx ? S.dev<const double>(o_cf) : nullptr;
    hipLaunchKernelGGL(k_bloch_train_run_sched, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, dws, S.dev<const double2>(Ts.o_rep),
                       S.dev<const int>(Ts.o_gi), S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(o_vp), S.dev<const BlochCkDev>(o_ck),
                       S.dev<const double>(B.o_m0), demod, ced, ced ? ced + E : nullptr, ced ? ced + 2 * E : nullptr, cfd,
                       cfd ? cfd + O : nullptr, cfd ? cfd + 2 * O : nullptr, ck, part, want_m0 ? gm : nullptr,
                       want_m0 ? gm + O : nullptr, want_m0 ? gm + 2 * O : nullptr);
    hipLaunchKernelGGL(k_bloch_train_sched_fold, dim3((unsigned)nfold), dim3(256), 0, st, part, S.dev<const VjpPulseDev>(o_vp),
                       S.dev<const SimBlock>(o_fb), nscale, grad);
    std::vector<double> h((size_t)R * 2 + (want_m0 ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    for (long k = 0; k < R; ++k) {
        if (ggain) ggain[k] = h[2 * k];
        if (gphi) gphi[k] = h[2 * k + 1];
    }
    if (want_m0) {
        const double* hm = h.data() + 2 * R;
        std::copy(hm, hm + O, gmx);
        std::copy(hm + O, hm + 2 * O, gmy);
        std::copy(hm + 2 * O, hm + 3 * O, gmz);
    }
}

}  // namespace mbfir
