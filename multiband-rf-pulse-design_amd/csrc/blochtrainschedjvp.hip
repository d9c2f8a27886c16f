// Tangent of the pulse train in its schedule: the Jacobian-vector product of bloch_train_batch's echoes and final state
// with respect to the gain and the RF phase of every repetition and to the initial magnetisation.  In blochtrainsched.hip's notation,
// per point and scale, with g the gain index of repetition k, J v = (-v_y, v_x, 0) the generator of Z, (dA, dB, dA_e, dB_e) the
// derivative of the gain's planes in the gain (k_bloch_train_prop_dgain's planes), along a direction (dg, dp, dm_0):
//     u_k  = Z(+phi_k) m_k                 du_k  = Z(+phi_k) dm_k + dp_k J u_k
//     n_k  = A u_k + meq B                 dn_k  = A du_k   + dg_k (dA u_k   + meq dB)
//     ne_k = A_e u_k + meq B_e             dne_k = A_e du_k + dg_k (dA_e u_k + meq dB_e)
//     m_{k+1} = Z(-phi_k) n_k              dm_{k+1} = Z(-phi_k) (dn_k  - dp_k J n_k)
//     echo_k  = Z(-phi_k) ne_k             decho_k  = Z(-phi_k) (dne_k - dp_k J ne_k)      (demod: decho_k = dne_k)
// Nothing is divided by a gain, and dp is per radian.  The planes' tangents depend on the gain's value and not on the direction, so
// the period is swept once more per (scale, distinct gain) whatever the number of directions, and not at all without a gains
// direction.  One kernel after the shipped k_bloch_train_prop and k_bloch_train_prop_dgain, no atomics, no reduction:
//   k_bloch_train_run_sched_jvp: k_bloch_train_run_jvp's layout, the forward table times the groups of TSJ_K directions; a thread
//                                carries m and the group's dm.  u, n, ne and the two vectors dA u + meq dB, dA_e u + meq dB_e are
//                                formed once per repetition and serve every direction of the group, which then costs two 3 x 3
//                                products and a few fma.  The directions' (dg_k, dp_k) of 256 repetitions are staged through LDS next
//                                to the repetition table.
// Gains and phases directions lie as the repetition table does, direction k of pulse p at ndir r_off + k ntr.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Directions per workgroup: the largest of 1, 2, 4, 8 without scratch at no less than k_bloch_train_run's occupancy (5 waves per
// SIMD) minus one (DESIGN 8ae has the table).  As in k_bloch_train_run_jvp the 24 primal planes in registers leave room for one
// direction at four waves: two need 140 VGPRs.  The tangent planes are streamed twelve at a time every repetition; held next to
// the primal planes they would not fit at all.
#ifndef TSJ_K
#define TSJ_K 1
#endif

// train_sj_in and train_sj_map, the two statements of a direction's repetition, are in sim_dev.h, shared with the fused products of
// the schedule (blochtrainschedgn.hip).

// blocks: the forward table (pulse, scale, chunk of 256 points) times the direction groups (pad).  ws: the primal planes; dws: their
// tangents in the gain, laid out alike (null: no gains direction).  rep, gidx, m0, demod: k_bloch_train_run's.  dgain / dphi (either
// null: zero): direction k of a pulse at ndir r_off + k ntr.  dm0, ex .., fx .., dex, dfx, NE, NO: k_bloch_train_run_jvp's.
__global__ __launch_bounds__(256) void k_bloch_train_run_sched_jvp(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const SimBlock* __restrict__ blocks,
    const double* __restrict__ m0, const double* __restrict__ dgain, const double* __restrict__ dphi, const double* __restrict__ dm0,
    int demod, int ndir, int nscale, long NE, long NO, double* __restrict__ ex, double* __restrict__ ey, double* __restrict__ ez,
    double* __restrict__ fx, double* __restrict__ fy, double* __restrict__ fz, double* __restrict__ dex, double* __restrict__ dfx) {
    __shared__ double2 scs[256];
    __shared__ int sgi[256];
    __shared__ double2 sdr[TSJ_K][256];                                   // (dg_k, dp_k) of the group's directions
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain;
    const double meq = Tr.meq;
    const int k0 = bk.pad * TSJ_K, kcnt = min(TSJ_K, ndir - k0);
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;
    const long blk = (long)bk.scale * npair + pair;
    const long comb0 = (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    const double* wb = ws + Tr.w_off + comb0;
    const double* db = dws ? dws + Tr.w_off + comb0 : nullptr;
    const long sbase = (long)ndir * Tr.r_off + (long)k0 * ntr;            // the group's first direction in dgain / dphi
    const bool first = bk.pad == 0;
    double m[3] = {0, 0, 1}, W[TRAIN_ENT], dm[TSJ_K][3];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int k = 0; k < TSJ_K; ++k) {
        dm[k][0] = dm[k][1] = dm[k][2] = 0;
        if (k < kcnt && live && dm0) {
            const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * npair + pair;
            dm[k][0] = dm0[o]; dm[k][1] = dm0[NO + o]; dm[k][2] = dm0[2 * NO + o];
        }
    }
    if (G == 1) {                                                         // one distinct gain: the primal planes are loaded once
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wb[e * npair];
    }
    double* eo = (ex && first) ? ex + Tr.e_off + (long)bk.scale * ntr * npair + pair : nullptr;
    const long dy = ey - ex, dz = ez - ex;                                // the three planes are laid out alike
    // the echoes of direction k0 at this scale; a direction is nscale ntr npair entries
    double* deo = dex ? dex + (long)ndir * Tr.e_off + ((long)k0 * nscale + bk.scale) * ntr * npair + pair : nullptr;
    const long estr = (long)nscale * ntr * npair;
    for (int r0 = 0; r0 < ntr; r0 += 256) {
        __syncthreads();
        const int cnt = min(256, ntr - r0);
        if (tid < cnt) {
            scs[tid] = rep[Tr.r_off + r0 + tid];
            sgi[tid] = gidx[Tr.r_off + r0 + tid];
#pragma unroll
            for (int k = 0; k < TSJ_K; ++k)
                if (k < kcnt) {
                    const long o = sbase + (long)k * ntr + r0 + tid;
                    sdr[k][tid] = make_double2(dgain ? dgain[o] : 0.0, dphi ? dphi[o] : 0.0);
                }
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const double c = scs[q].x, s = scs[q].y;
            if (G != 1) {
                const double* wg = wb + (long)sgi[q] * TRAIN_ENT * npair;
#pragma unroll
                for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wg[e * npair];
            }
            const double* dg = db ? db + (long)sgi[q] * TRAIN_ENT * npair : nullptr;
            train_zp(c, s, m);                                            // u = Z(+phi) m
#pragma unroll
            for (int k = 0; k < TSJ_K; ++k)
                if (k < kcnt) train_sj_in(c, s, sdr[k][q].y, m, dm[k]);   // du
            // the echo's half first and the state's half after it, so that the shared vectors of one are dead before the other's live
            if (deo || eo) {
                double e[3], ge[3] = {0, 0, 0};
                train_affine(W + 12, W + 21, meq, m, e);                  // ne before it is turned back
                if (deo) {
                    if (dg) {                                             // dA_e u + meq dB_e
                        double dW[12];
#pragma unroll
                        for (int i = 0; i < 12; ++i) dW[i] = dg[(12 + i) * npair];
                        train_affine(dW, dW + 9, meq, m, ge);
                    }
#pragma unroll
                    for (int k = 0; k < TSJ_K; ++k)
                        if (k < kcnt) {
                            const double2 d = sdr[k][q];
                            double dn[3];
                            train_sj_map(W + 12, ge, e, d.x, d.y, !demod, dm[k], dn);
                            if (!demod) train_zm(c, s, dn);
                            double* o = deo + k * estr + (long)(r0 + q) * npair;
                            o[0] = dn[0]; o[NE] = dn[1]; o[2 * NE] = dn[2];
                        }
                }
                if (!demod) train_zm(c, s, e);
                if (eo) {
                    double* o = eo + (long)(r0 + q) * npair;
                    o[0] = e[0]; o[dy] = e[1]; o[dz] = e[2];
                }
            }
            double n[3], gn[3] = {0, 0, 0};
            train_affine(W, W + 9, meq, m, n);
            if (dg) {                                                     // dA u + meq dB
                double dW[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) dW[i] = dg[i * npair];
                train_affine(dW, dW + 9, meq, m, gn);
            }
#pragma unroll
            for (int k = 0; k < TSJ_K; ++k)
                if (k < kcnt) {
                    const double2 d = sdr[k][q];
                    double dn[3];
                    train_sj_map(W, gn, n, d.x, d.y, true, dm[k], dn);
                    train_zm(c, s, dn);
                    dm[k][0] = dn[0]; dm[k][1] = dn[1]; dm[k][2] = dn[2];
                }
            train_zm(c, s, n);
            m[0] = n[0]; m[1] = n[1]; m[2] = n[2];
        }
    }
    if (!live) return;
    if (fx && first) {
        const long o = P.o_off + blk;
        fx[o] = m[0]; fy[o] = m[1]; fz[o] = m[2];
    }
    if (dfx) {
#pragma unroll
        for (int k = 0; k < TSJ_K; ++k)
            if (k < kcnt) {
                const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * npair + pair;
                dfx[o] = dm[k][0]; dfx[NO + o] = dm[k][1]; dfx[2 * NO + o] = dm[k][2];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_jvp_sched_batch (arguments checked by api.cpp): the forward train's staging (bloch_stage,
// train_stage) plus the directions and the two tables; one upload, three launches (two without a gains direction), one download.
// The output region is bloch_train_jvp_batch_run's, then what stays on the device: the primal planes and, with a gains direction,
// their tangents in the gain: 2 W doubles whatever ndir is.
int bloch_train_sched_jvp_group() { return TSJ_K; }

void bloch_train_jvp_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, int ndir, const double* dgain, const double* dphi, const double* dm0x,
                                     const double* dm0y, const double* dm0z, double* ex, double* ey, double* ez, double* fx, double* fy,
                                     double* fz, double* dex, double* dey, double* dez, double* dfx, double* dfy, double* dfz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    Staging& S = B.S;
    const size_t O = (size_t)B.O, E = (size_t)Ts.E, NO = (size_t)ndir * O, NE = (size_t)ndir * E, D = (size_t)ndir * roff[npulse];
    const int ngr = (ndir + TSJ_K - 1) / TSJ_K;
    const size_t o_g = dgain ? S.add(D * 8) : 0, o_p = dphi ? S.add(D * 8) : 0, o_d = dm0x ? S.add(3 * NO * 8) : 0;
    const size_t o_jb = sim_group_table(S, ngr);
    if (dgain) std::copy(dgain, dgain + D, S.at<double>(o_g));
    if (dphi) std::copy(dphi, dphi + D, S.at<double>(o_p));
    if (dm0x) {
        double* d = S.at<double>(o_d);
        std::copy(dm0x, dm0x + NO, d);
        std::copy(dm0y, dm0y + NO, d + NO);
        std::copy(dm0z, dm0z + NO, d + 2 * NO);
    }
    long nwg = 0;                                                         // workgroups of the period's tangent
    const size_t o_qb = dgain ? train_jvp_table(Ts, nscale, 1, nwg) : 0;
    const size_t te = dex ? 3 * NE : 0, tf = dfx ? 3 * NO : 0, pe = ex ? 3 * E : 0, pf = fx ? 3 * O : 0, W = (size_t)Ts.W;
    S.upload((te + tf + pe + pf + W + (dgain ? W : 0)) * 8, st);
    double* out = S.dev<double>(S.o_out);
    double* dte = out;
    double* dtf = dte + te;
    double* dpe = dtf + tf;
    double* dpf = dpe + pe;
    double* ws = dpf + pf;
    double* dws = dgain ? ws + W : nullptr;
    train_launch_prop(Ts, st, ws);
    if (dgain) train_launch_prop_dgain(Ts, st, o_qb, nwg, dws);
    hipLaunchKernelGGL(k_bloch_train_run_sched_jvp, dim3((unsigned)(S.nblk * ngr)), dim3(256), 0, st, ws, dws,
                       S.dev<const double2>(Ts.o_rep), S.dev<const int>(Ts.o_gi), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(o_jb), S.dev<const double>(B.o_m0),
                       dgain ? S.dev<const double>(o_g) : nullptr, dphi ? S.dev<const double>(o_p) : nullptr,
                       dm0x ? S.dev<const double>(o_d) : nullptr, demod, ndir, nscale, (long)NE, (long)NO, ex ? dpe : nullptr,
                       ex ? dpe + E : nullptr, ex ? dpe + 2 * E : nullptr, fx ? dpf : nullptr, fx ? dpf + O : nullptr,
                       fx ? dpf + 2 * O : nullptr, dex ? dte : nullptr, dfx ? dtf : nullptr);
    std::vector<double> h(te + tf + pe + pf);
    S.download(h.data(), h.size() * 8, st);
    auto triple = [](const double* src, size_t n, double* x, double* y, double* z) {
        std::copy(src, src + n, x);
        std::copy(src + n, src + 2 * n, y);
        std::copy(src + 2 * n, src + 3 * n, z);
    };
    if (dex) triple(h.data(), NE, dex, dey, dez);
    if (dfx) triple(h.data() + te, NO, dfx, dfy, dfz);
    if (ex) triple(h.data() + te + tf, E, ex, ey, ez);
    if (fx) triple(h.data() + te + tf + pe, O, fx, fy, fz);
}

}  // namespace mbfir
