// Tangent of the pulse train: the Jacobian-vector product of bloch_train_batch's echoes and final state with respect to
// the period's b1 samples and to the initial magnetisation.  In blochtrain.hip's notation, along a b1 direction v and an m0
// direction dm_0, per (scale, point):
//   the period:      the four columns of X_t = [A_t | B_t] each obey the sample recursion, so their tangents obey blochjvp.hip's:
//                    dX_t = D_t (R_t dX_{t-1} + dR_t[dn_t] X_{t-1}),  dn_t = (((-(Re v_t amp)) gamma) dt_t, ((Im v_t amp) gamma) dt_t, 0),
//                    amp = scale x gain (the float64 product train_stage uploads), dX_0 = 0; the recovery term has no tangent.
//                    (dA_e, dB_e) is dX after `echo` samples.
//   the repetitions: u_k = Z(+phi_k) m_k, du_k = Z(+phi_k) dm_k, g the gain index of repetition k,
//                    decho_k  = Z(-phi_k) (A_e du_k + dA_e u_k + meq dB_e)      (demod: without the leading Z(-phi_k))
//                    dm_{k+1} = Z(-phi_k) (A du_k + dA u_k + meq dB)
// Two kernels after the shipped k_bloch_train_prop (which leaves the primal planes: the primal echoes keep bloch_train_batch's bits),
// no atomics, no reduction:
//   k_bloch_train_prop_jvp: k_bloch_train_prop_vjp's thread layout (wave w of a workgroup owns column w of X, lane l the point: 64
//                           points per workgroup, the recovery switch uniform over a wavefront), one workgroup per (pulse,
//                           combination, chunk of 64 points, group of TJVP_K directions).  A thread steps its primal column and the
//                           group's tangent columns as k_bloch_jvp_batch does (bloch_jvp_shared once per sample).
//   k_bloch_train_run_jvp:  k_bloch_train_run's layout times the groups of TJVP_RUN_K directions; carries m and the group's dm.
// The tangent planes lie [combination][direction][entry 0..23][point], the pulse's region from ndir x w_off.  Gains and phases have
// no tangent here.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Directions per workgroup of the two kernels: the largest of 1, 2, 4, 8 without scratch at no less than the matching forward
// kernel's occupancy minus one wave per SIMD (k_bloch_train_prop: 4, k_bloch_train_run: 5; DESIGN 8aa has the table).  The
// repetitions' kernel keeps the 24 primal planes in registers, which leaves room for one direction at four waves.  TJVP_K (4) is
// in sim_dev.h with the period's body, which the device Levenberg-Marquardt step (blochtrainlm.hip) shares.
#ifndef TJVP_RUN_K
#define TJVP_RUN_K 1
#endif

// blocks: (pulse, combination, chunk of 64 points), k_bloch_train_prop_vjp's order, every entry once per direction group (pad).
// v (interleaved): direction k of pulse p at ndir t_off + k ntime.  dws receives the tangent planes.
__global__ __launch_bounds__(256) void k_bloch_train_prop_jvp(const double* __restrict__ in, const double* __restrict__ df,
                                                              const double* __restrict__ pos3, const double* __restrict__ amp,
                                                              const BlochPulseDev* __restrict__ pulses,
                                                              const TrainPulseDev* __restrict__ trains,
                                                              const SimBlock* __restrict__ blocks, const double2* __restrict__ v,
                                                              int ndir, double* __restrict__ dws) {
    bloch_train_prop_jvp_body(blocks[blockIdx.x], in, df, pos3, amp, pulses, trains, v, ndir, dws);
}

// blocks: the forward table (pulse, scale, chunk of 256 points) times the direction groups (pad).  ws: the primal planes; dws: the
// tangent planes.  rep, gidx, m0, demod: k_bloch_train_run's.  dm0 (three planes of ndir O entries from dm0, null: zero), dex.. (null:
// not wanted; pulse p from ndir e_off, (direction, scale, repetition, point)) and dfx.. (null: not wanted; pulse p from ndir o_off,
// (direction, scale, point)); NE / NO: the entries of one tangent echo / final plane.  ex.. and fx.. (null: not wanted): the forward
// kernel's outputs, written by the workgroups of direction group 0 with its statements.
__global__ __launch_bounds__(256) void k_bloch_train_run_jvp(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const SimBlock* __restrict__ blocks,
    const double* __restrict__ m0, const double* __restrict__ dm0, int demod, int ndir, int nscale, long NE, long NO,
    double* __restrict__ ex, double* __restrict__ ey, double* __restrict__ ez, double* __restrict__ fx, double* __restrict__ fy,
    double* __restrict__ fz, double* __restrict__ dex, double* __restrict__ dfx) {
    __shared__ double2 scs[256];
    __shared__ int sgi[256];
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain;
    const double meq = Tr.meq;
    const int k0 = bk.pad * TJVP_RUN_K, kcnt = min(TJVP_RUN_K, ndir - k0);
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;
    const long blk = (long)bk.scale * npair + pair;
    const double* wb = ws + Tr.w_off + (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    // direction k0 of the scale's first combination; a combination is ndir directions of TRAIN_ENT npair doubles
    const double* db = dws + (long)ndir * Tr.w_off + ((long)bk.scale * G * ndir + k0) * TRAIN_ENT * npair + (live ? pair : 0);
    const long dstr = (long)TRAIN_ENT * npair;
    const bool first = bk.pad == 0;
    double m[3] = {0, 0, 1}, W[TRAIN_ENT], dm[TJVP_RUN_K][3];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int k = 0; k < TJVP_RUN_K; ++k) {
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
        if (tid < cnt) { scs[tid] = rep[Tr.r_off + r0 + tid]; sgi[tid] = gidx[Tr.r_off + r0 + tid]; }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const double c = scs[q].x, s = scs[q].y;
            if (G != 1) {
                const double* wg = wb + (long)sgi[q] * TRAIN_ENT * npair;
#pragma unroll
                for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wg[e * npair];
            }
            const double* dg = db + (long)sgi[q] * ndir * dstr;
            train_zp(c, s, m);                                            // u = Z(+phi) m
#pragma unroll
            for (int k = 0; k < TJVP_RUN_K; ++k)
                if (k < kcnt) {
                    const double* dk = dg + k * dstr;                     // twelve tangent entries at a time: half the registers
                    double dW[12], dn[3];
                    train_zp(c, s, dm[k]);                                // du = Z(+phi) dm
                    if (deo) {
#pragma unroll
                        for (int e = 0; e < 12; ++e) dW[e] = dk[(12 + e) * npair];
                        train_affine_jvp(W + 12, dW, dW + 9, meq, m, dm[k], dn);
                        if (!demod) train_zm(c, s, dn);
                        double* o = deo + k * estr + (long)(r0 + q) * npair;
                        o[0] = dn[0]; o[NE] = dn[1]; o[2 * NE] = dn[2];
                    }
#pragma unroll
                    for (int e = 0; e < 12; ++e) dW[e] = dk[e * npair];
                    train_affine_jvp(W, dW, dW + 9, meq, m, dm[k], dn);
                    train_zm(c, s, dn);
                    dm[k][0] = dn[0]; dm[k][1] = dn[1]; dm[k][2] = dn[2];
                }
            double e[3], n[3];
            train_affine(W + 12, W + 21, meq, m, e);
            train_affine(W, W + 9, meq, m, n);
            if (!demod) train_zm(c, s, e);
            train_zm(c, s, n);
            m[0] = n[0]; m[1] = n[1]; m[2] = n[2];
            if (eo) {
                double* o = eo + (long)(r0 + q) * npair;
                o[0] = e[0]; o[dy] = e[1]; o[dz] = e[2];
            }
        }
    }
    if (!live) return;
    if (fx && first) {
        const long o = P.o_off + blk;
        fx[o] = m[0]; fy[o] = m[1]; fz[o] = m[2];
    }
    if (dfx) {
#pragma unroll
        for (int k = 0; k < TJVP_RUN_K; ++k)
            if (k < kcnt) {
                const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * npair + pair;
                dfx[o] = dm[k][0]; dfx[NO + o] = dm[k][1]; dfx[2 * NO + o] = dm[k][2];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_jvp_batch (arguments checked by api.cpp): the forward train's staging (bloch_stage, train_stage)
// plus the directions, the m0 directions and the two kernels' tables; one upload, three launches, one download.  The output region
// is the tangent echoes (3 ndir E), the tangent final planes (3 ndir O), the primal echoes (3 E) and final planes (3 O), each only
// when wanted, then what stays on the device: the primal planes and the tangent planes.
int bloch_train_jvp_group(int which) { return which ? TJVP_RUN_K : TJVP_K; }

// The period tangent's table: k_bloch_train_prop_vjp's (the longest periods first, chunks of 64 points), once per direction group
size_t train_jvp_table(TrainStaged& Ts, int nscale, int ndir, long& nwg) {
    BlochStaged& B = Ts.B;
    Staging& S = B.S;
    const int npulse = (int)Ts.tr.size(), ngp = (ndir + TJVP_K - 1) / TJVP_K;
    nwg = 0;
    for (int p = 0; p < npulse; ++p) nwg += (B.npair[p] + 63) / 64 * nscale * Ts.tr[p].ngain * ngp;
    const size_t o_qb = S.add(nwg * sizeof(SimBlock));
    const SimBlock* fb = S.at<SimBlock>(S.o_bk);
    SimBlock* qb = S.at<SimBlock>(o_qb);
    for (long w = 0; w < S.nblk; ++w) {
        if (fb[w].scale != 0 || fb[w].chunk != 0) continue;               // the first workgroup of each pulse, in launch order
        const int p = fb[w].pulse;
        const int ncomb = nscale * Ts.tr[p].ngain, nch = int((B.npair[p] + 63) / 64);
        for (int c = 0; c < ncomb; ++c)
            for (int k = 0; k < nch; ++k)
                for (int g = 0; g < ngp; ++g) *qb++ = SimBlock{p, c, k, g};
    }
    return o_qb;
}

void train_launch_prop_jvp(TrainStaged& Ts, hipStream_t st, size_t o_qb, long nwg, size_t o_v, int ndir, double* dws) {
    Staging& S = Ts.B.S;
    hipLaunchKernelGGL(k_bloch_train_prop_jvp, dim3((unsigned)nwg), dim3(256), 0, st, S.dev<const double>(Ts.B.o_in),
                       S.dev<const double>(Ts.B.o_df), S.dev<const double>(Ts.B.o_pos), S.dev<const double>(Ts.o_amp),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(o_qb),
                       S.dev<const double2>(o_v), ndir, dws);
}

void bloch_train_jvp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                               int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                               const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                               const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                               const double* m0x, const double* m0y, const double* m0z, int ndir, const double* v_re,
                               const double* v_im, const double* dm0x, const double* dm0y, const double* dm0z, double* ex, double* ey,
                               double* ez, double* fx, double* fy, double* fz, double* dex, double* dey, double* dez, double* dfx,
                               double* dfy, double* dfz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    Staging& S = B.S;
    const size_t O = (size_t)B.O, E = (size_t)Ts.E, NO = (size_t)ndir * O, NE = (size_t)ndir * E, V = (size_t)ndir * toff[npulse];
    const int ngr = (ndir + TJVP_RUN_K - 1) / TJVP_RUN_K;
    const size_t o_v = S.add(V * 16), o_d = dm0x ? S.add(3 * NO * 8) : 0, o_jb = sim_group_table(S, ngr);
    pack_cplx(V, v_re, v_im, S.at<double2>(o_v));
    if (dm0x) {
        double* d = S.at<double>(o_d);
        std::copy(dm0x, dm0x + NO, d);
        std::copy(dm0y, dm0y + NO, d + NO);
        std::copy(dm0z, dm0z + NO, d + 2 * NO);
    }
    long nwg = 0;                                                         // workgroups of the period's tangent
    const size_t o_qb = train_jvp_table(Ts, nscale, ndir, nwg);
    const size_t te = dex ? 3 * NE : 0, tf = dfx ? 3 * NO : 0, pe = ex ? 3 * E : 0, pf = fx ? 3 * O : 0, W = (size_t)Ts.W;
    S.upload((te + tf + pe + pf + W + (size_t)ndir * W) * 8, st);
    double* out = S.dev<double>(S.o_out);
    double* dte = out;
    double* dtf = dte + te;
    double* dpe = dtf + tf;
    double* dpf = dpe + pe;
    double* ws = dpf + pf;
    double* dws = ws + W;
    train_launch_prop(Ts, st, ws);
    train_launch_prop_jvp(Ts, st, o_qb, nwg, o_v, ndir, dws);
    hipLaunchKernelGGL(k_bloch_train_run_jvp, dim3((unsigned)(S.nblk * ngr)), dim3(256), 0, st, ws, dws,
                       S.dev<const double2>(Ts.o_rep), S.dev<const int>(Ts.o_gi), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(o_jb), S.dev<const double>(B.o_m0),
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
