// Least-squares products of the Bloch simulator's steady state: with M_s = (I - A_s)^-1 B_s the steady state of the
// period at transmit gain s (k_bloch_batch's mode 1), weights w = (wx, wy, wz) >= 0 and targets t = (tx, ty, tz) per (scale,
// frequency, position) point, and J_s = dM_s / d(s b1) (real-linear),
//     L = 1/2 sum over the pulse's scales and points of sum_c w_c (M_c - t_c)^2
//   lsq: L and g = sum_s s J_s' W_s (M_s - t_s) = dL / d Re b1 + i dL / d Im b1       (k_bloch_ss_lsq_batch)
//   gn:  H v = sum_s s J_s' W_s J_s (s v) for a direction v of the b1 samples          (k_bloch_ss_gn_batch)
// Both are the steady state's adjoint (blochss.hip k_bloch_ss_vjp_batch) with the cotangent made where it is needed, inv being
// (I - A)^-1 of pass 0 (bloch_ss_pass0, which gives M mode 1's bits):
//   lsq: c = w (M - t) from pass 0's M itself, lambda = inv' c; then the forward sweep from M with its checkpoints and the reverse
//        sweep with the end cotangent lambda.  After lambda neither inv nor w nor t is live.
//   gn:  inv goes to the thread's column of its workgroup's global plane (k_bloch_ss_jvp_batch's sinv); the forward sweep from M
//        carries one tangent d from dm0 = 0 as bloch_gn_sweeps<true> does; inv comes back; dM = inv d, c = w dM, lambda = inv' c; then
//        the same reverse sweep.
// The launch shape, the staging of the rows, the checkpoints, the reverse loop, the reduction through the VJP_T x VJP_ROW tile and
// the fold (k_bloch_gn_fold, unchanged) are those of blochgn.hip, whose own loops stay where they are: the loops are restated here.
// No atomics: a pulse's L, g and H v bits depend only on the pulse, its grids, its weights, its targets or direction and the scale
// list.  Threads past the end of the grid and points of weight zero contribute exact zeros; scale 0 contributes an exact zero to g
// and H v through the fold's factor, and its loss (M = [0 0 1]) is counted.  No guard on det(I - A).
// LDS: the staged rows (16 KB) and the reduction tile (34 KB).  The staged (dnx, dny) row of gn is live only in the forward sweep
// and the tile only after it, so the row lies in the tile's storage.
// The Levenberg-Marquardt step solved on the device with these products (k_bloch_ss_lm_prep, k_bloch_ss_lm_sweep and
// the host side of mbfir_bloch_ss_lm_step_batch) follows the two kernels.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// The thread's point of either kernel: k_bloch_ss_vjp_batch's.  A thread past the end of the grid takes the first point.
struct BlochSsPoint {
    double px, py, pz, dfv;
    long o;                 // its entry in the planes of the weights, the targets and M
    bool live;
};
__device__ __forceinline__ BlochSsPoint bloch_ss_point(const SimBlock& bk, const BlochPulseDev& P, const double* __restrict__ df,
                                                       const double* __restrict__ pos3) {
    BlochSsPoint G;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + threadIdx.x;
    G.live = pair < npair;
    const int fi = G.live ? int(pair / P.npos) : 0, pi = G.live ? int(pair - (long)fi * P.npos) : 0;
    G.dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    G.px = pp[0]; G.py = pp[1]; G.pz = pp[2];
    G.o = P.o_off + (long)bk.scale * npair + (G.live ? pair : 0);
    return G;
}

// The reverse sweep and the reduction of k_bloch_ss_vjp_batch for one workgroup, the pulse's last tile being staged in sst: the
// partials of the end cotangent l into wpart.  Ends with a barrier.
__device__ __forceinline__ void bloch_ss_reverse(double (*sst)[8], double* red, const double* __restrict__ in, long t_off, int ntime,
                                                 double sc, double gamma, double px, double py, double pz, double dfv, bool live,
                                                 double l[3], double2* __restrict__ wpart, const double* wck) {
    const int tid = threadIdx.x, row = tid >> 4, ln = tid & 15;      // reduction: 16 lanes per row of the tile
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    for (int t0 = tlast; t0 >= 0; t0 -= BLOCH_CH) {
        if (t0 != tlast) bloch_ss_stage(sst, in, t_off, ntime, t0, sc, gamma);      // the forward sweep left the last tile staged
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int g0 = (cnt - 1) / VJP_T * VJP_T; g0 >= 0; g0 -= VJP_T) {
            const int ge = min(g0 + VJP_T, cnt);
            double ms[VJP_T][3];                                          // ms[j] = m before sample t0 + g0 + j
            const double* w = wck + (long)((t0 + g0) / VJP_T) * BLOCH_CK;
            ms[0][0] = w[0]; ms[0][1] = w[256]; ms[0][2] = w[512];
#pragma unroll
            for (int j = 1; j < VJP_T; ++j) {
                ms[j][0] = ms[j - 1][0]; ms[j][1] = ms[j - 1][1]; ms[j][2] = ms[j - 1][2];
                if (g0 + j < ge) {
                    const double* s = sst[g0 + j - 1];
                    bloch_fwd_step(s, bloch_rotz(s, px, py, pz, dfv), ms[j]);
                }
            }
#pragma unroll
            for (int j = VJP_T - 1; j >= 0; --j) {
                if (g0 + j < ge) {
                    const double* s = sst[g0 + j];
                    const double2 c = bloch_vjp_step(s, bloch_rotz(s, px, py, pz, dfv), ms[j], l);
                    red[(2 * j) * VJP_ROW + tid] = live ? c.x : 0.0;
                    red[(2 * j + 1) * VJP_ROW + tid] = live ? c.y : 0.0;
                }
            }
            __syncthreads();
            double sum = 0;                                               // row = 2 (sample - g0) + (0: rotx, 1: roty); rows past ge are not stored
            for (int k = 0; k < 16; ++k) sum += red[row * VJP_ROW + ln + 16 * k];
            for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
            if (ln == 0 && row < 2 * (ge - g0)) reinterpret_cast<double*>(wpart + t0 + g0)[row] = sum;
            __syncthreads();
        }
    }
}

// in, df, pos3, scales, pulses, blocks, vp, cks, part, ck, mx / my / mz: k_bloch_ss_vjp_batch's.  w, tg: three planes of O entries
// each (x, y, z), laid out as k_bloch_batch writes mx / my / mz in mode 1.  lp: a pulse's first loss partial, its workgroup (scale,
// chunk) at scale nch + chunk.
__global__ __launch_bounds__(256) void k_bloch_ss_lsq_batch(const double* __restrict__ in, const double* __restrict__ df,
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
        if (live) {
            wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o];
            tv[0] = tg[G.o]; tv[1] = tg[O + G.o]; tv[2] = tg[2 * O + G.o];
        }
        const double r0 = m[0] - tv[0], r1 = m[1] - tv[1], r2 = m[2] - tv[2];      // the residual of mode 1's own M
        const double c0 = live ? wv[0] * r0 : 0.0, c1 = live ? wv[1] * r1 : 0.0, c2 = live ? wv[2] * r2 : 0.0;
        for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c0 + inv[3 * j + 1] * c1 + inv[3 * j + 2] * c2;      // lambda = inv' c
        red[tid] = live ? 0.5 * (wv[0] * (r0 * r0) + wv[1] * (r1 * r1) + wv[2] * (r2 * r2)) : 0.0;      // the loss: row 0 of the tile
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
__global__ __launch_bounds__(256) void k_bloch_ss_gn_batch(const double* __restrict__ in, const double* __restrict__ df,
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
        if (live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o]; }
        double c[3];
        for (int i = 0; i < 3; ++i) {
            const double d = inv[i] * dm[0] + inv[3 + i] * dm[1] + inv[6 + i] * dm[2];      // dM = inv d
            c[i] = live ? wv[i] * d : 0.0;
        }
        for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c[0] + inv[3 * j + 1] * c[1] + inv[3 * j + 2] * c[2];      // lambda = inv' c
    }
    __syncthreads();                                                      // the direction row is read no more: the tile is free
    bloch_ss_reverse(sst, red, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, live, l, part + V.p_off + wg * V.n, wck);
}

// ------------------------------------------------------------------------------------------------
// The Levenberg-Marquardt step of the steady state on the device, the twin of blochgn.hip's: conjugate
// gradients on (H + mu I) d = b per pulse, H p by the sweep of k_bloch_ss_gn_batch on the device's own p, everything else of an
// iteration in k_bloch_lm_step (blochgn.hip, unchanged); then, with targets, the loss and gradient at b1 + d by
// k_bloch_ss_lsq_batch on the trial's input rows.  b1 is fixed within one solve, so pass 0 runs once per call, in
// k_bloch_ss_lm_prep, and every round reads its (I - A)^-1 and M back as the doubles they are.  Stages depend on each other
// through launch order alone.
constexpr int BLOCH_SSLM_PLANE = BLOCH_SSINV + 3 * 256;      // doubles per forward workgroup: (I - A)^-1 as sinv holds it, then M

// Pass 0 of the pulses that run: the forward call's block table.  A thread writes its inv to the columns 0 .. 8 of its
// workgroup's plane, as k_bloch_ss_gn_batch writes sinv, and its M to the columns 9 .. 11; k_bloch_ss_lm_sweep's thread of the same
// workgroup and index reads them back, nobody else.
__global__ __launch_bounds__(256) void k_bloch_ss_lm_prep(const double* __restrict__ in, const double* __restrict__ df,
                                                          const double* __restrict__ pos3, const double* __restrict__ scales,
                                                          const BlochPulseDev* __restrict__ pulses,
                                                          const SimBlock* __restrict__ blocks, const LmState* __restrict__ st,
                                                          double* __restrict__ plane) {
    __shared__ double sst[BLOCH_CH][8];
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    const BlochPulseDev P = pulses[bk.pulse];
    const BlochSsPoint G = bloch_ss_point(bk, P, df, pos3);
    double* wpl = plane + (long)blockIdx.x * BLOCH_SSLM_PLANE + threadIdx.x;
    double inv[9], m[3];
    bloch_ss_pass0(sst, in, P.t_off, P.ntime, scales[bk.scale], P.gamma, G.px, G.py, G.pz, G.dfv, inv, m);
    for (int e = 0; e < 9; ++e) wpl[e * 256] = inv[e];
    for (int e = 0; e < 3; ++e) wpl[(9 + e) * 256] = m[e];
}

// k_bloch_ss_gn_batch at ndir = 1 for the pulses that still run, pass 0 taken from k_bloch_ss_lm_prep's plane: the forward call's
// block table, the direction the device's p (laid out as b1 is).  The forward loop stages every tile itself, as the shipped one
// does; the loop, the cotangent and the reverse sweep are the shipped kernel's statements.
__global__ __launch_bounds__(256) void k_bloch_ss_lm_sweep(const double* __restrict__ in, const double* __restrict__ df,
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
        if (live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o]; }
        double c[3];
        for (int i = 0; i < 3; ++i) {
            const double d = inv[i] * dm[0] + inv[3 + i] * dm[1] + inv[6 + i] * dm[2];      // dM = inv d
            c[i] = live ? wv[i] * d : 0.0;
        }
        for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c[0] + inv[3 * j + 1] * c[1] + inv[3 * j + 2] * c[2];      // lambda = inv' c
    }
    __syncthreads();                                                      // the direction row is read no more: the tile is free
    bloch_ss_reverse(sst, red, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, live, l, part + V.p_off + wg * V.n, wck);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_ss_lsq_batch / mbfir_bloch_ss_gn_batch (arguments checked by api.cpp): the forward call's staging
// (bloch_stage at mode 1, no m0) plus the sections of bloch_gn_stage; one upload, two launches, one download of the ndir T results
// (and the npulse losses, and M when it is wanted).  The output region is the results (ndir T double2), the losses (padded to a
// whole double2), M (lsq: 3 O doubles padded to an even count), then the partials, the loss partials, the checkpoints and (gn) the
// workgroups' planes of (I - A)^-1, which stay on the device.
namespace {
void bloch_ss_gn_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                     const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                     const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                     const double* const w[3], const double* const tg[3], int ndir, const double* v_re, const double* v_im,
                     double* loss, double* o_re, double* o_im, double* mx, double* my, double* mz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool lsq = tg != nullptr, want_m = lsq && mx != nullptr;
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 1, nullptr, nullptr, nullptr);
    Staging& S = B.S;
    const BlochGnSections G = bloch_gn_stage(B, npulse, toff, nscale, w, tg, ndir, v_re, v_im);
    const long O = B.O;
    const long R = (long)ndir * toff[npulse], nl = lsq ? (npulse + 1) / 2 : 0;      // double2 entries of the results and of the losses
    const size_t O3 = lsq ? ((size_t)O * 3 + 1) & ~size_t(1) : 0;                  // an even count: the partials stay 16-byte aligned
    const long nblk = S.nblk * ndir;
    S.upload(((size_t)R + nl + G.npart) * 16 + (O3 + (size_t)(lsq ? G.nlp : 0) + G.nck + (lsq ? 0 : (size_t)nblk * BLOCH_SSINV)) * 8,
             st);
    double2* res = S.dev<double2>(S.o_out);
    double* dloss = reinterpret_cast<double*>(res + R);
    double* pm = reinterpret_cast<double*>(res + R + nl);
    double2* part = reinterpret_cast<double2*>(pm + O3);
    double* lpart = reinterpret_cast<double*>(part + G.npart);
    double* cks = lpart + (lsq ? G.nlp : 0);
    double* sinv = cks + G.nck;
    const double* in = S.dev<const double>(B.o_in);
    if (lsq) {
        hipLaunchKernelGGL(k_bloch_ss_lsq_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, in, S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const BlochCkDev>(G.o_ck),
                           S.dev<const long>(G.o_lp), S.dev<const double>(G.o_w), S.dev<const double>(G.o_t), O, part, cks, lpart,
                           want_m ? pm : nullptr, want_m ? pm + O : nullptr, want_m ? pm + 2 * O : nullptr);
    } else {
        hipLaunchKernelGGL(k_bloch_ss_gn_batch, dim3((unsigned)nblk), dim3(256), 0, st, in, S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const BlochCkDev>(G.o_ck),
                           S.dev<const double>(G.o_w), O, S.dev<const double2>(G.o_v), ndir, part, cks, sinv);
    }
    bloch_gn_fold_launch(st, G.nfold, part, S.dev<const VjpPulseDev>(G.o_vp), S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc),
                         nscale, in, S.dev<const BlochPulseDev>(S.o_pd), res, lsq ? lpart : nullptr, S.dev<const long>(G.o_lp),
                         lsq ? dloss : nullptr);
    std::vector<double> h(((size_t)R + nl) * 2 + (want_m ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(R, reinterpret_cast<const double2*>(h.data()), o_re, o_im);
    if (lsq) std::copy(h.data() + 2 * R, h.data() + 2 * R + npulse, loss);
    if (want_m) {
        const double* hm = h.data() + 2 * (R + nl);
        std::copy(hm, hm + O, mx);
        std::copy(hm + O, hm + 2 * O, my);
        std::copy(hm + 2 * O, hm + 3 * O, mz);
    }
}
}  // namespace

void bloch_ss_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* wx, const double* wy, const double* wz, const double* tx,
                            const double* ty, const double* tz, double* loss, double* g_re, double* g_im, double* mx, double* my,
                            double* mz) {
    const double* const w[3] = {wx, wy, wz};
    const double* const tg[3] = {tx, ty, tz};
    bloch_ss_gn_run(device, stream, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid,
                    poff, dx, dy, dz, nscale, scales, w, tg, 1, nullptr, nullptr, loss, g_re, g_im, mx, my, mz);
}

void bloch_ss_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                           const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                           const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                           int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                           const double* scales, const double* wx, const double* wy, const double* wz, int ndir, const double* v_re,
                           const double* v_im, double* h_re, double* h_im) {
    const double* const w[3] = {wx, wy, wz};
    bloch_ss_gn_run(device, stream, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid,
                    poff, dx, dy, dz, nscale, scales, w, nullptr, ndir, v_re, v_im, nullptr, h_re, h_im, nullptr, nullptr, nullptr);
}

// Host side of mbfir_bloch_ss_lm_step_batch (arguments checked by api.cpp): the forward staging at mode 1 and bloch_gn_stage at
// ndir = 1 with b as the direction section, which is the device's p from then on; mu; one upload; k_lm_init, k_bloch_ss_lm_prep, cg
// rounds of (k_bloch_ss_lm_sweep, k_bloch_lm_step), and with targets k_bloch_lm_trial, k_bloch_ss_lsq_batch on the trial rows (its
// pass 0 is at b1 + d and its own) and the fold; one download.  The output region:
//   d (T double2), the npulse states, [the gradient at b1 + d (T double2), the npulse losses]                      downloaded
//   r, hp (T double2 each), the trial rows (9 T doubles), the partials, the loss partials, the checkpoints, the planes   stay on the device
// The partials and the checkpoints are those of one direction, reused by every round and by the trial's lsq sweep.
void bloch_ss_lm_step_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const double* wx, const double* wy, const double* wz,
                                const double* b_re, const double* b_im, const double* mu, int cg, double rtol, const double* tx,
                                const double* ty, const double* tz, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                                int* status, double* loss, double* g_re, double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool trial = tx != nullptr;
    const double* const w[3] = {wx, wy, wz};
    const double* const tg[3] = {tx, ty, tz};
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 1, nullptr, nullptr, nullptr);
    Staging& S = B.S;
    const BlochGnSections G = bloch_gn_stage(B, npulse, toff, nscale, w, trial ? tg : nullptr, 1, b_re, b_im);
    const size_t o_mu = S.add((size_t)npulse * 8);
    std::copy(mu, mu + npulse, S.at<double>(o_mu));
    const long T = toff[npulse];
    auto pad16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t b_vec = (size_t)T * 16, b_st = pad16(npulse * sizeof(LmState)), b_loss = pad16((size_t)npulse * 8);
    const size_t b_down = b_vec + b_st + (trial ? b_vec + b_loss : 0), b_rows = pad16((size_t)T * BLOCH_IN * 8);
    S.upload(b_down + 2 * b_vec + b_rows + (size_t)G.npart * 16 +
                 ((size_t)G.nlp + G.nck + (size_t)S.nblk * BLOCH_SSLM_PLANE) * 8,
             st);
    char* out = S.dev<char>(S.o_out);
    double2* d = reinterpret_cast<double2*>(out);
    LmState* state = reinterpret_cast<LmState*>(out + b_vec);
    double2* grad = reinterpret_cast<double2*>(out + b_vec + b_st);
    double* dloss = reinterpret_cast<double*>(out + 2 * b_vec + b_st);
    double2* r = reinterpret_cast<double2*>(out + b_down);
    double2* hp = r + T;
    double* rows = reinterpret_cast<double*>(hp + T);
    double2* part = reinterpret_cast<double2*>(reinterpret_cast<char*>(rows) + b_rows);
    double* lpart = reinterpret_cast<double*>(part + G.npart);
    double* cks = lpart + G.nlp;
    double* plane = cks + G.nck;
    double2* p = S.dev<double2>(G.o_v);
    const VjpPulseDev* vp = S.dev<const VjpPulseDev>(G.o_vp);
    const double* in = S.dev<const double>(B.o_in);
    lm_init_launch(st, npulse, vp, S.dev<const double>(o_mu), cg, rtol, p, d, r, state);
    hipLaunchKernelGGL(k_bloch_ss_lm_prep, dim3((unsigned)S.nblk), dim3(256), 0, st, in, S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), state, plane);      // cg = 0: no pulse runs, every workgroup returns at once
    for (int k = 0; k < cg; ++k) {                                // rounds of a pulse that has stopped are early exits
        hipLaunchKernelGGL(k_bloch_ss_lm_sweep, dim3((unsigned)S.nblk), dim3(256), 0, st, in, S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(G.o_jb), vp, S.dev<const BlochCkDev>(G.o_ck), S.dev<const double>(G.o_w), B.O, p,
                           state, part, cks, plane);
        bloch_lm_step_launch(st, npulse, part, vp, S.dev<const double>(S.o_sc), nscale, in, S.dev<const BlochPulseDev>(S.o_pd), cg,
                             rtol, p, d, r, hp, state);
    }
    if (trial) {
        bloch_lm_trial_launch(st, in, d, T, rows);
        hipLaunchKernelGGL(k_bloch_ss_lsq_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, rows, S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(S.o_bk), vp, S.dev<const BlochCkDev>(G.o_ck), S.dev<const long>(G.o_lp),
                           S.dev<const double>(G.o_w), S.dev<const double>(G.o_t), B.O, part, cks, lpart, nullptr, nullptr, nullptr);
        bloch_gn_fold_launch(st, G.nfold, part, vp, S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc), nscale, rows,
                             S.dev<const BlochPulseDev>(S.o_pd), grad, lpart, S.dev<const long>(G.o_lp), dloss);
    }
    std::vector<char> h(b_down);
    S.download(h.data(), b_down, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), d_re, d_im);
    const LmState* hs = reinterpret_cast<const LmState*>(h.data() + b_vec);
    for (int q = 0; q < npulse; ++q) {
        rr[q] = hs[q].rr; gg[q] = hs[q].gg;
        ncg[q] = hs[q].ncg; status[q] = hs[q].status;
    }
    if (trial) {
        unpack_cplx(T, reinterpret_cast<const double2*>(h.data() + b_vec + b_st), g_re, g_im);
        std::copy(reinterpret_cast<const double*>(h.data() + 2 * b_vec + b_st),
                  reinterpret_cast<const double*>(h.data() + 2 * b_vec + b_st) + npulse, loss);
    }
}

}  // namespace mbfir
