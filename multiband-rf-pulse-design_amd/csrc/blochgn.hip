// Least-squares products of the Bloch simulator with relaxation: with the end point m_n = (mx, my, mz) of k_bloch_batch
// (mode 0), weights w = (wx, wy, wz) >= 0 and targets t = (tx, ty, tz) per (scale, frequency, position) point,
//     L = 1/2 sum over the pulse's scales and points of sum_c w_c (m_c - t_c)^2,     J = d m_n / d b1 (real-linear)
//   lsq: L and g = J' W (m_n - t) = dL / d Re b1 + i dL / d Im b1                    (k_bloch_lsq_batch)
//   gn:  H v = sum_s s J_s' W_s J_s (s v) for a direction v of the b1 samples        (k_bloch_gn_batch)
// Both are the adjoint's two sweeps (blochgrad.hip) with the cotangent made where it is needed: the forward sweep with its
// checkpoints -- for gn carrying one tangent dm through bloch_rotmat_trig<true> and bloch_jvp_shared as k_bloch_jvp_batch does, one
// sincos per sample; dm needs no checkpoints, the reverse sweep reads only m_{t-1} -- then the pointwise seed lambda_n = w (m_n - t)
// or w dm_n, then the reverse sweep and the reduction over the points of k_bloch_vjp_batch.  The profile is linear in m: there is
// no profile argument.  Nothing of point size is read but w, t and m0, and nothing of point size is written but the checkpoints,
// which stay on the device.
// One 256-thread workgroup per (pulse, scale, chunk of 256 points, and for gn one direction): the forward call's block table,
// repeated per direction with the direction in SimBlock::pad (sim_group_table).  One partial per (workgroup, sample) and one loss
// partial per workgroup, each summed in a fixed order through the VJP_T x VJP_ROW tile; k_bloch_gn_fold folds them with
// abr_vjp_fold_sum (chunks, then scales times s) and applies -(gamma dt_t) to the real part and +(gamma dt_t) to the imaginary
// part.  No atomics: a pulse's g, L and H v bits depend only on the pulse, its grids, its weights, its target or direction, m0 and
// the scale list.  Threads past the end of the grid and points of weight zero contribute exact zeros; scale 0 contributes an exact
// zero through the fold's factor.
// LDS: the staged rows (16 KB) and the reduction tile (34 KB), as k_bloch_vjp_batch.  The staged (dnx, dny) row of gn is live only in
// the forward sweep and the tile only after it, so the row lies in the tile's storage.
// Magnitude twins: k_bloch_lsq_batch_mag, k_bloch_gn_batch_mag and k_bloch_lm_sweep_mag fit (|Mxy|, mz) with pairs of
// weights (w_xy, w_z) and targets (t_xy, t_z).  They are the same sweeps with the other seed (bloch_gn_sweeps<TANGENT, MAG>;
// sim_dev.h bloch_mag_dir, bloch_mag_seed): rho = sqrt(mx mx + my my), u = (mx, my) / rho (0 where rho = 0),
//   lsq: c = (w_xy (rho - t_xy) u, w_z (mz - t_z));   gn: c = (w_xy (u . dm_xy) u, w_z dm_z).
// k_bloch_lsq_batch_mag's forward step is bloch_fwd_step_batch (sim_dev.h): bloch_fwd_step with R v rounded as k_bloch_batch's own
// sweep rounds it, so that the end point, and with it rho, has the forward call's bits.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// The sweeps of one workgroup (TANGENT: gn, else lsq).  (px, py, pz, dfv): the thread's point; live false: a thread past the end of
// the grid, which sweeps the first point from equilibrium with weight zero.  m: the point's m0; w: its weights; tg: its targets
// (lsq); vd: the ntime samples of the direction (gn).  wpart: this workgroup's ntime partials; wck: its checkpoints (at its thread);
// lpart: its loss partial (lsq).  The staging of the rows, the checkpoints, the reverse loop and the reduction are those of
// k_bloch_vjp_batch, whose own loops stay where they are.
template <bool TANGENT, bool MAG = false>
__device__ __forceinline__ void bloch_gn_sweeps(const double* __restrict__ in, const double2* __restrict__ vd, long t_off, int ntime,
                                                double sc, double gamma, double px, double py, double pz, double dfv, bool live,
                                                double m[3], const double w[3], const double tg[3], double2* __restrict__ wpart,
                                                double* wck, double* __restrict__ lpart) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ __align__(16) double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    static_assert(sizeof(double2) * BLOCH_CH <= sizeof(double) * 2 * VJP_T * VJP_ROW, "the direction row fits in the tile");
    double2* sdn = reinterpret_cast<double2*>(red);                   // (dnx, dny) of the staged rows: forward sweep of gn only
    const int tid = threadIdx.x;
    auto stage = [&](int t0, bool dir) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 s, as k_bloch_batch forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
            if (TANGENT && dir) {
                const double2 d = vd[t0 + tid];
                sdn[tid] = make_double2(((-(d.x * sc)) * gamma) * dt, ((d.y * sc) * gamma) * dt);      // as k_bloch_jvp_batch stages it
            }
        }
        __syncthreads();
    };
    double dm[3] = {0, 0, 0};
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        stage(t0, true);
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int q = 0; q < cnt; ++q) {
            if ((q & (VJP_T - 1)) == 0) {                                 // m before sample t0 + q: the group's checkpoint
                double* c = wck + (long)((t0 + q) / VJP_T) * BLOCH_CK;
                c[0] = m[0]; c[256] = m[1]; c[512] = m[2];
            }
            const double* s = sst[q];
            const double rotz = bloch_rotz(s, px, py, pz, dfv);
            if (TANGENT) {
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
            } else if (MAG) {
                bloch_fwd_step_batch(s, rotz, m);                         // the end point with bloch_batch's own bits
            } else {
                bloch_fwd_step(s, rotz, m);
            }
        }
    }
    const int row = tid >> 4, ln = tid & 15;                              // reduction: 16 lanes per row of the tile
    double l[3];
    if (TANGENT && MAG) {                                                 // the tangent branch carries the primal m beside dm
        const BlochMagDir D = bloch_mag_dir(m[0], m[1]);
        bloch_mag_seed(D, w, D.ux * dm[0] + D.uy * dm[1], dm[2], live, l);
        __syncthreads();                                                  // the direction row is read no more: the tile is free
    } else if (TANGENT) {
        l[0] = live ? w[0] * dm[0] : 0.0; l[1] = live ? w[1] * dm[1] : 0.0; l[2] = live ? w[2] * dm[2] : 0.0;
        __syncthreads();                                                  // the direction row is read no more: the tile is free
    } else if (MAG) {
        const BlochMagDir D = bloch_mag_dir(m[0], m[1]);
        const double r0 = D.rho - tg[0], r2 = m[2] - tg[1];
        bloch_mag_seed(D, w, r0, r2, live, l);
        red[tid] = live ? 0.5 * (w[0] * (r0 * r0) + w[1] * (r2 * r2)) : 0.0;      // the loss: row 0 of the tile
        __syncthreads();
        double sum = 0;                                                   // every row of threads sums row 0; thread 0 stores
        for (int k = 0; k < 16; ++k) sum += red[ln + 16 * k];
        for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
        if (tid == 0) *lpart = sum;
        __syncthreads();
    } else {
        const double r0 = m[0] - tg[0], r1 = m[1] - tg[1], r2 = m[2] - tg[2];
        l[0] = live ? w[0] * r0 : 0.0; l[1] = live ? w[1] * r1 : 0.0; l[2] = live ? w[2] * r2 : 0.0;
        red[tid] = live ? 0.5 * (w[0] * (r0 * r0) + w[1] * (r1 * r1) + w[2] * (r2 * r2)) : 0.0;      // the loss: row 0 of the tile
        __syncthreads();
        double sum = 0;                                                   // every row of threads sums row 0; thread 0 stores
        for (int k = 0; k < 16; ++k) sum += red[ln + 16 * k];
        for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
        if (tid == 0) *lpart = sum;
        __syncthreads();
    }
    for (int t0 = tlast; t0 >= 0; t0 -= BLOCH_CH) {
        if (t0 != tlast) stage(t0, false);                                // the forward sweep left the last tile staged
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int g0 = (cnt - 1) / VJP_T * VJP_T; g0 >= 0; g0 -= VJP_T) {
            const int ge = min(g0 + VJP_T, cnt);
            double ms[VJP_T][3];                                          // ms[j] = m before sample t0 + g0 + j
            const double* c = wck + (long)((t0 + g0) / VJP_T) * BLOCH_CK;
            ms[0][0] = c[0]; ms[0][1] = c[256]; ms[0][2] = c[512];
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
                    const double2 cg = bloch_vjp_step(s, bloch_rotz(s, px, py, pz, dfv), ms[j], l);
                    red[(2 * j) * VJP_ROW + tid] = live ? cg.x : 0.0;
                    red[(2 * j + 1) * VJP_ROW + tid] = live ? cg.y : 0.0;
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

// What a thread of either kernel reads of its point.
struct BlochGnPoint {
    double px, py, pz, dfv, m[3];
    long o;                 // its entry in the planes of the weights and the targets
    bool live;
};
__device__ __forceinline__ BlochGnPoint bloch_gn_point(const SimBlock& bk, const BlochPulseDev& P, const double* __restrict__ df,
                                                       const double* __restrict__ pos3, const double* __restrict__ m0) {
    BlochGnPoint G;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + threadIdx.x;
    G.live = pair < npair;
    const int fi = G.live ? int(pair / P.npos) : 0, pi = G.live ? int(pair - (long)fi * P.npos) : 0;
    G.dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    G.px = pp[0]; G.py = pp[1]; G.pz = pp[2];
    const long blk = (long)bk.scale * npair + (G.live ? pair : 0);
    G.o = P.o_off + blk;
    G.m[0] = 0; G.m[1] = 0; G.m[2] = 1;
    if (G.live) {
        const double* mi = m0 + 3 * (P.m_off + blk);
        G.m[0] = mi[0]; G.m[1] = mi[1]; G.m[2] = mi[2];
    }
    return G;
}

// in, df, pos3, scales, pulses, blocks, m0: k_bloch_vjp_batch's.  w, tg: three planes of O entries each (x, y, z), laid out as
// k_bloch_batch writes mx / my / mz in mode 0.  vp, cks: the partials' and the checkpoints' descriptors of (pulse, direction) at
// pulse ndir + direction (lsq: ndir = 1); lp: a pulse's first loss partial, its workgroup (scale, chunk) at scale nch + chunk.
// v (interleaved): direction k of pulse p at ndir t_off + k ntime, as k_bloch_jvp_batch takes it.
// MAG: w and tg are two planes each, (xy, z), and the seed is the magnitude fit's.
template <bool MAG>
__device__ __forceinline__ void bloch_lsq_body(const double* __restrict__ in, const double* __restrict__ df,
                                               const double* __restrict__ pos3, const double* __restrict__ scales,
                                               const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                               const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
                                               const long* __restrict__ lp, const double* __restrict__ m0,
                                               const double* __restrict__ w, const double* __restrict__ tg, long O,
                                               double2* __restrict__ part, double* ck, double* __restrict__ lpart) {
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    BlochGnPoint G = bloch_gn_point(bk, P, df, pos3, m0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;                   // the workgroup among its pulse's
    double wv[3] = {0, 0, 0}, tv[3] = {0, 0, 0};
    if (G.live && MAG) {
        wv[0] = w[G.o]; wv[1] = w[O + G.o];
        tv[0] = tg[G.o]; tv[1] = tg[O + G.o];
    } else if (G.live) {
        wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o];
        tv[0] = tg[G.o]; tv[1] = tg[O + G.o]; tv[2] = tg[2 * O + G.o];
    }
    bloch_gn_sweeps<false, MAG>(in, nullptr, P.t_off, P.ntime, scales[bk.scale], P.gamma, G.px, G.py, G.pz, G.dfv, G.live, G.m, wv,
                                tv, part + V.p_off + wg * V.n, ck + K.c_off + wg * K.ng * BLOCH_CK + threadIdx.x,
                                lpart + lp[bk.pulse] + wg);
}
__global__ __launch_bounds__(256) void k_bloch_lsq_batch(const double* __restrict__ in, const double* __restrict__ df,
    const double* __restrict__ pos3, const double* __restrict__ scales, const BlochPulseDev* __restrict__ pulses,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const long* __restrict__ lp, const double* __restrict__ m0, const double* __restrict__ w, const double* __restrict__ tg, long O,
    double2* __restrict__ part, double* ck, double* __restrict__ lpart) {
    bloch_lsq_body<false>(in, df, pos3, scales, pulses, blocks, vp, cks, lp, m0, w, tg, O, part, ck, lpart);
}
__global__ __launch_bounds__(256) void k_bloch_lsq_batch_mag(const double* __restrict__ in, const double* __restrict__ df,
    const double* __restrict__ pos3, const double* __restrict__ scales, const BlochPulseDev* __restrict__ pulses,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const long* __restrict__ lp, const double* __restrict__ m0, const double* __restrict__ w, const double* __restrict__ tg, long O,
    double2* __restrict__ part, double* ck, double* __restrict__ lpart) {
    bloch_lsq_body<true>(in, df, pos3, scales, pulses, blocks, vp, cks, lp, m0, w, tg, O, part, ck, lpart);
}

template <bool MAG>
__device__ __forceinline__ void bloch_gn_body(const double* __restrict__ in, const double* __restrict__ df,
                                              const double* __restrict__ pos3, const double* __restrict__ scales,
                                              const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                              const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
                                              const double* __restrict__ m0, const double* __restrict__ w, long O,
                                              const double2* __restrict__ v, int ndir, double2* __restrict__ part, double* ck) {
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[(long)bk.pulse * ndir + bk.pad];
    const BlochCkDev K = cks[(long)bk.pulse * ndir + bk.pad];
    BlochGnPoint G = bloch_gn_point(bk, P, df, pos3, m0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;
    double wv[3] = {0, 0, 0};
    const double tv[3] = {0, 0, 0};
    if (G.live && MAG) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; }
    else if (G.live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o]; }
    bloch_gn_sweeps<true, MAG>(in, v + (long)ndir * P.t_off + (long)bk.pad * P.ntime, P.t_off, P.ntime, scales[bk.scale], P.gamma,
                               G.px, G.py, G.pz, G.dfv, G.live, G.m, wv, tv, part + V.p_off + wg * V.n,
                               ck + K.c_off + wg * K.ng * BLOCH_CK + threadIdx.x, nullptr);
}
#define BLOCH_GN_KERNEL(NAME, MAG)                                                                                                  \
    __global__ __launch_bounds__(256) void NAME(                                                                                     \
        const double* __restrict__ in, const double* __restrict__ df, const double* __restrict__ pos3,                               \
        const double* __restrict__ scales, const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,            \
        const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0,                       \
        const double* __restrict__ w, long O, const double2* __restrict__ v, int ndir, double2* __restrict__ part, double* ck) {     \
        bloch_gn_body<MAG>(in, df, pos3, scales, pulses, blocks, vp, cks, m0, w, O, v, ndir, part, ck);                              \
    }
BLOCH_GN_KERNEL(k_bloch_gn_batch, false)
BLOCH_GN_KERNEL(k_bloch_gn_batch_mag, true)
#undef BLOCH_GN_KERNEL

// out[r_off + t] = (-(gamma dt_t) X, +(gamma dt_t) Y), (X, Y) = k_bloch_vjp_fold's sum of the partials of one (pulse, direction):
// one thread per sample, one workgroup per (pulse, direction, 256 samples) from its own table (SimBlock: entry of vp, 0, chunk of
// samples, the pulse).  lsq (loss not null): the first thread of a pulse's first workgroup also sums the pulse's nscale nch loss
// partials in index order.
__global__ __launch_bounds__(256) void k_bloch_gn_fold(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                       const SimBlock* __restrict__ blocks, const double* __restrict__ scales,
                                                       int nscale, const double* __restrict__ in,
                                                       const BlochPulseDev* __restrict__ pulses, double2* __restrict__ out,
                                                       const double* __restrict__ lpart, const long* __restrict__ lp,
                                                       double* __restrict__ loss) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int t = bk.chunk * 256 + threadIdx.x;
    if (t >= V.n) return;
    const BlochPulseDev P = pulses[bk.pad];
    const double2 g = abr_vjp_fold_sum(part, V, scales, nscale, t);
    const double f = P.gamma * in[BLOCH_IN * (P.t_off + t) + 8];
    out[V.r_off + t] = make_double2(-(f * g.x), f * g.y);
    if (loss && t == 0) {
        const double* q = lpart + lp[bk.pad];
        double s = 0;
        for (long k = 0; k < (long)nscale * V.nch; ++k) s += q[k];
        loss[bk.pad] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// The Levenberg-Marquardt step on the device, the Bloch twin of simgn.hip's: conjugate gradients on
// (H + mu I) d = b per pulse, H p by the sweep of k_bloch_gn_batch on the device's own p, everything else of an iteration in
// k_bloch_lm_step; then, with targets, the loss and gradient at b1 + d by k_bloch_lsq_batch on the trial's input rows.  k_lm_init
// (simgn.hip) starts it.  Stages depend on each other through launch order alone; LmState, lm_block_sum, lm_redot, lm_axpy and
// lm_goes_on are sim_dev.h's.

// The sweeps of k_bloch_gn_batch at ndir = 1 for the pulses that still run: the forward call's block table, the direction the
// device's p (laid out as b1 is).
template <bool MAG>
__device__ __forceinline__ void bloch_lm_sweep_body(const double* __restrict__ in, const double* __restrict__ df,
                                                    const double* __restrict__ pos3, const double* __restrict__ scales,
                                                    const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                    const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
                                                    const double* __restrict__ m0, const double* __restrict__ w, long O,
                                                    const double2* __restrict__ v, const LmState* __restrict__ st,
                                                    double2* __restrict__ part, double* ck) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    BlochGnPoint G = bloch_gn_point(bk, P, df, pos3, m0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;
    double wv[3] = {0, 0, 0};
    const double tv[3] = {0, 0, 0};
    if (G.live && MAG) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; }
    else if (G.live) { wv[0] = w[G.o]; wv[1] = w[O + G.o]; wv[2] = w[2 * O + G.o]; }
    bloch_gn_sweeps<true, MAG>(in, v + P.t_off, P.t_off, P.ntime, scales[bk.scale], P.gamma, G.px, G.py, G.pz, G.dfv, G.live, G.m, wv,
                               tv, part + V.p_off + wg * V.n, ck + K.c_off + wg * K.ng * BLOCH_CK + threadIdx.x, nullptr);
}
#define BLOCH_LM_SWEEP_KERNEL(NAME, MAG)                                                                                            \
    __global__ __launch_bounds__(256) void NAME(                                                                                     \
        const double* __restrict__ in, const double* __restrict__ df, const double* __restrict__ pos3,                               \
        const double* __restrict__ scales, const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,            \
        const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0,                       \
        const double* __restrict__ w, long O, const double2* __restrict__ v, const LmState* __restrict__ st,                         \
        double2* __restrict__ part, double* ck) {                                                                                    \
        bloch_lm_sweep_body<MAG>(in, df, pos3, scales, pulses, blocks, vp, cks, m0, w, O, v, st, part, ck);                          \
    }
BLOCH_LM_SWEEP_KERNEL(k_bloch_lm_sweep, false)
BLOCH_LM_SWEEP_KERNEL(k_bloch_lm_sweep_mag, true)
#undef BLOCH_LM_SWEEP_KERNEL

// k_lm_step (simgn.hip) with H p of sample t formed as k_bloch_gn_fold forms it: one CG iteration of one pulse per workgroup, after
// its sweep.  H p = (-(f X), f Y), (X, Y) = abr_vjp_fold_sum of the partials and f = gamma dt_t; ap = H p + mu p (kept in hp),
// pAp = <p, ap>; a pAp that is not finite or not > 0 stops the pulse with status 2 and nothing else changed; else alpha = rr / pAp,
// d += alpha p, r -= alpha ap, rr' = <r, r>, p = r + (rr' / rr) p, and the next run flag.  A thread owns the samples tid, tid + 256,
// ... in every pass, as in k_lm_init.
__global__ __launch_bounds__(256) void k_bloch_lm_step(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                       const double* __restrict__ scales, int nscale,
                                                       const double* __restrict__ in, const BlochPulseDev* __restrict__ pulses,
                                                       int cg, double rtol, double2* __restrict__ p, double2* __restrict__ d,
                                                       double2* __restrict__ r, double2* __restrict__ hp,
                                                       LmState* __restrict__ st) {
    __shared__ double sw[256];
    const LmState S = st[blockIdx.x];
    if (!S.run) return;
    const VjpPulseDev V = vp[blockIdx.x];
    const BlochPulseDev P = pulses[blockIdx.x];
    double s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const double2 g = abr_vjp_fold_sum(part, V, scales, nscale, m);
        const double f = P.gamma * in[BLOCH_IN * (P.t_off + m) + 8];
        const double2 h = make_double2(-(f * g.x), f * g.y), q = p[V.r_off + m], ap = lm_axpy(S.mu, q, h);
        hp[V.r_off + m] = ap;
        s += lm_redot(q, ap);
    }
    const double pap = lm_block_sum(s, sw);                      // every thread has read S before the sum's barriers
    if (!(pap > 0) || !isfinite(pap)) {
        if (threadIdx.x == 0) { st[blockIdx.x].run = 0; st[blockIdx.x].status = 2; }
        return;
    }
    const double alpha = S.rr / pap;
    s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        const double2 q = p[t], rn = lm_axpy(-alpha, hp[t], r[t]);
        d[t] = lm_axpy(alpha, q, d[t]);
        r[t] = rn;
        s += lm_redot(rn, rn);
    }
    const double rr = lm_block_sum(s, sw), beta = rr / S.rr;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        p[t] = lm_axpy(beta, p[t], r[t]);
    }
    if (threadIdx.x == 0) {
        const bool run = lm_goes_on(S.ncg + 1, cg, rr, rtol, S.gg);
        st[blockIdx.x] = LmState{rr, S.gg, S.mu, S.ncg + 1, run ? 1 : 0, rr > rtol * S.gg ? 1 : 0, 0};
    }
}

// The trial's input rows, sample by sample, for every pulse (a pulse that never ran has d = 0): entries 0 and 1 are b1 + d, one
// addition each; entries 2 to 8 are copied.
__global__ __launch_bounds__(256) void k_bloch_lm_trial(const double* __restrict__ in, const double2* __restrict__ d, long T,
                                                        double* __restrict__ trial) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const double* s = in + BLOCH_IN * t;
    double* o = trial + BLOCH_IN * t;
    o[0] = s[0] + d[t].x;
    o[1] = s[1] + d[t].y;
    for (int e = 2; e < BLOCH_IN; ++e) o[e] = s[e];
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_lsq_batch / mbfir_bloch_gn_batch (arguments checked by api.cpp): the forward call's staging (bloch_stage,
// mode 0) plus the weights, the targets or the directions, the descriptors and the two tables; one upload, two launches, one
// download of the ndir T results (and the npulse losses).  The output region is the results (ndir T double2), the losses (padded
// to a whole double2), then the partials, the loss partials and the checkpoints, which stay on the device.
// The sections the least-squares calls add to the forward staging, filled (pointers into B.S taken before this are stale), and the
// sizes of what stays on the device.  tg null: no targets; v_re null: no directions, and the sweep's table is the forward one.
// mag: the magnitude fits' pairs (xy, z) in w[0], w[1] and tg[0], tg[1]: two planes per section.
BlochGnSections bloch_gn_stage(BlochStaged& B, int npulse, const long* toff, int nscale, const double* const w[3],
                               const double* const tg[3], int ndir, const double* v_re, const double* v_im, bool mag) {
    Staging& S = B.S;
    BlochGnSections G;
    const long O = B.O, T = toff[npulse];
    const int nplane = mag ? 2 : 3;
    std::vector<VjpPulseDev> vp((size_t)npulse * ndir);
    std::vector<BlochCkDev> ck((size_t)npulse * ndir);
    std::vector<long> lp(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int n = B.ntime[p], nch = int((B.npair[p] + 255) / 256), ng = (n + VJP_T - 1) / VJP_T;
        lp[p] = G.nlp;
        G.nlp += (long)nscale * nch;
        for (int k = 0; k < ndir; ++k) {
            vp[(size_t)p * ndir + k] = VjpPulseDev{ndir * toff[p] + (long)k * n, G.npart, n, nch};
            ck[(size_t)p * ndir + k] = BlochCkDev{G.nck, ng, 0};
            G.npart += (long)nscale * nch * n;
            G.nck += (long)nscale * nch * ng * BLOCH_CK;
        }
        G.nfold += (long)ndir * ((n + 255) / 256);
    }
    G.o_w = S.add((size_t)O * 8 * nplane);
    if (tg) G.o_t = S.add((size_t)O * 8 * nplane);
    if (v_re) G.o_v = S.add((size_t)ndir * T * 16);
    G.o_vp = S.add(vp.size() * sizeof(VjpPulseDev));
    G.o_ck = S.add(ck.size() * sizeof(BlochCkDev));
    G.o_lp = S.add(npulse * sizeof(long));
    G.o_fb = S.add(G.nfold * sizeof(SimBlock));
    G.o_jb = v_re ? sim_group_table(S, ndir) : S.o_bk;
    for (int c = 0; c < nplane; ++c) {
        std::copy(w[c], w[c] + O, S.at<double>(G.o_w) + c * O);
        if (tg) std::copy(tg[c], tg[c] + O, S.at<double>(G.o_t) + c * O);
    }
    if (v_re) pack_cplx((size_t)ndir * T, v_re, v_im, S.at<double2>(G.o_v));
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(G.o_vp));
    std::copy(ck.begin(), ck.end(), S.at<BlochCkDev>(G.o_ck));
    std::copy(lp.begin(), lp.end(), S.at<long>(G.o_lp));
    SimBlock* fb = S.at<SimBlock>(G.o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int k = 0; k < ndir; ++k)
            for (int c = 0; c < (B.ntime[p] + 255) / 256; ++c) *fb++ = SimBlock{p * ndir + k, 0, c, p};
    return G;
}
// Launches k_bloch_gn_fold on nfold workgroups: the fold of the steady state's products (blochssgn.hip) is this one.
void bloch_gn_fold_launch(hipStream_t st, long nfold, const double2* part, const VjpPulseDev* vp, const SimBlock* blocks,
                          const double* scales, int nscale, const double* in, const BlochPulseDev* pulses, double2* out,
                          const double* lpart, const long* lp, double* loss) {
    hipLaunchKernelGGL(k_bloch_gn_fold, dim3((unsigned)nfold), dim3(256), 0, st, part, vp, blocks, scales, nscale, in, pulses, out, lpart,
                       lp, loss);
}
// Launch k_bloch_lm_step on npulse workgroups and k_bloch_lm_trial on the T samples: the steady state's step (blochssgn.hip) folds
// the same partials and tries the same rows.
void bloch_lm_step_launch(hipStream_t st, int npulse, const double2* part, const VjpPulseDev* vp, const double* scales, int nscale,
                          const double* in, const BlochPulseDev* pulses, int cg, double rtol, double2* p, double2* d, double2* r,
                          double2* hp, LmState* state) {
    hipLaunchKernelGGL(k_bloch_lm_step, dim3((unsigned)npulse), dim3(256), 0, st, part, vp, scales, nscale, in, pulses, cg, rtol, p, d, r,
                       hp, state);
}
void bloch_lm_trial_launch(hipStream_t st, const double* in, const double2* d, long T, double* trial) {
    hipLaunchKernelGGL(k_bloch_lm_trial, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, in, d, T, trial);
}
namespace {
// k_bloch_lsq_batch on the input rows `in` (the staged ones, or a trial's) and the fold into grad and loss.
void bloch_lsq_launch(BlochStaged& B, const BlochGnSections& G, int nscale, const double* in, double2* part, double* cks,
                      double* lpart, double2* grad, double* loss, hipStream_t st, bool mag) {
    Staging& S = B.S;
    hipLaunchKernelGGL(mag ? k_bloch_lsq_batch_mag : k_bloch_lsq_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, in,
                       S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const BlochCkDev>(G.o_ck),
                       S.dev<const long>(G.o_lp), S.dev<const double>(B.o_m0), S.dev<const double>(G.o_w),
                       S.dev<const double>(G.o_t), B.O, part, cks, lpart);
    hipLaunchKernelGGL(k_bloch_gn_fold, dim3((unsigned)G.nfold), dim3(256), 0, st, part, S.dev<const VjpPulseDev>(G.o_vp),
                       S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc), nscale, in, S.dev<const BlochPulseDev>(S.o_pd),
                       grad, lpart, S.dev<const long>(G.o_lp), loss);
}

void bloch_gn_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                  const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                  const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                  const double* dx, const double* dy, const double* dz, int nscale, const double* scales, const double* m0x,
                  const double* m0y, const double* m0z, const double* const w[3], const double* const tg[3], int ndir,
                  const double* v_re, const double* v_im, double* loss, double* o_re, double* o_im, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool lsq = tg != nullptr;
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    Staging& S = B.S;
    const BlochGnSections G = bloch_gn_stage(B, npulse, toff, nscale, w, tg, ndir, v_re, v_im, mag);
    const long O = B.O;
    const long R = (long)ndir * toff[npulse], nl = lsq ? (npulse + 1) / 2 : 0;      // double2 entries of the results and of the losses
    S.upload(((size_t)R + nl + G.npart) * 16 + ((size_t)(lsq ? G.nlp : 0) + G.nck) * 8, st);
    double2* res = S.dev<double2>(S.o_out);
    double* dloss = reinterpret_cast<double*>(res + R);
    double2* part = res + R + nl;
    double* lpart = reinterpret_cast<double*>(part + G.npart);
    double* cks = lpart + (lsq ? G.nlp : 0);
    if (lsq) {
        bloch_lsq_launch(B, G, nscale, S.dev<const double>(B.o_in), part, cks, lpart, res, dloss, st, mag);
    } else {
        hipLaunchKernelGGL(mag ? k_bloch_gn_batch_mag : k_bloch_gn_batch, dim3((unsigned)(S.nblk * ndir)), dim3(256), 0, st,
                           S.dev<const double>(B.o_in),
                           S.dev<const double>(B.o_df), S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc),
                           S.dev<const BlochPulseDev>(S.o_pd), S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp),
                           S.dev<const BlochCkDev>(G.o_ck), S.dev<const double>(B.o_m0), S.dev<const double>(G.o_w), O,
                           S.dev<const double2>(G.o_v), ndir, part, cks);
        hipLaunchKernelGGL(k_bloch_gn_fold, dim3((unsigned)G.nfold), dim3(256), 0, st, part, S.dev<const VjpPulseDev>(G.o_vp),
                           S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc), nscale, S.dev<const double>(B.o_in),
                           S.dev<const BlochPulseDev>(S.o_pd), res, nullptr, S.dev<const long>(G.o_lp), nullptr);
    }
    std::vector<double2> h((size_t)R + nl);
    S.download(h.data(), h.size() * 16, st);
    unpack_cplx(R, h.data(), o_re, o_im);
    if (lsq) std::copy(reinterpret_cast<const double*>(h.data() + R), reinterpret_cast<const double*>(h.data() + R) + npulse, loss);
}
}  // namespace

void bloch_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                         const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                         const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                         int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                         const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* wx,
                         const double* wy, const double* wz, const double* tx, const double* ty, const double* tz, double* loss,
                         double* g_re, double* g_im, bool mag) {
    const double* const w[3] = {wx, wy, wz};
    const double* const tg[3] = {tx, ty, tz};
    bloch_gn_run(device, stream, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff,
                 dx, dy, dz, nscale, scales, m0x, m0y, m0z, w, tg, 1, nullptr, nullptr, loss, g_re, g_im, mag);
}

void bloch_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                        const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                        const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                        int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                        const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* wx,
                        const double* wy, const double* wz, int ndir, const double* v_re, const double* v_im, double* h_re,
                        double* h_im, bool mag) {
    const double* const w[3] = {wx, wy, wz};
    bloch_gn_run(device, stream, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff,
                 dx, dy, dz, nscale, scales, m0x, m0y, m0z, w, nullptr, ndir, v_re, v_im, nullptr, h_re, h_im, mag);
}

// Host side of mbfir_bloch_lm_step_batch (arguments checked by api.cpp): the forward staging and bloch_gn_stage at ndir = 1 with b as
// the direction section, which is the device's p from then on; mu; one upload; k_lm_init, cg rounds of (k_bloch_lm_sweep,
// k_bloch_lm_step), and with targets k_bloch_lm_trial, the lsq sweep on the trial rows and the fold; one download.  The output region:
//   d (T double2), the npulse states, [the gradient at b1 + d (T double2), the npulse losses]            downloaded
//   r, hp (T double2 each), the trial rows (9 T doubles), the partials, the loss partials, the checkpoints   stay on the device
// The partials and the checkpoints are those of one direction, reused by every round and by the trial's lsq sweep.
void bloch_lm_step_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* wx,
                             const double* wy, const double* wz, const double* b_re, const double* b_im, const double* mu, int cg,
                             double rtol, const double* tx, const double* ty, const double* tz, double* d_re, double* d_im, int* ncg,
                             double* rr, double* gg, int* status, double* loss, double* g_re, double* g_im, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool trial = tx != nullptr;
    const double* const w[3] = {wx, wy, wz};
    const double* const tg[3] = {tx, ty, tz};
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    Staging& S = B.S;
    const BlochGnSections G = bloch_gn_stage(B, npulse, toff, nscale, w, trial ? tg : nullptr, 1, b_re, b_im, mag);
    const size_t o_mu = S.add((size_t)npulse * 8);
    std::copy(mu, mu + npulse, S.at<double>(o_mu));
    const long T = toff[npulse];
    auto pad16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t b_vec = (size_t)T * 16, b_st = pad16(npulse * sizeof(LmState)), b_loss = pad16((size_t)npulse * 8);
    const size_t b_down = b_vec + b_st + (trial ? b_vec + b_loss : 0), b_rows = pad16((size_t)T * BLOCH_IN * 8);
    S.upload(b_down + 2 * b_vec + b_rows + (size_t)G.npart * 16 + ((size_t)G.nlp + G.nck) * 8, st);
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
    double2* p = S.dev<double2>(G.o_v);
    const VjpPulseDev* vp = S.dev<const VjpPulseDev>(G.o_vp);
    const double* in = S.dev<const double>(B.o_in);
    lm_init_launch(st, npulse, vp, S.dev<const double>(o_mu), cg, rtol, p, d, r, state);
    for (int k = 0; k < cg; ++k) {                                // rounds of a pulse that has stopped are early exits
        hipLaunchKernelGGL(mag ? k_bloch_lm_sweep_mag : k_bloch_lm_sweep, dim3((unsigned)S.nblk), dim3(256), 0, st, in,
                           S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(G.o_jb), vp, S.dev<const BlochCkDev>(G.o_ck), S.dev<const double>(B.o_m0),
                           S.dev<const double>(G.o_w), B.O, p, state, part, cks);
        hipLaunchKernelGGL(k_bloch_lm_step, dim3((unsigned)npulse), dim3(256), 0, st, part, vp, S.dev<const double>(S.o_sc), nscale, in,
                           S.dev<const BlochPulseDev>(S.o_pd), cg, rtol, p, d, r, hp, state);
    }
    if (trial) {
        hipLaunchKernelGGL(k_bloch_lm_trial, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, in, d, T, rows);
        bloch_lsq_launch(B, G, nscale, rows, part, cks, lpart, grad, dloss, st, mag);
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
