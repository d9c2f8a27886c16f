// Least-squares products of the batched Cayley-Klein simulators: for a profile f(a, b) of the simulated (a, b), a real
// weight w >= 0 and a target t per point and scale, L = 1/2 sum w |f - t|^2 over a pulse's points and scales, and with J = df / drf
//   lsq: g = J^H W (f - t) = dL / d Re rf + i dL / d Im rf, and L          (k_abr_lsq_batch, k_abr2_lsq_batch)
//   gn:  H v = J^H W J v for a direction v of the rf samples               (k_abr_gn_batch, k_abr2_gn_batch)
// Both are the adjoint's two sweeps (simgrad.hip) with the cotangent made where it is needed: a forward sweep to psi_n -- for gn
// carrying one tangent dpsi through abr_jvp_step on the trigonometry abr_step_trig<true> kept, one sincos per sample -- then the
// pointwise seed lambda_n = F^H c with c = w (f - t) or c = w F dpsi_n (F = df / dpsi), then the reverse sweep and the reduction
// over the points of k_abr_vjp_batch.  Nothing of point size is read but w and t, and nothing of point size is written.
//   kind      f              F dpsi                           (lambda_a, lambda_b)
//   0  ex     2 conj(a) b    2 (conj(da) b + conj(a) db)      (2 b conj(c), 2 a c)
//   1  se     i b^2          2i b db                          (0, -2i conj(b) c)
//   2  inv    1 - 2 |b|^2    -4 Re(conj(b) db)                (0, -4 b Re c)
//   3  st     i a^2          2i a da                          (-2i conj(a) c, 0)
// One 256-thread workgroup per (pulse, scale, chunk of 256 points, and for gn one direction): the forward kernels' block table,
// repeated per direction with the direction in SimBlock::pad as simjvp.hip repeats it per direction group.  One partial per
// (workgroup, sample) and one loss partial per workgroup, each summed in a fixed order; k_abr_gn_fold folds them with
// k_abr_vjp_fold's sum (abr_vjp_fold_sum).  No atomics: a pulse's g, L and H v bits depend only on the pulse, its grid, its
// weights, target or direction, and the scale list.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// f(a, b) and, for da, db a tangent of (a, b), F dpsi; kinds as in the table above.
__device__ __forceinline__ double2 gn_profile(int kind, double2 a, double2 b) {
    if (kind == 0) { const double2 p = cjmul(a, b); return make_double2(2 * p.x, 2 * p.y); }
    if (kind == 2) return make_double2(1 - 2 * (b.x * b.x + b.y * b.y), 0);
    const double2 z = kind == 1 ? b : a, p = cmul(z, z);
    return make_double2(-p.y, p.x);
}
__device__ __forceinline__ double2 gn_dprofile(int kind, double2 a, double2 b, double2 da, double2 db) {
    if (kind == 0) { const double2 p = cjmul(da, b), q = cjmul(a, db); return make_double2(2 * (p.x + q.x), 2 * (p.y + q.y)); }
    if (kind == 2) return make_double2(-4 * redot(b, db), 0);
    const double2 p = kind == 1 ? cmul(b, db) : cmul(a, da);
    return make_double2(-2 * p.y, 2 * p.x);
}
// lambda_n = F^H c.
__device__ __forceinline__ void gn_seed(int kind, double2 a, double2 b, double2 c, double2& la, double2& lb) {
    la = lb = make_double2(0, 0);
    if (kind == 0) {
        const double2 p = cjmul(c, b), q = cmul(a, c);
        la = make_double2(2 * p.x, 2 * p.y);
        lb = make_double2(2 * q.x, 2 * q.y);
    } else if (kind == 2) {
        lb = make_double2(-4 * c.x * b.x, -4 * c.x * b.y);
    } else {
        const double2 p = cjmul(kind == 1 ? b : a, c), s = make_double2(2 * p.y, -2 * p.x);      // -2i conj(z) c
        if (kind == 1) lb = s; else la = s;
    }
}

// The sweeps of one workgroup (TWO_D: om = fma(x, gx, y gy) as k_abr2_batch forms it, else om = x g as k_abr_batch; TANGENT: gn,
// else lsq).  xv, yv: the thread's point; live false: a thread past the end of the grid, which sweeps a point at the origin with
// weight zero and contributes exact zeros, as a point of weight zero does.  w: the point's weight; tg: its target (lsq); vd: the n
// samples of the direction (gn).  part: this workgroup's n partials; lpart: its loss partial (lsq).  The staging, the reverse loop
// and the reduction tile are those of abr_vjp_sweeps (simgrad.hip), whose own loop stays where it is: hoisting it into a shared
// function changed the register allocation of k_abr_vjp_batch.
template <bool TWO_D, bool TANGENT>
__device__ __forceinline__ void abr_gn_sweeps(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                              const double* __restrict__ gy, const double2* __restrict__ vd, long r_off, int n,
                                              double sc, int mode, int kind, double xv, double yv, bool live, double w, double2 tg,
                                              double2* __restrict__ part, double* __restrict__ lpart) {
    __shared__ double2 srf[256];
    __shared__ double sgx[256], sgy[TWO_D ? 256 : 1];
    __shared__ double2 sv[TANGENT ? 256 : 1];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    const int tid = threadIdx.x;
    auto stage = [&](int m0, bool dir) {
        __syncthreads();
        const int mm = m0 + tid;
        if (mm < n) {
            const long t = r_off + mm;
            srf[tid] = make_double2(rf_il[2 * t] * sc, rf_il[2 * t + 1] * sc);
            sgx[tid] = gx[t];
            if (TWO_D) sgy[tid] = gy[t];
            if (TANGENT && dir) {
                const double2 v = vd[mm];
                sv[tid] = make_double2(v.x * sc, v.y * sc);
            }
        }
        __syncthreads();
    };
    auto angle = [&](int q) { return TWO_D ? fma(xv, sgx[q], yv * sgy[q]) : xv * sgx[q]; };
    double2 a = make_double2(1, 0), b = make_double2(0, 0);
    double2 da[JVP_K], db[JVP_K];
#pragma unroll
    for (int k = 0; k < JVP_K; ++k) da[k] = db[k] = make_double2(0, 0);
    const int mlast = (n - 1) / 256 * 256;
    for (int m0 = 0; m0 < n; m0 += 256) {
        stage(m0, true);
        const int cnt = min(256, n - m0);
        for (int q = 0; q < cnt; ++q) {
            if (TANGENT) {
                const double om = angle(q);
                AbrTrig t;
                const CayleyKlein ck = abr_step_trig<true>(mode, srf[q], om, a, b, t);
                abr_jvp_step(mode, srf[q], om, t, a, b, sv + q, 1, da, db);
                a = ck.a; b = ck.b;
            } else {
                const CayleyKlein ck = abr_step(mode, srf[q], angle(q), a, b);
                a = ck.a; b = ck.b;
            }
        }
    }
    const int row = tid >> 4, l = tid & 15;                       // reduction: 16 lanes per row of the tile
    double2 c;
    if (TANGENT) {
        const double2 d = gn_dprofile(kind, a, b, da[0], db[0]);
        c = make_double2(live ? w * d.x : 0.0, live ? w * d.y : 0.0);
    } else {
        const double2 f = gn_profile(kind, a, b), r = make_double2(f.x - tg.x, f.y - tg.y);
        c = make_double2(live ? w * r.x : 0.0, live ? w * r.y : 0.0);
        red[tid] = live ? 0.5 * w * (r.x * r.x + r.y * r.y) : 0.0;     // the loss: row 0 of the tile, summed as a row is
        __syncthreads();
        double s = 0;                                             // every row of threads sums row 0; thread 0 stores
        for (int k = 0; k < 16; ++k) s += red[l + 16 * k];
        for (int o = 8; o > 0; o >>= 1) s += __shfl_down(s, o, 16);
        if (tid == 0) *lpart = s;
        __syncthreads();
    }
    double2 la, lb;
    gn_seed(kind, a, b, c, la, lb);
    for (int m0 = mlast; m0 >= 0; m0 -= 256) {
        if (m0 != mlast) stage(m0, false);                        // the forward sweep left the last tile staged
        const int cnt = min(256, n - m0);
        for (int g0 = (cnt - 1) / VJP_T * VJP_T; g0 >= 0; g0 -= VJP_T) {
            const int ge = min(g0 + VJP_T, cnt);
            for (int q = ge - 1; q >= g0; --q) {
                const double2 cg = abr_vjp_step(mode, srf[q], angle(q), a, b, la, lb);
                red[(2 * (q - g0)) * VJP_ROW + tid] = live ? cg.x : 0.0;
                red[(2 * (q - g0) + 1) * VJP_ROW + tid] = live ? cg.y : 0.0;
            }
            __syncthreads();
            double s = 0;                                         // row = 2 (sample - g0) + (0: Re, 1: Im); rows past ge are not stored
            for (int k = 0; k < 16; ++k) s += red[row * VJP_ROW + l + 16 * k];
            for (int o = 8; o > 0; o >>= 1) s += __shfl_down(s, o, 16);
            if (l == 0 && row < 2 * (ge - g0)) reinterpret_cast<double*>(part + m0 + g0)[row] = s;
            __syncthreads();
        }
    }
}

// w and tg (interleaved) lie where k_abr_batch / k_abr2_batch write a: S x nx (x ny) per pulse, scale-major.  vp: the partials'
// descriptor of (pulse, direction) at pulse ndir + direction (lsq: ndir = 1); lp: a pulse's first loss partial, its workgroup
// (scale, chunk) at scale nch + chunk.  v (interleaved): direction k of pulse p at ndir r_off + k n, as k_abr_jvp_batch takes it.
__global__ __launch_bounds__(256) void k_abr_lsq_batch(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                       const double* __restrict__ x, const double* __restrict__ scales,
                                                       const AbrPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                       const VjpPulseDev* __restrict__ vp, const long* __restrict__ lp, int mode,
                                                       int kind, const double* __restrict__ w, const double2* __restrict__ tg,
                                                       double2* __restrict__ part, double* __restrict__ lpart) {
    const SimBlock bk = blocks[blockIdx.x];
    const AbrPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const int i = bk.chunk * 256 + threadIdx.x;
    const bool live = i < P.nx;
    const long o = P.o_off + (long)bk.scale * P.nx + (live ? i : 0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;
    abr_gn_sweeps<false, false>(rf_il, g, nullptr, nullptr, P.r_off, P.n, scales[bk.scale], mode, kind, live ? x[P.x_off + i] : 0.0,
                                0.0, live, live ? w[o] : 0.0, live ? tg[o] : make_double2(0, 0), part + V.p_off + wg * V.n,
                                lpart + lp[bk.pulse] + wg);
}

__global__ __launch_bounds__(256) void k_abr2_lsq_batch(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                        const double* __restrict__ gy, const double* __restrict__ x,
                                                        const double* __restrict__ y, const double* __restrict__ scales,
                                                        const Abr2PulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                        const VjpPulseDev* __restrict__ vp, const long* __restrict__ lp, int mode,
                                                        int kind, const double* __restrict__ w, const double2* __restrict__ tg,
                                                        double2* __restrict__ part, double* __restrict__ lpart) {
    const SimBlock bk = blocks[blockIdx.x];
    const Abr2PulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * P.ny;
    const bool live = i < tot;
    const long kx = live ? i / P.ny : 0;
    const long o = P.o_off + (long)bk.scale * tot + (live ? i : 0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;
    abr_gn_sweeps<true, false>(rf_il, gx, gy, nullptr, P.r_off, P.n, scales[bk.scale], mode, kind, live ? x[P.x_off + kx] : 0.0,
                               live ? y[P.y_off + (i - kx * P.ny)] : 0.0, live, live ? w[o] : 0.0,
                               live ? tg[o] : make_double2(0, 0), part + V.p_off + wg * V.n, lpart + lp[bk.pulse] + wg);
}

__global__ __launch_bounds__(256) void k_abr_gn_batch(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                      const double* __restrict__ x, const double* __restrict__ scales,
                                                      const AbrPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                      const VjpPulseDev* __restrict__ vp, int mode, int kind,
                                                      const double* __restrict__ w, const double2* __restrict__ v, int ndir,
                                                      double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    const AbrPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[(long)bk.pulse * ndir + bk.pad];
    const int i = bk.chunk * 256 + threadIdx.x;
    const bool live = i < P.nx;
    const long o = P.o_off + (long)bk.scale * P.nx + (live ? i : 0);
    abr_gn_sweeps<false, true>(rf_il, g, nullptr, v + (long)ndir * P.r_off + (long)bk.pad * P.n, P.r_off, P.n, scales[bk.scale],
                               mode, kind, live ? x[P.x_off + i] : 0.0, 0.0, live, live ? w[o] : 0.0, make_double2(0, 0),
                               part + V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n, nullptr);
}

__global__ __launch_bounds__(256) void k_abr2_gn_batch(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                       const double* __restrict__ gy, const double* __restrict__ x,
                                                       const double* __restrict__ y, const double* __restrict__ scales,
                                                       const Abr2PulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                       const VjpPulseDev* __restrict__ vp, int mode, int kind,
                                                       const double* __restrict__ w, const double2* __restrict__ v, int ndir,
                                                       double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    const Abr2PulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[(long)bk.pulse * ndir + bk.pad];
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * P.ny;
    const bool live = i < tot;
    const long kx = live ? i / P.ny : 0;
    const long o = P.o_off + (long)bk.scale * tot + (live ? i : 0);
    abr_gn_sweeps<true, true>(rf_il, gx, gy, v + (long)ndir * P.r_off + (long)bk.pad * P.n, P.r_off, P.n, scales[bk.scale], mode,
                              kind, live ? x[P.x_off + kx] : 0.0, live ? y[P.y_off + (i - kx * P.ny)] : 0.0, live,
                              live ? w[o] : 0.0, make_double2(0, 0), part + V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n,
                              nullptr);
}

// out[r_off + m] = k_abr_vjp_fold's sum of the partials of one (pulse, direction): one thread per sample, one workgroup per
// (pulse, direction, 256 samples) from its own table (SimBlock: entry of vp, 0, chunk of samples, the pulse).  lsq (loss not
// null): the first thread of a pulse's first workgroup also sums the pulse's nscale nch loss partials in index order.
__global__ __launch_bounds__(256) void k_abr_gn_fold(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                     const SimBlock* __restrict__ blocks, const double* __restrict__ scales,
                                                     int nscale, double2* __restrict__ out, const double* __restrict__ lpart,
                                                     const long* __restrict__ lp, double* __restrict__ loss) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int m = bk.chunk * 256 + threadIdx.x;
    if (m >= V.n) return;
    out[V.r_off + m] = abr_vjp_fold_sum(part, V, scales, nscale, m);
    if (loss && m == 0) {
        const double* q = lpart + lp[bk.pad];
        double s = 0;
        for (long k = 0; k < (long)nscale * V.nch; ++k) s += q[k];
        loss[bk.pad] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// The Levenberg-Marquardt step on the device: conjugate gradients on (H + mu I) d = b per pulse, H p by the sweep of
// k_abr_gn_batch on the device's own p, everything else of an iteration in k_lm_step; then, with a target, the loss and gradient at
// rf + d by k_abr_lsq_batch.  Stages depend on each other through launch order alone.  A pulse whose CG has stopped has run = 0:
// its workgroups of every later launch return at once, so its bits do not depend on how long its neighbours go on.
// LmState, the fixed LDS tree lm_block_sum, the uncontracted lm_redot / lm_axpy and lm_goes_on are in sim_dev.h, shared with the
// Bloch twin of this step (blochgn.hip).

// One workgroup per pulse: p holds b.  d = 0, r = b, rr = gg = <b, b>.  A thread owns the samples tid, tid + 256, ... in every
// pass of this kernel and of k_lm_step, so the dots are summed in an order that n alone fixes and no pass reads another thread's.
__global__ __launch_bounds__(256) void k_lm_init(const VjpPulseDev* __restrict__ vp, const double* __restrict__ mu, int cg,
                                                 double rtol, const double2* __restrict__ p, double2* __restrict__ d,
                                                 double2* __restrict__ r, LmState* __restrict__ st) {
    __shared__ double sw[256];
    const VjpPulseDev V = vp[blockIdx.x];
    double s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const double2 b = p[V.r_off + m];
        d[V.r_off + m] = make_double2(0, 0);
        r[V.r_off + m] = b;
        s += lm_redot(b, b);
    }
    const double gg = lm_block_sum(s, sw);
    if (threadIdx.x == 0) {
        const bool run = lm_goes_on(0, cg, gg, rtol, gg);
        st[blockIdx.x] = LmState{gg, gg, mu[blockIdx.x], 0, run ? 1 : 0, gg > rtol * gg ? 1 : 0, 0};
    }
}

void lm_init_launch(hipStream_t st, int npulse, const VjpPulseDev* vp, const double* mu, int cg, double rtol, const double2* p,
                    double2* d, double2* r, LmState* state) {
    hipLaunchKernelGGL(k_lm_init, dim3((unsigned)npulse), dim3(256), 0, st, vp, mu, cg, rtol, p, d, r, state);
}

// The sweeps of k_abr_gn_batch / k_abr2_gn_batch at ndir = 1 for the pulses that still run; the direction is the device's p.
__global__ __launch_bounds__(256) void k_abr_lm_sweep(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                      const double* __restrict__ x, const double* __restrict__ scales,
                                                      const AbrPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                      const VjpPulseDev* __restrict__ vp, int mode, int kind,
                                                      const double* __restrict__ w, const double2* __restrict__ v,
                                                      const LmState* __restrict__ st, double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    const AbrPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const int i = bk.chunk * 256 + threadIdx.x;
    const bool live = i < P.nx;
    const long o = P.o_off + (long)bk.scale * P.nx + (live ? i : 0);
    abr_gn_sweeps<false, true>(rf_il, g, nullptr, v + P.r_off, P.r_off, P.n, scales[bk.scale], mode, kind,
                               live ? x[P.x_off + i] : 0.0, 0.0, live, live ? w[o] : 0.0, make_double2(0, 0),
                               part + V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n, nullptr);
}

__global__ __launch_bounds__(256) void k_abr2_lm_sweep(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                       const double* __restrict__ gy, const double* __restrict__ x,
                                                       const double* __restrict__ y, const double* __restrict__ scales,
                                                       const Abr2PulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                       const VjpPulseDev* __restrict__ vp, int mode, int kind,
                                                       const double* __restrict__ w, const double2* __restrict__ v,
                                                       const LmState* __restrict__ st, double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;
    const Abr2PulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * P.ny;
    const bool live = i < tot;
    const long kx = live ? i / P.ny : 0;
    const long o = P.o_off + (long)bk.scale * tot + (live ? i : 0);
    abr_gn_sweeps<true, true>(rf_il, gx, gy, v + P.r_off, P.r_off, P.n, scales[bk.scale], mode, kind, live ? x[P.x_off + kx] : 0.0,
                              live ? y[P.y_off + (i - kx * P.ny)] : 0.0, live, live ? w[o] : 0.0, make_double2(0, 0),
                              part + V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n, nullptr);
}

// One CG iteration of one pulse per workgroup, after its sweep: H p by k_abr_gn_fold's sum of the partials, ap = H p + mu p (kept
// in hp), pAp = <p, ap>; a pAp that is not finite or not > 0 stops the pulse with status 2 and nothing else changed; else
// alpha = rr / pAp, d += alpha p, r -= alpha ap, rr' = <r, r>, p = r + (rr' / rr) p, and the next run flag.
__global__ __launch_bounds__(256) void k_lm_step(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                 const double* __restrict__ scales, int nscale, int cg, double rtol,
                                                 double2* __restrict__ p, double2* __restrict__ d, double2* __restrict__ r,
                                                 double2* __restrict__ hp, LmState* __restrict__ st) {
    __shared__ double sw[256];
    const LmState S = st[blockIdx.x];
    if (!S.run) return;
    const VjpPulseDev V = vp[blockIdx.x];
    double s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const double2 h = abr_vjp_fold_sum(part, V, scales, nscale, m), q = p[V.r_off + m], ap = lm_axpy(S.mu, q, h);
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

// trial = rf + d, sample by sample, for every pulse (a pulse that never ran has d = 0).
__global__ __launch_bounds__(256) void k_lm_trial(const double2* __restrict__ rf, const double2* __restrict__ d, long R,
                                                  double2* __restrict__ trial) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < R) trial[t] = make_double2(rf[t].x + d[t].x, rf[t].y + d[t].y);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_abr_lsq_batch / mbfir_abr_gn_batch and their 2D twins (arguments checked by api.cpp): the forward call's staging
// plus the weights, the targets or the directions, the partial descriptors and the two tables; one upload, two launches, one
// download of the ndir R results (and the npulse losses).

namespace {
struct GnSections {
    size_t o_w = 0, o_t = 0, o_v = 0, o_vp = 0, o_lp = 0, o_fb = 0, o_jb = 0;
    long nfold = 0, npart = 0, nlp = 0, nblk = 0;              // fold workgroups; double2 partials; loss partials; sweep workgroups
};
// Adds and fills the sections of S (after the forward sections: pointers into S taken before this are stale).  lsq: t_re not null
// (t_im may be: a real target), ndir = 1; gn: v_re / v_im.
GnSections gn_stage(Staging& S, int npulse, const long* roff, const std::vector<int>& ntime, const std::vector<long>& npoint,
                    int nscale, long O, int ndir, const double* w, const double* t_re, const double* t_im, const double* v_re,
                    const double* v_im) {
    GnSections G;
    const long R = roff[npulse];
    std::vector<VjpPulseDev> vp((size_t)npulse * ndir);
    std::vector<long> lp(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int nch = int((npoint[p] + 255) / 256);
        lp[p] = G.nlp;
        G.nlp += (long)nscale * nch;
        for (int k = 0; k < ndir; ++k) {
            vp[(size_t)p * ndir + k] = VjpPulseDev{ndir * roff[p] + (long)k * ntime[p], G.npart, ntime[p], nch};
            G.npart += (long)nscale * nch * ntime[p];
        }
        G.nfold += (long)ndir * ((ntime[p] + 255) / 256);
    }
    G.nblk = S.nblk * ndir;
    G.o_w = S.add((size_t)O * 8);
    if (t_re) G.o_t = S.add((size_t)O * 16);
    if (v_re) G.o_v = S.add((size_t)ndir * R * 16);
    G.o_vp = S.add(vp.size() * sizeof(VjpPulseDev));
    G.o_lp = S.add(npulse * sizeof(long));
    G.o_fb = S.add(G.nfold * sizeof(SimBlock));
    if (v_re) G.o_jb = S.add(G.nblk * sizeof(SimBlock));
    std::copy(w, w + O, S.at<double>(G.o_w));
    if (t_re) pack_cplx(O, t_re, t_im, S.at<double2>(G.o_t));
    if (v_re) pack_cplx((size_t)ndir * R, v_re, v_im, S.at<double2>(G.o_v));
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(G.o_vp));
    std::copy(lp.begin(), lp.end(), S.at<long>(G.o_lp));
    SimBlock* fb = S.at<SimBlock>(G.o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int k = 0; k < ndir; ++k)
            for (int c = 0; c < (ntime[p] + 255) / 256; ++c) *fb++ = SimBlock{p * ndir + k, 0, c, p};
    if (v_re) {
        const SimBlock* bk = S.at<SimBlock>(S.o_bk);
        SimBlock* jb = S.at<SimBlock>(G.o_jb);
        for (long q = 0; q < S.nblk; ++q)
            for (int k = 0; k < ndir; ++k) *jb++ = SimBlock{bk[q].pulse, bk[q].scale, bk[q].chunk, k};
    }
    return G;
}
// The output region: the ndir R results, the npulse losses (lsq; padded to a whole double2), then the partials and the loss
// partials, which stay on the device.
struct GnOut {
    long T, nl;                                                 // double2 entries of the results and of the losses
    double2 *res, *part;
    double *loss, *lpart;
};
GnOut gn_upload(Staging& S, const GnSections& G, long R, int ndir, int npulse, bool lsq, hipStream_t st) {
    GnOut o;
    o.T = (long)ndir * R;
    o.nl = lsq ? (npulse + 1) / 2 : 0;
    S.upload(((size_t)o.T + o.nl + G.npart) * 16 + (lsq ? (size_t)G.nlp * 8 : 0), st);
    o.res = S.dev<double2>(S.o_out);
    o.loss = reinterpret_cast<double*>(o.res + o.T);
    o.part = o.res + o.T + o.nl;
    o.lpart = reinterpret_cast<double*>(o.part + G.npart);
    return o;
}
// The second launch and the download.
void gn_fold_download(Staging& S, const GnSections& G, const GnOut& o, int nscale, int npulse, bool lsq, hipStream_t st, double* loss,
                      double* h_re, double* h_im) {
    hipLaunchKernelGGL(k_abr_gn_fold, dim3((unsigned)G.nfold), dim3(256), 0, st, o.part, S.dev<const VjpPulseDev>(G.o_vp),
                       S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc), nscale, o.res, lsq ? o.lpart : nullptr,
                       S.dev<const long>(G.o_lp), lsq ? o.loss : nullptr);
    std::vector<double2> h((size_t)o.T + o.nl);
    S.download(h.data(), h.size() * 16, st);
    unpack_cplx(o.T, h.data(), h_re, h_im);
    if (lsq) std::copy(reinterpret_cast<const double*>(h.data() + o.T), reinterpret_cast<const double*>(h.data() + o.T) + npulse, loss);
}
}  // namespace

void abr_lsq_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                       int profile, const double* w, const double* t_re, const double* t_im, double* loss, double* g_re,
                       double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const GnSections G = gn_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, 1, w, t_re, t_im, nullptr, nullptr);
    const GnOut o = gn_upload(S, G, roff[npulse], 1, npulse, true, st);
    hipLaunchKernelGGL(k_abr_lsq_batch, dim3((unsigned)G.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_g), S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc),
                       S.dev<const AbrPulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(G.o_vp),
                       S.dev<const long>(G.o_lp), mode, profile, S.dev<const double>(G.o_w), S.dev<const double2>(G.o_t), o.part,
                       o.lpart);
    gn_fold_download(S, G, o, nscale, npulse, true, st, loss, g_re, g_im);
}

void abr2_lsq_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                        const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                        const long* yoff, const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                        const double* t_re, const double* t_im, double* loss, double* g_re, double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const GnSections G = gn_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, 1, w, t_re, t_im, nullptr, nullptr);
    const GnOut o = gn_upload(S, G, roff[npulse], 1, npulse, true, st);
    hipLaunchKernelGGL(k_abr2_lsq_batch, dim3((unsigned)G.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_gx), S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x),
                       S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const long>(G.o_lp), mode, profile,
                       S.dev<const double>(G.o_w), S.dev<const double2>(G.o_t), o.part, o.lpart);
    gn_fold_download(S, G, o, nscale, npulse, true, st, loss, g_re, g_im);
}

void abr_gn_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                      const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                      int profile, const double* w, int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const GnSections G = gn_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, ndir, w, nullptr, nullptr, v_re, v_im);
    const GnOut o = gn_upload(S, G, roff[npulse], ndir, npulse, false, st);
    hipLaunchKernelGGL(k_abr_gn_batch, dim3((unsigned)G.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_g), S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc),
                       S.dev<const AbrPulseDev>(S.o_pd), S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp), mode,
                       profile, S.dev<const double>(G.o_w), S.dev<const double2>(G.o_v), ndir, o.part);
    gn_fold_download(S, G, o, nscale, npulse, false, st, nullptr, h_re, h_im);
}

void abr2_gn_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                       const long* yoff, const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                       int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const GnSections G = gn_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, ndir, w, nullptr, nullptr, v_re, v_im);
    const GnOut o = gn_upload(S, G, roff[npulse], ndir, npulse, false, st);
    hipLaunchKernelGGL(k_abr2_gn_batch, dim3((unsigned)G.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_gx), S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x),
                       S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd),
                       S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp), mode, profile, S.dev<const double>(G.o_w),
                       S.dev<const double2>(G.o_v), ndir, o.part);
    gn_fold_download(S, G, o, nscale, npulse, false, st, nullptr, h_re, h_im);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_abr_lm_step_batch / mbfir_abr2_lm_step_batch (arguments checked by api.cpp): the forward staging and gn_stage at
// ndir = 1 with b as the direction section, which is the device's p from then on; mu; one upload; k_lm_init, cg rounds of (sweep,
// k_lm_step), and with a target k_lm_trial, the lsq sweep on the trial rf and the fold; one download.  The output region:
//   d (R double2), the npulse states, [the gradient at rf + d (R double2), the npulse losses]      downloaded
//   r, hp, the trial rf (R double2 each), the partials, the loss partials                          stay on the device
namespace {
struct LmArgs {
    int npulse, nscale, cg;
    const long* roff;
    const double *w, *b_re, *b_im, *mu, *t_re, *t_im;
    double rtol;
    double *d_re, *d_im, *rr, *gg, *loss, *g_re, *g_im;
    int *ncg, *status;
};
// sweep(G, p, state, part) and lsq(G, trial rf, part, lpart) launch the 1D or the 2D kernels on the staged sections.
template <class Sweep, class Lsq>
void lm_run(Staging& S, size_t o_rf, const std::vector<int>& ntime, const std::vector<long>& npoint, long O, const LmArgs& a,
            hipStream_t st, Sweep sweep, Lsq lsq) {
    const int npulse = a.npulse;
    const long R = a.roff[npulse];
    const bool trial = a.t_re != nullptr;
    const GnSections G = gn_stage(S, npulse, a.roff, ntime, npoint, a.nscale, O, 1, a.w, a.t_re, a.t_im, a.b_re, a.b_im);
    const size_t o_mu = S.add((size_t)npulse * 8);
    std::copy(a.mu, a.mu + npulse, S.at<double>(o_mu));
    auto pad16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t b_vec = (size_t)R * 16, b_st = pad16(npulse * sizeof(LmState)), b_loss = pad16((size_t)npulse * 8);
    const size_t b_down = b_vec + b_st + (trial ? b_vec + b_loss : 0);
    S.upload(b_down + 3 * b_vec + (size_t)G.npart * 16 + (size_t)G.nlp * 8, st);
    char* out = S.dev<char>(S.o_out);
    double2* d = reinterpret_cast<double2*>(out);
    LmState* state = reinterpret_cast<LmState*>(out + b_vec);
    double2* grad = reinterpret_cast<double2*>(out + b_vec + b_st);
    double* loss = reinterpret_cast<double*>(out + 2 * b_vec + b_st);
    double2* r = reinterpret_cast<double2*>(out + b_down);
    double2 *hp = r + R, *trf = hp + R, *part = trf + R;
    double* lpart = reinterpret_cast<double*>(part + G.npart);
    double2* p = S.dev<double2>(G.o_v);
    const VjpPulseDev* vp = S.dev<const VjpPulseDev>(G.o_vp);
    lm_init_launch(st, npulse, vp, S.dev<const double>(o_mu), a.cg, a.rtol, p, d, r, state);
    for (int k = 0; k < a.cg; ++k) {                              // rounds of a pulse that has stopped are early exits
        sweep(G, p, state, part);
        hipLaunchKernelGGL(k_lm_step, dim3((unsigned)npulse), dim3(256), 0, st, part, vp, S.dev<const double>(S.o_sc), a.nscale, a.cg,
                           a.rtol, p, d, r, hp, state);
    }
    if (trial) {
        hipLaunchKernelGGL(k_lm_trial, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, S.dev<const double2>(o_rf), d, R, trf);
        lsq(G, reinterpret_cast<const double*>(trf), part, lpart);
        hipLaunchKernelGGL(k_abr_gn_fold, dim3((unsigned)G.nfold), dim3(256), 0, st, part, vp, S.dev<const SimBlock>(G.o_fb),
                           S.dev<const double>(S.o_sc), a.nscale, grad, lpart, S.dev<const long>(G.o_lp), loss);
    }
    std::vector<char> h(b_down);
    S.download(h.data(), b_down, st);
    unpack_cplx(R, reinterpret_cast<const double2*>(h.data()), a.d_re, a.d_im);
    const LmState* hs = reinterpret_cast<const LmState*>(h.data() + b_vec);
    for (int q = 0; q < npulse; ++q) {
        a.rr[q] = hs[q].rr; a.gg[q] = hs[q].gg;
        a.ncg[q] = hs[q].ncg; a.status[q] = hs[q].status;
    }
    if (trial) {
        unpack_cplx(R, reinterpret_cast<const double2*>(h.data() + b_vec + b_st), a.g_re, a.g_im);
        std::copy(reinterpret_cast<const double*>(h.data() + 2 * b_vec + b_st),
                  reinterpret_cast<const double*>(h.data() + 2 * b_vec + b_st) + npulse, a.loss);
    }
}
}  // namespace

void abr_lm_step_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                           const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                           int profile, const double* w, const double* b_re, const double* b_im, const double* mu, int cg,
                           double rtol, const double* t_re, const double* t_im, double* d_re, double* d_im, int* ncg, double* rr,
                           double* gg, int* status, double* loss, double* g_re, double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const LmArgs a{npulse, nscale, cg, roff, w, b_re, b_im, mu, t_re, t_im, rtol, d_re, d_im, rr, gg, loss, g_re, g_im, ncg, status};
    lm_run(S, A.o_rf, A.ntime, A.npoint, A.O, a, st,
           [&](const GnSections& G, const double2* p, const LmState* state, double2* part) {
               hipLaunchKernelGGL(k_abr_lm_sweep, dim3((unsigned)G.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                                  S.dev<const double>(A.o_g), S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc),
                                  S.dev<const AbrPulseDev>(S.o_pd), S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp),
                                  mode, profile, S.dev<const double>(G.o_w), p, state, part);
           },
           [&](const GnSections& G, const double* trf, double2* part, double* lpart) {
               hipLaunchKernelGGL(k_abr_lsq_batch, dim3((unsigned)G.nblk), dim3(256), 0, st, trf, S.dev<const double>(A.o_g),
                                  S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc), S.dev<const AbrPulseDev>(S.o_pd),
                                  S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const long>(G.o_lp), mode,
                                  profile, S.dev<const double>(G.o_w), S.dev<const double2>(G.o_t), part, lpart);
           });
}

void abr2_lm_step_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                            const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                            const long* yoff, const double* y, int nscale, const double* scales, int mode, int profile,
                            const double* w, const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                            const double* t_re, const double* t_im, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                            int* status, double* loss, double* g_re, double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const LmArgs a{npulse, nscale, cg, roff, w, b_re, b_im, mu, t_re, t_im, rtol, d_re, d_im, rr, gg, loss, g_re, g_im, ncg, status};
    lm_run(S, A.o_rf, A.ntime, A.npoint, A.O, a, st,
           [&](const GnSections& G, const double2* p, const LmState* state, double2* part) {
               hipLaunchKernelGGL(k_abr2_lm_sweep, dim3((unsigned)G.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                                  S.dev<const double>(A.o_gx), S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x),
                                  S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd),
                                  S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp), mode, profile,
                                  S.dev<const double>(G.o_w), p, state, part);
           },
           [&](const GnSections& G, const double* trf, double2* part, double* lpart) {
               hipLaunchKernelGGL(k_abr2_lsq_batch, dim3((unsigned)G.nblk), dim3(256), 0, st, trf, S.dev<const double>(A.o_gx),
                                  S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x), S.dev<const double>(A.o_y),
                                  S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk),
                                  S.dev<const VjpPulseDev>(G.o_vp), S.dev<const long>(G.o_lp), mode, profile,
                                  S.dev<const double>(G.o_w), S.dev<const double2>(G.o_t), part, lpart);
           });
}

}  // namespace mbfir
