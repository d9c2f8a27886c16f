// Adjoint of the batched Cayley-Klein simulators: the vector-Jacobian product of k_abr_batch / k_abr2_batch with
// respect to the rf samples, in both models.  Per point and sample the forward step is psi_m = Q_m psi_{m-1} (abr_step, sim_dev.h),
// psi = (a, b), Q_m in SU(2) built from r = s rf_m and the precession angle om.  With the cotangents (abar, bbar) of the outputs,
// dL = Re(conj(abar) da + conj(bbar) db):
//   forward sweep to psi_n, staged as the forward kernels stage it; then over the samples in reverse
//     psi_{m-1} = Q_m^H psi_m                                       (the rotations are unitary: no stored trajectory)
//     gbar_m   += Re <lambda_m, (dQ_m / dp) psi_{m-1}>,  p = Re r, Im r
//     lambda_{m-1} = Q_m^H lambda_m,  lambda_n = (abar, bbar)
// k_abr_vjp_batch / k_abr2_vjp_batch: one 256-thread workgroup per (pulse, scale, chunk of 256 points) from the forward kernels'
// block table, one thread per point.  The 256 contributions to a sample are summed in a fixed order (VJP_T samples at a time
// through an LDS tile) into one partial per (workgroup, sample); k_abr_vjp_fold sums a pulse's partials over chunks, then over
// scales (times s: the chain rule of r = s rf), in index order.  No atomics: a pulse's gradient bits depend only on the pulse, its
// grid and the scale list.  The step of the reverse sweep (abr_vjp_step), the tile's constants, the partials' descriptor and the
// fold's sum live in sim_dev.h, which simgn.hip shares.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// The sweeps of one workgroup (TWO_D: om = fma(x, gx, y gy) as k_abr2_batch forms it, else om = x g as k_abr_batch).  xv, yv:
// the thread's point; live false: a thread past the end of the grid, which sweeps a point at the origin with zero cotangents and
// contributes exact zeros.  part: this workgroup's n partials.
template <bool TWO_D>
__device__ __forceinline__ void abr_vjp_sweeps(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                               const double* __restrict__ gy, long r_off, int n, double sc, int mode, double xv,
                                               double yv, bool live, double2 la, double2 lb, double2* __restrict__ part) {
    __shared__ double2 srf[256];
    __shared__ double sgx[256], sgy[TWO_D ? 256 : 1];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    const int tid = threadIdx.x;
    auto stage = [&](int m0) {
        __syncthreads();
        const int mm = m0 + tid;
        if (mm < n) {
            const long t = r_off + mm;
            srf[tid] = make_double2(rf_il[2 * t] * sc, rf_il[2 * t + 1] * sc);
            sgx[tid] = gx[t];
            if (TWO_D) sgy[tid] = gy[t];
        }
        __syncthreads();
    };
    auto angle = [&](int q) { return TWO_D ? fma(xv, sgx[q], yv * sgy[q]) : xv * sgx[q]; };
    double2 a = make_double2(1, 0), b = make_double2(0, 0);
    const int mlast = (n - 1) / 256 * 256;
    for (int m0 = 0; m0 < n; m0 += 256) {
        stage(m0);
        const int cnt = min(256, n - m0);
        for (int q = 0; q < cnt; ++q) {
            const CayleyKlein ck = abr_step(mode, srf[q], angle(q), a, b);
            a = ck.a; b = ck.b;
        }
    }
    const int row = tid >> 4, l = tid & 15;                       // reduction: 16 lanes per row of the tile
    for (int m0 = mlast; m0 >= 0; m0 -= 256) {
        if (m0 != mlast) stage(m0);                               // the forward sweep left the last tile staged
        const int cnt = min(256, n - m0);
        for (int g0 = (cnt - 1) / VJP_T * VJP_T; g0 >= 0; g0 -= VJP_T) {
            const int ge = min(g0 + VJP_T, cnt);
            for (int q = ge - 1; q >= g0; --q) {
                const double2 c = abr_vjp_step(mode, srf[q], angle(q), a, b, la, lb);
                red[(2 * (q - g0)) * VJP_ROW + tid] = live ? c.x : 0.0;
                red[(2 * (q - g0) + 1) * VJP_ROW + tid] = live ? c.y : 0.0;
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

// Cotangents ca / cb (interleaved) lie where k_abr_batch / k_abr2_batch write a / b: S x nx (x ny) per pulse, scale-major.
__global__ __launch_bounds__(256) void k_abr_vjp_batch(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                       const double* __restrict__ x, const double* __restrict__ scales,
                                                       const AbrPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                       const VjpPulseDev* __restrict__ vp, int mode, const double2* __restrict__ ca,
                                                       const double2* __restrict__ cb, double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    const AbrPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const int i = bk.chunk * 256 + threadIdx.x;
    const bool live = i < P.nx;
    const long o = P.o_off + (long)bk.scale * P.nx + (live ? i : 0);
    const double2 zero = make_double2(0, 0);
    abr_vjp_sweeps<false>(rf_il, g, nullptr, P.r_off, P.n, scales[bk.scale], mode, live ? x[P.x_off + i] : 0.0, 0.0, live,
                          live ? ca[o] : zero, live ? cb[o] : zero, part + V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n);
}

__global__ __launch_bounds__(256) void k_abr2_vjp_batch(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                        const double* __restrict__ gy, const double* __restrict__ x,
                                                        const double* __restrict__ y, const double* __restrict__ scales,
                                                        const Abr2PulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                        const VjpPulseDev* __restrict__ vp, int mode, const double2* __restrict__ ca,
                                                        const double2* __restrict__ cb, double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    const Abr2PulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * P.ny;
    const bool live = i < tot;
    const long kx = live ? i / P.ny : 0;
    const long o = P.o_off + (long)bk.scale * tot + (live ? i : 0);
    const double2 zero = make_double2(0, 0);
    abr_vjp_sweeps<true>(rf_il, gx, gy, P.r_off, P.n, scales[bk.scale], mode, live ? x[P.x_off + kx] : 0.0,
                         live ? y[P.y_off + (i - kx * P.ny)] : 0.0, live, live ? ca[o] : zero, live ? cb[o] : zero,
                         part + V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n);
}

// grad[r_off + m] = sum_s scales[s] (sum_c part(s, c, m)), chunks then scales in index order; one thread per sample, one
// workgroup per (pulse, 256 samples) from its own table (SimBlock: pulse, 0, chunk of samples).
__global__ __launch_bounds__(256) void k_abr_vjp_fold(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                      const SimBlock* __restrict__ blocks, const double* __restrict__ scales,
                                                      int nscale, double2* __restrict__ grad) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int m = bk.chunk * 256 + threadIdx.x;
    if (m >= V.n) return;
    grad[V.r_off + m] = abr_vjp_fold_sum(part, V, scales, nscale, m);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_abr_vjp_batch / mbfir_abr2_vjp_batch (arguments checked by api.cpp): the forward call's staging plus the
// cotangents, the partial descriptors and the fold kernel's table (vjp_stage, sim_dev.h); one upload, two launches, one download.

namespace {
// The second launch and the download: the output region is the gradient (R entries), then the partials.
void vjp_fold_download(Staging& S, const VjpSections& V, long R, int nscale, hipStream_t st, double* g_re, double* g_im) {
    double2* grad = S.dev<double2>(S.o_out);
    hipLaunchKernelGGL(k_abr_vjp_fold, dim3((unsigned)V.nfold), dim3(256), 0, st, grad + R, S.dev<const VjpPulseDev>(V.o_vp),
                       S.dev<const SimBlock>(V.o_fb), S.dev<const double>(S.o_sc), nscale, grad);
    std::vector<double2> h(R);
    S.download(h.data(), h.size() * 16, st);
    unpack_cplx(R, h.data(), g_re, g_im);
}
}  // namespace

void abr_vjp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                       const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im, double* g_re,
                       double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const VjpSections V = vjp_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, ca_re, ca_im, cb_re, cb_im);
    const long R = roff[npulse];
    S.upload((size_t)(R + V.npart) * 16, st);
    hipLaunchKernelGGL(k_abr_vjp_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_g), S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc),
                       S.dev<const AbrPulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(V.o_vp), mode,
                       S.dev<const double2>(V.o_ca), S.dev<const double2>(V.o_cb), S.dev<double2>(S.o_out) + R);
    vjp_fold_download(S, V, R, nscale, st, g_re, g_im);
}

void abr2_vjp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                        const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                        const long* yoff, const double* y, int nscale, const double* scales, int mode, const double* ca_re,
                        const double* ca_im, const double* cb_re, const double* cb_im, double* g_re, double* g_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const VjpSections V = vjp_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, ca_re, ca_im, cb_re, cb_im);
    const long R = roff[npulse];
    S.upload((size_t)(R + V.npart) * 16, st);
    hipLaunchKernelGGL(k_abr2_vjp_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_gx), S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x),
                       S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(V.o_vp), mode, S.dev<const double2>(V.o_ca),
                       S.dev<const double2>(V.o_cb), S.dev<double2>(S.o_out) + R);
    vjp_fold_download(S, V, R, nscale, st, g_re, g_im);
}

}  // namespace mbfir
