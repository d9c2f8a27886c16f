// Adjoint of the batched Cayley-Klein simulators with respect to rf and to the gradient waveform.  The reverse sweep of
// simgrad.hip holds, per point and sample, the state before the sample, both multipliers and the sample's trigonometry; the
// derivative with respect to the precession angle om (abr_vjp_step_g, sim_dev.h) is a few more multiply-adds on them.  With
// om = x g (1D) or x gx + y gy (2D),
//   dL / d g_m = sum_i x_i dom_{m,i};   dL / d gx_m = sum x_k dom,  dL / d gy_m = sum y_j dom
// summed over the scales without a factor: a scale multiplies rf, not g.
// k_abr_vjp_rfg_batch / k_abr2_vjp_rfg_batch: the workgroups, staging and sweeps of k_abr_vjp_batch / k_abr2_vjp_batch; per sample a
// thread hands the reduction the rf pair and x dom (and y dom).  The tile holds VJG_T samples x four rows, summed in the rf
// adjoint's fixed order into one partial per (workgroup, sample, component): the rf pair where k_abr_vjp_batch puts it, the g
// components in a plane of their own with the same index.  k_abr_vjp_rfg_fold sums both over chunks, then over scales, in index
// order (rf times s through abr_vjp_fold_sum, g without).  No atomics: a pulse's gradient bits depend only on the pulse, its grid
// and the scale list.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// As abr_vjp_sweeps (simgrad.hip).  NG = components of g (1, or 2 in 2D); gpart: this workgroup's n x NG partials of g.
template <bool TWO_D>
__device__ __forceinline__ void abr_vjp_rfg_sweeps(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                   const double* __restrict__ gy, long r_off, int n, double sc, int mode, double xv,
                                                   double yv, bool live, double2 la, double2 lb, double2* __restrict__ part,
                                                   double* __restrict__ gpart) {
    constexpr int NG = TWO_D ? 2 : 1;
    __shared__ double2 srf[256];
    __shared__ double sgx[256], sgy[TWO_D ? 256 : 1];
    __shared__ double red[4 * VJG_T * VJP_ROW];
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
    if (!TWO_D) {                                                 // the fourth row of a sample is summed but never stored
        for (int k = 0; k < VJG_T; ++k) red[(4 * k + 3) * VJP_ROW + tid] = 0.0;
    }
    const int row = tid >> 4, l = tid & 15;                       // reduction: 16 lanes per row of the tile
    const int rs = row >> 2, rc = row & 3;                        // row = 4 (sample - g0) + (0: Re, 1: Im, 2: x dom, 3: y dom)
    for (int m0 = mlast; m0 >= 0; m0 -= 256) {
        if (m0 != mlast) stage(m0);                               // the forward sweep left the last tile staged
        const int cnt = min(256, n - m0);
        for (int g0 = (cnt - 1) / VJG_T * VJG_T; g0 >= 0; g0 -= VJG_T) {
            const int ge = min(g0 + VJG_T, cnt);
            for (int q = ge - 1; q >= g0; --q) {
                double dom;
                const double2 c = abr_vjp_step_g(mode, srf[q], angle(q), a, b, la, lb, dom);
                double* r4 = red + (4 * (q - g0)) * VJP_ROW + tid;
                r4[0] = live ? c.x : 0.0;
                r4[VJP_ROW] = live ? c.y : 0.0;
                r4[2 * VJP_ROW] = live ? xv * dom : 0.0;
                if (TWO_D) r4[3 * VJP_ROW] = live ? yv * dom : 0.0;
            }
            __syncthreads();
            double s = 0;                                         // rows of samples past ge hold an earlier tile: not stored
            for (int k = 0; k < 16; ++k) s += red[row * VJP_ROW + l + 16 * k];
            for (int o = 8; o > 0; o >>= 1) s += __shfl_down(s, o, 16);
            if (l == 0 && rs < ge - g0) {
                const int m = m0 + g0 + rs;
                if (rc < 2) reinterpret_cast<double*>(part + m)[rc] = s;
                else if (rc - 2 < NG) gpart[(long)m * NG + (rc - 2)] = s;
            }
            __syncthreads();
        }
    }
}

// Cotangents as k_abr_vjp_batch takes them.  gpart: entry e of part has its g component(s) at gpart[e NG].
__global__ __launch_bounds__(256) void k_abr_vjp_rfg_batch(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                           const double* __restrict__ x, const double* __restrict__ scales,
                                                           const AbrPulseDev* __restrict__ pulses,
                                                           const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                           int mode, const double2* __restrict__ ca,
                                                           const double2* __restrict__ cb, double2* __restrict__ part,
                                                           double* __restrict__ gpart) {
    const SimBlock bk = blocks[blockIdx.x];
    const AbrPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const int i = bk.chunk * 256 + threadIdx.x;
    const bool live = i < P.nx;
    const long o = P.o_off + (long)bk.scale * P.nx + (live ? i : 0);
    const long e = V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n;
    const double2 zero = make_double2(0, 0);
    abr_vjp_rfg_sweeps<false>(rf_il, g, nullptr, P.r_off, P.n, scales[bk.scale], mode, live ? x[P.x_off + i] : 0.0, 0.0, live,
                              live ? ca[o] : zero, live ? cb[o] : zero, part + e, gpart + e);
}

__global__ __launch_bounds__(256) void k_abr2_vjp_rfg_batch(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                            const double* __restrict__ gy, const double* __restrict__ x,
                                                            const double* __restrict__ y, const double* __restrict__ scales,
                                                            const Abr2PulseDev* __restrict__ pulses,
                                                            const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                            int mode, const double2* __restrict__ ca,
                                                            const double2* __restrict__ cb, double2* __restrict__ part,
                                                            double* __restrict__ gpart) {
    const SimBlock bk = blocks[blockIdx.x];
    const Abr2PulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * P.ny;
    const bool live = i < tot;
    const long kx = live ? i / P.ny : 0;
    const long o = P.o_off + (long)bk.scale * tot + (live ? i : 0);
    const long e = V.p_off + ((long)bk.scale * V.nch + bk.chunk) * V.n;
    const double2 zero = make_double2(0, 0);
    abr_vjp_rfg_sweeps<true>(rf_il, gx, gy, P.r_off, P.n, scales[bk.scale], mode, live ? x[P.x_off + kx] : 0.0,
                             live ? y[P.y_off + (i - kx * P.ny)] : 0.0, live, live ? ca[o] : zero, live ? cb[o] : zero, part + e,
                             gpart + 2 * e);
}

// grad[r_off + m] as k_abr_vjp_fold; gg[(r_off + m) NG + c] = sum_s (sum_c' gpart(s, c', m, c)), chunks then scales in index order,
// no factor.  The table of k_abr_vjp_fold with 256 x 2 threads per workgroup: one thread per sample for rf (threadIdx.y = 0: waves
// 0..3) and one for g (waves 4..7), whose serial sums then run side by side; the NG components of g share a loop.
template <int NG>
__global__ __launch_bounds__(512) void k_abr_vjp_rfg_fold(const double2* __restrict__ part, const double* __restrict__ gpart,
                                                          const VjpPulseDev* __restrict__ vp, const SimBlock* __restrict__ blocks,
                                                          const double* __restrict__ scales, int nscale, double2* __restrict__ grad,
                                                          double* __restrict__ gg) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int m = bk.chunk * 256 + threadIdx.x;
    if (m >= V.n) return;
    if (threadIdx.y == 0) {
        grad[V.r_off + m] = abr_vjp_fold_sum(part, V, scales, nscale, m);
        return;
    }
    double g[NG] = {};
    for (int s = 0; s < nscale; ++s) {
        double t[NG] = {};
        const double* row = gpart + (V.p_off + (long)s * V.nch * V.n + m) * NG;
        for (int k = 0; k < V.nch; ++k)
#pragma unroll
            for (int c = 0; c < NG; ++c) t[c] += row[(long)k * V.n * NG + c];
#pragma unroll
        for (int c = 0; c < NG; ++c) g[c] += t[c];
    }
#pragma unroll
    for (int c = 0; c < NG; ++c) gg[(V.r_off + m) * NG + c] = g[c];
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_abr_vjp_rfg_batch / mbfir_abr2_vjp_rfg_batch (arguments checked by api.cpp): the staging of the rf adjoint
// (abr_stage / abr2_stage, vjp_stage); one upload, two launches, one download.  The output region is the rf gradient (R double2),
// the g gradient (R ng doubles, padded to a double2 boundary), then the partials of rf and of g, which stay on the device.

namespace {
struct RfgRegion {
    size_t b_gg, b_part, b_gpart, bytes;                        // byte offsets within the output region, and its size
    size_t down;                                                 // bytes to download: both gradients
};
RfgRegion rfg_region(long R, long npart, int ng) {
    RfgRegion o;
    o.b_gg = (size_t)R * 16;
    o.down = o.b_gg + (size_t)R * ng * 8;
    o.b_part = (o.down + 15) & ~size_t(15);
    o.b_gpart = o.b_part + (size_t)npart * 16;
    o.bytes = o.b_gpart + (size_t)npart * ng * 8;
    return o;
}
// The second launch and the download.  ggy null: 1D.
void rfg_fold_download(Staging& S, const VjpSections& V, const RfgRegion& o, long R, int ng, int nscale, hipStream_t st,
                       double* g_re, double* g_im, double* ggx, double* ggy) {
    char* out = S.dev<char>(S.o_out);
    auto fold = ng == 2 ? k_abr_vjp_rfg_fold<2> : k_abr_vjp_rfg_fold<1>;
    hipLaunchKernelGGL(fold, dim3((unsigned)V.nfold), dim3(256, 2), 0, st, reinterpret_cast<const double2*>(out + o.b_part),
                       reinterpret_cast<const double*>(out + o.b_gpart), S.dev<const VjpPulseDev>(V.o_vp),
                       S.dev<const SimBlock>(V.o_fb), S.dev<const double>(S.o_sc), nscale, reinterpret_cast<double2*>(out),
                       reinterpret_cast<double*>(out + o.b_gg));
    std::vector<double2> h((o.down + 15) / 16);
    S.download(h.data(), o.down, st);
    unpack_cplx(R, h.data(), g_re, g_im);
    if (ng == 2) unpack_cplx(R, h.data() + R, ggx, ggy);
    else std::memcpy(ggx, h.data() + R, (size_t)R * 8);
}
}  // namespace

void abr_vjp_rfg_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                           const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales,
                           int mode, const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im,
                           double* g_re, double* g_im, double* gg) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const VjpSections V = vjp_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, ca_re, ca_im, cb_re, cb_im);
    const long R = roff[npulse];
    const RfgRegion o = rfg_region(R, V.npart, 1);
    S.upload(o.bytes, st);
    char* out = S.dev<char>(S.o_out);
    hipLaunchKernelGGL(k_abr_vjp_rfg_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_g), S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc),
                       S.dev<const AbrPulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(V.o_vp), mode,
                       S.dev<const double2>(V.o_ca), S.dev<const double2>(V.o_cb), reinterpret_cast<double2*>(out + o.b_part),
                       reinterpret_cast<double*>(out + o.b_gpart));
    rfg_fold_download(S, V, o, R, 1, nscale, st, g_re, g_im, gg, nullptr);
}

void abr2_vjp_rfg_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                            const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                            const long* yoff, const double* y, int nscale, const double* scales, int mode, const double* ca_re,
                            const double* ca_im, const double* cb_re, const double* cb_im, double* g_re, double* g_im,
                            double* ggx, double* ggy) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const VjpSections V = vjp_stage(S, npulse, roff, A.ntime, A.npoint, nscale, A.O, ca_re, ca_im, cb_re, cb_im);
    const long R = roff[npulse];
    const RfgRegion o = rfg_region(R, V.npart, 2);
    S.upload(o.bytes, st);
    char* out = S.dev<char>(S.o_out);
    hipLaunchKernelGGL(k_abr2_vjp_rfg_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_gx), S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x),
                       S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(V.o_vp), mode, S.dev<const double2>(V.o_ca),
                       S.dev<const double2>(V.o_cb), reinterpret_cast<double2*>(out + o.b_part),
                       reinterpret_cast<double*>(out + o.b_gpart));
    rfg_fold_download(S, V, o, R, 2, nscale, st, g_re, g_im, ggx, ggy);
}

}  // namespace mbfir
