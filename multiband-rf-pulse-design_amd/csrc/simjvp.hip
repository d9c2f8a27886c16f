// Tangent of the batched Cayley-Klein simulators: the Jacobian-vector product of k_abr_batch / k_abr2_batch with
// respect to the rf samples, in both models.  Per point and sample the forward step is psi_m = Q_m psi_{m-1} (abr_step, sim_dev.h),
// psi = (a, b), Q_m in SU(2) built from r = s rf_m and the precession angle om.  For a direction v of the rf samples, dr = s v_m:
//     dpsi_m = Q_m dpsi_{m-1} + (dQ_m[dr]) psi_{m-1},   dpsi_0 = 0
// one forward sweep, no reduction over points.  k_abr_jvp_batch / k_abr2_jvp_batch: one 256-thread workgroup per (pulse, scale,
// chunk of 256 points, group of JVP_K directions): the forward kernels' block table times the direction groups; one thread per
// point.  The JVP_K tangents of a thread share the sample's sincos, inv, D and the primal state, which advances through abr_step's
// body (abr_step_trig, which also hands out the sample's trigonometry) by value as in the forward kernels: the (a, b) written here (by the workgroups of group 0) have k_abr_batch / k_abr2_batch's bits.  Every
// direction runs the same instructions on its own registers, so a tangent's bits depend only on its pulse, scale, point and
// direction.  JVP_K and the step of the sweep (abr_jvp_step) live in sim_dev.h, which simgn.hip shares.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// The sweep of one workgroup (TWO_D: om = fma(x, gx, y gy) as k_abr2_batch forms it, else om = x g as k_abr_batch), staged as the
// forward kernels stage theirs: rf times the scale, the weights, and s v of the group's kcnt directions (vg: the first of them, n
// double2 each), 256 samples at a time.  Directions past kcnt are neither read nor computed.
template <bool TWO_D>
__device__ __forceinline__ void abr_jvp_sweep(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                              const double* __restrict__ gy, const double2* __restrict__ vg, long r_off, int n,
                                              double sc, int mode, double xv, double yv, int kcnt, double2& a, double2& b,
                                              double2 (&da)[JVP_K], double2 (&db)[JVP_K]) {
    __shared__ double2 srf[256];
    __shared__ double sgx[256], sgy[TWO_D ? 256 : 1];
    __shared__ double2 sv[JVP_K * 256];
    const int tid = threadIdx.x;
    a = make_double2(1, 0); b = make_double2(0, 0);
#pragma unroll
    for (int k = 0; k < JVP_K; ++k) da[k] = db[k] = make_double2(0, 0);
    for (int m0 = 0; m0 < n; m0 += 256) {
        __syncthreads();
        const int mm = m0 + tid;
        if (mm < n) {
            const long t = r_off + mm;
            srf[tid] = make_double2(rf_il[2 * t] * sc, rf_il[2 * t + 1] * sc);
            sgx[tid] = gx[t];
            if (TWO_D) sgy[tid] = gy[t];
#pragma unroll
            for (int k = 0; k < JVP_K; ++k)
                if (k < kcnt) {
                    const double2 v = vg[(long)k * n + mm];
                    sv[k * 256 + tid] = make_double2(v.x * sc, v.y * sc);
                }
        }
        __syncthreads();
        const int cnt = min(256, n - m0);
        for (int q = 0; q < cnt; ++q) {
            const double om = TWO_D ? fma(xv, sgx[q], yv * sgy[q]) : xv * sgx[q];
            AbrTrig t;
            const CayleyKlein ck = abr_step_trig<true>(mode, srf[q], om, a, b, t);
            abr_jvp_step(mode, srf[q], om, t, a, b, sv + q, kcnt, da, db);
            a = ck.a; b = ck.b;
        }
    }
}

// v (interleaved): direction k of pulse p at ndir r_off + k n.  a / b: the forward kernels' layout, written by the workgroups of
// direction group 0.  da / db: pulse p from ndir o_off, (direction, scale, point) row-major.  blocks: SimBlock with pad = the
// direction group.
__global__ __launch_bounds__(256) void k_abr_jvp_batch(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                       const double* __restrict__ x, const double* __restrict__ scales,
                                                       const AbrPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                       int mode, const double2* __restrict__ v, int ndir, int nscale,
                                                       double2* __restrict__ ao, double2* __restrict__ bo, double2* __restrict__ dao,
                                                       double2* __restrict__ dbo) {
    const SimBlock bk = blocks[blockIdx.x];
    const AbrPulseDev P = pulses[bk.pulse];
    const int k0 = bk.pad * JVP_K, kcnt = min(JVP_K, ndir - k0);
    const int i = bk.chunk * 256 + threadIdx.x;
    double2 a, b, da[JVP_K], db[JVP_K];
    abr_jvp_sweep<false>(rf_il, g, nullptr, v + (long)ndir * P.r_off + (long)k0 * P.n, P.r_off, P.n, scales[bk.scale], mode,
                         i < P.nx ? x[P.x_off + i] : 0.0, 0.0, kcnt, a, b, da, db);
    if (i >= P.nx) return;
    if (bk.pad == 0) {
        const long o = P.o_off + (long)bk.scale * P.nx + i;
        ao[o] = a; bo[o] = b;
    }
#pragma unroll
    for (int k = 0; k < JVP_K; ++k)
        if (k < kcnt) {
            const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * P.nx + i;
            dao[o] = da[k]; dbo[o] = db[k];
        }
}

__global__ __launch_bounds__(256) void k_abr2_jvp_batch(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                        const double* __restrict__ gy, const double* __restrict__ x,
                                                        const double* __restrict__ y, const double* __restrict__ scales,
                                                        const Abr2PulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                        int mode, const double2* __restrict__ v, int ndir, int nscale,
                                                        double2* __restrict__ ao, double2* __restrict__ bo, double2* __restrict__ dao,
                                                        double2* __restrict__ dbo) {
    const SimBlock bk = blocks[blockIdx.x];
    const Abr2PulseDev P = pulses[bk.pulse];
    const int k0 = bk.pad * JVP_K, kcnt = min(JVP_K, ndir - k0);
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * P.ny;
    const bool live = i < tot;
    const long kx = live ? i / P.ny : 0;
    double2 a, b, da[JVP_K], db[JVP_K];
    abr_jvp_sweep<true>(rf_il, gx, gy, v + (long)ndir * P.r_off + (long)k0 * P.n, P.r_off, P.n, scales[bk.scale], mode,
                        x[P.x_off + kx], y[P.y_off + (live ? i - kx * P.ny : 0)], kcnt, a, b, da, db);
    if (!live) return;
    if (bk.pad == 0) {
        const long o = P.o_off + (long)bk.scale * tot + i;
        ao[o] = a; bo[o] = b;
    }
#pragma unroll
    for (int k = 0; k < JVP_K; ++k)
        if (k < kcnt) {
            const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * tot + i;
            dao[o] = da[k]; dbo[o] = db[k];
        }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_abr_jvp_batch / mbfir_abr2_jvp_batch (arguments checked by api.cpp): the forward call's staging plus the
// directions and the block table times the direction groups; one upload, one launch, one download.

int jvp_group() { return JVP_K; }

namespace {
struct JvpSections {
    size_t o_v = 0, o_jb = 0;
    long nblk = 0;                                              // workgroups: the forward table's times the direction groups
};
// Adds and fills the tangent's sections of S (after the forward sections: pointers into S taken before this are stale).
JvpSections jvp_stage(Staging& S, long R, int ndir, const double* v_re, const double* v_im) {
    JvpSections J;
    const int ngrp = (ndir + JVP_K - 1) / JVP_K;
    J.nblk = S.nblk * ngrp;
    J.o_v = S.add((size_t)ndir * R * 16);
    J.o_jb = sim_group_table(S, ngrp);
    pack_cplx((size_t)ndir * R, v_re, v_im, S.at<double2>(J.o_v));
    return J;
}
// The output region: da, db (ndir O entries each), then a, b (O each), which are downloaded only when the caller wants them.
void jvp_download(Staging& S, long O, int ndir, hipStream_t st, double* a_re, double* a_im, double* b_re, double* b_im,
                  double* da_re, double* da_im, double* db_re, double* db_im) {
    const size_t T = (size_t)ndir * O;
    std::vector<double2> h(2 * T + (a_re ? 2 * (size_t)O : 0));
    S.download(h.data(), h.size() * 16, st);
    unpack_cplx(T, h.data(), da_re, da_im);
    unpack_cplx(T, h.data() + T, db_re, db_im);
    if (a_re) {
        unpack_cplx(O, h.data() + 2 * T, a_re, a_im);
        unpack_cplx(O, h.data() + 2 * T + O, b_re, b_im);
    }
}
}  // namespace

void abr_jvp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                       int ndir, const double* v_re, const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im,
                       double* da_re, double* da_im, double* db_re, double* db_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const JvpSections J = jvp_stage(S, roff[npulse], ndir, v_re, v_im);
    const long O = A.O;
    const size_t T = (size_t)ndir * O;
    S.upload((2 * T + 2 * (size_t)O) * 16, st);
    double2* out = S.dev<double2>(S.o_out);
    hipLaunchKernelGGL(k_abr_jvp_batch, dim3((unsigned)J.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_g), S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc),
                       S.dev<const AbrPulseDev>(S.o_pd), S.dev<const SimBlock>(J.o_jb), mode, S.dev<const double2>(J.o_v), ndir,
                       nscale, out + 2 * T, out + 2 * T + O, out, out + T);
    jvp_download(S, O, ndir, st, a_re, a_im, b_re, b_im, da_re, da_im, db_re, db_im);
}

void abr2_jvp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                        const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                        const long* yoff, const double* y, int nscale, const double* scales, int mode, int ndir, const double* v_re,
                        const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im, double* da_re, double* da_im,
                        double* db_re, double* db_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const JvpSections J = jvp_stage(S, roff[npulse], ndir, v_re, v_im);
    const long O = A.O;
    const size_t T = (size_t)ndir * O;
    S.upload((2 * T + 2 * (size_t)O) * 16, st);
    double2* out = S.dev<double2>(S.o_out);
    hipLaunchKernelGGL(k_abr2_jvp_batch, dim3((unsigned)J.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf),
                       S.dev<const double>(A.o_gx), S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x),
                       S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc), S.dev<const Abr2PulseDev>(S.o_pd),
                       S.dev<const SimBlock>(J.o_jb), mode, S.dev<const double2>(J.o_v), ndir, nscale, out + 2 * T,
                       out + 2 * T + O, out, out + T);
    jvp_download(S, O, ndir, st, a_re, a_im, b_re, b_im, da_re, da_im, db_re, db_im);
}

}  // namespace mbfir
