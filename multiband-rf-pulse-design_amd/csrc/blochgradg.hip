// Adjoint of the Bloch simulator with relaxation with respect to b1, the gradient waveform and the off-resonance.  The
// reverse sweep of blochgrad.hip holds, per point and sample, the state before the sample, the multiplier and the sample's
// trigonometry; the derivative with respect to the axis component rotz (bloch_vjp_step_z, sim_dev.h) is a few more multiply-adds on
// them.  With rotz_t = -((gx_t gamma dt_t) x + (gy_t gamma dt_t) y + (gz_t gamma dt_t) z + df (TWOPI dt_t)) and dz_t(s, f, p) that
// derivative per scale, frequency, position and sample,
//     dL / d g_{t,a}   = -(gamma dt_t) sum_s sum_{f,p} pos_{p,a} dz_t(s, f, p)     a = x, y, z; no factor s: a scale multiplies b1, not gr
//     dL / d df(s,f,p) = -sum_t (TWOPI dt_t) dz_t(s, f, p)                         per point and scale, no reduction
// k_bloch_vjp_gr_batch: the workgroups, staging, checkpoints and sweeps of k_bloch_vjp_batch.  Per sample a thread hands the
// reduction five rows: the rf pair, px dz, py dz, pz dz.  Eight samples x five rows do not fit the 16-row tile, so the backward
// walk of a group of VJP_T samples goes in sub-groups of BGR_T = 3 samples (15 rows), each summed in the rf adjoint's fixed order
// into one partial per (workgroup, sample, component): the rf pair where k_bloch_vjp_batch puts it, the g components in three planes
// of their own with the same index.  k_bloch_vjp_gr_fold sums both over chunks, then over scales, in index order (rf times s
// through abr_vjp_fold_sum, g without) and applies the factors of gamma dt_t.  No atomics: the bits of every result depend only on
// the pulse, its grids, its cotangents and the scale list.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Arguments as k_bloch_vjp_batch takes them, then gpart: plane a (x, y, z) of the g partials at a npart, indexed as part; gdf (DF
// only): dL / d df where dL / d m0 goes, one entry per (scale, frequency, position).
template <bool DF>
__global__ __launch_bounds__(256) void k_bloch_vjp_gr_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                            const double* __restrict__ pos3, const double* __restrict__ scales,
                                                            const BlochPulseDev* __restrict__ pulses,
                                                            const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                            const BlochCkDev* __restrict__ cks, const double* __restrict__ m0,
                                                            const double* __restrict__ cx, const double* __restrict__ cy,
                                                            const double* __restrict__ cz, double2* __restrict__ part,
                                                            double* __restrict__ gpart, long npart, double* ck,
                                                            double* __restrict__ gx, double* __restrict__ gy, double* __restrict__ gz,
                                                            double* __restrict__ gdf) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    static_assert(BGR_T * BGR_ROWS <= 2 * VJP_T, "a sub-group's rows lie within the rf adjoint's tile");
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos;
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const long blk = (long)bk.scale * npair + (live ? pair : 0), o = P.o_off + blk;
    const long wg = (long)bk.scale * V.nch + bk.chunk;                   // the workgroup among its pulse's
    const long e0 = V.p_off + wg * V.n;                                   // its first partial, in part and in every plane of gpart
    double* wck = ck + K.c_off + wg * K.ng * BLOCH_CK + tid;
    // a thread past the end of the grid sweeps the first point from equilibrium with zero cotangents and contributes exact zeros
    double m[3] = {0, 0, 1}, l[3] = {0, 0, 0};
    if (live) {
        const double* mi = m0 + 3 * (P.m_off + blk);
        m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2];
        l[0] = cx[o]; l[1] = cy[o]; l[2] = cz[o];
    }
    auto stage = [&](int t0) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 s, as k_bloch_batch forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
        }
        __syncthreads();
    };
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        stage(t0);
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int q = 0; q < cnt; ++q) {
            if ((q & (VJP_T - 1)) == 0) {                                 // m before sample t0 + q: the group's checkpoint
                double* w = wck + (long)((t0 + q) / VJP_T) * BLOCH_CK;
                w[0] = m[0]; w[256] = m[1]; w[512] = m[2];
            }
            const double* s = sst[q];
            bloch_fwd_step(s, bloch_rotz(s, px, py, pz, dfv), m);
        }
    }
    const int row = tid >> 4, ln = tid & 15;                              // reduction: 16 lanes per row of the tile
    const int rs = row / BGR_ROWS, rc = row - rs * BGR_ROWS;              // row = 5 (sample - u0) + (0: rotx, 1: roty, 2..4: px, py, pz dz)
    double adf = 0;                                                       // sum_t (TWOPI dt_t) dz_t of this point
    for (int t0 = tlast; t0 >= 0; t0 -= BLOCH_CH) {
        if (t0 != tlast) stage(t0);                                       // the forward sweep left the last tile staged
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
            for (int u = (VJP_T - 1) / BGR_T; u >= 0; --u) {             // sub-groups of samples g0 + 3 u .. g0 + 3 u + 2, the last first
                const int u0 = g0 + BGR_T * u;
                if (u0 < ge) {                                            // the same for every thread of the workgroup
#pragma unroll
                    for (int k = BGR_T - 1; k >= 0; --k) {
                        const int j = BGR_T * u + k;
                        if (j < VJP_T && g0 + j < ge) {
                            const double* s = sst[g0 + j];
                            const double3 c = bloch_vjp_step_z(s, bloch_rotz(s, px, py, pz, dfv), ms[j], l);
                            double* r5 = red + (BGR_ROWS * k) * VJP_ROW + tid;
                            r5[0] = live ? c.x : 0.0;
                            r5[VJP_ROW] = live ? c.y : 0.0;
                            r5[2 * VJP_ROW] = live ? px * c.z : 0.0;
                            r5[3 * VJP_ROW] = live ? py * c.z : 0.0;
                            r5[4 * VJP_ROW] = live ? pz * c.z : 0.0;
                            if (DF) adf = fma(s[5], c.z, adf);
                        }
                    }
                    __syncthreads();
                    double sum = 0;                                       // rows of samples past ge hold an earlier sub-group: not stored
                    for (int k = 0; k < 16; ++k) sum += red[row * VJP_ROW + ln + 16 * k];
                    for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
                    if (ln == 0 && rs < BGR_T && u0 + rs < ge) {
                        const long e = e0 + t0 + u0 + rs;
                        if (rc < 2) reinterpret_cast<double*>(part + e)[rc] = sum;
                        else gpart[(rc - 2) * npart + e] = sum;
                    }
                    __syncthreads();
                }
            }
        }
    }
    if (live) {
        gx[o] = l[0]; gy[o] = l[1]; gz[o] = l[2];
        if (DF) gdf[o] = -adf;
    }
}

// grad[t_off + t] as k_bloch_vjp_fold; gg[a T + t_off + t] = -(gamma dt_t) sum_s (sum_c gpart_a(s, c, t)), chunks then scales in
// index order, no factor s.  The table of k_bloch_vjp_fold with 256 x 4 threads per workgroup: one thread per sample for rf
// (threadIdx.y = 0: waves 0..3) and one per component of g (waves 4..15), so that the four serial sums run side by side.
__global__ __launch_bounds__(1024) void k_bloch_vjp_gr_fold(const double2* __restrict__ part, const double* __restrict__ gpart,
                                                            long npart, const VjpPulseDev* __restrict__ vp,
                                                            const SimBlock* __restrict__ blocks, const double* __restrict__ scales,
                                                            int nscale, const double* __restrict__ in,
                                                            const BlochPulseDev* __restrict__ pulses, double2* __restrict__ grad,
                                                            double* __restrict__ gg, long T) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int t = bk.chunk * 256 + threadIdx.x;
    if (t >= V.n) return;
    const double f = pulses[bk.pulse].gamma * in[BLOCH_IN * (V.r_off + t) + 8];
    if (threadIdx.y == 0) {
        const double2 g = abr_vjp_fold_sum(part, V, scales, nscale, t);
        grad[V.r_off + t] = make_double2(-(f * g.x), f * g.y);
        return;
    }
    const int a = threadIdx.y - 1;
    double g = 0;
    for (int s = 0; s < nscale; ++s) {
        double u = 0;
        const double* rowp = gpart + a * npart + V.p_off + (long)s * V.nch * V.n + t;
        for (int c = 0; c < V.nch; ++c) u += rowp[(long)c * V.n];
        g += u;
    }
    gg[a * T + V.r_off + t] = -(f * g);
}

// Launches k_bloch_vjp_gr_fold on nfold workgroups for the callers outside this file (blochssg.hip).
void bloch_vjp_gr_fold_launch(hipStream_t st, long nfold, const double2* part, const double* gpart, long npart, const VjpPulseDev* vp,
                              const SimBlock* blocks, const double* scales, int nscale, const double* in,
                              const BlochPulseDev* pulses, double2* grad, double* gg, long T) {
    hipLaunchKernelGGL(k_bloch_vjp_gr_fold, dim3((unsigned)nfold), dim3(256, 4), 0, st, part, gpart, npart, vp, blocks, scales, nscale,
                       in, pulses, grad, gg, T);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_vjp_gr_batch (arguments checked by api.cpp): the staging of bloch_vjp_batch_run; one upload, two
// launches, one download.  The output region is the b1 gradient (T double2), the three planes of dL / d g (3 T doubles), dL / d df
// (O doubles, only when wanted), dL / d m0 (3 O doubles), then the partials of rf and of g and the checkpoints, which stay on the
// device.
void bloch_vjp_gr_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* cmx,
                            const double* cmy, const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y,
                            double* gm0z, double* ggx, double* ggy, double* ggz, double* gdf) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    Staging& S = B.S;
    const long O = B.O, T = toff[npulse];
    std::vector<VjpPulseDev> vp(npulse);
    std::vector<BlochCkDev> ck(npulse);
    long npart = 0, nck = 0, nfold = 0;                         // double2 partials, checkpoint doubles, workgroups of the fold
    for (int p = 0; p < npulse; ++p) {
        const int n = B.ntime[p], nch = int((B.npair[p] + 255) / 256), ng = (n + VJP_T - 1) / VJP_T;
        vp[p] = VjpPulseDev{toff[p], npart, n, nch};
        ck[p] = BlochCkDev{nck, ng, 0};
        npart += (long)nscale * nch * n;
        nck += (long)nscale * nch * ng * BLOCH_CK;
        nfold += (n + 255) / 256;
    }
    const size_t o_c = S.add((size_t)O * 24), o_vp = S.add(npulse * sizeof(VjpPulseDev)), o_ck = S.add(npulse * sizeof(BlochCkDev)),
                 o_fb = S.add(nfold * sizeof(SimBlock));
    double* c = S.at<double>(o_c);
    std::copy(cmx, cmx + O, c);
    std::copy(cmy, cmy + O, c + O);
    std::copy(cmz, cmz + O, c + 2 * O);
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(o_vp));
    std::copy(ck.begin(), ck.end(), S.at<BlochCkDev>(o_ck));
    SimBlock* fb = S.at<SimBlock>(o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int k = 0; k < (B.ntime[p] + 255) / 256; ++k) *fb++ = SimBlock{p, 0, k, 0};
    const bool want_m0 = gm0x != nullptr, want_df = gdf != nullptr;
    const size_t n_g = (size_t)T * 5, n_df = want_df ? (size_t)O : 0;  // doubles of both gradients; of dL / d df
    const size_t n_pt = (n_g + n_df + (size_t)O * 3 + 1) & ~size_t(1);  // an even count: the partials after it stay 16-byte aligned
    S.upload((n_pt + (size_t)npart * 5 + (size_t)nck) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* gg = reinterpret_cast<double*>(grad + T);
    double* gd = gg + 3 * T;
    double* gm = gd + n_df;
    double2* part = reinterpret_cast<double2*>(reinterpret_cast<double*>(grad) + n_pt);
    double* gpart = reinterpret_cast<double*>(part + npart);
    double* cks = gpart + 3 * npart;
    const double* cd = S.dev<const double>(o_c);
    auto sweep = want_df ? k_bloch_vjp_gr_batch<true> : k_bloch_vjp_gr_batch<false>;
    hipLaunchKernelGGL(sweep, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(B.o_in), S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(o_vp), S.dev<const BlochCkDev>(o_ck),
                       S.dev<const double>(B.o_m0), cd, cd + O, cd + 2 * O, part, gpart, npart, cks, gm, gm + O, gm + 2 * O,
                       want_df ? gd : nullptr);
    hipLaunchKernelGGL(k_bloch_vjp_gr_fold, dim3((unsigned)nfold), dim3(256, 4), 0, st, part, gpart, npart,
                       S.dev<const VjpPulseDev>(o_vp), S.dev<const SimBlock>(o_fb), S.dev<const double>(S.o_sc), nscale,
                       S.dev<const double>(B.o_in), S.dev<const BlochPulseDev>(S.o_pd), grad, gg, T);
    std::vector<double> h(n_g + n_df + (want_m0 ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), g_re, g_im);
    const double* hg = h.data() + 2 * T;
    std::copy(hg, hg + T, ggx);
    std::copy(hg + T, hg + 2 * T, ggy);
    std::copy(hg + 2 * T, hg + 3 * T, ggz);
    if (want_df) std::copy(hg + 3 * T, hg + 3 * T + O, gdf);
    if (want_m0) {
        const double* hm = h.data() + n_g + n_df;
        std::copy(hm, hm + O, gm0x);
        std::copy(hm + O, hm + 2 * O, gm0y);
        std::copy(hm + 2 * O, hm + 3 * O, gm0z);
    }
}

}  // namespace mbfir
