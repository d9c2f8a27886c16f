// Adjoint of the Bloch simulator with relaxation: the vector-Jacobian product of k_bloch_batch's end point (mode 0)
// with respect to the b1 samples and to the initial magnetisation.  Per (scale, frequency, position) point and sample t the
// forward step is m_t = D_t R_t m_{t-1} + c_t with D_t = diag(e2, e2, e1), c_t = (0, 0, 1 - e1) and R_t = bloch_rotmat(rotx_t,
// roty_t, rotz_t) (sim_dev.h), rotx_t = ((-(Re b1_t s)) gamma) dt_t, roty_t = ((Im b1_t s) gamma) dt_t.  With the cotangent
// lambda_n = (cmx, cmy, cmz) of m_n, over the samples in reverse
//     dL / d rotx_t += (D_t lambda_t)' (dR_t / d rotx) m_{t-1}          (and the same for roty)
//     lambda_{t-1}   = R_t' D_t lambda_t,                               lambda_0 = dL / d m_0
// The step is a contraction: undoing it would divide by e1 and e2 and amplify rounding by exp(T / T2), so m_{t-1} is never
// recovered from m_t.  The forward sweep writes m to a scratch array before every VJP_T-th sample; the reverse sweep, per group of
// VJP_T samples, steps the group's states forwards again from its checkpoint into registers and then walks the group backwards.
// The steps (bloch_fwd_step, bloch_vjp_step) and the checkpoints' descriptor are in sim_dev.h, shared with blochgn.hip.
// k_bloch_vjp_batch: one 256-thread workgroup per (pulse, scale, chunk of 256 points) from the forward call's block table, one
// thread per point, the sample rows staged through LDS as k_bloch_batch stages them.  The 256 contributions to a sample are summed
// in a fixed order through the VJP_T x VJP_ROW tile of the rf adjoints (simgrad.hip) into one partial per (workgroup, sample);
// k_bloch_vjp_fold sums a pulse's partials over chunks, then over scales (times s), in index order (abr_vjp_fold_sum) and applies
// -(gamma dt_t) to the real part and +(gamma dt_t) to the imaginary part.  No atomics: a pulse's gradient bits depend only on the
// pulse, its grids, its cotangents and the scale list.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Cotangents cx / cy / cz lie where k_bloch_batch writes mx / my / mz in mode 0: S x nf x npos per pulse, scale-major; gx / gy / gz
// (dL / d m0) the same.  part: one double2 (sum of dL / d rotx, sum of dL / d roty) per (workgroup, sample), VjpPulseDev's layout.
__global__ __launch_bounds__(256) void k_bloch_vjp_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                         const double* __restrict__ pos3, const double* __restrict__ scales,
                                                         const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                         const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
                                                         const double* __restrict__ m0, const double* __restrict__ cx,
                                                         const double* __restrict__ cy, const double* __restrict__ cz,
                                                         double2* __restrict__ part, double* ck, double* __restrict__ gx,
                                                         double* __restrict__ gy, double* __restrict__ gz) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
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
    double2* wpart = part + V.p_off + wg * V.n;
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
    if (live) { gx[o] = l[0]; gy[o] = l[1]; gz[o] = l[2]; }
}

// grad[t_off + t] = (-(gamma dt_t) X, +(gamma dt_t) Y), (X, Y) = sum_s scales[s] (sum_c part(s, c, t)), chunks then scales in index
// order; one thread per sample, one workgroup per (pulse, 256 samples) from its own table (SimBlock: pulse, 0, chunk of samples).
__global__ __launch_bounds__(256) void k_bloch_vjp_fold(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                        const SimBlock* __restrict__ blocks, const double* __restrict__ scales,
                                                        int nscale, const double* __restrict__ in,
                                                        const BlochPulseDev* __restrict__ pulses, double2* __restrict__ grad) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int t = bk.chunk * 256 + threadIdx.x;
    if (t >= V.n) return;
    const double2 g = abr_vjp_fold_sum(part, V, scales, nscale, t);
    const double f = pulses[bk.pulse].gamma * in[BLOCH_IN * (V.r_off + t) + 8];
    grad[V.r_off + t] = make_double2(-(f * g.x), f * g.y);
}

// Launches k_bloch_vjp_fold on nfold workgroups for the callers outside this file (blochss.hip).
void bloch_vjp_fold_launch(hipStream_t st, long nfold, const double2* part, const VjpPulseDev* vp, const SimBlock* blocks,
                           const double* scales, int nscale, const double* in, const BlochPulseDev* pulses, double2* grad) {
    hipLaunchKernelGGL(k_bloch_vjp_fold, dim3((unsigned)nfold), dim3(256), 0, st, part, vp, blocks, scales, nscale, in, pulses, grad);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_vjp_batch (arguments checked by api.cpp): the forward call's staging (bloch_stage, mode 0) plus the
// cotangents, the partial and checkpoint descriptors and the fold kernel's table; one upload, two launches, one download.  The
// output region is the gradient (T double2), dL / d m0 (3 O doubles), then the partials and the checkpoints, which stay on the device.
void bloch_vjp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                         const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                         const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                         int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                         const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* cmx,
                         const double* cmy, const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y,
                         double* gm0z) {
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
    const size_t O3 = ((size_t)O * 3 + 1) & ~size_t(1);          // an even count: the partials after it stay 16-byte aligned
    S.upload(((size_t)T * 2 + O3 + (size_t)npart * 2 + (size_t)nck) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* gm = reinterpret_cast<double*>(grad + T);
    double2* part = reinterpret_cast<double2*>(gm + O3);
    double* cks = reinterpret_cast<double*>(part + npart);
    const double* cd = S.dev<const double>(o_c);
    hipLaunchKernelGGL(k_bloch_vjp_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(B.o_in),
                       S.dev<const double>(B.o_df), S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(o_vp),
                       S.dev<const BlochCkDev>(o_ck), S.dev<const double>(B.o_m0), cd, cd + O, cd + 2 * O, part, cks, gm, gm + O,
                       gm + 2 * O);
    hipLaunchKernelGGL(k_bloch_vjp_fold, dim3((unsigned)nfold), dim3(256), 0, st, part, S.dev<const VjpPulseDev>(o_vp),
                       S.dev<const SimBlock>(o_fb), S.dev<const double>(S.o_sc), nscale, S.dev<const double>(B.o_in),
                       S.dev<const BlochPulseDev>(S.o_pd), grad);
    const bool want_m0 = gm0x != nullptr;
    std::vector<double> h((size_t)T * 2 + (want_m0 ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), g_re, g_im);
    if (want_m0) {
        const double* hm = h.data() + 2 * T;
        std::copy(hm, hm + O, gm0x);
        std::copy(hm + O, hm + 2 * O, gm0y);
        std::copy(hm + 2 * O, hm + 3 * O, gm0z);
    }
}

}  // namespace mbfir
