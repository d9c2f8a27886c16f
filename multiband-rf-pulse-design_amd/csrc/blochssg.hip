// Adjoint of the Bloch simulator's steady state with respect to b1, the gradient waveform and the off-resonance.  One
// period is F(m) = A m + B and the steady state its fixed point M = F(M) (blochss.hip has the notation), so for any parameter of
// the period dM = (I - A)^-1 dF|_{m0 = M}: for a cotangent c of M, lambda = (I - A)^-T c, and dL / dgr and dL / ddf are the
// transient adjoint's (blochgradg.hip) on the sweep started from m0 = M with the end cotangent lambda:
//     dL / d g_{t,a}   = -(gamma dt_t) sum_s sum_{f,p} pos_{p,a} dz_t(s, f, p)     a = x, y, z; no factor s
//     dL / d df(s,f,p) = -sum_t (TWOPI dt_t) dz_t(s, f, p)                         per point and scale, no reduction
// There is no dL / dm0.  k_bloch_ss_vjp_gr_batch is k_bloch_ss_vjp_batch's pass 0 and forward sweep followed by
// k_bloch_vjp_gr_batch's reverse sweep: the same launch shape, staging, checkpoints, sub-group walk and partials, folded by
// k_bloch_vjp_gr_fold (blochgradg.hip, unchanged).  No guard on det, as in blochss.hip.  No atomics: the bits of every result
// depend only on the pulse, its grids, its cotangents and the scale list.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Arguments as k_bloch_ss_vjp_batch takes them, then gpart and npart as k_bloch_vjp_gr_batch takes them, and gdf (DF only): dL / d df
// in the cotangents' layout, one entry per (scale, frequency, position).
template <bool DF>
__global__ __launch_bounds__(256) void k_bloch_ss_vjp_gr_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                               const double* __restrict__ pos3, const double* __restrict__ scales,
                                                               const BlochPulseDev* __restrict__ pulses,
                                                               const SimBlock* __restrict__ blocks,
                                                               const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
                                                               const double* __restrict__ cx, const double* __restrict__ cy,
                                                               const double* __restrict__ cz, double2* __restrict__ part,
                                                               double* __restrict__ gpart, long npart, double* ck,
                                                               double* __restrict__ mx, double* __restrict__ my,
                                                               double* __restrict__ mz, double* __restrict__ gdf) {
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
    const long o = P.o_off + (long)bk.scale * npair + (live ? pair : 0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;                   // the workgroup among its pulse's
    const long e0 = V.p_off + wg * V.n;                                   // its first partial, in part and in every plane of gpart
    double* wck = ck + K.c_off + wg * K.ng * BLOCH_CK + tid;
    // a thread past the end of the grid sweeps the first point with zero cotangents and contributes exact zeros
    double m[3], l[3];
    {
        double inv[9];
        bloch_ss_pass0(sst, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, inv, m);
        const double c0 = live ? cx[o] : 0.0, c1 = live ? cy[o] : 0.0, c2 = live ? cz[o] : 0.0;
        for (int j = 0; j < 3; ++j) l[j] = inv[3 * j] * c0 + inv[3 * j + 1] * c1 + inv[3 * j + 2] * c2;      // lambda = inv' c
    }
    if (live && mx) { mx[o] = m[0]; my[o] = m[1]; mz[o] = m[2]; }
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        if (t0 != tlast || t0 != 0) bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);      // pass 0 left the last tile staged
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
        if (t0 != tlast) bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);      // the forward sweep left the last tile staged
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
    if (DF && live) gdf[o] = -adf;
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_ss_vjp_gr_batch (arguments checked by api.cpp): the staging of bloch_ss_vjp_batch_run; one upload, two
// launches, one download.  The output region is the b1 gradient (T double2), the three planes of dL / d g (3 T doubles), dL / d df
// (O doubles, only when wanted), M (3 O doubles), then the partials of rf and of g and the checkpoints, which stay on the device.
void bloch_ss_vjp_gr_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                               const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                               int nscale, const double* scales, const double* cmx, const double* cmy, const double* cmz,
                               double* g_re, double* g_im, double* mx, double* my, double* mz, double* ggx, double* ggy, double* ggz,
                               double* gdf) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, nullptr, nullptr, nullptr);
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
    const bool want_m = mx != nullptr, want_df = gdf != nullptr;
    const size_t n_g = (size_t)T * 5, n_df = want_df ? (size_t)O : 0;  // doubles of both gradients; of dL / d df
    const size_t n_pt = (n_g + n_df + (size_t)O * 3 + 1) & ~size_t(1);  // an even count: the partials after it stay 16-byte aligned
    S.upload((n_pt + (size_t)npart * 5 + (size_t)nck) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* gg = reinterpret_cast<double*>(grad + T);
    double* gd = gg + 3 * T;
    double* pm = gd + n_df;
    double2* part = reinterpret_cast<double2*>(reinterpret_cast<double*>(grad) + n_pt);
    double* gpart = reinterpret_cast<double*>(part + npart);
    double* cks = gpart + 3 * npart;
    const double* cd = S.dev<const double>(o_c);
    auto sweep = want_df ? k_bloch_ss_vjp_gr_batch<true> : k_bloch_ss_vjp_gr_batch<false>;
    hipLaunchKernelGGL(sweep, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(B.o_in), S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(o_vp), S.dev<const BlochCkDev>(o_ck), cd, cd + O,
                       cd + 2 * O, part, gpart, npart, cks, want_m ? pm : nullptr, want_m ? pm + O : nullptr,
                       want_m ? pm + 2 * O : nullptr, want_df ? gd : nullptr);
    bloch_vjp_gr_fold_launch(st, nfold, part, gpart, npart, S.dev<const VjpPulseDev>(o_vp), S.dev<const SimBlock>(o_fb),
                             S.dev<const double>(S.o_sc), nscale, S.dev<const double>(B.o_in), S.dev<const BlochPulseDev>(S.o_pd), grad,
                             gg, T);
    std::vector<double> h(n_g + n_df + (want_m ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), g_re, g_im);
    const double* hg = h.data() + 2 * T;
    std::copy(hg, hg + T, ggx);
    std::copy(hg + T, hg + 2 * T, ggy);
    std::copy(hg + 2 * T, hg + 3 * T, ggz);
    if (want_df) std::copy(hg + 3 * T, hg + 3 * T + O, gdf);
    if (want_m) {
        const double* hm = h.data() + n_g + n_df;
        std::copy(hm, hm + O, mx);
        std::copy(hm + O, hm + 2 * O, my);
        std::copy(hm + 2 * O, hm + 3 * O, mz);
    }
}

}  // namespace mbfir
