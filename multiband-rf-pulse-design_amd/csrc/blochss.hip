// Derivatives of the Bloch simulator's steady state: the adjoint and the tangent of k_bloch_batch's mode 1 with respect
// to the b1 samples.  One period is the map F(m) = A m + B with A = prod D_t R_t (blochgrad.hip has the notation); the steady state
// is its fixed point M = (I - A)^-1 B.  A and B depend on b1, and F(M) = M, so
//     dM = (I - A)^-1 (dA M + dB) = (I - A)^-1 dF|_{m0 = M}
// that is, the derivative of the transient end point started from m0 = M with m0 held fixed, through (I - A)^-1:
//   adjoint: for a cotangent c of M, lambda = (I - A)^-T c, and dL / db1 is the transient adjoint (blochgrad.hip) from m0 = M with the
//            end cotangent lambda.  There is no dL / dm0: the steady state does not depend on m0.
//   tangent: along a b1 direction v, d = the transient tangent (blochjvp.hip) from m0 = M with dm0 = 0, and dM = (I - A)^-1 d.
// Both kernels start with k_bloch_batch's pass 0 over the samples (bloch_ss_pass0: the same statements, with the A update's fused
// products written out as k_bloch_batch compiles them -- bloch_ss_rot_col -- so that M has mode 1's bits), then
// run the sweeps of k_bloch_vjp_batch / k_bloch_jvp_batch from M with the same launch shape, staging, checkpoints, reduction and
// fold (k_bloch_vjp_fold, unchanged).  No guard on det: where mode 1's forward is not finite (T1 so long that e1 rounds to 1), the
// derivatives are not finite either.  No atomics.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Directions per workgroup of the tangent (DESIGN 8t has the table).
#ifndef BSSJ_K
#define BSSJ_K 8
#endif
// in, df, pos3, scales, pulses, blocks, vp, cks, part, ck: k_bloch_vjp_batch's.  Cotangents cx / cy / cz lie where k_bloch_batch
// writes mx / my / mz in mode 1: S x nf x npos per pulse, scale-major; mx / my / mz (null: not wanted) receive M in that layout.
__global__ __launch_bounds__(256) void k_bloch_ss_vjp_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                            const double* __restrict__ pos3, const double* __restrict__ scales,
                                                            const BlochPulseDev* __restrict__ pulses,
                                                            const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                            const BlochCkDev* __restrict__ cks, const double* __restrict__ cx,
                                                            const double* __restrict__ cy, const double* __restrict__ cz,
                                                            double2* __restrict__ part, double* ck, double* __restrict__ mx,
                                                            double* __restrict__ my, double* __restrict__ mz) {
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
    const long o = P.o_off + (long)bk.scale * npair + (live ? pair : 0);
    const long wg = (long)bk.scale * V.nch + bk.chunk;                   // the workgroup among its pulse's
    double2* wpart = part + V.p_off + wg * V.n;
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

// in, df, pos3, scales, pulses, blocks (pad = the direction group), v, ndir, nscale, O and the outputs: k_bloch_jvp_batch's, the
// primal being M.  Every direction group recomputes pass 0; group 0 writes M.  inv survives the sweep in this thread's column of
// its workgroup's plane of sinv (global, 9 x 256 doubles per workgroup, written and read back coalesced by the same thread), so the
// sweep's registers and LDS are k_bloch_jvp_batch's (in registers or in LDS it costs a wave per SIMD: DESIGN 8t).
__global__ __launch_bounds__(256) void k_bloch_ss_jvp_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                            const double* __restrict__ pos3, const double* __restrict__ scales,
                                                            const BlochPulseDev* __restrict__ pulses,
                                                            const SimBlock* __restrict__ blocks, const double2* __restrict__ v,
                                                            int ndir, int nscale, long O, double* __restrict__ mx,
                                                            double* __restrict__ my, double* __restrict__ mz,
                                                            double* __restrict__ dmx, double* __restrict__ dmy,
                                                            double* __restrict__ dmz, double* sinv) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double2 sdn[BSSJ_K][BLOCH_CH];
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos;
    const int k0 = bk.pad * BSSJ_K, kcnt = min(BSSJ_K, ndir - k0);
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const long blk = (long)bk.scale * npair + pair, o0 = P.o_off + blk;
    const double2* vg = v + (long)ndir * P.t_off + (long)k0 * ntime;          // the group's first direction
    double* winv = sinv + (long)blockIdx.x * BLOCH_SSINV + tid;
    double m[3], dm[BSSJ_K][3];
    {
        double inv[9];
        bloch_ss_pass0(sst, in, P.t_off, ntime, sc, gamma, px, py, pz, dfv, inv, m);
        for (int e = 0; e < 9; ++e) winv[e * 256] = inv[e];               // read back by this thread alone
    }
    if (live && bk.pad == 0) { mx[o0] = m[0]; my[o0] = m[1]; mz[o0] = m[2]; }
#pragma unroll
    for (int k = 0; k < BSSJ_K; ++k) dm[k][0] = dm[k][1] = dm[k][2] = 0;
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 s, as k_bloch_batch forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
#pragma unroll
            for (int k = 0; k < BSSJ_K; ++k)
                if (k < kcnt) {
                    const double2 d = vg[(long)k * ntime + t0 + tid];
                    sdn[k][tid] = make_double2(((-(d.x * sc)) * gamma) * dt, ((d.y * sc) * gamma) * dt);      // (dnx, dny)
                }
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const double* s = sst[q];
            const double rotz = -((s[2] * px + s[3] * py + s[4] * pz) + dfv * s[5]);
            Rot3 R;
            BlochTrig tr;
            bloch_rotmat_trig<true>(s[0], s[1], rotz, R, tr);
            const double e1 = s[6], e2 = s[7];
            BlochJvpShared W;
            bloch_jvp_shared(s[0], s[1], rotz, tr, m, W);
#pragma unroll
            for (int k = 0; k < BSSJ_K; ++k)
                if (k < kcnt) {
                    const double2 dn = sdn[k][q];
                    const double nd = s[0] * dn.x + s[1] * dn.y;
                    double o[3];
                    rot_vec(R, dm[k], o);
                    dm[k][0] = e2 * (o[0] + (nd * W.U[0] + dn.x * W.Vx[0] + dn.y * W.Vy[0]));
                    dm[k][1] = e2 * (o[1] + (nd * W.U[1] + dn.x * W.Vx[1] + dn.y * W.Vy[1]));
                    dm[k][2] = e1 * (o[2] + (nd * W.U[2] + dn.x * W.Vx[2] + dn.y * W.Vy[2]));
                }
            double o[3];
            rot_vec(R, m, o);
            m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = e1 * o[2] + (1 - e1);
        }
    }
    if (!live) return;
    double inv[9];
    for (int e = 0; e < 9; ++e) inv[e] = winv[e * 256];
#pragma unroll
    for (int k = 0; k < BSSJ_K; ++k)
        if (k < kcnt) {
            const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * npair + pair;
            double d[3];
            for (int i = 0; i < 3; ++i) d[i] = inv[i] * dm[k][0] + inv[3 + i] * dm[k][1] + inv[6 + i] * dm[k][2];      // dM = inv d
            dmx[o] = d[0]; dmy[o] = d[1]; dmz[o] = d[2];
        }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_ss_vjp_batch (arguments checked by api.cpp): the forward call's staging (bloch_stage; no m0) plus the
// cotangents, the partial and checkpoint descriptors and the fold kernel's table; one upload, two launches, one download.  The
// output region is the gradient (T double2), M (3 O doubles), then the partials and the checkpoints, which stay on the device.
void bloch_ss_vjp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* cmx, const double* cmy, const double* cmz, double* g_re, double* g_im,
                            double* mx, double* my, double* mz) {
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
    const size_t O3 = ((size_t)O * 3 + 1) & ~size_t(1);          // an even count: the partials after it stay 16-byte aligned
    S.upload(((size_t)T * 2 + O3 + (size_t)npart * 2 + (size_t)nck) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* pm = reinterpret_cast<double*>(grad + T);
    double2* part = reinterpret_cast<double2*>(pm + O3);
    double* cks = reinterpret_cast<double*>(part + npart);
    const double* cd = S.dev<const double>(o_c);
    const bool want_m = mx != nullptr;
    hipLaunchKernelGGL(k_bloch_ss_vjp_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(B.o_in),
                       S.dev<const double>(B.o_df), S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(o_vp),
                       S.dev<const BlochCkDev>(o_ck), cd, cd + O, cd + 2 * O, part, cks, want_m ? pm : nullptr,
                       want_m ? pm + O : nullptr, want_m ? pm + 2 * O : nullptr);
    bloch_vjp_fold_launch(st, nfold, part, S.dev<const VjpPulseDev>(o_vp), S.dev<const SimBlock>(o_fb), S.dev<const double>(S.o_sc),
                          nscale, S.dev<const double>(B.o_in), S.dev<const BlochPulseDev>(S.o_pd), grad);
    std::vector<double> h((size_t)T * 2 + (want_m ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(T, reinterpret_cast<const double2*>(h.data()), g_re, g_im);
    if (want_m) {
        const double* hm = h.data() + 2 * T;
        std::copy(hm, hm + O, mx);
        std::copy(hm + O, hm + 2 * O, my);
        std::copy(hm + 2 * O, hm + 3 * O, mz);
    }
}

// Host side of mbfir_bloch_ss_jvp_batch (arguments checked by api.cpp): the forward call's staging (no m0) plus the directions and
// the block table times the direction groups; one upload, one launch, one download.  The output region is dmx, dmy, dmz (ndir O
// entries each), then mx, my, mz (O each), which are downloaded only when the caller wants them, then the workgroups' planes of
// (I - A)^-1, which stay on the device.
int bloch_ss_jvp_group() { return BSSJ_K; }

void bloch_ss_jvp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, int ndir, const double* v_re, const double* v_im, double* mx, double* my,
                            double* mz, double* dmx, double* dmy, double* dmz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, nullptr, nullptr, nullptr);
    Staging& S = B.S;
    const long O = B.O;
    const size_t T = (size_t)ndir * O, V = (size_t)ndir * toff[npulse];
    const int ngrp = (ndir + BSSJ_K - 1) / BSSJ_K;
    const long nblk = S.nblk * ngrp;
    const size_t o_v = S.add(V * 16), o_jb = sim_group_table(S, ngrp);
    pack_cplx(V, v_re, v_im, S.at<double2>(o_v));
    S.upload((3 * T + 3 * (size_t)O + (size_t)nblk * BLOCH_SSINV) * 8, st);
    double* out = S.dev<double>(S.o_out);
    double* pr = out + 3 * T;
    hipLaunchKernelGGL(k_bloch_ss_jvp_batch, dim3((unsigned)nblk), dim3(256), 0, st, S.dev<const double>(B.o_in),
                       S.dev<const double>(B.o_df), S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const SimBlock>(o_jb), S.dev<const double2>(o_v), ndir, nscale, O, pr,
                       pr + O, pr + 2 * O, out, out + T, out + 2 * T, pr + 3 * O);
    std::vector<double> h(3 * T + (mx ? 3 * (size_t)O : 0));
    S.download(h.data(), h.size() * 8, st);
    std::copy(h.begin(), h.begin() + T, dmx);
    std::copy(h.begin() + T, h.begin() + 2 * T, dmy);
    std::copy(h.begin() + 2 * T, h.begin() + 3 * T, dmz);
    if (mx) {
        const double* hp = h.data() + 3 * T;
        std::copy(hp, hp + O, mx);
        std::copy(hp + O, hp + 2 * O, my);
        std::copy(hp + 2 * O, hp + 3 * O, mz);
    }
}

}  // namespace mbfir
