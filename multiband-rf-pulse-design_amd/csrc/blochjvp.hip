// Tangent of the Bloch simulator with relaxation: the Jacobian-vector product of k_bloch_batch's end point (mode 0)
// with respect to the b1 samples and to the initial magnetisation.  Per (scale, frequency, position) point and sample t the
// forward step is m_t = D_t R_t m_{t-1} + c_t (blochgrad.hip has the notation).  Along a b1 direction v and an m0 direction dm_0
//     dm_t = D_t ( R_t dm_{t-1} + dR_t[dn_t] m_{t-1} ),   dn_t = (dnx, dny, 0)
//     dnx = ((-(Re v_t s)) gamma) dt_t,   dny = ((Im v_t s) gamma) dt_t          (formed as rotx / roty are formed from b1)
// one forward sweep, no reduction over points; c_t has no tangent.  k_bloch_jvp_batch: one 256-thread workgroup per (pulse, scale,
// chunk of 256 points, group of BJVP_K directions): the forward kernel's block table times the direction groups, one thread per
// point.  The BJVP_K tangents of a thread share the sample's sincos, sp, D, the rotation and the three vectors U, Vx, Vy (bloch_jvp_shared, sim_dev.h).
// The primal state advances through bloch_rotmat's body (bloch_rotmat_trig, which also hands out the sample's trigonometry) and
// rot_vec as in k_bloch_batch: the (mx, my, mz) written here (by the workgroups of group 0) have k_bloch_batch's bits.  Every
// direction runs the same instructions on its own registers, so a tangent's bits depend only on its pulse, scale, point and
// direction.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Directions per workgroup: the largest of 1, 2, 4, 8 without scratch at no less than k_bloch_batch's occupancy minus one wave per
// SIMD (DESIGN 8q has the table).
#ifndef BJVP_K
#define BJVP_K 8
#endif

// in, df, pos3, scales, pulses, m0: k_bloch_batch's.  blocks: SimBlock with pad = the direction group.  v (interleaved): direction k
// of pulse p at ndir t_off + k ntime.  dm0 (three planes of ndir O entries from dm0, null: zero) and dmx / dmy / dmz: pulse p from
// ndir o_off, (direction, scale, point) row-major.  mx / my / mz: the forward kernel's mode-0 layout, written by the workgroups of
// direction group 0.
__global__ __launch_bounds__(256) void k_bloch_jvp_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                         const double* __restrict__ pos3, const double* __restrict__ scales,
                                                         const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                         const double* __restrict__ m0, const double2* __restrict__ v,
                                                         const double* __restrict__ dm0, int ndir, int nscale, long O,
                                                         double* __restrict__ mx, double* __restrict__ my, double* __restrict__ mz,
                                                         double* __restrict__ dmx, double* __restrict__ dmy,
                                                         double* __restrict__ dmz) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double2 sdn[BJVP_K][BLOCH_CH];
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos;
    const int k0 = bk.pad * BJVP_K, kcnt = min(BJVP_K, ndir - k0);
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 256 + threadIdx.x;
    const bool live = pair < npair;
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const long blk = (long)bk.scale * npair + pair, o0 = P.o_off + blk;
    const long T = (long)ndir * O;                                          // entries of one tangent plane
    const double2* vg = v + (long)ndir * P.t_off + (long)k0 * ntime;          // the group's first direction
    double m[3] = {0, 0, 1}, dm[BJVP_K][3];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
#pragma unroll
    for (int k = 0; k < BJVP_K; ++k) {
        dm[k][0] = dm[k][1] = dm[k][2] = 0;
        if (k < kcnt && live && dm0) {
            const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * npair + pair;
            dm[k][0] = dm0[o]; dm[k][1] = dm0[T + o]; dm[k][2] = dm0[2 * T + o];
        }
    }
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if ((int)threadIdx.x < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + threadIdx.x);
            const double dt = s[8];
            sst[threadIdx.x][0] = ((-(s[0] * sc)) * gamma) * dt;          // rotx of the pulse b1 s, as k_bloch_batch forms it
            sst[threadIdx.x][1] = ((s[1] * sc) * gamma) * dt;             // roty
            for (int e = 2; e < 8; ++e) sst[threadIdx.x][e] = s[e];
#pragma unroll
            for (int k = 0; k < BJVP_K; ++k)
                if (k < kcnt) {
                    const double2 d = vg[(long)k * ntime + t0 + threadIdx.x];
                    sdn[k][threadIdx.x] = make_double2(((-(d.x * sc)) * gamma) * dt, ((d.y * sc) * gamma) * dt);      // (dnx, dny)
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
            for (int k = 0; k < BJVP_K; ++k)
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
    if (bk.pad == 0) { mx[o0] = m[0]; my[o0] = m[1]; mz[o0] = m[2]; }
#pragma unroll
    for (int k = 0; k < BJVP_K; ++k)
        if (k < kcnt) {
            const long o = (long)ndir * P.o_off + ((long)(k0 + k) * nscale + bk.scale) * npair + pair;
            dmx[o] = dm[k][0]; dmy[o] = dm[k][1]; dmz[o] = dm[k][2];
        }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_jvp_batch (arguments checked by api.cpp): the forward call's staging (bloch_stage, mode 0) plus the
// directions, the m0 directions and the block table times the direction groups; one upload, one launch, one download.  The output
// region is dmx, dmy, dmz (ndir O entries each), then mx, my, mz (O each), which are downloaded only when the caller wants them.

int bloch_jvp_group() { return BJVP_K; }

void bloch_jvp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                         const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                         const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                         int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                         const double* scales, const double* m0x, const double* m0y, const double* m0z, int ndir, const double* v_re,
                         const double* v_im, const double* dm0x, const double* dm0y, const double* dm0z, double* mx, double* my,
                         double* mz, double* dmx, double* dmy, double* dmz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    Staging& S = B.S;
    const long O = B.O;
    const size_t T = (size_t)ndir * O, V = (size_t)ndir * toff[npulse];
    const int ngrp = (ndir + BJVP_K - 1) / BJVP_K;
    const long nblk = S.nblk * ngrp;
    const size_t o_v = S.add(V * 16), o_d = dm0x ? S.add(3 * T * 8) : 0, o_jb = sim_group_table(S, ngrp);
    pack_cplx(V, v_re, v_im, S.at<double2>(o_v));
    if (dm0x) {
        double* d = S.at<double>(o_d);
        std::copy(dm0x, dm0x + T, d);
        std::copy(dm0y, dm0y + T, d + T);
        std::copy(dm0z, dm0z + T, d + 2 * T);
    }
    S.upload((3 * T + 3 * (size_t)O) * 8, st);
    double* out = S.dev<double>(S.o_out);
    double* pr = out + 3 * T;
    hipLaunchKernelGGL(k_bloch_jvp_batch, dim3((unsigned)nblk), dim3(256), 0, st, S.dev<const double>(B.o_in),
                       S.dev<const double>(B.o_df), S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const SimBlock>(o_jb), S.dev<const double>(B.o_m0),
                       S.dev<const double2>(o_v), dm0x ? S.dev<const double>(o_d) : nullptr, ndir, nscale, O, pr, pr + O, pr + 2 * O,
                       out, out + T, out + 2 * T);
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
