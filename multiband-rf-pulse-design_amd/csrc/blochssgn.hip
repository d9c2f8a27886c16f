// Least-squares products of the Bloch simulator's steady state: with M_s = (I - A_s)^-1 B_s the steady state of the
// period at transmit gain s (k_bloch_batch's mode 1), weights w = (wx, wy, wz) >= 0 and targets t = (tx, ty, tz) per (scale,
// frequency, position) point, and J_s = dM_s / d(s b1) (real-linear),
//     L = 1/2 sum over the pulse's scales and points of sum_c w_c (M_c - t_c)^2
//   lsq: L and g = sum_s s J_s' W_s (M_s - t_s) = dL / d Re b1 + i dL / d Im b1       (k_bloch_ss_lsq_batch)
//   gn:  H v = sum_s s J_s' W_s J_s (s v) for a direction v of the b1 samples          (k_bloch_ss_gn_batch)
// Both are the steady state's adjoint (blochss.hip k_bloch_ss_vjp_batch) with the cotangent made where it is needed, inv being
// (I - A)^-1 of pass 0 (bloch_ss_pass0, which gives M mode 1's bits):
//   lsq: c = w (M - t) from pass 0's M itself, lambda = inv' c; then the forward sweep from M with its checkpoints and the reverse
//        sweep with the end cotangent lambda.  After lambda neither inv nor w nor t is live.
//   gn:  inv goes to the thread's column of its workgroup's global plane (k_bloch_ss_jvp_batch's sinv); the forward sweep from M
//        carries one tangent d from dm0 = 0 as bloch_gn_sweeps<true> does; inv comes back; dM = inv d, c = w dM, lambda = inv' c; then
//        the same reverse sweep.
// The launch shape, the staging of the rows, the checkpoints, the reverse loop, the reduction through the VJP_T x VJP_ROW tile and
// the fold (k_bloch_gn_fold, unchanged) are those of blochgn.hip, whose own loops stay where they are: the loops are restated here.
// No atomics: a pulse's L, g and H v bits depend only on the pulse, its grids, its weights, its targets or direction and the scale
// list.  Threads past the end of the grid and points of weight zero contribute exact zeros; scale 0 contributes an exact zero to g
// and H v through the fold's factor, and its loss (M = [0 0 1]) is counted.  No guard on det(I - A).
// LDS: the staged rows (16 KB) and the reduction tile (34 KB).  The staged (dnx, dny) row of gn is live only in the forward sweep
// and the tile only after it, so the row lies in the tile's storage.
// The Levenberg-Marquardt step solved on the device with these products (k_bloch_ss_lm_prep, k_bloch_ss_lm_sweep and
// the host side of mbfir_bloch_ss_lm_step_batch) follows the two kernels.
// The three sweep kernels lie in blochssgn_kernels.inc, which is included twice: as the component fits above, and as the magnitude
// fits of (|Mxy|, mz) (k_bloch_ss_lsq_batch_mag, k_bloch_ss_gn_batch_mag, k_bloch_ss_lm_sweep_mag), which differ in the
// block that makes c: c = (w_xy (rho - t_xy) u, w_z (M_z - t_z)) or (w_xy (u . dM_xy) u, w_z dM_z), rho = |M_xy|, u = M_xy / rho.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// The thread's point of either kernel: k_bloch_ss_vjp_batch's.  A thread past the end of the grid takes the first point.
struct BlochSsPoint {
    double px, py, pz, dfv;
    long o;                 // its entry in the planes of the weights, the targets and M
    bool live;
};
__device__ __forceinline__ BlochSsPoint bloch_ss_point(const SimBlock& bk, const BlochPulseDev& P, const double* __restrict__ df,
                                                       const double* __restrict__ pos3) {
    BlochSsPoint G;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + threadIdx.x;
    G.live = pair < npair;
    const int fi = G.live ? int(pair / P.npos) : 0, pi = G.live ? int(pair - (long)fi * P.npos) : 0;
    G.dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    G.px = pp[0]; G.py = pp[1]; G.pz = pp[2];
    G.o = P.o_off + (long)bk.scale * npair + (G.live ? pair : 0);
    return G;
}

// The reverse sweep and the reduction of k_bloch_ss_vjp_batch for one workgroup, the pulse's last tile being staged in sst: the
// partials of the end cotangent l into wpart.  Ends with a barrier.
__device__ __forceinline__ void bloch_ss_reverse(double (*sst)[8], double* red, const double* __restrict__ in, long t_off, int ntime,
                                                 double sc, double gamma, double px, double py, double pz, double dfv, bool live,
                                                 double l[3], double2* __restrict__ wpart, const double* wck) {
    const int tid = threadIdx.x, row = tid >> 4, ln = tid & 15;      // reduction: 16 lanes per row of the tile
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    for (int t0 = tlast; t0 >= 0; t0 -= BLOCH_CH) {
        if (t0 != tlast) bloch_ss_stage(sst, in, t_off, ntime, t0, sc, gamma);      // the forward sweep left the last tile staged
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

// ------------------------------------------------------------------------------------------------
// The Levenberg-Marquardt step of the steady state on the device, the twin of blochgn.hip's: conjugate
// gradients on (H + mu I) d = b per pulse, H p by the sweep of k_bloch_ss_gn_batch on the device's own p, everything else of an
// iteration in k_bloch_lm_step (blochgn.hip, unchanged); then, with targets, the loss and gradient at b1 + d by
// k_bloch_ss_lsq_batch on the trial's input rows.  b1 is fixed within one solve, so pass 0 runs once per call, in
// k_bloch_ss_lm_prep, and every round reads its (I - A)^-1 and M back as the doubles they are.  Stages depend on each other
// through launch order alone.
constexpr int BLOCH_SSLM_PLANE = BLOCH_SSINV + 3 * 256;      // doubles per forward workgroup: (I - A)^-1 as sinv holds it, then M

// Pass 0 of the pulses that run: the forward call's block table.  A thread writes its inv to the columns 0 .. 8 of its
// workgroup's plane, as k_bloch_ss_gn_batch writes sinv, and its M to the columns 9 .. 11; k_bloch_ss_lm_sweep's thread of the same
// workgroup and index reads them back, nobody else.
__global__ __launch_bounds__(256) void k_bloch_ss_lm_prep(const double* __restrict__ in, const double* __restrict__ df,
                                                          const double* __restrict__ pos3, const double* __restrict__ scales,
                                                          const BlochPulseDev* __restrict__ pulses,
                                                          const SimBlock* __restrict__ blocks, const LmState* __restrict__ st,
                                                          double* __restrict__ plane) {
    __shared__ double sst[BLOCH_CH][8];
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    const BlochPulseDev P = pulses[bk.pulse];
    const BlochSsPoint G = bloch_ss_point(bk, P, df, pos3);
    double* wpl = plane + (long)blockIdx.x * BLOCH_SSLM_PLANE + threadIdx.x;
    double inv[9], m[3];
    bloch_ss_pass0(sst, in, P.t_off, P.ntime, scales[bk.scale], P.gamma, G.px, G.py, G.pz, G.dfv, inv, m);
    for (int e = 0; e < 9; ++e) wpl[e * 256] = inv[e];
    for (int e = 0; e < 3; ++e) wpl[(9 + e) * 256] = m[e];
}

// ------------------------------------------------------------------------------------------------
// k_bloch_ss_lsq_batch, k_bloch_ss_gn_batch and k_bloch_ss_lm_sweep, then their magnitude twins k_bloch_ss_lsq_batch_mag,
// k_bloch_ss_gn_batch_mag and k_bloch_ss_lm_sweep_mag: one text, blochssgn_kernels.inc, compiled twice.
#define BLOCH_SS_KERNEL(name) name
#define BLOCH_SS_MAG false
#include "blochssgn_kernels.inc"
#undef BLOCH_SS_MAG
#undef BLOCH_SS_KERNEL
#define BLOCH_SS_KERNEL(name) name##_mag
#define BLOCH_SS_MAG true
#include "blochssgn_kernels.inc"
#undef BLOCH_SS_MAG
#undef BLOCH_SS_KERNEL

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_ss_lsq_batch / mbfir_bloch_ss_gn_batch (arguments checked by api.cpp): the forward call's staging
// (bloch_stage at mode 1, no m0) plus the sections of bloch_gn_stage; one upload, two launches, one download of the ndir T results
// (and the npulse losses, and M when it is wanted).  The output region is the results (ndir T double2), the losses (padded to a
// whole double2), M (lsq: 3 O doubles padded to an even count), then the partials, the loss partials, the checkpoints and (gn) the
// workgroups' planes of (I - A)^-1, which stay on the device.
namespace {
void bloch_ss_gn_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                     const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                     const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                     const double* const w[3], const double* const tg[3], int ndir, const double* v_re, const double* v_im,
                     double* loss, double* o_re, double* o_im, double* mx, double* my, double* mz, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool lsq = tg != nullptr, want_m = lsq && mx != nullptr;
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 1, nullptr, nullptr, nullptr);
    Staging& S = B.S;
    const BlochGnSections G = bloch_gn_stage(B, npulse, toff, nscale, w, tg, ndir, v_re, v_im, mag);
    const long O = B.O;
    const long R = (long)ndir * toff[npulse], nl = lsq ? (npulse + 1) / 2 : 0;      // double2 entries of the results and of the losses
    const size_t O3 = lsq ? ((size_t)O * 3 + 1) & ~size_t(1) : 0;                  // an even count: the partials stay 16-byte aligned
    const long nblk = S.nblk * ndir;
    S.upload(((size_t)R + nl + G.npart) * 16 + (O3 + (size_t)(lsq ? G.nlp : 0) + G.nck + (lsq ? 0 : (size_t)nblk * BLOCH_SSINV)) * 8,
             st);
    double2* res = S.dev<double2>(S.o_out);
    double* dloss = reinterpret_cast<double*>(res + R);
    double* pm = reinterpret_cast<double*>(res + R + nl);
    double2* part = reinterpret_cast<double2*>(pm + O3);
    double* lpart = reinterpret_cast<double*>(part + G.npart);
    double* cks = lpart + (lsq ? G.nlp : 0);
    double* sinv = cks + G.nck;
    const double* in = S.dev<const double>(B.o_in);
    if (lsq) {
        hipLaunchKernelGGL(mag ? k_bloch_ss_lsq_batch_mag : k_bloch_ss_lsq_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, in,
                           S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(S.o_bk), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const BlochCkDev>(G.o_ck),
                           S.dev<const long>(G.o_lp), S.dev<const double>(G.o_w), S.dev<const double>(G.o_t), O, part, cks, lpart,
                           want_m ? pm : nullptr, want_m ? pm + O : nullptr, want_m ? pm + 2 * O : nullptr);
    } else {
        hipLaunchKernelGGL(mag ? k_bloch_ss_gn_batch_mag : k_bloch_ss_gn_batch, dim3((unsigned)nblk), dim3(256), 0, st, in,
                           S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(G.o_jb), S.dev<const VjpPulseDev>(G.o_vp), S.dev<const BlochCkDev>(G.o_ck),
                           S.dev<const double>(G.o_w), O, S.dev<const double2>(G.o_v), ndir, part, cks, sinv);
    }
    bloch_gn_fold_launch(st, G.nfold, part, S.dev<const VjpPulseDev>(G.o_vp), S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc),
                         nscale, in, S.dev<const BlochPulseDev>(S.o_pd), res, lsq ? lpart : nullptr, S.dev<const long>(G.o_lp),
                         lsq ? dloss : nullptr);
    std::vector<double> h(((size_t)R + nl) * 2 + (want_m ? (size_t)O * 3 : 0));
    S.download(h.data(), h.size() * 8, st);
    unpack_cplx(R, reinterpret_cast<const double2*>(h.data()), o_re, o_im);
    if (lsq) std::copy(h.data() + 2 * R, h.data() + 2 * R + npulse, loss);
    if (want_m) {
        const double* hm = h.data() + 2 * (R + nl);
        std::copy(hm, hm + O, mx);
        std::copy(hm + O, hm + 2 * O, my);
        std::copy(hm + 2 * O, hm + 3 * O, mz);
    }
}
}  // namespace

void bloch_ss_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* wx, const double* wy, const double* wz, const double* tx,
                            const double* ty, const double* tz, double* loss, double* g_re, double* g_im, double* mx, double* my,
                            double* mz, bool mag) {
    const double* const w[3] = {wx, wy, wz};
    const double* const tg[3] = {tx, ty, tz};
    bloch_ss_gn_run(device, stream, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid,
                    poff, dx, dy, dz, nscale, scales, w, tg, 1, nullptr, nullptr, loss, g_re, g_im, mx, my, mz, mag);
}

void bloch_ss_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                           const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                           const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                           int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                           const double* scales, const double* wx, const double* wy, const double* wz, int ndir, const double* v_re,
                           const double* v_im, double* h_re, double* h_im, bool mag) {
    const double* const w[3] = {wx, wy, wz};
    bloch_ss_gn_run(device, stream, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid,
                    poff, dx, dy, dz, nscale, scales, w, nullptr, ndir, v_re, v_im, nullptr, h_re, h_im, nullptr, nullptr, nullptr, mag);
}

// Host side of mbfir_bloch_ss_lm_step_batch (arguments checked by api.cpp): the forward staging at mode 1 and bloch_gn_stage at
// ndir = 1 with b as the direction section, which is the device's p from then on; mu; one upload; k_lm_init, k_bloch_ss_lm_prep, cg
// rounds of (k_bloch_ss_lm_sweep, k_bloch_lm_step), and with targets k_bloch_lm_trial, k_bloch_ss_lsq_batch on the trial rows (its
// pass 0 is at b1 + d and its own) and the fold; one download.  The output region:
//   d (T double2), the npulse states, [the gradient at b1 + d (T double2), the npulse losses]                      downloaded
//   r, hp (T double2 each), the trial rows (9 T doubles), the partials, the loss partials, the checkpoints, the planes   stay on the device
// The partials and the checkpoints are those of one direction, reused by every round and by the trial's lsq sweep.
void bloch_ss_lm_step_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const double* wx, const double* wy, const double* wz,
                                const double* b_re, const double* b_im, const double* mu, int cg, double rtol, const double* tx,
                                const double* ty, const double* tz, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                                int* status, double* loss, double* g_re, double* g_im, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool trial = tx != nullptr;
    const double* const w[3] = {wx, wy, wz};
    const double* const tg[3] = {tx, ty, tz};
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 1, nullptr, nullptr, nullptr);
    Staging& S = B.S;
    const BlochGnSections G = bloch_gn_stage(B, npulse, toff, nscale, w, trial ? tg : nullptr, 1, b_re, b_im, mag);
    const size_t o_mu = S.add((size_t)npulse * 8);
    std::copy(mu, mu + npulse, S.at<double>(o_mu));
    const long T = toff[npulse];
    auto pad16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t b_vec = (size_t)T * 16, b_st = pad16(npulse * sizeof(LmState)), b_loss = pad16((size_t)npulse * 8);
    const size_t b_down = b_vec + b_st + (trial ? b_vec + b_loss : 0), b_rows = pad16((size_t)T * BLOCH_IN * 8);
    S.upload(b_down + 2 * b_vec + b_rows + (size_t)G.npart * 16 +
                 ((size_t)G.nlp + G.nck + (size_t)S.nblk * BLOCH_SSLM_PLANE) * 8,
             st);
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
    double* plane = cks + G.nck;
    double2* p = S.dev<double2>(G.o_v);
    const VjpPulseDev* vp = S.dev<const VjpPulseDev>(G.o_vp);
    const double* in = S.dev<const double>(B.o_in);
    lm_init_launch(st, npulse, vp, S.dev<const double>(o_mu), cg, rtol, p, d, r, state);
    hipLaunchKernelGGL(k_bloch_ss_lm_prep, dim3((unsigned)S.nblk), dim3(256), 0, st, in, S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), state, plane);      // cg = 0: no pulse runs, every workgroup returns at once
    for (int k = 0; k < cg; ++k) {                                // rounds of a pulse that has stopped are early exits
        hipLaunchKernelGGL(mag ? k_bloch_ss_lm_sweep_mag : k_bloch_ss_lm_sweep, dim3((unsigned)S.nblk), dim3(256), 0, st, in,
                           S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(G.o_jb), vp, S.dev<const BlochCkDev>(G.o_ck), S.dev<const double>(G.o_w), B.O, p,
                           state, part, cks, plane);
        bloch_lm_step_launch(st, npulse, part, vp, S.dev<const double>(S.o_sc), nscale, in, S.dev<const BlochPulseDev>(S.o_pd), cg,
                             rtol, p, d, r, hp, state);
    }
    if (trial) {
        bloch_lm_trial_launch(st, in, d, T, rows);
        hipLaunchKernelGGL(mag ? k_bloch_ss_lsq_batch_mag : k_bloch_ss_lsq_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, rows,
                           S.dev<const double>(B.o_df),
                           S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const SimBlock>(S.o_bk), vp, S.dev<const BlochCkDev>(G.o_ck), S.dev<const long>(G.o_lp),
                           S.dev<const double>(G.o_w), S.dev<const double>(G.o_t), B.O, part, cks, lpart, nullptr, nullptr, nullptr);
        bloch_gn_fold_launch(st, G.nfold, part, vp, S.dev<const SimBlock>(G.o_fb), S.dev<const double>(S.o_sc), nscale, rows,
                             S.dev<const BlochPulseDev>(S.o_pd), grad, lpart, S.dev<const long>(G.o_lp), dloss);
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
