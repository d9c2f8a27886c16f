// Adjoint of the pulse train with respect to b1, the initial magnetisation, the gradient waveform and the off-resonance.
// Nothing changes in the repetition walk: gr and df enter a period only through a sample's rotz_t, which neither the RF phase
// Z(phi_k) nor the gain touches.  k_bloch_train_run_vjp (blochtrainvjp.hip) therefore delivers, as it stands, the cotangents
// [Abar | Bbar] and [Abar_e | Bbar_e] of every (scale, distinct gain) combination c and point, and the four columns of X = [A | B]
// are swept as k_bloch_train_prop_vjp sweeps them.  With rotz_t = -((gx_t gamma dt_t) x + (gy_t gamma dt_t) y + (gz_t gamma dt_t) z +
// df (TWOPI dt_t)) and dz_t(c, col, f, p) what bloch_vjp_step_z (sim_dev.h) returns on column col (the recovery term does not
// depend on rotz: the same function serves columns 0..2 and column 3),
//     dL / d g_{t,a}   = -(gamma dt_t) sum_c sum_{f,p} pos_{p,a} sum_col dz_t      a = x, y, z; no factor scale x gain
//     dL / d df(s,f,p) = -sum_t (TWOPI dt_t) sum_{g in gains of s} sum_col dz_t    per scale and point
// k_bloch_train_prop_vjp_gr: the workgroups, table, seeds and forward half of k_bloch_train_prop_vjp (sim_dev.h) and a backward half
// of its own, blochgradg.hip's: a group of VJP_T samples is walked in sub-groups of BGR_T samples x BGR_ROWS rows (the rf pair,
// px dz, py dz, pz dz) of the 16-row tile, each summed in the rf adjoint's fixed order into one partial per (workgroup, sample,
// component).  k_bloch_train_vjp_gr_fold sums them over chunks, then over the pulse's combinations in index order (rf times scale x
// gain through abr_vjp_fold_sum, g without) and applies the factors of gamma dt_t; k_bloch_train_vjp_df_fold sums a scale's distinct
// gains in index order.  No atomics: the bits of every result depend only on the pulse, its grids, its train, its cotangents and
// the scale list.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// Arguments as k_bloch_train_prop_vjp takes them, then gpart: plane a (x, y, z) of the g partials at a npart, indexed as part; dfw
// (DF only): sum_t (TWOPI dt_t) sum_col dz_t, one double per (combination, point), the pulse's from w_off / TRAIN_ENT.
template <bool DF>
__global__ __launch_bounds__(256) void k_bloch_train_prop_vjp_gr(
    const double* __restrict__ in, const double* __restrict__ df, const double* __restrict__ pos3, const double* __restrict__ amp,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const SimBlock* __restrict__ blocks,
    const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks, const double* __restrict__ cw, double2* __restrict__ part,
    double* __restrict__ gpart, long npart, double* ck, double* __restrict__ dfw) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    static_assert(BLOCH_CH % VJP_T == 0, "a group of samples lies within one staged tile");
    static_assert(BGR_T * BGR_ROWS <= 2 * VJP_T, "a sub-group's rows lie within the rf adjoint's tile");
    const SimBlock bk = blocks[blockIdx.x];
    const TrainPropVjpThread C = bloch_train_prop_vjp_thread(bk, df, pos3, amp, pulses, trains, vp, cks, part, ck);
    double l[3] = {0, 0, 0}, le[3] = {0, 0, 0};
    bloch_train_prop_vjp_seed(C, bk, cw, l, le);
    bloch_train_prop_vjp_forward(C, sst, in);
    // the backward half, the pulse's last tile being staged in sst and the checkpoints written
    const BlochPulseDev& P = C.P;
    const double sc = C.sc, gamma = C.gamma, px = C.px, py = C.py, pz = C.pz, dfv = C.dfv;
    const int ntime = C.ntime, echo = C.echo, tid = threadIdx.x;
    const bool rec = C.rec, live = C.live;
    double2* wpart = C.wpart;
    double* wg = gpart + (C.wpart - part);                                // the workgroup's first partial in every plane of gpart
    const double* wck = C.wck;
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    const int row = tid >> 4, ln = tid & 15;                              // reduction: 16 lanes per row of the tile
    const int rs = row / BGR_ROWS, rc = row - rs * BGR_ROWS;              // row = 5 (sample - u0) + (0: rotx, 1: roty, 2..4: px, py, pz dz)
    double adf = 0;                                                       // sum_t (TWOPI dt_t) dz_t of this column and point
    for (int t0 = tlast; t0 >= 0; t0 -= BLOCH_CH) {
        if (t0 != tlast) bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);      // the forward sweep left the last tile staged
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int g0 = (cnt - 1) / VJP_T * VJP_T; g0 >= 0; g0 -= VJP_T) {
            const int ge = min(g0 + VJP_T, cnt);
            double ms[VJP_T][3];                                          // ms[j] = the column before sample t0 + g0 + j
            const double* w = wck + (long)((t0 + g0) / VJP_T) * BLOCH_CK;
            ms[0][0] = w[0]; ms[0][1] = w[256]; ms[0][2] = w[512];
#pragma unroll
            for (int j = 1; j < VJP_T; ++j) {
                ms[j][0] = ms[j - 1][0]; ms[j][1] = ms[j - 1][1]; ms[j][2] = ms[j - 1][2];
                if (g0 + j < ge) {
                    const double* s = sst[g0 + j - 1];
                    const double rz = bloch_rotz(s, px, py, pz, dfv);
                    if (rec) bloch_fwd_step(s, rz, ms[j]); else bloch_hom_step(s, rz, ms[j]);
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
                            if (t0 + g0 + j + 1 == echo) { l[0] += le[0]; l[1] += le[1]; l[2] += le[2]; }      // the state after `echo` samples
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
                        const long e = t0 + u0 + rs;
                        if (rc < 2) reinterpret_cast<double*>(wpart + e)[rc] = sum;
                        else wg[(rc - 2) * npart + e] = sum;
                    }
                    __syncthreads();
                }
            }
        }
    }
    if (DF) {                                                             // the four columns of a point in column order; the tile is free
        red[tid] = live ? adf : 0.0;
        __syncthreads();
        if (tid < 64 && live)
            dfw[C.Tr.w_off / TRAIN_ENT + (long)bk.scale * C.npair + C.pair] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
    }
}

// grad[t_off + t] as k_bloch_train_vjp_fold; gg[a T + t_off + t] = -(gamma dt_t) sum_c (sum over chunks of gpart_a(c, chunk, t)),
// chunks then the pulse's combinations in index order, no amplitude factor.  The table of k_bloch_train_vjp_fold with 256 x 4
// threads per workgroup: one thread per sample for rf (threadIdx.y = 0) and one per component of g, as k_bloch_vjp_gr_fold.
__global__ __launch_bounds__(1024) void k_bloch_train_vjp_gr_fold(const double2* __restrict__ part, const double* __restrict__ gpart,
                                                                  long npart, const VjpPulseDev* __restrict__ vp,
                                                                  const SimBlock* __restrict__ blocks, const double* __restrict__ amp,
                                                                  const TrainPulseDev* __restrict__ trains, int nscale,
                                                                  const double* __restrict__ in,
                                                                  const BlochPulseDev* __restrict__ pulses, double2* __restrict__ grad,
                                                                  double* __restrict__ gg, long T) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const int t = bk.chunk * 256 + threadIdx.x;
    if (t >= V.n) return;
    const int ncomb = nscale * Tr.ngain;
    const double f = pulses[bk.pulse].gamma * in[BLOCH_IN * (V.r_off + t) + 8];
    if (threadIdx.y == 0) {
        const double2 g = abr_vjp_fold_sum(part, V, amp + Tr.a_off, ncomb, t);
        grad[V.r_off + t] = make_double2(-(f * g.x), f * g.y);
        return;
    }
    const int a = threadIdx.y - 1;
    double g = 0;
    for (int c = 0; c < ncomb; ++c) {
        double u = 0;
        const double* rowp = gpart + a * npart + V.p_off + (long)c * V.nch * V.n + t;
        for (int k = 0; k < V.nch; ++k) u += rowp[(long)k * V.n];
        g += u;
    }
    gg[a * T + V.r_off + t] = -(f * g);
}

// gdf(s, f, p) = -sum_g dfw(s ngain + g, (f, p)), the scale's distinct gains in index order, in the final planes' layout.  blocks:
// the forward table (pulse, scale, chunk of 256 points).
__global__ __launch_bounds__(256) void k_bloch_train_vjp_df_fold(const double* __restrict__ dfw, const BlochPulseDev* __restrict__ pulses,
                                                                 const TrainPulseDev* __restrict__ trains,
                                                                 const SimBlock* __restrict__ blocks, double* __restrict__ gdf) {
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + threadIdx.x;
    if (pair >= npair) return;
    const double* w = dfw + Tr.w_off / TRAIN_ENT + (long)bk.scale * Tr.ngain * npair + pair;
    double g = 0;
    for (int k = 0; k < Tr.ngain; ++k) g += w[(long)k * npair];
    gdf[P.o_off + (long)bk.scale * npair + pair] = -g;
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_vjp_gr_batch (arguments checked by api.cpp): the staging of bloch_train_vjp_batch_run; one upload,
// four launches and the fold of dL / d df when it is wanted, one download.  The output region is the b1 gradient (T double2), the
// three planes of dL / d g (3 T doubles), dL / d df (O doubles, only when wanted), dL / d m0 (3 O doubles), then what stays on the
// device: the propagators' planes, their cotangents, the partials of rf and of g, the df workspace and the two kernels' checkpoints.
void bloch_train_vjp_gr_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                  const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                  const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                  const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                  int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                  const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                  const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                  const double* cex, const double* cey, const double* cez, const double* cfx, const double* cfy,
                                  const double* cfz, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz, double* ggx,
                                  double* ggy, double* ggz, double* gdf) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    Staging& S = B.S;
    const long O = B.O, T = toff[npulse], E = Ts.E;
    const size_t o_ce = S.add(cex ? (size_t)E * 24 : 0), o_cf = S.add(cfx ? (size_t)O * 24 : 0);
    if (cex) {
        double* c = S.at<double>(o_ce);
        std::copy(cex, cex + E, c);
        std::copy(cey, cey + E, c + E);
        std::copy(cez, cez + E, c + 2 * E);
    }
    if (cfx) {
        double* c = S.at<double>(o_cf);
        std::copy(cfx, cfx + O, c);
        std::copy(cfy, cfy + O, c + O);
        std::copy(cfz, cfz + O, c + 2 * O);
    }
    const TrainVjpSections V = train_vjp_stage(Ts, npulse, toff, nscale, ntr);
    const long npart = V.npart, nckr = V.nckr, nckp = V.nckp;
    const bool want_m0 = gmx != nullptr, want_df = gdf != nullptr;
    const size_t W = (size_t)Ts.W, n_g = (size_t)T * 5, n_df = want_df ? (size_t)O : 0;       // doubles of both gradients; of dL / d df
    const size_t n_pt = (n_g + n_df + (size_t)O * 3 + 1) & ~size_t(1);  // an even count: the partials after the planes stay 16-byte aligned
    const size_t n_dw = want_df ? W / TRAIN_ENT : 0;                    // one double per (combination, point)
    S.upload((n_pt + 2 * W + (size_t)npart * 5 + n_dw + (size_t)nckr + (size_t)nckp) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* gg = reinterpret_cast<double*>(grad + T);
    double* gd = gg + 3 * T;
    double* gm = gd + n_df;
    double* ws = reinterpret_cast<double*>(grad) + n_pt;
    double* cw = ws + W;
    double2* part = reinterpret_cast<double2*>(cw + W);
    double* gpart = reinterpret_cast<double*>(part + npart);
    double* dfw = gpart + 3 * npart;
    double* ck1 = dfw + n_dw;
    double* ck2 = ck1 + nckr;
    MBFIR_HIP(hipMemsetAsync(cw, 0, W * 8, st));                 // upload does not zero the output region
    train_launch_prop(Ts, st, ws);
    const double* ced = cex ? S.dev<const double>(o_ce) : nullptr;
    const double* cfd = cfx ? S.dev<const double>(o_cf) : nullptr;
    train_launch_run_vjp(Ts, V, st, ws, demod, ced, cfd, ck1, cw, want_m0 ? gm : nullptr);
    auto sweep = want_df ? k_bloch_train_prop_vjp_gr<true> : k_bloch_train_prop_vjp_gr<false>;
    hipLaunchKernelGGL(sweep, dim3((unsigned)V.nwg), dim3(256), 0, st, S.dev<const double>(B.o_in), S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(Ts.o_amp), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(V.o_vb), S.dev<const VjpPulseDev>(V.o_vp),
                       S.dev<const BlochCkDev>(V.o_ckp), cw, part, gpart, npart, ck2, want_df ? dfw : nullptr);
    hipLaunchKernelGGL(k_bloch_train_vjp_gr_fold, dim3((unsigned)V.nfold), dim3(256, 4), 0, st, part, gpart, npart,
                       S.dev<const VjpPulseDev>(V.o_vp), S.dev<const SimBlock>(V.o_fb), S.dev<const double>(Ts.o_amp),
                       S.dev<const TrainPulseDev>(Ts.o_tr), nscale, S.dev<const double>(B.o_in), S.dev<const BlochPulseDev>(S.o_pd),
                       grad, gg, T);
    if (want_df)
        hipLaunchKernelGGL(k_bloch_train_vjp_df_fold, dim3((unsigned)S.nblk), dim3(256), 0, st, dfw, S.dev<const BlochPulseDev>(S.o_pd),
                           S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(S.o_bk), gd);
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
        std::copy(hm, hm + O, gmx);
        std::copy(hm + O, hm + 2 * O, gmy);
        std::copy(hm + 2 * O, hm + 3 * O, gmz);
    }
}

}  // namespace mbfir
