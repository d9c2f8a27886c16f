// Fused least-squares and Gauss-Newton products of the pulse train's schedule: 8ab's loss with the gain and the RF phase
// of every repetition as the variable.  In blochtrainsched.hip's and blochtrainschedjvp.hip's notation, per pulse,
//     L = 1/2 sum_s sum_k rw_k sum_points sum_c w_c (echo_{k,c} - t_c)^2 + 1/2 sum_s sum_points sum_c wf_c (m_{N,c} - tf_c)^2
//     lsq: L, dL / dgains[k], dL / dphases[k] (per radian): 8ad's contraction at ce_k = rw_k w (echo_k - t), cf = wf (m_N - tf)
//     gn:  H v = J' W J v for v = (dg, dp): 8ae's recursion along v from dm_0 = 0 gives decho_k and dm_N; 8ad's contraction at
//          ce_k = rw_k w decho_k, cf = wf dm_N, taken at the primal u_k
// Everything between the echoes (or their tangents) and the cotangents is pointwise and the thread that owns the point holds every
// operand, so nothing echo-sized is written or read: what comes down is 2 ntr numbers per pulse (and direction) and the loss.
//   k_bloch_train_run_sched_lsq: k_bloch_train_run_sched's launch shape, table, forward walk and checkpoints.  On the way back the
//                                echo of repetition k is formed from the recomputed u_k with k_bloch_train_run's statements, the
//                                residual, ce_k and the thread's share of the loss as in k_bloch_train_run_lsq, then
//                                k_bloch_train_run_sched's two contractions and its reduction through the VJP_T x 2 tile.  The loss
//                                goes through a fixed tree in LDS (lm_block_sum) to one partial per (scale, chunk).
//   k_bloch_train_run_sched_gn:  the forward table times the directions, one direction per workgroup.  The forward walk carries
//                                (m, dm) with train_sj_in / train_sj_map as k_bloch_train_run_sched_jvp does and checkpoints both;
//                                the backward walk recomputes (u_k, du_k), forms decho_k, ce_k = rw_k (w decho_k), lambda_N = wf dm_N,
//                                and contracts at the primal u_k into direction d's own partials.
//   k_bloch_train_sched_gn_fold: k_bloch_train_sched_fold's sum (chunks, then scales, in index order) per (pulse, direction), and the
//                                loss partials of a pulse in index order.
// The propagators' planes come from the shipped k_bloch_train_prop, their tangents in the gain from the shipped
// k_bloch_train_prop_dgain, which is skipped when neither a gains direction nor a gains output is asked for: the workspace is 2 W
// doubles whatever the number of directions.  No atomics.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// k_bloch_train_run_sched_gn's body, its switch TSGN_HOIST and train_sg_back are in sim_dev.h (bloch_train_run_sched_gn_body), shared
// with the schedule's device Levenberg-Marquardt step (blochtrainschedlm.hip).

// k_bloch_train_run_sched_lsq: blochtrainschedgn_lsq.inc as it is.  Its magnitude twin k_bloch_train_run_sched_lsq_mag
// is the same text in blochtrainmag.hip: a second kernel with this one's LDS arrays in this file gave this one another LDS layout.
#define TRAIN_LSQ_KERNEL(name) name
#define TRAIN_MAG false
#include "blochtrainschedgn_lsq.inc"
#undef TRAIN_LSQ_KERNEL
#undef TRAIN_MAG

// blocks: the forward table times the directions (pad).  dws (null: no gains direction and no gains output), rep, gidx, m0, demod:
// k_bloch_train_run_sched_jvp's; dgain / dphi (either null: zeros): direction d of a pulse at ndir r_off + d ntr.  rw, we, PE, wf,
// PO, ebcast: k_bloch_train_run_gn's.  ck: direction d's checkpoints from 2 d CK, a group 2 x 3 x 256 doubles (m, then dm); part:
// direction d's partials from d NP, laid out as k_bloch_train_run_sched's.
__global__ __launch_bounds__(256) void k_bloch_train_run_sched_gn(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const double* __restrict__ m0, const double* __restrict__ dgain, const double* __restrict__ dphi, int demod, int ebcast, int ndir,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, long CK, long NP, double* ck,
    double2* __restrict__ part) {
    bloch_train_run_sched_gn_body(blocks[blockIdx.x], ws, dws, rep, gidx, rw, pulses, trains, vp, cks, m0, dgain, dphi, demod, ebcast, ndir,
                                  we, PE, wf, PO, CK, NP, ck, part);
}
// The magnitude twin: we / wf are two planes (xy, z), PE / PO apart.
__global__ __launch_bounds__(256) void k_bloch_train_run_sched_gn_mag(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const double* __restrict__ m0, const double* __restrict__ dgain, const double* __restrict__ dphi, int demod, int ebcast, int ndir,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, long CK, long NP, double* ck,
    double2* __restrict__ part) {
    bloch_train_run_sched_gn_body_mag(blocks[blockIdx.x], ws, dws, rep, gidx, rw, pulses, trains, vp, cks, m0, dgain, dphi, demod, ebcast,
                                      ndir, we, PE, wf, PO, CK, NP, ck, part);
}

// out[ndir r_off + d n + k] = k_bloch_train_sched_fold's value from direction d's partials (part + d NP): one thread per repetition,
// one workgroup per (pulse, direction, 256 repetitions) from its own table (SimBlock: pulse, direction, chunk of repetitions).  lsq
// (loss not null, ndir = 1): the first thread of a pulse's first workgroup also sums the pulse's nscale nch loss partials in index
// order.
__global__ __launch_bounds__(256) void k_bloch_train_sched_gn_fold(const double2* __restrict__ part, long NP,
                                                                   const VjpPulseDev* __restrict__ vp,
                                                                   const SimBlock* __restrict__ blocks, int nscale, int ndir,
                                                                   double2* __restrict__ out, const double* __restrict__ lpart,
                                                                   const long* __restrict__ lp, double* __restrict__ loss) {
    const SimBlock bk = blocks[blockIdx.x];
    const VjpPulseDev V = vp[bk.pulse];
    const int k = bk.chunk * 256 + threadIdx.x;
    if (loss && bk.scale == 0 && k == 0) {
        const double* q = lpart + lp[bk.pulse];
        const long nw = (long)nscale * V.nch;
        double s = 0;
        for (long i = 0; i < nw; ++i) s += q[i];
        loss[bk.pulse] = s;
    }
    if (k >= V.n) return;
    double2 g = make_double2(0, 0);
    for (int s = 0; s < nscale; ++s) {
        double2 t = make_double2(0, 0);
        const double2* rw = part + (long)bk.scale * NP + V.p_off + (long)s * V.nch * V.n + k;
        for (int c = 0; c < V.nch; ++c) {
            const double2 v = rw[(long)c * V.n];
            t.x += v.x; t.y += v.y;
        }
        g.x += t.x; g.y += t.y;
    }
    out[(long)ndir * V.r_off + (long)bk.scale * V.n + k] = g;
}

// The two launches of bloch_train_lsq_sched_batch_run for the schedule's device step (blochtrainschedlm.hip), which
// evaluates with the shipped kernels: arguments as the kernels take them, no dL / dm0, one direction.
void train_sched_lsq_launch(hipStream_t st, long nblk, const double* ws, const double* dws, const double2* rep, const int* gidx,
                            const double* rw, const BlochPulseDev* pulses, const TrainPulseDev* trains, const SimBlock* blocks,
                            const VjpPulseDev* vp, const BlochCkDev* cks, const long* lp, const double* m0, int demod, int ebcast,
                            const double* we, const double* te, long PE, const double* wf, const double* tf, long PO, double* ck,
                            double2* part, double* lpart, bool mag) {
    if (mag) {
        train_sched_lsq_mag_launch(st, nblk, ws, dws, rep, gidx, rw, pulses, trains, blocks, vp, cks, lp, m0, demod, ebcast, we, te, PE,
                                   wf, tf, PO, ck, part, nullptr, nullptr, nullptr, lpart);
        return;
    }
    hipLaunchKernelGGL(k_bloch_train_run_sched_lsq, dim3((unsigned)nblk), dim3(256), 0, st, ws, dws, rep, gidx, rw, pulses, trains,
                       blocks, vp, cks, lp, m0, demod, ebcast, we, te, PE, wf, tf, PO, ck, part, nullptr, nullptr, nullptr, lpart);
}
void train_sched_gn_fold_launch(hipStream_t st, long nfold, const double2* part, long NP, const VjpPulseDev* vp, const SimBlock* blocks,
                                int nscale, double2* out, const double* lpart, const long* lp, double* loss) {
    hipLaunchKernelGGL(k_bloch_train_sched_gn_fold, dim3((unsigned)nfold), dim3(256), 0, st, part, NP, vp, blocks, nscale, 1, out, lpart,
                       lp, loss);
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_lsq_sched_batch and mbfir_bloch_train_gn_sched_batch (arguments checked by api.cpp): the forward
// train's staging (bloch_stage, train_stage), the weights and targets, the partial and checkpoint descriptors, the loss partials'
// offsets, the tables of the period's tangent and of the fold and, for gn, the directions and the forward table times the
// directions; one upload, the launches, one download.  The output region is what comes down (the gradient halves or the products as
// double2, the loss, dL / dm0), then what stays on the device: the partials per direction, the loss partials, the primal planes,
// their tangents in the gain and the checkpoints per direction.
// SchedGnCall (sim_dev.h): the sections both calls, and the schedule's device step (blochtrainschedlm.hip), add after train_stage;
// t* null for gn.
void sched_gn_stage(SchedGnCall& Cl, int npulse, int nscale, const int* ntr, const long* roff, int ebcast, int ndir,
                    const double* const w[3], const double* const t[3], const double* rw, const double* const wf[3],
                    const double* const tf[3], bool mag) {
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    Staging& S = B.S;
    const int np = mag ? 2 : 3;
    Cl.PE = ebcast ? B.O : Ts.E;
    Cl.o_we = add_planes(S, w, Cl.PE, np);
    Cl.o_te = add_planes(S, t, Cl.PE, np);
    Cl.o_wf = add_planes(S, wf, B.O, np);
    Cl.o_tf = add_planes(S, tf, B.O, np);
    Cl.o_rw = S.add(rw ? (size_t)roff[npulse] * 8 : 0);
    if (rw) std::copy(rw, rw + roff[npulse], S.at<double>(Cl.o_rw));
    std::vector<VjpPulseDev> vp(npulse);
    std::vector<BlochCkDev> ckr(npulse);
    std::vector<long> lp(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int nch = int((B.npair[p] + 255) / 256), ngr = (ntr[p] + TRV_T - 1) / TRV_T;
        vp[p] = VjpPulseDev{roff[p], Cl.npart, ntr[p], nch};
        ckr[p] = BlochCkDev{Cl.nck, ngr, 0};
        lp[p] = Cl.nlp;
        Cl.npart += (long)nscale * nch * ntr[p];
        Cl.nck += (long)nscale * nch * ngr * BLOCH_CK;
        Cl.nlp += (long)nscale * nch;
        Cl.nfold += (long)ndir * ((ntr[p] + 255) / 256);
    }
    Cl.o_vp = S.add(npulse * sizeof(VjpPulseDev));
    Cl.o_ck = S.add(npulse * sizeof(BlochCkDev));
    Cl.o_lp = S.add(npulse * sizeof(long));
    Cl.o_fb = S.add(Cl.nfold * sizeof(SimBlock));
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(Cl.o_vp));
    std::copy(ckr.begin(), ckr.end(), S.at<BlochCkDev>(Cl.o_ck));
    std::copy(lp.begin(), lp.end(), S.at<long>(Cl.o_lp));
    SimBlock* fb = S.at<SimBlock>(Cl.o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int d = 0; d < ndir; ++d)
            for (int k = 0; k < (ntr[p] + 255) / 256; ++k) *fb++ = SimBlock{p, d, k, 0};
}

namespace {

// what came down as R double2 -> the two halves the caller wants
void unpack_halves(size_t n, const double* h, double* a, double* b) {
    for (size_t k = 0; k < n; ++k) {
        if (a) a[k] = h[2 * k];
        if (b) b[k] = h[2 * k + 1];
    }
}

}  // namespace

void bloch_train_lsq_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, int ebcast, const double* const w[3], const double* const t[3],
                                     const double* rw, const double* const wf[3], const double* const tf[3], double* loss,
                                     double* ggain, double* gphi, double* gmx, double* gmy, double* gmz, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    SchedGnCall Cl;
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    sched_gn_stage(Cl, npulse, nscale, ntr, roff, ebcast, 1, w, t, rw, wf, tf, mag);
    Staging& S = B.S;
    const long O = B.O, R = roff[npulse];
    const bool want_g = ggain != nullptr, want_m0 = gmx != nullptr, echo_t = w[0] != nullptr, fin_t = wf[0] != nullptr;
    long nwg = 0;                                                         // workgroups of the period's tangent
    const size_t o_qb = want_g ? train_jvp_table(Ts, nscale, 1, nwg) : 0;
    // even counts: the partials after them stay 16-byte aligned
    const size_t NL = ((size_t)npulse + 1) & ~size_t(1), O3 = want_m0 ? ((size_t)O * 3 + 1) & ~size_t(1) : 0;
    const size_t W = (size_t)Ts.W, LP = ((size_t)Cl.nlp + 1) & ~size_t(1);
    S.upload(((size_t)R * 2 + NL + O3 + (size_t)Cl.npart * 2 + LP + W + (want_g ? W : 0) + (size_t)Cl.nck) * 8, st);
    double2* grad = S.dev<double2>(S.o_out);
    double* dloss = reinterpret_cast<double*>(grad + R);
    double* gm = dloss + NL;
    double2* part = reinterpret_cast<double2*>(gm + O3);
    double* lpart = reinterpret_cast<double*>(part + Cl.npart);
    double* ws = lpart + LP;
    double* dws = want_g ? ws + W : nullptr;
    double* ck = ws + W + (want_g ? W : 0);
    train_launch_prop(Ts, st, ws);
    if (want_g) train_launch_prop_dgain(Ts, st, o_qb, nwg, dws);
    const double* wed = echo_t ? S.dev<const double>(Cl.o_we) : nullptr;
    const double* ted = echo_t ? S.dev<const double>(Cl.o_te) : nullptr;
    const double* wfd = fin_t ? S.dev<const double>(Cl.o_wf) : nullptr;
    const double* tfd = fin_t ? S.dev<const double>(Cl.o_tf) : nullptr;
    if (mag) {
        train_sched_lsq_mag_launch(st, (long)S.nblk, ws, dws, S.dev<const double2>(Ts.o_rep), S.dev<const int>(Ts.o_gi),
                                   rw ? S.dev<const double>(Cl.o_rw) : nullptr, S.dev<const BlochPulseDev>(S.o_pd),
                                   S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(S.o_bk),
                                   S.dev<const VjpPulseDev>(Cl.o_vp), S.dev<const BlochCkDev>(Cl.o_ck), S.dev<const long>(Cl.o_lp),
                                   S.dev<const double>(B.o_m0), demod, ebcast, wed, ted, Cl.PE, wfd, tfd, O, ck, part,
                                   want_m0 ? gm : nullptr, want_m0 ? gm + O : nullptr, want_m0 ? gm + 2 * O : nullptr, lpart);
    } else {
        hipLaunchKernelGGL(k_bloch_train_run_sched_lsq, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, dws,
                           S.dev<const double2>(Ts.o_rep), S.dev<const int>(Ts.o_gi), rw ? S.dev<const double>(Cl.o_rw) : nullptr,
                           S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(S.o_bk),
                           S.dev<const VjpPulseDev>(Cl.o_vp), S.dev<const BlochCkDev>(Cl.o_ck), S.dev<const long>(Cl.o_lp),
                           S.dev<const double>(B.o_m0), demod, ebcast, wed, ted, Cl.PE, wfd, tfd, O, ck, part,
                           want_m0 ? gm : nullptr, want_m0 ? gm + O : nullptr, want_m0 ? gm + 2 * O : nullptr, lpart);
    }
    hipLaunchKernelGGL(k_bloch_train_sched_gn_fold, dim3((unsigned)Cl.nfold), dim3(256), 0, st, part, Cl.npart,
                       S.dev<const VjpPulseDev>(Cl.o_vp), S.dev<const SimBlock>(Cl.o_fb), nscale, 1, grad, lpart,
                       S.dev<const long>(Cl.o_lp), dloss);
    std::vector<double> h((size_t)R * 2 + NL + O3);
    S.download(h.data(), h.size() * 8, st);
    unpack_halves((size_t)R, h.data(), ggain, gphi);
    std::copy(h.data() + 2 * R, h.data() + 2 * R + npulse, loss);
    if (want_m0) {
        const double* hm = h.data() + 2 * R + NL;
        std::copy(hm, hm + O, gmx);
        std::copy(hm + O, hm + 2 * O, gmy);
        std::copy(hm + 2 * O, hm + 3 * O, gmz);
    }
}

void bloch_train_gn_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                    const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                    const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                    const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                    const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                    const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                    const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                    const double* m0z, int ebcast, const double* const w[3], const double* rw,
                                    const double* const wf[3], int ndir, const double* dgain, const double* dphi, double* hgain,
                                    double* hphi, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    SchedGnCall Cl;
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    const double* const none[3] = {nullptr, nullptr, nullptr};
    sched_gn_stage(Cl, npulse, nscale, ntr, roff, ebcast, ndir, w, none, rw, wf, none, mag);
    Staging& S = B.S;
    const long O = B.O;
    const size_t D = (size_t)ndir * roff[npulse], W = (size_t)Ts.W, K = (size_t)ndir;
    const size_t o_g = dgain ? S.add(D * 8) : 0, o_p = dphi ? S.add(D * 8) : 0;
    const size_t o_jb = sim_group_table(S, ndir);
    if (dgain) std::copy(dgain, dgain + D, S.at<double>(o_g));
    if (dphi) std::copy(dphi, dphi + D, S.at<double>(o_p));
    const bool tang = dgain != nullptr || hgain != nullptr;               // the planes' tangents in the gain are needed
    long nwg = 0;
    const size_t o_qb = tang ? train_jvp_table(Ts, nscale, 1, nwg) : 0;
    S.upload((D * 2 + K * (size_t)Cl.npart * 2 + W + (tang ? W : 0) + 2 * K * (size_t)Cl.nck) * 8, st);
    double2* out = S.dev<double2>(S.o_out);
    double2* part = out + D;
    double* ws = reinterpret_cast<double*>(part + K * (size_t)Cl.npart);
    double* dws = tang ? ws + W : nullptr;
    double* ck = ws + W + (tang ? W : 0);
    train_launch_prop(Ts, st, ws);
    if (tang) train_launch_prop_dgain(Ts, st, o_qb, nwg, dws);
    hipLaunchKernelGGL(mag ? k_bloch_train_run_sched_gn_mag : k_bloch_train_run_sched_gn, dim3((unsigned)(S.nblk * ndir)), dim3(256), 0, st, ws, dws,
                       S.dev<const double2>(Ts.o_rep), S.dev<const int>(Ts.o_gi), rw ? S.dev<const double>(Cl.o_rw) : nullptr,
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(o_jb),
                       S.dev<const VjpPulseDev>(Cl.o_vp), S.dev<const BlochCkDev>(Cl.o_ck), S.dev<const double>(B.o_m0),
                       dgain ? S.dev<const double>(o_g) : nullptr, dphi ? S.dev<const double>(o_p) : nullptr, demod, ebcast, ndir,
                       w[0] ? S.dev<const double>(Cl.o_we) : nullptr, Cl.PE, wf[0] ? S.dev<const double>(Cl.o_wf) : nullptr, O, Cl.nck,
                       Cl.npart, ck, part);
    hipLaunchKernelGGL(k_bloch_train_sched_gn_fold, dim3((unsigned)Cl.nfold), dim3(256), 0, st, part, Cl.npart,
                       S.dev<const VjpPulseDev>(Cl.o_vp), S.dev<const SimBlock>(Cl.o_fb), nscale, ndir, out, nullptr,
                       S.dev<const long>(Cl.o_lp), nullptr);
    std::vector<double> h(D * 2);
    S.download(h.data(), h.size() * 8, st);
    unpack_halves(D, h.data(), hgain, hphi);
}

}  // namespace mbfir
