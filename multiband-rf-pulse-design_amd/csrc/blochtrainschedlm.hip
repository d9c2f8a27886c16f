// The Levenberg-Marquardt step of the pulse train's schedule on the device, the schedule's twin of blochtrainlm.hip's
// (8ac): one call that evaluates and solves at the same schedule, so the propagators' planes and their tangents in the gain are
// computed once and serve both.
//   1. with targets: L, dL / dgains, dL / dphases at the call's schedule, by the shipped k_bloch_train_run_sched_lsq and
//      k_bloch_train_sched_gn_fold launched as bloch_train_lsq_sched_batch_run launches them: that call's bits;
//   2. conjugate gradients on (H + mu I) d = b per pulse from d = 0, H = J' W J restricted to the varied halves as
//      bloch_train_gn_sched_batch applies it at that schedule, b given or the negated gradient of 1. left on the device.
// The trial of the sibling steps is not here: a trial has other gains, so other planes, and its cos / sin and gain tables are the
// host's.  The caller evaluates the trial with the next call, which solves the next step at the same time.
// One upload, a chain of launches ordered by the stream, one download; the host reads nothing in between.  Once per call:
//   k_bloch_train_prop (shipped)          the primal planes
//   k_bloch_train_prop_dgain (shipped)    their tangents in the gain, only when the gains vary
//   k_bloch_train_run_sched_lsq, k_bloch_train_sched_gn_fold (shipped)    with targets
//   k_bloch_train_lm_sched_init           r = p = b (or -g), d = 0, gg = <b, b>, the run flags
// and a round, over the pulses whose LmState.run is set (a workgroup of a stopped pulse returns at once), is
//   k_bloch_train_lm_sched_run            k_bloch_train_run_sched_gn's body (sim_dev.h) at one direction, the device's own p
//   k_bloch_train_lm_sched_step           H p folded as k_bloch_train_sched_gn_fold folds it, the non-varied half masked to zero,
//                                         plus mu p; then k_bloch_train_lm_step's update
// p lies split, gains then phases, as the run kernel reads a direction at ndir = 1; d, r and H p are double2 (dg_k, dp_k) as the
// fold writes them.  The partials and the checkpoints of one direction serve 1. and every round.  No atomics.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// One workgroup per pulse.  bg / bp (null: that half of b is not given): b laid out as cosphi; grad (used for a half that is not
// given): b = -g, exact.  vg / vp: whether the half varies; a half that does not is zero throughout.  pg / pp (null for a half that
// does not vary) receive p = b, r receives b, d zeros; rr = gg = <b, b> by k_lm_init's tree and its first run flag.
__global__ __launch_bounds__(256) void k_bloch_train_lm_sched_init(const VjpPulseDev* __restrict__ vp_, const double* __restrict__ mu,
                                                                   int cg, double rtol, const double* __restrict__ bg,
                                                                   const double* __restrict__ bp, const double2* __restrict__ grad,
                                                                   int vg, int vp, double* __restrict__ pg, double* __restrict__ pp,
                                                                   double2* __restrict__ d, double2* __restrict__ r,
                                                                   LmState* __restrict__ st) {
    __shared__ double sw[256];
    const VjpPulseDev V = vp_[blockIdx.x];
    double s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        double2 b = make_double2(0, 0);
        if (vg) b.x = bg ? bg[t] : -grad[t].x;
        if (vp) b.y = bp ? bp[t] : -grad[t].y;
        d[t] = make_double2(0, 0);
        r[t] = b;
        if (vg) pg[t] = b.x;
        if (vp) pp[t] = b.y;
        s += lm_redot(b, b);
    }
    const double gg = lm_block_sum(s, sw);
    if (threadIdx.x == 0) {
        const bool run = lm_goes_on(0, cg, gg, rtol, gg);
        st[blockIdx.x] = LmState{gg, gg, mu[blockIdx.x], 0, run ? 1 : 0, gg > rtol * gg ? 1 : 0, 0};
    }
}

// blocks: the forward table at one direction.  pg / pp: the device's p (either null: zeros), read as a direction at ndir = 1.
__global__ __launch_bounds__(256) void k_bloch_train_lm_sched_run(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const double* __restrict__ m0, const double* __restrict__ pg, const double* __restrict__ pp, int demod, int ebcast,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, const LmState* __restrict__ st, double* ck,
    double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    bloch_train_run_sched_gn_body(bk, ws, dws, rep, gidx, rw, pulses, trains, vp, cks, m0, pg, pp, demod, ebcast, 1, we, PE, wf, PO, 0, 0,
                                  ck, part);
}
// The magnitude twin: k_bloch_train_run_sched_gn_mag's body; we / wf are two planes (xy, z), PE / PO apart.
__global__ __launch_bounds__(256) void k_bloch_train_lm_sched_run_mag(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp, const BlochCkDev* __restrict__ cks,
    const double* __restrict__ m0, const double* __restrict__ pg, const double* __restrict__ pp, int demod, int ebcast,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, const LmState* __restrict__ st, double* ck,
    double2* __restrict__ part) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    bloch_train_run_sched_gn_body_mag(bk, ws, dws, rep, gidx, rw, pulses, trains, vp, cks, m0, pg, pp, demod, ebcast, 1, we, PE, wf, PO, 0,
                                      0, ck, part);
}

// k_bloch_train_lm_step (blochtrainlm.hip) with H p of repetition k formed as k_bloch_train_sched_gn_fold forms it (chunks, then
// scales, in index order), the half that does not vary masked to exact zero.  One workgroup per pulse, one CG iteration; a pAp that
// is not finite or not > 0 stops the pulse with status 2 and nothing else changed.  The loops stride by 256: any ntr is served.
__global__ __launch_bounds__(256) void k_bloch_train_lm_sched_step(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp_,
                                                                   int nscale, int cg, double rtol, int vg, int vp,
                                                                   double* __restrict__ pg, double* __restrict__ pp,
                                                                   double2* __restrict__ d, double2* __restrict__ r,
                                                                   double2* __restrict__ hp, LmState* __restrict__ st) {
    __shared__ double sw[256];
    const LmState S = st[blockIdx.x];
    if (!S.run) return;
    const VjpPulseDev V = vp_[blockIdx.x];
    double s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        double2 g = make_double2(0, 0);
        for (int sc = 0; sc < nscale; ++sc) {
            double2 a = make_double2(0, 0);
            const double2* rw = part + V.p_off + (long)sc * V.nch * V.n + m;
            for (int c = 0; c < V.nch; ++c) {
                const double2 v = rw[(long)c * V.n];
                a.x += v.x; a.y += v.y;
            }
            g.x += a.x; g.y += a.y;
        }
        const double2 h = make_double2(vg ? g.x : 0.0, vp ? g.y : 0.0);
        const double2 q = make_double2(vg ? pg[t] : 0.0, vp ? pp[t] : 0.0), ap = lm_axpy(S.mu, q, h);
        hp[t] = ap;
        s += lm_redot(q, ap);
    }
    const double pap = lm_block_sum(s, sw);                      // every thread has read S before the sum's barriers
    if (!(pap > 0) || !isfinite(pap)) {
        if (threadIdx.x == 0) { st[blockIdx.x].run = 0; st[blockIdx.x].status = 2; }
        return;
    }
    const double alpha = S.rr / pap;
    s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        const double2 q = make_double2(vg ? pg[t] : 0.0, vp ? pp[t] : 0.0), rn = lm_axpy(-alpha, hp[t], r[t]);
        d[t] = lm_axpy(alpha, q, d[t]);
        r[t] = rn;
        s += lm_redot(rn, rn);
    }
    const double rr = lm_block_sum(s, sw), beta = rr / S.rr;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        const double2 q = make_double2(vg ? pg[t] : 0.0, vp ? pp[t] : 0.0), pn = lm_axpy(beta, q, r[t]);
        if (vg) pg[t] = pn.x;
        if (vp) pp[t] = pn.y;
    }
    if (threadIdx.x == 0) {
        const bool run = lm_goes_on(S.ncg + 1, cg, rr, rtol, S.gg);
        st[blockIdx.x] = LmState{rr, S.gg, S.mu, S.ncg + 1, run ? 1 : 0, rr > rtol * S.gg ? 1 : 0, 0};
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_lm_step_sched_batch (arguments checked by api.cpp): bloch_train_lsq_sched_batch_run's staging through
// the same sched_gn_stage (the forward train, the weights and targets, the descriptors of one direction's partials and checkpoints,
// the fold's table), then b when given and mu; one upload; the launches above; one download.  The output region:
//   d (R double2), the npulse states, [the gradient (R double2), the npulse losses]                                  downloaded
//   r, H p (R double2 each), p (R doubles per varied half), the partials, the loss partials, the primal planes, their tangents in
//   the gain when the gains vary, and the checkpoints of (m, dm), of which the lsq walk uses the first half       stay on the device
void bloch_train_lm_step_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re,
                                         const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                                         const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                         const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                         const double* dy, const double* dz, int nscale, const double* scales, const int* ntr,
                                         const long* roff, const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                         const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                         const double* m0y, const double* m0z, int ebcast, const double* const w[3],
                                         const double* const t[3], const double* rw, const double* const wf[3],
                                         const double* const tf[3], const double* bgain, const double* bphi, const double* mu, int cg,
                                         double rtol, double* dgain, double* dphi, int* ncg, double* rr, double* gg, int* status,
                                         double* loss, double* ggain, double* gphi, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vg = dgain != nullptr, vp = dphi != nullptr, eval = t[0] != nullptr || tf[0] != nullptr;
    const bool echo_w = w[0] != nullptr, fin_w = wf[0] != nullptr;
    SchedGnCall Cl;
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    sched_gn_stage(Cl, npulse, nscale, ntr, roff, ebcast, 1, w, t, rw, wf, tf, mag);      // bloch_train_lsq_sched_batch_run's own staging
    Staging& S = B.S;
    const long O = B.O, R = roff[npulse], PE = Cl.PE, npart = Cl.npart, nck = Cl.nck, nlp = Cl.nlp, nfold = Cl.nfold;
    const size_t o_we = Cl.o_we, o_te = Cl.o_te, o_wf = Cl.o_wf, o_tf = Cl.o_tf, o_rw = Cl.o_rw, o_vp = Cl.o_vp, o_ck = Cl.o_ck;
    const size_t o_lp = Cl.o_lp, o_fb = Cl.o_fb;
    const size_t o_bg = S.add(bgain ? (size_t)R * 8 : 0), o_bp = S.add(bphi ? (size_t)R * 8 : 0), o_mu = S.add((size_t)npulse * 8);
    const size_t o_jb = sim_group_table(S, 1);
    if (bgain) std::copy(bgain, bgain + R, S.at<double>(o_bg));
    if (bphi) std::copy(bphi, bphi + R, S.at<double>(o_bp));
    std::copy(mu, mu + npulse, S.at<double>(o_mu));
    long nwg = 0;                                                         // workgroups of the period's tangent
    const size_t o_qb = vg ? train_jvp_table(Ts, nscale, 1, nwg) : 0;
    auto pad16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t b_vec = (size_t)R * 16, b_st = pad16(npulse * sizeof(LmState)), b_loss = pad16((size_t)npulse * 8);
    const size_t b_half = pad16((size_t)R * 8), b_down = b_vec + b_st + (eval ? b_vec + b_loss : 0);
    const size_t W = (size_t)Ts.W, LP = ((size_t)nlp + 1) & ~size_t(1);
    S.upload(b_down + 2 * b_vec + 2 * b_half + ((size_t)npart * 2 + LP + W + (vg ? W : 0) + 2 * (size_t)nck) * 8, st);
    char* out = S.dev<char>(S.o_out);
    double2* d = reinterpret_cast<double2*>(out);
    LmState* state = reinterpret_cast<LmState*>(out + b_vec);
    double2* grad = reinterpret_cast<double2*>(out + b_vec + b_st);
    double* dloss = reinterpret_cast<double*>(out + 2 * b_vec + b_st);
    double2* r = reinterpret_cast<double2*>(out + b_down);
    double2* hp = r + R;
    double* pg = reinterpret_cast<double*>(hp + R);
    double* pp = reinterpret_cast<double*>(reinterpret_cast<char*>(pg) + b_half);
    double2* part = reinterpret_cast<double2*>(reinterpret_cast<char*>(pp) + b_half);
    double* lpart = reinterpret_cast<double*>(part + npart);
    double* ws = lpart + LP;
    double* dws = vg ? ws + W : nullptr;
    double* ck = ws + W + (vg ? W : 0);
    const VjpPulseDev* vpv = S.dev<const VjpPulseDev>(o_vp);
    const BlochCkDev* ckd = S.dev<const BlochCkDev>(o_ck);
    const BlochPulseDev* pd = S.dev<const BlochPulseDev>(S.o_pd);
    const TrainPulseDev* tr = S.dev<const TrainPulseDev>(Ts.o_tr);
    const double2* rep = S.dev<const double2>(Ts.o_rep);
    const int* gi = S.dev<const int>(Ts.o_gi);
    const double* rwd = rw ? S.dev<const double>(o_rw) : nullptr;
    const double* wed = echo_w ? S.dev<const double>(o_we) : nullptr;
    const double* wfd = fin_w ? S.dev<const double>(o_wf) : nullptr;
    const double* m0d = S.dev<const double>(B.o_m0);
    train_launch_prop(Ts, st, ws);
    if (vg) train_launch_prop_dgain(Ts, st, o_qb, nwg, dws);
    if (eval) {                                                   // bloch_train_lsq_sched_batch_run's two launches
        train_sched_lsq_launch(st, (long)S.nblk, ws, dws, rep, gi, rwd, pd, tr, S.dev<const SimBlock>(S.o_bk), vpv, ckd,
                               S.dev<const long>(o_lp), m0d, demod, ebcast, t[0] ? wed : nullptr,
                               t[0] ? S.dev<const double>(o_te) : nullptr, PE, tf[0] ? wfd : nullptr,
                               tf[0] ? S.dev<const double>(o_tf) : nullptr, O, ck, part, lpart, mag);
        train_sched_gn_fold_launch(st, nfold, part, npart, vpv, S.dev<const SimBlock>(o_fb), nscale, grad, lpart,
                                   S.dev<const long>(o_lp), dloss);
    }
    hipLaunchKernelGGL(k_bloch_train_lm_sched_init, dim3((unsigned)npulse), dim3(256), 0, st, vpv, S.dev<const double>(o_mu), cg, rtol,
                       bgain ? S.dev<const double>(o_bg) : nullptr, bphi ? S.dev<const double>(o_bp) : nullptr, grad, vg ? 1 : 0,
                       vp ? 1 : 0, pg, pp, d, r, state);
    for (int k = 0; k < cg; ++k) {                                // rounds of a pulse that has stopped are early exits
        hipLaunchKernelGGL(mag ? k_bloch_train_lm_sched_run_mag : k_bloch_train_lm_sched_run, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, dws, rep, gi, rwd, pd, tr,
                           S.dev<const SimBlock>(o_jb), vpv, ckd, m0d, vg ? pg : nullptr, vp ? pp : nullptr, demod, ebcast, wed, PE,
                           wfd, O, state, ck, part);
        hipLaunchKernelGGL(k_bloch_train_lm_sched_step, dim3((unsigned)npulse), dim3(256), 0, st, part, vpv, nscale, cg, rtol,
                           vg ? 1 : 0, vp ? 1 : 0, pg, pp, d, r, hp, state);
    }
    std::vector<char> h(b_down);
    S.download(h.data(), b_down, st);
    const double* hd = reinterpret_cast<const double*>(h.data());
    for (long k = 0; k < R; ++k) {
        if (dgain) dgain[k] = hd[2 * k];
        if (dphi) dphi[k] = hd[2 * k + 1];
    }
    const LmState* hs = reinterpret_cast<const LmState*>(h.data() + b_vec);
    for (int q = 0; q < npulse; ++q) {
        rr[q] = hs[q].rr; gg[q] = hs[q].gg;
        ncg[q] = hs[q].ncg; status[q] = hs[q].status;
    }
    if (eval) {
        const double* hg = reinterpret_cast<const double*>(h.data() + b_vec + b_st);
        for (long k = 0; k < R; ++k) {
            if (ggain) ggain[k] = hg[2 * k];
            if (gphi) gphi[k] = hg[2 * k + 1];
        }
        std::copy(reinterpret_cast<const double*>(h.data() + 2 * b_vec + b_st),
                  reinterpret_cast<const double*>(h.data() + 2 * b_vec + b_st) + npulse, loss);
    }
}

}  // namespace mbfir
