// The Levenberg-Marquardt step of the pulse train solved on the device, the train's twin of blochgn.hip's (8s) and
// blochssgn.hip's (8v): conjugate gradients on (H + mu I) d = b per pulse from d = 0, H = J' W J as bloch_train_gn_batch applies it
// (echo term, rep_weights, final term, the scales' and gains' chain rule); then, with targets, the loss and gradient of
// bloch_train_lsq_batch at b1 + d.  One upload, a chain of launches ordered by the stream, one download; the host reads nothing in
// between.  b1 is fixed within a solve, so what depends on b1 alone runs once per call:
//   k_bloch_train_prop (shipped)  the primal planes
//   k_bloch_train_lm_prep         the forward half of k_bloch_train_prop_vjp: the checkpoints of the primal columns
// and a round, over the pulses whose LmState.run is set (a workgroup of a stopped pulse returns at once), is
//   k_bloch_train_lm_jvp          k_bloch_train_prop_jvp's body along the device's own p (laid out as b1 is: the ndir = 1 layout)
//   k_bloch_train_lm_run          k_bloch_train_run_gn's body at one direction, on cotangent planes zeroed before every round
//   k_bloch_train_lm_pvjp         the backward half of k_bloch_train_prop_vjp on the checkpoints the prep left
//   k_bloch_train_lm_step         k_bloch_lm_step with H p of sample t formed as k_bloch_train_gn_fold forms it
// The bodies are sim_dev.h's, which the shipped kernels call too, so H p has the bits of the shipped product.  The trial launches
// the shipped kernels in bloch_train_lsq_batch_run's order on the rows at b1 + d.  No atomics.  The tangent planes, the cotangent
// planes, the partials and the checkpoints are those of one direction, reused by every round and by the trial.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// blocks: the period adjoint's table (pulse, combination, chunk of 64 points).  Writes the checkpoints of the primal columns into
// the period adjoint's checkpoint region ck and nothing else.
__global__ __launch_bounds__(256) void k_bloch_train_lm_prep(const double* __restrict__ in, const double* __restrict__ df,
                                                             const double* __restrict__ pos3, const double* __restrict__ amp,
                                                             const BlochPulseDev* __restrict__ pulses,
                                                             const TrainPulseDev* __restrict__ trains,
                                                             const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                             const BlochCkDev* __restrict__ cks, const LmState* __restrict__ st,
                                                             double2* __restrict__ part, double* ck) {
    __shared__ double sst[BLOCH_CH][8];
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    // part: the period adjoint's partials, for the thread's descriptor alone; the forward half does not touch them
    const TrainPropVjpThread C = bloch_train_prop_vjp_thread(bk, df, pos3, amp, pulses, trains, vp, cks, part, ck);
    bloch_train_prop_vjp_forward(C, sst, in);
}

// blocks: the period tangent's table at one direction.  v: the device's p; dws receives the tangent planes.
__global__ __launch_bounds__(256) void k_bloch_train_lm_jvp(const double* __restrict__ in, const double* __restrict__ df,
                                                            const double* __restrict__ pos3, const double* __restrict__ amp,
                                                            const BlochPulseDev* __restrict__ pulses,
                                                            const TrainPulseDev* __restrict__ trains,
                                                            const SimBlock* __restrict__ blocks, const double2* __restrict__ v,
                                                            const LmState* __restrict__ st, double* __restrict__ dws) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    bloch_train_prop_jvp_body(bk, in, df, pos3, amp, pulses, trains, v, 1, dws);
}

// blocks: the forward table at one direction.  cw: the cotangent planes, zero on entry.
__global__ __launch_bounds__(256) void k_bloch_train_lm_run(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0, int demod, int ebcast,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, const LmState* __restrict__ st, double* ck,
    double* cw) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    bloch_train_run_gn_body(bk, ws, dws, rep, gidx, rw, pulses, trains, cks, m0, demod, ebcast, 1, we, PE, wf, PO, 0, 0, ck, cw);
}
// The magnitude twin: k_bloch_train_run_gn_mag's body; we / wf are two planes (xy, z), PE / PO apart.
__global__ __launch_bounds__(256) void k_bloch_train_lm_run_mag(
    const double* __restrict__ ws, const double* __restrict__ dws, const double2* __restrict__ rep, const int* __restrict__ gidx,
    const double* __restrict__ rw, const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains,
    const SimBlock* __restrict__ blocks, const BlochCkDev* __restrict__ cks, const double* __restrict__ m0, int demod, int ebcast,
    const double* __restrict__ we, long PE, const double* __restrict__ wf, long PO, const LmState* __restrict__ st, double* ck,
    double* cw) {
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    bloch_train_run_gn_body_mag(bk, ws, dws, rep, gidx, rw, pulses, trains, cks, m0, demod, ebcast, 1, we, PE, wf, PO, 0, 0, ck, cw);
}

// blocks, cw, part, ck: k_bloch_train_prop_vjp's; ck holds the checkpoints of k_bloch_train_lm_prep.
__global__ __launch_bounds__(256) void k_bloch_train_lm_pvjp(const double* __restrict__ in, const double* __restrict__ df,
                                                             const double* __restrict__ pos3, const double* __restrict__ amp,
                                                             const BlochPulseDev* __restrict__ pulses,
                                                             const TrainPulseDev* __restrict__ trains,
                                                             const SimBlock* __restrict__ blocks, const VjpPulseDev* __restrict__ vp,
                                                             const BlochCkDev* __restrict__ cks, const double* __restrict__ cw,
                                                             const LmState* __restrict__ st, double2* __restrict__ part, double* ck) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double red[2 * VJP_T * VJP_ROW];
    const SimBlock bk = blocks[blockIdx.x];
    if (!st[bk.pulse].run) return;                               // uniform over the workgroup, written by an earlier launch
    const TrainPropVjpThread C = bloch_train_prop_vjp_thread(bk, df, pos3, amp, pulses, trains, vp, cks, part, ck);
    double l[3] = {0, 0, 0}, le[3] = {0, 0, 0};
    bloch_train_prop_vjp_seed(C, bk, cw, l, le);
    const int tlast = (C.ntime - 1) / BLOCH_CH * BLOCH_CH;       // the tile the forward half would have left staged
    bloch_ss_stage(sst, in, C.P.t_off, C.ntime, tlast, C.sc, C.gamma);
    bloch_train_prop_vjp_backward(C, sst, red, in, l, le);
}

// k_bloch_lm_step (blochgn.hip) with H p of sample t formed as k_bloch_train_gn_fold forms it: abr_vjp_fold_sum over the pulse's
// nscale ngain combinations with amp + a_off, then f = gamma dt_t.  One workgroup per pulse, one CG iteration; a pAp that is not
// finite or not > 0 stops the pulse with status 2 and nothing else changed.
__global__ __launch_bounds__(256) void k_bloch_train_lm_step(const double2* __restrict__ part, const VjpPulseDev* __restrict__ vp,
                                                             const double* __restrict__ amp, const TrainPulseDev* __restrict__ trains,
                                                             int nscale, const double* __restrict__ in,
                                                             const BlochPulseDev* __restrict__ pulses, int cg, double rtol,
                                                             double2* __restrict__ p, double2* __restrict__ d,
                                                             double2* __restrict__ r, double2* __restrict__ hp,
                                                             LmState* __restrict__ st) {
    __shared__ double sw[256];
    const LmState S = st[blockIdx.x];
    if (!S.run) return;
    const VjpPulseDev V = vp[blockIdx.x];
    const BlochPulseDev P = pulses[blockIdx.x];
    const TrainPulseDev Tr = trains[blockIdx.x];
    double s = 0;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const double2 g = abr_vjp_fold_sum(part, V, amp + Tr.a_off, nscale * Tr.ngain, m);
        const double f = P.gamma * in[BLOCH_IN * (V.r_off + m) + 8];
        const double2 h = make_double2(-(f * g.x), f * g.y), q = p[V.r_off + m], ap = lm_axpy(S.mu, q, h);
        hp[V.r_off + m] = ap;
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
        const double2 q = p[t], rn = lm_axpy(-alpha, hp[t], r[t]);
        d[t] = lm_axpy(alpha, q, d[t]);
        r[t] = rn;
        s += lm_redot(rn, rn);
    }
    const double rr = lm_block_sum(s, sw), beta = rr / S.rr;
    for (int m = threadIdx.x; m < V.n; m += 256) {
        const long t = V.r_off + m;
        p[t] = lm_axpy(beta, p[t], r[t]);
    }
    if (threadIdx.x == 0) {
        const bool run = lm_goes_on(S.ncg + 1, cg, rr, rtol, S.gg);
        st[blockIdx.x] = LmState{rr, S.gg, S.mu, S.ncg + 1, run ? 1 : 0, rr > rtol * S.gg ? 1 : 0, 0};
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_lm_step_batch (arguments checked by api.cpp): the staging of bloch_train_gn_batch_run at ndir = 1
// with b as the direction section, which is the device's p from then on, the targets when given, and mu; one upload; k_lm_init,
// k_bloch_train_prop, k_bloch_train_lm_prep, cg rounds of (memset, jvp, run, pvjp, step) and, with targets, the trial; one download.
// The output region:
//   d (T double2), the npulse states, [the gradient at b1 + d (T double2), the npulse losses]                       downloaded
//   r, hp (T double2 each), the trial rows (9 T doubles), the primal planes, one direction's tangent planes, cotangent planes,
//   partials, loss partials and the two kernels' checkpoints                                                        stay on the device
void bloch_train_lm_step_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                   const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                   const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                   const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                   int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                   const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                   const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z, int ebcast,
                                   const double* const w[3], const double* rw, const double* const wf[3], const double* b_re,
                                   const double* b_im, const double* mu, int cg, double rtol, const double* const t[3],
                                   const double* const tf[3], double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                                   int* status, double* loss, double* g_re, double* g_im, bool mag) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool trial = t[0] != nullptr || tf[0] != nullptr;
    TrainGnCall Cl;
    TrainStaged& Ts = Cl.Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    train_gn_stage(Cl, npulse, toff, nscale, ntr, roff, ebcast, 1, w, t, rw, wf, tf, mag);
    Staging& S = B.S;
    const TrainVjpSections& V = Cl.V;
    const long O = B.O, T = toff[npulse];
    const size_t o_v = S.add((size_t)T * 16), o_jb = sim_group_table(S, 1), o_mu = S.add((size_t)npulse * 8);
    pack_cplx(T, b_re, b_im, S.at<double2>(o_v));
    std::copy(mu, mu + npulse, S.at<double>(o_mu));
    long nwq = 0;
    const size_t o_qb = train_jvp_table(Ts, nscale, 1, nwq);
    auto pad16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t b_vec = (size_t)T * 16, b_st = pad16(npulse * sizeof(LmState)), b_loss = pad16((size_t)npulse * 8);
    const size_t b_down = b_vec + b_st + (trial ? b_vec + b_loss : 0), b_rows = pad16((size_t)T * BLOCH_IN * 8);
    const size_t W = (size_t)Ts.W, LP = ((size_t)Cl.nlp + 1) & ~size_t(1);
    S.upload(b_down + 2 * b_vec + b_rows + (3 * W + (size_t)V.npart * 2 + LP + 2 * (size_t)V.nckr + (size_t)V.nckp) * 8, st);
    char* out = S.dev<char>(S.o_out);
    double2* d = reinterpret_cast<double2*>(out);
    LmState* state = reinterpret_cast<LmState*>(out + b_vec);
    double2* grad = reinterpret_cast<double2*>(out + b_vec + b_st);
    double* dloss = reinterpret_cast<double*>(out + 2 * b_vec + b_st);
    double2* r = reinterpret_cast<double2*>(out + b_down);
    double2* hp = r + T;
    double* rows = reinterpret_cast<double*>(hp + T);
    double* ws = reinterpret_cast<double*>(reinterpret_cast<char*>(rows) + b_rows);
    double* dws = ws + W;
    double* cw = dws + W;
    double2* part = reinterpret_cast<double2*>(cw + W);
    double* lpart = reinterpret_cast<double*>(part + V.npart);
    double* ck1 = lpart + LP;
    double* ck2 = ck1 + 2 * (size_t)V.nckr;
    double2* p = S.dev<double2>(o_v);
    const VjpPulseDev* vp = S.dev<const VjpPulseDev>(V.o_vp);
    const double* in = S.dev<const double>(B.o_in);
    const double* ddf = S.dev<const double>(B.o_df);
    const double* dpos = S.dev<const double>(B.o_pos);
    const double* amp = S.dev<const double>(Ts.o_amp);
    const BlochPulseDev* pd = S.dev<const BlochPulseDev>(S.o_pd);
    const TrainPulseDev* tr = S.dev<const TrainPulseDev>(Ts.o_tr);
    const SimBlock* vb = S.dev<const SimBlock>(V.o_vb);
    const BlochCkDev* ckp = S.dev<const BlochCkDev>(V.o_ckp);
    const bool has_e = w[0] != nullptr, has_f = wf[0] != nullptr, has_rw = rw != nullptr;
    lm_init_launch(st, npulse, vp, S.dev<const double>(o_mu), cg, rtol, p, d, r, state);
    train_launch_prop(Ts, st, ws);
    hipLaunchKernelGGL(k_bloch_train_lm_prep, dim3((unsigned)V.nwg), dim3(256), 0, st, in, ddf, dpos, amp, pd, tr, vb, vp, ckp, state,
                       part, ck2);                                      // no pulse runs (cg = 0, or rtol met at once): every workgroup returns
    for (int k = 0; k < cg; ++k) {                                // rounds of a pulse that has stopped are early exits
        MBFIR_HIP(hipMemsetAsync(cw, 0, W * 8, st));              // the walk accumulates into the cotangent planes
        hipLaunchKernelGGL(k_bloch_train_lm_jvp, dim3((unsigned)nwq), dim3(256), 0, st, in, ddf, dpos, amp, pd, tr,
                           S.dev<const SimBlock>(o_qb), p, state, dws);
        hipLaunchKernelGGL(mag ? k_bloch_train_lm_run_mag : k_bloch_train_lm_run, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, dws, S.dev<const double2>(Ts.o_rep),
                           S.dev<const int>(Ts.o_gi), has_rw ? S.dev<const double>(Cl.o_rw) : nullptr, pd, tr,
                           S.dev<const SimBlock>(o_jb), S.dev<const BlochCkDev>(V.o_ckr), S.dev<const double>(B.o_m0), demod, ebcast,
                           has_e ? S.dev<const double>(Cl.o_we) : nullptr, Cl.PE, has_f ? S.dev<const double>(Cl.o_wf) : nullptr, O,
                           state, ck1, cw);
        hipLaunchKernelGGL(k_bloch_train_lm_pvjp, dim3((unsigned)V.nwg), dim3(256), 0, st, in, ddf, dpos, amp, pd, tr, vb, vp, ckp, cw,
                           state, part, ck2);
        hipLaunchKernelGGL(k_bloch_train_lm_step, dim3((unsigned)npulse), dim3(256), 0, st, part, vp, amp, tr, nscale, in, pd, cg, rtol,
                           p, d, r, hp, state);
    }
    if (trial) {                                                  // bloch_train_lsq_batch_run's launches on the rows at b1 + d
        bloch_lm_trial_launch(st, in, d, T, rows);
        MBFIR_HIP(hipMemsetAsync(cw, 0, W * 8, st));
        train_launch_prop(Ts, st, ws, rows);
        train_launch_run_lsq(Cl, st, demod, ebcast, has_e, has_rw, has_f, ws, ck1, cw, nullptr, lpart);
        train_launch_prop_vjp(Ts, V, st, cw, part, ck2, rows);
        train_launch_lsq_fold(Cl, st, nscale, part, rows, grad, lpart, dloss);
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
