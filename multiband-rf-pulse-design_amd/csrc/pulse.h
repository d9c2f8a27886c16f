// Host side of the pulse tools (slr.hip, simgrad.hip, simgradg.hip, simjvp.hip, simgn.hip, blochgrad.hip, flip.hip, remez.hip, specfact.hip): RF-pulse operations beside the conic solver, called by
// api.cpp with its arguments checked.  Every runner takes host arrays in and out, makes `device` current first, runs on `stream`
// (a hipStream_t), returns once the results are on the host, and throws HipError.  No HIP headers: api.cpp is built by the host
// compiler.
#pragma once

namespace mbfir {

// Inverse SLR (slr.hip; b2a.m:15-32, ab2rf.m:14-29).  b: n complex taps.  a_in null: a = b2a(b), else a = a_in.
// a_out (optional) receives a; rf (optional) receives ab2rf(a, b), n <= 2048.
void slr_run(int device, void* stream, int n, const double* b_re, const double* b_im, const double* a_in_re, const double* a_in_im,
             double* a_re, double* a_im, double* rf_re, double* rf_im);
// Batched inverse SLR (slr.hip k_b2rf_batch): count x n row-major planes in and out (b_im may be null), 2 <= n <= 2048, count >= 1;
// one workgroup per polynomial, one launch.
void slr_b2rf_batch_run(int device, void* stream, int n, int count, const double* b_re, const double* b_im, double* rf_re,
                        double* rf_im);
// 2D inverse SLR (slr.hip k_b2rf_batch, k_slr2d_mid, k_slr2d_out; dzepse.m:39-49): count x m x n row-major planes in and out
// (r_im may be null), 2 <= m, n <= 2048, m even; one upload, one download.  literal: dzepse.m's sin(conj(theta) / 2) middle stage.
void slr_slr2d_batch_run(int device, void* stream, int m, int n, int count, const double* r_re, const double* r_im, double* out_re,
                         double* out_im, int literal);
// Work split of the batched simulators (slr.hip k_bloch_batch, k_abr_batch, k_abr2_batch): one 256-thread workgroup per (pulse, scale, chunk of
// 256 points); pulses in descending order of ntime (ties in list order), then scale, then chunk.  npoint: points per pulse
// ((frequency, position) pairs, positions, or (x, y) points).  Returns the table's length; writes the table to out when out is not null.
struct SimBlock {
    int pulse, scale, chunk, pad;
};
long sim_block_table(int npulse, const int* ntime, const long* npoint, int nscale, SimBlock* out);
// Bloch simulation with relaxation (slr.hip k_bloch_batch; blochC.c:422-512) and forward simulation (k_abr_batch; g null = 2 pi / n
// per sample; mode 0 abrm.m, 1 hard pulse): P pulses x S scales, one upload, one launch, one download.  Offsets and layouts as
// mbfir_bloch_batch / mbfir_abr_batch document them (include/mbfir.h).  m*: in = initial magnetisation at the first sample of
// every (scale, frequency, position) block, out = the result.  mbfir_bloch and mbfir_abr call these with one pulse at scale 1.0.
void bloch_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                     const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                     const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                     const double* dx, const double* dy, const double* dz, int nscale, const double* scales, int mode, double* mx,
                     double* my, double* mz);
void abr_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                   int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, double* a_re,
                   double* a_im, double* b_re, double* b_im);
// 2D forward simulation (slr.hip k_abr2_batch, abrm.m:39-57): a, b at (x_k, y_j) -> index k ny + j for every (pulse, scale); gx null
// = 2 pi / n, gy null = 0; mode 0 abrm.m, 1 the hard-pulse model with the precession angle x gx + y gy.  Offsets and layout as
// mbfir_abr2_batch documents them; sim_block_table's npoint is nx ny.  mbfir_abr2 calls it with one pulse at scale 1.0.
void abr2_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                    const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff, const double* y,
                    int nscale, const double* scales, int mode, double* a_re, double* a_im, double* b_re, double* b_im);
// Adjoints of abr_batch_run / abr2_batch_run with respect to rf (simgrad.hip k_abr_vjp_batch, k_abr2_vjp_batch, k_abr_vjp_fold): the
// forward call's inputs; c*: the cotangents of a and b in the forward outputs' layout (dL = Re(conj(ca) da + conj(cb) db)); g_re /
// g_im: dL / d Re rf, dL / d Im rf per rf sample, summed over the pulse's points and scales.  One upload, two launches, one download.
void abr_vjp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                       const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im, double* g_re,
                       double* g_im);
void abr2_vjp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                        const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                        const long* yoff, const double* y, int nscale, const double* scales, int mode, const double* ca_re,
                        const double* ca_im, const double* cb_re, const double* cb_im, double* g_re, double* g_im);
// Adjoint of bloch_batch_run's end point (mode 0) with respect to b1 and the initial magnetisation (blochgrad.hip k_bloch_vjp_batch,
// k_bloch_vjp_fold): the forward call's inputs; m0*: the initial magnetisation in the layout of the mode-0 outputs (all null: [0 0
// 1]); cm*: the cotangents of mx / my / mz in that layout; g_re / g_im: dL / d Re b1, dL / d Im b1 per sample, summed over the
// pulse's points and scales; gm0*: dL / d m0 per (scale, frequency, position) (all null: not downloaded).  One upload, two launches,
// one download.
void bloch_vjp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                         const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                         const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                         int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                         const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* cmx,
                         const double* cmy, const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y,
                         double* gm0z);
// bloch_vjp_batch_run plus the adjoint with respect to the gradient waveform and the off-resonance (blochgradg.hip
// k_bloch_vjp_gr_batch, k_bloch_vjp_gr_fold): ggx / ggy / ggz: dL / d gx, gy, gz per sample, laid out as gx / gy / gz, summed over
// the pulse's points and scales without a factor (a null gx / gy / gz is differentiated at zero); gdf: dL / d df per (scale,
// frequency, position) in gm0x's layout (null: not formed).  One upload, two launches, one download.
void bloch_vjp_gr_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* cmx,
                            const double* cmy, const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y,
                            double* gm0z, double* ggx, double* ggy, double* ggz, double* gdf);
// Tangent of bloch_batch_run's end point (mode 0) with respect to b1 and the initial magnetisation (blochjvp.hip k_bloch_jvp_batch):
// the forward call's inputs and m0* as above; ndir >= 1 directions per pulse, direction k of pulse p at ndir toff[p] + k n_p of v_re
// / v_im; dm0*: the m0 directions, pulse p from ndir times its forward output offset, (direction, scale, point) row-major (all
// null: zero); m*: the forward call's outputs with its bits (all null: not downloaded); dm*: laid out as dm0.  One upload, one
// launch of bloch_jvp_group() directions per workgroup, one download.
int bloch_jvp_group();
void bloch_jvp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                         const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                         const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                         int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                         const double* scales, const double* m0x, const double* m0y, const double* m0z, int ndir, const double* v_re,
                         const double* v_im, const double* dm0x, const double* dm0y, const double* dm0z, double* mx, double* my,
                         double* mz, double* dmx, double* dmy, double* dmz);
// Adjoint and tangent of bloch_batch_run's steady state (mode 1) with respect to b1 (blochss.hip k_bloch_ss_vjp_batch,
// k_bloch_ss_jvp_batch): the forward call's inputs; cm*: the cotangents of the mode-1 outputs in their layout; g_re /
// g_im as above; m*: the steady state with mode 1's bits (all null: not downloaded); v, dm*: as bloch_jvp_batch_run's.  There is no
// m0: the steady state does not depend on it.  The adjoint: one upload, two launches (the second is k_bloch_vjp_fold), one
// download; the tangent: one upload, one launch of bloch_ss_jvp_group() directions per workgroup, one download.
void bloch_ss_vjp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* cmx, const double* cmy, const double* cmz, double* g_re, double* g_im,
                            double* mx, double* my, double* mz);
// bloch_ss_vjp_batch_run plus the adjoint with respect to the gradient waveform and the off-resonance (blochssg.hip
// k_bloch_ss_vjp_gr_batch, with blochgradg.hip's k_bloch_vjp_gr_fold): ggx / ggy / ggz and gdf as
// bloch_vjp_gr_batch_run's, gdf in the cotangents' layout (null: not formed).  One upload, two launches, one download.
void bloch_ss_vjp_gr_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                               const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                               int nscale, const double* scales, const double* cmx, const double* cmy, const double* cmz,
                               double* g_re, double* g_im, double* mx, double* my, double* mz, double* ggx, double* ggy, double* ggz,
                               double* gdf);
int bloch_ss_jvp_group();
void bloch_ss_jvp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, int ndir, const double* v_re, const double* v_im, double* mx, double* my,
                            double* mz, double* dmx, double* dmy, double* dmz);
// The echo-by-echo transient of a pulse train (blochtrain.hip k_bloch_train_prop, k_bloch_train_run): the forward call's
// inputs, each pulse one period; per pulse ntr repetitions whose (cos phi, sin phi, gain index) lie at roff[p] .. of cosphi /
// sinphi / gidx, its distinct gains at goff[p] .. goff[p + 1] - 1 of gains, the echo sample and meq; m0* as bloch_vjp_batch_run's;
// e*: the echoes, S x ntr x nf x npos per pulse (all null: not downloaded); f*: m after the last repetition in the layout of the
// mode-0 outputs (all null: not downloaded).  One upload, two launches, one download.  bloch_prop_batch_run is the first launch
// alone at gain 1: a / ae (9, column-major) and b / be (3) per (scale, frequency, position), pulse p from 9 (or 3) times its mode-0
// output offset.
void bloch_train_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                           const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                           const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                           int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                           const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                           const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                           const double* m0x, const double* m0y, const double* m0z, double* ex, double* ey, double* ez, double* fx,
                           double* fy, double* fz);
void bloch_prop_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                          const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                          const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                          int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                          const double* scales, const int* echo, double* a, double* b, double* ae, double* be);
// Adjoint of bloch_train_batch_run with respect to b1 and m0 (blochtrainvjp.hip k_bloch_train_run_vjp, k_bloch_train_prop_vjp,
// k_bloch_train_vjp_fold after blochtrain.hip's k_bloch_train_prop): the forward call's inputs, the cotangents of the
// echoes (ce*: all null = none) and of the final state (cf*: all null = none) where the forward call writes them; g_*: the gradient
// per b1 sample; gm*: dL / d m0 in the final planes' layout (all null: not downloaded).  One upload, four launches, one download.
void bloch_train_vjp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                               int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                               const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                               const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                               const double* m0x, const double* m0y, const double* m0z, const double* cex, const double* cey,
                               const double* cez, const double* cfx, const double* cfy, const double* cfz, double* g_re, double* g_im,
                               double* gmx, double* gmy, double* gmz);
// bloch_train_vjp_batch_run plus the adjoint with respect to the gradient waveform and the off-resonance (blochtrainvjpg.hip
// k_bloch_train_prop_vjp_gr, k_bloch_train_vjp_gr_fold, k_bloch_train_vjp_df_fold after the shipped k_bloch_train_prop and
// k_bloch_train_run_vjp): ggx / ggy / ggz: dL / d gx, gy, gz per sample of the period, laid out as gx / gy / gz, summed
// over the points, the scales and the gains without a factor (a null gx / gy / gz is differentiated at zero); gdf: dL / d df per
// (scale, frequency, position) in the final planes' layout, summed over the scale's distinct gains (null: not formed).  One upload,
// four launches (five with gdf), one download.
void bloch_train_vjp_gr_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                  const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                  const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                  const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                  int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                  const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                  const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                  const double* cex, const double* cey, const double* cez, const double* cfx, const double* cfy,
                                  const double* cfz, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz, double* ggx,
                                  double* ggy, double* ggz, double* gdf);
// Adjoint of bloch_train_batch_run with respect to the gain and the RF phase of every repetition (blochtrainsched.hip
// k_bloch_train_prop_dgain, k_bloch_train_run_sched, k_bloch_train_sched_fold after blochtrain.hip's k_bloch_train_prop):
// bloch_train_vjp_batch_run's inputs; ggain / gphi: one entry per repetition, laid out as cosphi (either null: not wanted, not
// both); gm*: dL / d m0 with bloch_train_vjp_batch_run's bits (all null: not downloaded).  One upload, three launches and the fold
// (two when ggain is null), one download.
void bloch_train_vjp_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, const double* cex, const double* cey, const double* cez, const double* cfx,
                                     const double* cfy, const double* cfz, double* ggain, double* gphi, double* gmx, double* gmy,
                                     double* gmz);
// Tangent of bloch_train_batch_run with respect to b1 and m0 (blochtrainjvp.hip k_bloch_train_prop_jvp, k_bloch_train_run_jvp after
// blochtrain.hip's k_bloch_train_prop): the forward call's inputs; ndir >= 1 directions per pulse, v and dm0* as
// bloch_jvp_batch_run's; e* / f*: the forward call's outputs with its bits (either triple all null: not downloaded); de*: the
// tangent echoes, pulse p from ndir times its echo offset, (direction, scale, repetition, point) row-major; df*: the tangent of the
// final state, laid out as dm0 (either triple all null: not wanted, not both).  One upload, three launches, one download.
// bloch_train_jvp_group(0 / 1): the directions one workgroup of the period's / the repetitions' kernel carries.
int bloch_train_jvp_group(int which);
void bloch_train_jvp_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                               int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                               const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                               const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                               const double* m0x, const double* m0y, const double* m0z, int ndir, const double* v_re,
                               const double* v_im, const double* dm0x, const double* dm0y, const double* dm0z, double* ex, double* ey,
                               double* ez, double* fx, double* fy, double* fz, double* dex, double* dey, double* dez, double* dfx,
                               double* dfy, double* dfz);
// Tangent of bloch_train_batch_run with respect to the gain and the RF phase of every repetition and to m0 (blochtrainschedjvp.hip
// k_bloch_train_run_sched_jvp after blochtrain.hip's k_bloch_train_prop and blochtrainsched.hip's k_bloch_train_prop_dgain; DESIGN
// 8ae): bloch_train_jvp_batch_run's arguments with dgain / dphi in place of v: direction k of pulse p at ndir roff[p] + k ntr_p
// (either null: that part does not move).  One upload, three launches (two when dgain is null), one download.
// bloch_train_sched_jvp_group(): the directions one workgroup of the repetitions' kernel carries.
int bloch_train_sched_jvp_group();
void bloch_train_jvp_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, int ndir, const double* dgain, const double* dphi, const double* dm0x,
                                     const double* dm0y, const double* dm0z, double* ex, double* ey, double* ez, double* fx, double* fy,
                                     double* fz, double* dex, double* dey, double* dez, double* dfx, double* dfy, double* dfz);
// Fused least-squares and Gauss-Newton products of bloch_train_batch_run (blochtraingn.hip k_bloch_train_run_lsq,
// k_bloch_train_run_gn, k_bloch_train_gn_fold with the shipped k_bloch_train_prop, k_bloch_train_prop_jvp and k_bloch_train_prop_vjp;
// DESIGN 8ab): the forward call's inputs; w / t: the echo weights and targets (w[0] null: no echo term), laid out as the echoes
// (ebcast 0) or as the final planes and used at every repetition (ebcast 1); rw (null: ones): one factor per repetition, laid out as
// cosphi; wf / tf: the final weights and targets (wf[0] null: no final term).  lsq: loss per pulse, the gradient per b1 sample,
// gm* = dL / dm0 (all null: not downloaded).  gn: ndir directions per pulse as bloch_train_jvp_batch_run takes them, h_* = J' W J v
// in the same layout.  One upload, one download; nothing echo-sized comes down.
// mag (here, in the schedule's two calls and in the two train steps below): the magnitude fits of (|Mxy|, mz) per echo
// and at the final state, by the kernels' _mag twins; w, t, wf and tf hold pairs (xy, z) in their first two entries.
void bloch_train_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                               int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                               const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                               const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                               const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* const w[3],
                               const double* const t[3], const double* rw, const double* const wf[3], const double* const tf[3],
                               double* loss, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz, bool mag = false);
void bloch_train_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                              const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                              const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                              int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                              const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                              const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                              const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* const w[3],
                              const double* rw, const double* const wf[3], int ndir, const double* v_re, const double* v_im,
                              double* h_re, double* h_im, bool mag = false);
// Fused least-squares and Gauss-Newton products of bloch_train_batch_run in its schedule, the gain and the RF phase of every
// repetition (blochtrainschedgn.hip k_bloch_train_run_sched_lsq, k_bloch_train_run_sched_gn, k_bloch_train_sched_gn_fold with the
// shipped k_bloch_train_prop and k_bloch_train_prop_dgain): the inputs, weights and targets of bloch_train_lsq_batch_run /
// bloch_train_gn_batch_run.  lsq: loss per pulse, ggain / gphi per repetition (either null: not wanted), dL/dm0 when wanted; gn:
// dgain / dphi (either null: zeros) and hgain / hphi (either null: not wanted), direction k of pulse p at ndir roff[p] + k ntr_p.
// One upload, three launches and the fold (the period's tangent is skipped when no gains half is given or wanted), one download.
void bloch_train_lsq_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, int ebcast, const double* const w[3], const double* const t[3],
                                     const double* rw, const double* const wf[3], const double* const tf[3], double* loss,
                                     double* ggain, double* gphi, double* gmx, double* gmy, double* gmz, bool mag = false);
void bloch_train_gn_sched_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                    const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                    const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                    const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                    const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                    const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                    const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                    const double* m0z, int ebcast, const double* const w[3], const double* rw,
                                    const double* const wf[3], int ndir, const double* dgain, const double* dphi, double* hgain,
                                    double* hphi, bool mag = false);
// Least-squares products of bloch_batch_run's steady state (mode 1; blochssgn.hip k_bloch_ss_lsq_batch, k_bloch_ss_gn_batch, with
// blochgn.hip's k_bloch_gn_fold): the forward call's inputs (no m0), the weights and the targets or the ndir directions in
// the mode-1 outputs' layout, as bloch_lsq_batch_run / bloch_gn_batch_run take them.  lsq: loss per pulse, the gradient per b1
// sample and, when wanted, the steady state with mode 1's bits (m* all null: not downloaded); gn: sum_s s J_s' W_s J_s (s v).  One
// upload, two launches, one download.
void bloch_ss_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* wx, const double* wy, const double* wz, const double* tx,
                            const double* ty, const double* tz, double* loss, double* g_re, double* g_im, double* mx, double* my,
                            double* mz, bool mag = false);
void bloch_ss_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                           const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                           const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                           int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                           const double* scales, const double* wx, const double* wy, const double* wz, int ndir, const double* v_re,
                           const double* v_im, double* h_re, double* h_im, bool mag = false);
// Adjoints with respect to rf and to the gradient waveform (simgradg.hip k_abr_vjp_rfg_batch, k_abr2_vjp_rfg_batch,
// k_abr_vjp_rfg_fold): as the calls above, plus gg (1D) or ggx / ggy (2D): dL / d g per rf sample, laid out as g, summed over the
// pulse's points and scales (no factor s: a scale multiplies rf).  A null g / gx / gy differentiates at its default.
void abr_vjp_rfg_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                           const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales,
                           int mode, const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im,
                           double* g_re, double* g_im, double* gg);
void abr2_vjp_rfg_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                            const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                            const long* yoff, const double* y, int nscale, const double* scales, int mode, const double* ca_re,
                            const double* ca_im, const double* cb_re, const double* cb_im, double* g_re, double* g_im,
                            double* ggx, double* ggy);
// Tangents of abr_batch_run / abr2_batch_run with respect to rf (simjvp.hip k_abr_jvp_batch, k_abr2_jvp_batch): the forward call's
// inputs and ndir >= 1 directions per pulse, direction k of pulse p at ndir roff[p] + k n_p of v_re / v_im.  a / b: the forward
// call's outputs with its bits (all four null: not downloaded); da / db: pulse p from ndir times its forward offset, (direction,
// scale, point) row-major.  One upload, one launch of jvp_group() directions per workgroup, one download.
int jvp_group();
void abr_jvp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                       int ndir, const double* v_re, const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im,
                       double* da_re, double* da_im, double* db_re, double* db_im);
void abr2_jvp_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                        const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                        const long* yoff, const double* y, int nscale, const double* scales, int mode, int ndir, const double* v_re,
                        const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im, double* da_re, double* da_im,
                        double* db_re, double* db_im);
// Least-squares products of abr_batch_run / abr2_batch_run (simgn.hip k_abr_lsq_batch, k_abr_gn_batch, their 2D twins, k_abr_gn_fold):
// the forward call's inputs, the profile (0 ex, 1 se, 2 inv, 3 st), the weights and the targets (t_im may be null) or the ndir
// directions (as abr_jvp_batch_run takes them) in the forward outputs' layout.  lsq: loss per pulse and the gradient per rf sample;
// gn: J^H W J v, pulse p from ndir roff[p], direction-major.  One upload, two launches, one download of rf size.
void abr_lsq_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                       int profile, const double* w, const double* t_re, const double* t_im, double* loss, double* g_re,
                       double* g_im);
void abr2_lsq_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                        const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                        const long* yoff, const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                        const double* t_re, const double* t_im, double* loss, double* g_re, double* g_im);
void abr_gn_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                      const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                      int profile, const double* w, int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im);
void abr2_gn_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                       const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                       const long* yoff, const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                       int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im);
// Least-squares products of bloch_batch_run's end point (mode 0; blochgn.hip k_bloch_lsq_batch, k_bloch_gn_batch, k_bloch_gn_fold): the
// forward call's inputs, m0 as bloch_vjp_batch_run takes it, the weights (wx, wy, wz) and the targets (tx, ty, tz) or the ndir
// directions (as bloch_jvp_batch_run takes them) in the forward outputs' layout.  lsq: loss per pulse and the gradient per b1
// sample; gn: sum_s s J_s' W_s J_s (s v), pulse p from ndir toff[p], direction-major.  One upload, two launches, one download of
// b1 size; the partials and the checkpoints stay on the device.
// mag, here and in the steady state's and the Levenberg-Marquardt steps' calls below: the magnitude fit of (|Mxy|, mz).
// The pair of weights (w_xy, w_z) comes in (wx, wy) and the pair of targets (t_xy, t_z) in (tx, ty); wz and tz are not read.  The
// staging, the launches and the downloads are the component calls'; only the kernels of the sweeps are the magnitude twins.
void bloch_lsq_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                         const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                         const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                         int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                         const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* wx,
                         const double* wy, const double* wz, const double* tx, const double* ty, const double* tz, double* loss,
                         double* g_re, double* g_im, bool mag = false);
void bloch_gn_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                        const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                        const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                        int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                        const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* wx,
                        const double* wy, const double* wz, int ndir, const double* v_re, const double* v_im, double* h_re,
                        double* h_im, bool mag = false);
// The Levenberg-Marquardt step on the device (simgn.hip): CG on (H + mu I) d = b per pulse and, with t_re, the loss and gradient at
// rf + d (loss, g_re, g_im may be null without one).
void abr_lm_step_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                           const double* g, int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                           int profile, const double* w, const double* b_re, const double* b_im, const double* mu, int cg,
                           double rtol, const double* t_re, const double* t_im, double* d_re, double* d_im, int* ncg, double* rr,
                           double* gg, int* status, double* loss, double* g_re, double* g_im);
void abr2_lm_step_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                            const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                            const long* yoff, const double* y, int nscale, const double* scales, int mode, int profile,
                            const double* w, const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                            const double* t_re, const double* t_im, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                            int* status, double* loss, double* g_re, double* g_im);
// The Levenberg-Marquardt step of the Bloch model on the device (blochgn.hip k_bloch_lm_sweep, k_bloch_lm_step, k_bloch_lm_trial with
// simgn.hip's k_lm_init): CG on (H + mu I) d = b per pulse, H as bloch_gn_batch_run applies it, and, with tx / ty / tz, the loss and
// gradient of bloch_lsq_batch_run at b1 + d (loss, g_re, g_im may be null without them).
void bloch_lm_step_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* wx,
                             const double* wy, const double* wz, const double* b_re, const double* b_im, const double* mu, int cg,
                             double rtol, const double* tx, const double* ty, const double* tz, double* d_re, double* d_im, int* ncg,
                             double* rr, double* gg, int* status, double* loss, double* g_re, double* g_im, bool mag = false);
// The Levenberg-Marquardt step of the steady state on the device (blochssgn.hip k_bloch_ss_lm_prep, k_bloch_ss_lm_sweep with
// blochgn.hip's k_bloch_lm_step, k_bloch_lm_trial and simgn.hip's k_lm_init): CG on (H + mu I) d = b per pulse, H as
// bloch_ss_gn_batch_run applies it, and, with tx / ty / tz, the loss and gradient of bloch_ss_lsq_batch_run at b1 + d (loss, g_re,
// g_im may be null without them).  No m0.
void bloch_ss_lm_step_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const double* wx, const double* wy, const double* wz,
                                const double* b_re, const double* b_im, const double* mu, int cg, double rtol, const double* tx,
                                const double* ty, const double* tz, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                                int* status, double* loss, double* g_re, double* g_im, bool mag = false);
// The Levenberg-Marquardt step of the pulse train on the device (blochtrainlm.hip k_bloch_train_lm_prep, k_bloch_train_lm_jvp,
// k_bloch_train_lm_run, k_bloch_train_lm_pvjp, k_bloch_train_lm_step with the shipped k_bloch_train_prop, simgn.hip's k_lm_init and, for
// the trial, blochgn.hip's k_bloch_lm_trial and the kernels of bloch_train_lsq_batch_run): CG on (H + mu I) d = b per
// pulse, H as bloch_train_gn_batch_run applies it at one direction, and, with targets (t[0] or tf[0] not null), the loss and gradient
// of bloch_train_lsq_batch_run at b1 + d (loss, g_re, g_im may be null without them).
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
                                   int* status, double* loss, double* g_re, double* g_im, bool mag = false);
// The Levenberg-Marquardt step of the train's schedule on the device (blochtrainschedlm.hip k_bloch_train_lm_sched_init,
// k_bloch_train_lm_sched_run, k_bloch_train_lm_sched_step with the shipped k_bloch_train_prop, k_bloch_train_prop_dgain and, with
// targets, k_bloch_train_run_sched_lsq and k_bloch_train_sched_gn_fold): with targets (t[0] or tf[0] not null) the loss
// and gradient of bloch_train_lsq_sched_batch_run at the call's schedule, then CG on (H + mu I) d = b per pulse, H as
// bloch_train_gn_sched_batch_run applies it there, restricted to the halves whose dgain / dphi is not null; bgain / bphi both null: b
// is the negated gradient, left on the device (loss, ggain, gphi may be null without targets).
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
                                         double* loss, double* ggain, double* gphi, bool mag = false);
// What mbfir_test_flip_stages adds to a search (include/mbfir.h says what each block holds): the overrides, the selected candidates
// and the host blocks the search's per-workgroup bests, the report and the stages go to (interleaved re, im where complex).
struct FlipStages {
    int force_mode, max_blocks, nsel;
    const long* sel;
    double* blk_p;
    long* blk_i;
    double *beta, *bf, *xl, *xlfp, *afa, *a, *theta, *peak;
    long* report;
};
// Root-flip search (flip.hip): returns the winner, -1 when no candidate has a finite peak.  With `hook` the same launches under its
// overrides, then the stage launch; a forced mode that does not fit the device's LDS throws std::invalid_argument before any launch.
long flip_search_run(int device, void* stream, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re,
                     const double* z_im, const double* zf_re, const double* zf_im, long ncand, const unsigned* masks,
                     const int* enum_bits, int scale_rule, double s_re, double s_im, int criterion, int tie_high, double* peaks,
                     double* beta_re, double* beta_im, double* winner_peak, const FlipStages* hook = nullptr);

// Batched Parks-McClellan exchange (remez.hip): one workgroup per design.  status: 0 converged, 1 maxiter reached (last iterate
// returned), 2 the exchange lost the alternation (no valid iterate).
struct RemezJobHost {
    int numtaps, nband;
    const double *edges, *desired, *weight;    // 2 nband, 2 nband, nband
    double* h;                                 // numtaps
    double* ext;                               // L + 1 or null
    int *status, *iterations;
    double* delta;
};
// Dense-grid size and per-band point counts (counts: nband ints) of the grid k_remez builds.
int remez_grid_counts(int numtaps, int nband, const double* edges, int density, int* counts);
void remez_run(int device, void* stream, int njobs, const RemezJobHost* jobs, int density, int maxiter);

// fmp.m (specfact.hip k_fmp): odd l <= 2047 taps of h (h_im may be null) -> (l + 1) / 2 minimum-phase taps.
void fmp_run(int device, void* stream, int l, const double* h_re, const double* h_im, double* out_re, double* out_im);
// mbfir_test_specfact_stages (specfact.hip): k_specfact (kind 0, n = order) or k_fmp (kind 1, n = filter length) through the
// instantiation that stores its stages, on one guarded device arena.  layout (18 longs) is always written; raw null: nothing else.
void specfact_stages_run(int device, void* stream, int kind, int n, int nlanes, const double* in_re, const double* in_im, int guard,
                         double fill, long extra, long* layout, double* raw);

}  // namespace mbfir
