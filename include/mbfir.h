/*
 * mbfir.h -- C ABI of the MI355X-native convex FIR / SLR beta-polynomial designer.
 *
 * Drop-in boundary for the four convex designers of
 * shanghong/Multiband-RF-pulse-Design.  Each mbfir_*_solve() replaces the body
 * of one reference function from "create optimisation arrays" to "return taps"
 * -- i.e. problem assembly, the external solver call (CVX / linprog / quadprog)
 * and the tap extraction -- and is what a MEX gateway (matlab/mbfir_mex.c) or a
 * ctypes binding (the Python host mirror in this repository) binds to:
 *
 *   mbfir_ap_solve         <- [h,status] = fir_ap_cvx(n,f,a,d,obj,Peak,dbg)   reference fir_ap_cvx.m:1,44-202
 *   mbfir_qp_solve         <- [h,status] = fir_qp_cvx(n,f,a,d,k,obj,dbg)      reference fir_qp_cvx.m:1,34-209
 *   mbfir_linprog_solve    <- [h,status] = fir_linprog(n,f,a,d,h0,dbg)        reference ss/fir_linprog.m:2,46-271
 *   mbfir_qprog_phs_solve  <- [h,status] = fir_qprog_phs(n,f,ac,dc,x0,dbg)    reference ss/fir_qprog_phs.m:1,49-394
 *
 * Conventions (from the reference's MEX precedent rf_tools/mex5/b2a.c:31-68,
 * abrx.c:35-62: plain double arrays, separate real/imaginary planes):
 *   - all arrays are caller-owned, contiguous double; complex data is passed as
 *     separate re/im arrays; `f` has 2*nband entries in [-1,1], `a` 2*nband, `d` nband;
 *   - taps are written to h_re/h_im (n entries each, caller-allocated);
 *   - nothing throws across the ABI, nothing calls exit(); the context is
 *     reusable across calls (bisection wrappers call ~10 times in a row) and is
 *     not thread-safe (distinct contexts are).
 *
 * Return codes of the solve functions:
 *    0  MBFIR_SOLVED        status 'Solved'   (taps written)
 *    1  MBFIR_INFEASIBLE    status 'Failed'   (primal/dual infeasibility certificate found)
 *    2  MBFIR_NUMERICAL     status 'Failed'   (iteration limit / numerical breakdown)
 *    3  MBFIR_EARLY_FAIL    status 'Failed'   (reference returns Failed before solving,
 *                                              ss/fir_linprog.m:66-75, ss/fir_qprog_phs.m:193-202)
 *   <0  usage / HIP error; mbfir_last_error(ctx) holds the message
 *       -1 MBFIR_E_ARG (the reference's error() cases), -2 MBFIR_E_HIP, -3 MBFIR_E_NODEVICE
 */
#ifndef MBFIR_H
#define MBFIR_H

#ifdef __cplusplus
extern "C" {
#endif

#define MBFIR_SOLVED 0
#define MBFIR_INFEASIBLE 1
#define MBFIR_NUMERICAL 2
#define MBFIR_EARLY_FAIL 3
#define MBFIR_E_ARG (-1)
#define MBFIR_E_HIP (-2)
#define MBFIR_E_NODEVICE (-3)

typedef struct mbfir_ctx mbfir_ctx;

/* Solver options.  Zero-initialise (or call mbfir_default_opts) for the defaults. */
typedef struct mbfir_opts {
    int grid_m;        /* number of linspace samples of the frequency grid; 0 = the reference's
                          rule (2*n*15 ap, 10*n qp, 15*n|30*n linprog, 30*n qprog_phs)        */
    int max_iter;      /* 0 -> 200 */
    double feastol;    /* 0 -> 1e-8  relative primal/dual residual                              */
    double abstol;     /* 0 -> 1e-10 absolute gap                                               */
    double reltol;     /* 0 -> 1e-8  relative gap                                               */
    int refine;        /* -1 -> 2  iterative-refinement sweeps per KKT solve; values above 8 are clamped to 8 */
    int verbose;       /* 1: one line per IPM iteration on stderr                               */
    int shard_rank;    /* frequency-row sharding (multi-GPU): this process's rank ...           */
    int shard_size;    /* ... out of shard_size (0 or 1 = not sharded)                          */
    int dense_trig;    /* 0: use the lattice structure of the trig columns / frequency grid when it
                          is there (no trig matrix, moments instead of the dense Gram products);
                          1: always materialise the trig matrix and use the dense MFMA Gram kernel */
    int ddkkt;         /* extended-precision (double-double) KKT solve for nearly active cones whose NT weights
                          exceed 1e6 x the typical weight (fir_qp_cvx's error cones):
                          0 = automatic (on for mbfir_qp_solve, off for the other designers), 1 = on, -1 = off */
    int lanes;         /* mbfir_solve_batch: designs of one shape that advance in LOCK STEP on one context (one stream,
                          one launch per phase, the design index a grid dimension).  0 = automatic (as many as the
                          shape allows while every context still gets a unit), 1 = never, k > 1 = k per unit   */
} mbfir_opts;

/* Per-solve report. */
typedef struct mbfir_info {
    int status;        /* same as the return code */
    int iters;         /* IPM iterations */
    int n_unknowns;    /* N  (columns of the conic program) */
    int n_rows;        /* R  (rows of G) */
    int n_freq;        /* M_f (distinct frequency rows of the trig matrix) */
    int n_lp, n_q3, n_big;
    double pcost, dcost, gap, relgap, pres, dres;
    double ms_assemble, ms_solve, ms_post, ms_total;   /* host wall-clock */
    double ms_gram;      /* device time (HIP events on the solver stream), summed over the builds, of the
                            normal-matrix products: dense mode = the k_gram launches alone; lattice mode =
                            moment kernels + fold + H assembly                                          */
    double ms_chol;      /* device time of the factorisation launches (Cholesky + triangular inverse), summed */
    double gram_flop;    /* algorithmic flop of ONE build: dense nw * Mf * Nt * (Nt+1); lattice: the
                            moment recurrences, (3 D - 1) * Mf * (4 + 4 nw)                              */
    int gram_launches;   /* k_gram launches behind ms_gram (= builds * nw; builds = iterations + 1); 0 in
                            lattice mode                                                                */
    int lattice;         /* 1 if the solve ran in lattice (matrix-free) mode                             */
    double chol_flop;    /* flop of one factorisation + triangular inverse: 2/3 np^3                      */
    int chol_launches;   /* factorisation launches behind ms_chol: ONE k_chol_dag launch per build for lock-step units and
                            from np = 4096 on (round 3); builds * (np/64 + 1) k_chol_step launches for one or two smaller designs */
    int builds;          /* normal-matrix builds (= iterations + 1; + 1 more when the head of the next iteration --
                            scaling, normal matrix, factorisation -- went to the stream before the host had seen the
                            final iterate: that last build is never used, its pivot counter never read; ms_gram,
                            ms_chol and chol_launches count it too)                                               */
    int dd_iters;        /* iterations that ran the extended-precision KKT solve (opts.ddkkt)              */
    int dd_kmax;         /* largest number of strong eigen-directions it carried                          */
    int collectives;     /* all-reduces a row-sharded solve issued (0 otherwise)                                   */
    int lanes;           /* designs that shared this design's lock-step batch (ms_solve, ms_gram, ms_chol are then
                            those of the whole batch)                                                      */
    int dd_form;         /* form of the extended-precision solve that ran: 0 capacitance (saddle-point) form in plain double on
                            the matrix cores, 1 double-double factorisation of the whole matrix, -1 none            */
    double ms_cap;       /* capacitance form: device time of its three matrix-core products (Yt = U M', Zt = Yt M,
                            S = Yt Yt' + X^-1), summed over the builds                                     */
    double cap_flop;     /* ... and their flop, summed over the builds                                     */
    double collective_bytes;   /* bytes the all-reduces of a row-sharded solve carried on this rank (dense path: the PACKED lower
                                  triangle of the normal matrix per build, N (N + 1) / 2 doubles rounded up to 64 x 64 tiles)    */
    int correctors;      /* centrality-corrector solves (one per iteration for programs with orthant rows; 0 with
                            MBFIR_CORRECTOR=0) ...                                                                     */
    int correctors_taken;/* ... and the iterations that took the corrected direction (its step was 1 % longer)         */
    int gv_passes;       /* passes over the frequency rows the solve launched, all iterations: row responses G v ...    */
    int gtv_passes;      /* ... and transposed products G'v (a two-vector pass counts once; a lock-step unit's count)    */
    int pair_passes;     /* ... and how many lattice passes (these and the normal-matrix moment passes) ran one thread per PAIR of lanes */
} mbfir_info;

/* All-reduce hook for row-sharded solves (one process per GPU).  `buf` is a DEVICE pointer to
 * `count` doubles on the context's stream-ordered memory; op 0 = sum, 1 = max.  The hook must
 * return after the reduction is complete and visible to the device (0 = ok).  The Python host
 * wires this to torch.distributed (RCCL over xGMI).  What goes through it per IPM iteration: the
 * trigonometric moments of the normal matrix (~100 KB; dense_trig: the np x np normal matrix itself),
 * every G'v and preconditioner application (N doubles each) and a few scalars -- all ranks make the
 * same sequence of calls. */
typedef int (*mbfir_allreduce_fn)(void* buf, long count, int op, void* user);

/* RCCL communicator for row-sharded solves (one process per GPU): rank 0 calls mbfir_comm_unique_id and
 * hands the 128 bytes to the other ranks (the host language's own channel: torch.distributed, MPI, a file), every rank
 * then calls mbfir_comm_init with its rank.  With a communicator the per-iteration reductions are ncclAllReduce calls
 * (ncclDouble, sum / max) enqueued on the solver's stream: no host synchronisation and no callback per collective.
 * Without one, mbfir_set_allreduce's hook is used (the CPU/gloo rehearsal path).  RCCL is bound at run time.      */
int  mbfir_comm_unique_id(mbfir_ctx* ctx, char* id128);
int  mbfir_comm_init(mbfir_ctx* ctx, int nranks, int rank, const char* id128);
void mbfir_comm_destroy(mbfir_ctx* ctx);
/* test hook: all-reduce the host array v (n doubles; op 0 sum, 1 max) through the context's communicator, on its stream */
int  mbfir_test_comm_allreduce(mbfir_ctx* ctx, double* v, long n, int op);

mbfir_ctx*  mbfir_create(int device_id);
void        mbfir_destroy(mbfir_ctx* ctx);
const char* mbfir_last_error(mbfir_ctx* ctx);
void        mbfir_default_opts(mbfir_opts* opts);
void        mbfir_set_allreduce(mbfir_ctx* ctx, mbfir_allreduce_fn fn, void* user);
const char* mbfir_version(void);

int mbfir_ap_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* a,
                   const double* d, double obj, double peak, const mbfir_opts* opts,
                   double* h_re, double* h_im, mbfir_info* info);

int mbfir_qp_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* a,
                   const double* d, double kquad, const double* obj, int nobj,
                   const mbfir_opts* opts, double* h_re, double* h_im, mbfir_info* info);

int mbfir_linprog_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* a,
                        const double* d, const mbfir_opts* opts,
                        double* h_re, double* h_im, mbfir_info* info);

int mbfir_qprog_phs_solve(mbfir_ctx* ctx, int n, int nband, const double* f,
                          const double* ac_re, const double* ac_im,
                          const double* dc_re, const double* dc_im, const mbfir_opts* opts,
                          double* h_re, double* h_im, mbfir_info* info);

/* Batch of independent designs -- the shape of the reference's outer loops (min-order / min-
 * duration bisections probe several n, fir_ap_cvx.m callers such as bSSFP_pulse_sb_mb.m:56-99
 * and dzbeta_min_order; parameter sweeps over obj / Peak).  The jobs are spread over `nctx`
 * contexts (all on one device, or one per device), one host thread per context; each context
 * has its own HIP stream, so the latency-bound phases of different designs overlap on the GPU.
 * `which`: 0 fir_ap_cvx (params = obj, Peak), 1 fir_qp_cvx (params = k, obj[0], obj[1], nobj),
 * 2 fir_linprog, 3 fir_qprog_phs (a: 2*nband and d: nband complex values, re/im interleaved).
 * Every job gets its own rc / info, as from the single-design entry points; returns 0 or the
 * most negative rc of the batch. */
typedef struct mbfir_job {
    int which, n, nband, rc;
    const double *f, *a, *d;
    double params[4];
    double *h_re, *h_im;          /* n doubles each, caller-allocated */
    mbfir_info info;
    double *z;                    /* optional: receives the conic solution (as mbfir_last_solution), up to z_cap doubles */
    int z_cap;
    char err[128];                /* message of the context that ran the job when rc < 0 */
} mbfir_job;

int mbfir_solve_batch(mbfir_ctx* const* ctxs, int nctx, mbfir_job* jobs, int njobs,
                      const mbfir_opts* opts);

/* Conic solution z = [x ; y] / tau of the last solve on this context (n_unknowns doubles of
 * mbfir_info; returns the count copied, or <0).  For fir_ap_cvx x is the autocorrelation
 * [r(0), Re r(1..n-1), Im r(1..n-1)] (fir_ap_cvx.m:185-186), for the others [Re h ; Im h] or the
 * half filter.  Lets callers check feasibility / optimality of what the solver returned. */
int mbfir_last_solution(mbfir_ctx* ctx, double* z, int capacity);

/* ---- introspection / test hooks (host only unless stated) --------------------------------
 * mbfir_assemble(): run the product's problem assembly for designer `which`
 *   (0 ap, 1 qp, 2 linprog, 3 qprog_phs) WITHOUT touching the GPU and return an opaque
 *   program; the accessors below expose its structured rows so tests can expand them to the
 *   dense (c,G,h) and compare with the oracle.  p1..: designer scalars (ap: obj,peak;
 *   qp: kquad,obj0,obj1,nobj).  For qprog_phs `a`,`d` hold interleaved re,im pairs.      */
typedef struct mbfir_program mbfir_program;
int  mbfir_assemble(int which, int n, int nband, const double* f, const double* a, const double* d,
                    const double* params, int grid_m, mbfir_program** out, char* err, int errlen);
void mbfir_program_free(mbfir_program* p);
/* the rows process `rank` of `size` keeps in a row-sharded solve (see mbfir_opts.shard_*): the frequencies are dealt out by
 * folded +w / -w PAIRS (pair q goes to rank q % size: both partners on one rank, one lattice recurrence serves them) with their
 * rows and cones; rows without a frequency (identity rows, spike / per-tap cones, the big cone) are REPLICATED on every rank and
 * counted once in the sums over the rows (mbfir_program_rep) */
int  mbfir_program_shard(const mbfir_program* p, int rank, int size, mbfir_program** out);
/* dims[0..9] = Nt, Ne, R, l, nq3, big, Mf, quad(0/1), nnz_id, reserved */
void mbfir_program_dims(const mbfir_program* p, int* dims);
/* w[Mf]; col_kind[Nt] (0 cos,1 sin); col_tau[Nt]; col_scale[Nt]; pcol[Nt]; psign[Nt]; c[N]     */
void mbfir_program_trig(const mbfir_program* p, double* w, int* col_kind, double* col_tau,
                        double* col_scale, int* pcol, double* psign, double* c);
/* per row: freq (or -1), col (or -1), alpha, beta, ey[3], h                                     */
/* rep[r] = 1 for the rows a row-sharded solve holds on EVERY rank (rows / cones without a frequency, the big cone): R ints */
void mbfir_program_replicated(const mbfir_program* p, int* rep);
void mbfir_program_rows(const mbfir_program* p, int* freq, int* col, double* alpha, double* beta,
                        double* ey, double* h);

/* ---- Inverse SLR: what dzrf_mb.m:239-240 does with the designed beta polynomial ----
 * n complex taps in, host arrays, all caller-allocated with n doubles each.
 *  mbfir_b2a  : minimum-phase alpha of beta, `a = b2a(b)`            (rf_tools/b2a.m:15-32, mag2mp.m:21-31)
 *  mbfir_ab2rf: RF pulse of (alpha, beta), `rf = ab2rf(a, b)`, n <= 2048   (rf_tools/ab2rf.m:14-29)
 *  mbfir_b2rf : `rf = b2rf(b)` = ab2rf(b2a(b), b) without the round trip   (rf_tools/mex5/b2rf.c)
 * rf is in radians per sample, as the reference returns it (dzrf_mb.m:244 rescales it to Gauss). */
int mbfir_b2a(mbfir_ctx* ctx, int n, const double* b_re, const double* b_im, double* a_re, double* a_im);
int mbfir_ab2rf(mbfir_ctx* ctx, int n, const double* a_re, const double* a_im, const double* b_re,
                const double* b_im, double* rf_re, double* rf_im);
int mbfir_b2rf(mbfir_ctx* ctx, int n, const double* b_re, const double* b_im, double* rf_re, double* rf_im);
/* mbfir_b2rf_batch: `rf(q, :) = b2rf(b(q, :))` for count independent polynomials of n taps in ONE launch, one workgroup each
 *   (the inner loops of dzepse.m:39-49).  b and rf are row-major count x n planes (b_im may be NULL = 0); 2 <= n <= 2048,
 *   count >= 1, else MBFIR_E_ARG.  The same chain as mbfir_b2rf (b2a.m:15-32 with its 8 n padding and max|bf| >= 1 rescale,
 *   mag2mp.m:21-31, ab2rf.m:14-29) summed in another order: it agrees with mbfir_b2rf to rounding, not to the bit.  A pulse's
 *   bits depend neither on count nor on its row: a row of a batch equals the same row alone. */
int mbfir_b2rf_batch(mbfir_ctx* ctx, int n, int count, const double* b_re, const double* b_im, double* rf_re, double* rf_im);

/* mbfir_slr2d_batch: the 2D inverse SLR of dzepse.m:39-49 for count complex m x n matrices r in one call (rows: spatial samples,
 *   columns: spectral samples; r and the result row-major count x m x n planes, r_im may be NULL = 0).  Returns rn2, radians per
 *   sample: stage 1 rn1(q, :) = b2rf(r(q, :)); per column theta = rn1(:, j) the hard-pulse beta
 *   s = sin(|theta| / 2) exp(-i arg theta) (dzepse's sin(conj(theta) / 2) for a real theta) and
 *   p2_j = fftcp(s, 2m)(m/2 + 1 : 3m/2) / 2m; stage 2 rn2(:, j) = conj(b2rf(p2_j)).  The b2rf steps are mbfir_b2rf_batch's; the
 *   intermediates stay on the device (one upload, one download).  2 <= n <= 2048, 2 <= m <= 2048 with m even, count >= 1 and
 *   count max(m, n) < 2^31, else MBFIR_E_ARG.  A matrix's bits depend neither on count nor on its place in the batch.
 *   literal = 1 takes dzepse.m:45's s = sin(conj(theta) / 2) instead (dzepse's own stage-1 angles are not real: parity with it);
 *   literal must be 0 or 1. */
int mbfir_slr2d_batch(mbfir_ctx* ctx, int m, int n, int count, const double* r_re, const double* r_im, double* out_re,
                      double* out_im, int literal);

/* ---- Forward simulation over off-resonance ----------------------------------------------
 * Cayley-Klein parameters (a, b) of the rotation an n-sample pulse produces at nx positions x
 * (rf in radians per sample; g: n per-sample gradient / time weights, NULL = 2 pi / n each, so that x counts
 * cycles over the pulse = frequency x duration).
 *  mode 0: `[a b] = abrm(rf, g, x)` (rf_tools/abrm.m:24-62, the .m twin of the MEX abrx that abr.m:26-30 calls
 *          and that sim_rf_spectral.m's blochC run agrees with for T1, T2 >> pulse length): one rotation about
 *          (Re rf, Im rf, x g) per sample;
 *  mode 1: the hard-pulse model that ab2rf inverts exactly (precession, then the hard pulse) -- closes the loop
 *          b -> mbfir_b2rf -> mbfir_abr -> B(w) to rounding.
 * abr.m's convention is b = -conj(b) of mode 0; mxy = 2 conj(a) b, mz = 1 - 2 |b|^2 (abr.m:11-14). */
int mbfir_abr(mbfir_ctx* ctx, int n, const double* rf_re, const double* rf_im, const double* g, int nx,
              const double* x, int mode, double* a_re, double* a_im, double* b_re, double* b_im);
/* mbfir_abr2: `[a b] = abrm(rf, g, x, y)` of a 2D pulse (rf_tools/abrm.m:39-57): g = gx + i gy complex, one rotation about
 *   (Re rf, Im rf, x_k gx_m + y_j gy_m) per sample at every (x_k, y_j); a and b hold nx x ny entries, abrm's a(k, j) at
 *   a[k * ny + j] (row-major).  gx NULL = 2 pi / n per sample as in mbfir_abr, gy NULL = 0.  abrm.m's joint rotation only
 *   (mbfir_abr's mode 0); abr.m's convention is b = -conj(b) of this result (abr.m:26-32). */
int mbfir_abr2(mbfir_ctx* ctx, int n, const double* rf_re, const double* rf_im, const double* gx, const double* gy, int nx,
               const double* x, int ny, const double* y, double* a_re, double* a_im, double* b_re, double* b_im);

/* Bloch-equation simulation with relaxation on the device: replaces the MEX bloch_simulation/blochC.c / blochH.c (mexFunction
 * :514-933 -> blochsimfz :422-512 -> blochsim :283-418, calcrotmat :171-236) that sim_rf_spectral.m:63-78 runs on the designed
 * pulse.  b1 in Gauss (re / im planes, ntime samples), gx/gy/gz in G/cm (each may be NULL = 0), tsteps = the ntime interval lengths
 * in s, t1/t2 in s, df in Hz (nfreq), dx/dy/dz in cm (npos; each may be NULL = 0), mode bit 0: steady state, bit 1: record every
 * sample (the reference's `mode`), gamma in rad/s/G (6726.1 for C-13 = blochC.c:5, 26754 for H-1 = blochH.c:6).  mx/my/mz: nfreq *
 * npos * (mode & 2 ? ntime : 1) doubles, block (f, p) at (f * npos + p) * ntout; on entry the first entry of every block holds the
 * initial magnetisation (the gateway's :826-866 convention; [0 0 1] for equilibrium), on exit the result.  Runs as
 * mbfir_bloch_batch's one pulse at scale 1.0, with its size limits (MBFIR_E_ARG; sizes beyond them could not launch before either). */
int mbfir_bloch(mbfir_ctx* ctx, int ntime, const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                const double* gz, const double* tsteps, double t1, double t2, int nfreq, const double* df, int npos,
                const double* dx, const double* dy, const double* dz, int mode, double gamma, double* mx, double* my, double* mz);

/* ---- Batched simulation: many pulses x transmit-gain scales in one launch ----------------------------------------------------
 * The pulses (and their grids) are concatenated; an offset table of count + 1 longs says where each item starts: item i owns
 * entries off[i] .. off[i + 1] - 1, off[0] = 0, strictly ascending.  One upload, one launch, one download on the context's stream;
 * one 256-thread workgroup per (pulse, scale, 256 points), the pulses with the most samples first.  A result's bits depend only on
 * its own pulse, scale and point: not on the number of pulses, their order, or the other scales.
 * mbfir_bloch_batch: mbfir_bloch for every (pulse p, scale s).
 *   toff (npulse + 1): the samples of pulse p, ntime_p = toff[p + 1] - toff[p] >= 1, in b1_re / b1_im (Gauss) and gx / gy / gz
 *     (G/cm; each NULL = 0 for every pulse).
 *   tsoff (npulse + 1), tsteps: the intervals of pulse p in s, tsoff[p + 1] - tsoff[p] = 1 (one interval for every sample) or
 *     ntime_p (end times are converted by the caller, as for mbfir_bloch).
 *   t1, t2 (s, > 0), gamma (rad/s/G): npulse each.  E1 = exp(-dt / T1), E2 = exp(-dt / T2) per sample on the host, as mbfir_bloch.
 *   nfgrid = 1 (one grid of off-resonances shared by every pulse) or npulse (grid p for pulse p); foff (nfgrid + 1) into df (Hz).
 *   npgrid, poff (npgrid + 1), dx / dy / dz (cm; each NULL = 0): the positions, the same way.
 *   scales (nscale >= 1): scale s multiplies b1 before the gamma dt product, rotx = ((-(b1_re s)) gamma) dt and roty =
 *     ((b1_im s) gamma) dt, mbfir_bloch's products for the pulse b1 s: with s = 1 a pulse sees mbfir_bloch's per-sample values.
 *   mode: mbfir_bloch's, for every pulse.
 *   mx / my / mz: pulse p from O_p = sum_{q < p} nscale nf_q npos_q ntout_q (ntout = ntime with mode & 2, else 1), laid out
 *     (scale, frequency, position[, time]) row-major: block (s, f, k) at O_p + ((s nf_p + f) npos_p + k) ntout_p.  On entry the
 *     first entry of every block holds its initial magnetisation ([0 0 1] for equilibrium, as mbfir_bloch), on exit the result.
 * mbfir_abr_batch: mbfir_abr for every (pulse p, scale s).  roff (npulse + 1) into rf_re / rf_im (radians per sample) and g (one
 *   weight per sample; NULL = 2 pi / n_p for every sample of pulse p, mbfir_abr's default, which a caller with g for only some
 *   pulses writes for the others); nxgrid = 1 or npulse, xoff (nxgrid + 1) into x; scale s multiplies rf; mode: mbfir_abr's (0
 *   abrm.m, 1 the hard-pulse model).  a / b (re, im planes): pulse p from sum_{q < p} nscale nx_q, (scale, position) row-major.
 * mbfir_abr2_batch: mbfir_abr2 for every (pulse p, scale s), in both models.  roff (npulse + 1) into rf_re / rf_im and gx / gy (one
 *   weight each per sample; gx NULL = 2 pi / n_p and gy NULL = 0 for every sample, mbfir_abr2's defaults); nxgrid and nygrid = 1
 *   or npulse each, xoff (nxgrid + 1) into x and yoff (nygrid + 1) into y; scale s multiplies rf; mode 0: abrm.m:39-57, one
 *   rotation about (Re rf, Im rf, x_k gx_m + y_j gy_m) per sample, with mbfir_abr2's bits; mode 1: mbfir_abr's hard-pulse model
 *   with the precession angle x_k gx_m + y_j gy_m.  a / b (re, im planes): pulse p from sum_{q < p} nscale nx_q ny_q, laid out
 *   (scale, x, y) row-major: point (s, k, j) at ((s nx_p + k) ny_p + j).
 * All three return MBFIR_E_ARG, with the reason in mbfir_last_error and no device work done, for: npulse < 1, nscale < 1, a pulse with
 *   no samples, an offset table that does not start at 0 or does not ascend, an empty grid, a grid count neither 1 nor npulse, a
 *   tsteps length neither 1 nor ntime_p, t1 or t2 not positive, a mode out of range, a required array NULL, and a total output
 *   or workgroup count that overflows. */
int mbfir_bloch_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                      const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                      const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                      const double* dx, const double* dy, const double* dz, int nscale, const double* scales, int mode, double* mx,
                      double* my, double* mz);
int mbfir_abr_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                    int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, double* a_re,
                    double* a_im, double* b_re, double* b_im);
int mbfir_abr2_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                     const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff, const double* y,
                     int nscale, const double* scales, int mode, double* a_re, double* a_im, double* b_re, double* b_im);
/* ---- Adjoints of mbfir_abr_batch / mbfir_abr2_batch with respect to the rf samples -----------------------------------------------
 * The vector-Jacobian product of the forward call, in both models: the forward call's arguments, with the four output planes
 * replaced by the cotangents of a and b in the same layout (ca, cb; dL = Re(conj(ca) da + conj(cb) db) for a real L, that is ca =
 * dL/dRe a + i dL/dIm a), and two outputs of one entry per rf sample, g_re = dL/dRe rf and g_im = dL/dIm rf, laid out as rf_re /
 * rf_im.  A sample's gradient is summed over the points of its pulse and over the scales (scale s contributes s times the gradient
 * with respect to s rf); g / gx / gy, the grids and the scales are not differentiated.  One upload, two launches (the sweeps with
 * one partial per workgroup and sample, then the sum of a pulse's partials over chunks and scales in index order), one download; no
 * atomics, so a pulse's gradient bits depend only on the pulse, its grid and the scale list.  The argument checks and their
 * MBFIR_E_ARG messages are those of the forward calls (a cotangent or gradient plane NULL is a required array NULL). */
int mbfir_abr_vjp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                        int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                        const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im, double* g_re,
                        double* g_im);
int mbfir_abr2_vjp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                         const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                         const double* y, int nscale, const double* scales, int mode, const double* ca_re, const double* ca_im,
                         const double* cb_re, const double* cb_im, double* g_re, double* g_im);
/* ---- Adjoints of mbfir_abr_batch / mbfir_abr2_batch with respect to the rf samples and the gradient waveform ----------------------
 * mbfir_abr_vjp_batch / mbfir_abr2_vjp_batch with one more output (1D: gg) or two (2D: ggx, ggy) of one entry per rf sample, laid
 * out as g / gx / gy: gg = dL/dg, ggx = dL/dgx, ggy = dL/dgy.  The precession angle of a sample at a point is x g (1D) or x gx +
 * y gy (2D), so a sample's entry is the sum over the points of its pulse of the point's coordinate times dL/d(angle), summed over
 * the scales without a factor (a scale multiplies rf, not g).  A NULL g / gx / gy is differentiated at its default (2 pi / n per
 * sample; gy = 0) and the gradient is returned all the same.  g_re / g_im are the rf gradient of the calls above to rounding (the
 * sums run in another order), not to the bit.  One upload, two launches (the sweeps with one partial per workgroup, sample and
 * component; then the sum of a pulse's partials over chunks and scales in index order), one download; no atomics, so the bits of
 * both gradients depend only on the pulse, its grid and the scale list.  Argument checks and MBFIR_E_ARG messages as above. */
int mbfir_abr_vjp_rfg_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                            int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                            const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im, double* g_re,
                            double* g_im, double* gg);
int mbfir_abr2_vjp_rfg_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                             const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                             const long* yoff, const double* y, int nscale, const double* scales, int mode, const double* ca_re,
                             const double* ca_im, const double* cb_re, const double* cb_im, double* g_re, double* g_im,
                             double* ggx, double* ggy);
/* ---- Adjoint of mbfir_bloch_batch with respect to the b1 samples and the initial magnetisation ----------------------------------
 * The vector-Jacobian product of the end point (mode 0) of mbfir_bloch_batch, relaxation included: the forward call's input
 * arguments up to nscale and scales (no mode: the steady state is differentiated by mbfir_bloch_ss_vjp_batch below, the recorded trajectory is not), then
 *   m0x / m0y / m0z: the initial magnetisation in the layout of the mode-0 outputs, block (s, f, k) of pulse p at O_p + (s nf_p + f)
 *     npos_p + k with O_p = sum_{q < p} nscale nf_q npos_q; all three NULL = [0 0 1] everywhere.
 *   cmx / cmy / cmz: the cotangents of mx / my / mz in the same layout, dL = sum cmx dmx + cmy dmy + cmz dmz.
 *   g_re / g_im: one entry per b1 sample, laid out as b1_re / b1_im: dL/dRe b1 and dL/dIm b1, summed over the points of the pulse
 *     and over the scales (scale s contributes s times the gradient with respect to s b1).
 *   gm0x / gm0y / gm0z: dL/dm0 of every (scale, frequency, position) block, in the same layout; all three NULL = not wanted.
 * gx / gy / gz, the intervals, t1, t2, the grids and the scales are not differentiated.  The step m_t = D_t R_t m_{t-1} + c_t is a
 * contraction, so the reverse sweep never divides by E1 or E2: the forward sweep keeps m before every 8th sample in a device
 * scratch array (3 ceil(ntime_p / 8) doubles per point and scale) and the reverse sweep steps each group of 8 samples forwards
 * again from its checkpoint before it walks it backwards.  One upload, two launches (the sweeps with one partial per workgroup and
 * sample, then the sum of a pulse's partials over chunks and scales in index order, times gamma dt), one download; no atomics, so a
 * pulse's gradient bits depend only on the pulse, its grids, its cotangents and the scale list.  The argument checks and their
 * MBFIR_E_ARG messages are those of mbfir_bloch_batch; further MBFIR_E_ARG cases, each with its reason in mbfir_last_error and no
 * device work done: a cotangent or gradient plane NULL, m0x / m0y / m0z only partly given, gm0x / gm0y / gm0z only partly given.  A
 * NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_vjp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                          const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                          const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                          const double* m0x, const double* m0y, const double* m0z, const double* cmx, const double* cmy,
                          const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y, double* gm0z);
/* ---- Adjoint of mbfir_bloch_batch with respect to b1, the initial magnetisation, the gradient waveform and the off-resonance -------
 * mbfir_bloch_vjp_batch with four more outputs after its own arguments:
 *   ggx / ggy / ggz: one entry per sample of every pulse, laid out as gx / gy / gz: dL/dgx, dL/dgy, dL/dgz.  The axis component of
 *     a sample's rotation at a point is -((gx x + gy y + gz z) gamma dt + df TWOPI dt), so a sample's entry is -(gamma dt) times the
 *     sum over the points of its pulse of the point's coordinate times dL/d(that component), summed over the scales without a factor
 *     (a scale multiplies b1, not the gradient).  All three are required; a NULL input plane gx / gy / gz (an axis no pulse plays) is
 *     differentiated at zero and its gradient is returned all the same: it is zero only where the positions lack that axis too.
 *   gdf: dL/ddf of every (scale, frequency, position) in the layout of gm0x, -sum_t (TWOPI dt_t) dL/d(axis component); the caller
 *     sums over whatever shares an off-resonance.  NULL = not wanted: it is then neither formed nor downloaded.
 * g_re / g_im and gm0x / gm0y / gm0z are those of mbfir_bloch_vjp_batch to rounding (the sums run over other sub-groups of the same
 * order), not promised to the bit.  tp, t1, t2, the positions and the scales are not differentiated.  The checkpoints, the launch
 * shape and the staging are mbfir_bloch_vjp_batch's; one upload, two launches (the sweeps with one partial per workgroup, sample and
 * component; then the sum of a pulse's partials over chunks and scales in index order, times gamma dt), one download; no atomics,
 * so the bits of every result depend only on the pulse, its grids, its cotangents and the scale list.  Argument checks and
 * MBFIR_E_ARG messages as mbfir_bloch_vjp_batch's, and one more case: a NULL ggx, ggy or ggz.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_vjp_gr_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* cmx,
                             const double* cmy, const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y,
                             double* gm0z, double* ggx, double* ggy, double* ggz, double* gdf);
/* ---- Tangent of mbfir_bloch_batch with respect to the b1 samples and the initial magnetisation -----------------------------------
 * The Jacobian-vector product of the end point (mode 0) of mbfir_bloch_batch, relaxation included: the forward call's input
 * arguments up to nscale and scales (no mode), then
 *   m0x / m0y / m0z: the initial magnetisation, as mbfir_bloch_vjp_batch takes it; all three NULL = [0 0 1] everywhere.
 *   ndir >= 1 and v_re / v_im: the b1 directions, direction-major within a pulse: sample t of direction k of pulse p at ndir toff[p] +
 *     k ntime_p + t.
 *   dm0x / dm0y / dm0z: the directions of the initial magnetisation; pulse p starts at ndir times its forward output offset O_p and
 *     is laid out (direction, scale, point) row-major, the point index as in the forward call; all three NULL = zero.
 *   mx / my / mz: laid out as the forward call's mode-0 outputs, with its bits; all three NULL = not downloaded.
 *   dmx / dmy / dmz: the tangents, laid out as dm0: d/de m(b1 + e v, m0 + e dm0) at e = 0 for every direction, real-linear in (v,
 *     dm0); scale s contributes the tangent along s v at s b1, and a scale of 0 contributes the m0 part alone.
 * gx / gy / gz, the intervals, t1, t2, the grids and the scales are not differentiated.  One upload, one launch (one workgroup per
 * forward workgroup and group of mbfir_test_bloch_jvp_group() directions, which share each sample's trigonometry and rotation),
 * one download; no atomics, and a tangent's bits depend only on its pulse, scale, point and direction: not on the batch, its order,
 * ndir or the direction's place among the others.  The argument checks and their MBFIR_E_ARG messages are those of
 * mbfir_bloch_batch; further MBFIR_E_ARG cases, each with its reason in mbfir_last_error, in this order: a v or dm plane NULL; m0,
 * dm0 or mx / my / mz only partly given; ndir < 1; a direction array, tangent output or workgroup count that overflows.  No device
 * work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_jvp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                          const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                          const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                          const double* m0x, const double* m0y, const double* m0z, int ndir, const double* v_re, const double* v_im,
                          const double* dm0x, const double* dm0y, const double* dm0z, double* mx, double* my, double* mz,
                          double* dmx, double* dmy, double* dmz);
/* mbfir_test_bloch_jvp_group (host only): the directions one workgroup of the call above carries (a compile-time constant). */
int mbfir_test_bloch_jvp_group(void);
/* ---- Adjoint and tangent of mbfir_bloch_batch's steady state with respect to the b1 samples ---------------------------------------
 * Mode 1 of mbfir_bloch_batch returns the fixed point M = (I - A)^-1 B of one period m -> A m + B of the pulse (for balanced SSFP:
 * the pulse plus the dead time of one repetition).  A and B depend on b1 and dM = (I - A)^-1 dF at m0 = M, where dF is the
 * derivative of the mode-0 end point with m0 held fixed; so the adjoint is mbfir_bloch_vjp_batch's from m0 = M with the end
 * cotangent (I - A)^-T c, and the tangent is (I - A)^-1 times mbfir_bloch_jvp_batch's from m0 = M with dm0 = 0, each fused into one
 * kernel that starts with mode 1's own sweep.  Both take the forward call's input arguments up to nscale and scales (no mode and no
 * m0: the steady state does not depend on m0, and there is no dL/dm0), then
 *   vjp: cmx / cmy / cmz, the cotangents of the mode-1 outputs in their layout (S x nf x npos per pulse, as the mode-0 layout of
 *        mbfir_bloch_vjp_batch); g_re / g_im as there; mx / my / mz receive M with mode 1's bits, all three NULL = not downloaded.
 *   jvp: ndir >= 1 and v_re / v_im, then mx / my / mz (M; all three NULL = not downloaded) and dmx / dmy / dmz, all laid out as
 *        mbfir_bloch_jvp_batch lays them out; a workgroup carries mbfir_test_bloch_ss_jvp_group() directions.
 * One upload and one download each; the adjoint runs two launches (the second is the fold of mbfir_bloch_vjp_batch), the tangent
 * one.  No atomics: the bits depend only on the pulse, its grids, its cotangents or direction and the scale list.  The error of M
 * and of both products grows with kappa = ||(I - A)^-1||, about T1 / TR.  There is no guard on det(I - A): where mode 1 itself is
 * not finite (T1 so long that E1 rounds to 1) the derivatives are not finite either.  gx / gy / gz, the intervals, t1, t2, the
 * grids and the scales are not differentiated.  The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_batch;
 * further MBFIR_E_ARG cases, each with its reason in mbfir_last_error and no device work done: a cotangent, gradient, direction or
 * tangent plane NULL; mx / my / mz only partly given; ndir < 1; a partial, checkpoint, output or workgroup count that overflows.  A
 * NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_ss_vjp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* cmx, const double* cmy, const double* cmz, double* g_re, double* g_im,
                             double* mx, double* my, double* mz);
int mbfir_bloch_ss_jvp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, int ndir, const double* v_re, const double* v_im, double* mx, double* my,
                             double* mz, double* dmx, double* dmy, double* dmz);
/* mbfir_test_bloch_ss_jvp_group (host only): the directions one workgroup of the tangent above carries (a compile-time constant). */
int mbfir_test_bloch_ss_jvp_group(void);
/* ---- The echo-by-echo transient of a pulse train ----------------------------------------------------------------------------------
 * Each pulse of the call is one period, exactly as mbfir_bloch_batch takes it (dead time as zero-b1 samples with their own
 * interval); a train plays it ntr_p times, repetition k at gains[k] exp(i phi_k) b1, gradients and timing the same every repetition.
 * With (A, B) the period's propagator m -> A m + B at RF amplitude scale x gain and RF phase 0, (A_e, B_e) that of its first
 * echo_p samples, Z(th) = [[cos th, -sin th, 0], [sin th, cos th, 0], [0, 0, 1]] and m_0 = m0, per point
 *     u = Z(+phi_k) m_k,   echo_k = Z(-phi_k) (A_e u + meq B_e)   (demod != 0: without the leading Z(-phi_k)),
 *     m_{k+1} = Z(-phi_k) (A u + meq B).
 * meq scales every recovery term (1 - E1): 1 is mbfir_bloch's convention, 0 the hyperpolarised limit, in which the train is linear
 * in m0.  mbfir_bloch_train_batch takes mbfir_bloch_batch's input arguments up to nscale and scales, then
 *   ntr (npulse): the repetitions of pulse p, >= 1.
 *   roff (npulse + 1) into cosphi / sinphi / gidx: roff[p + 1] - roff[p] = ntr_p; entry roff[p] + k holds cos phi_k, sin phi_k and
 *     the index of repetition k's gain among the pulse's distinct gains.  The caller forms the cosines and sines in double.
 *   goff (npulse + 1) into gains: the ngain_p = goff[p + 1] - goff[p] distinct gains of pulse p, 1 <= ngain_p <= ntr_p.  The
 *     propagators are formed once per (scale, distinct gain), at the amplitude scales[s] * gains[g] (one double product).
 *   echo (npulse): the echo sample of pulse p in [0, ntime_p]; 0 gives (A_e, B_e) = (I, 0) and ntime_p gives (A, B).
 *   meq (npulse), demod.
 *   m0x / m0y / m0z: as mbfir_bloch_vjp_batch takes them; all three NULL = [0 0 1] everywhere.
 *   ex / ey / ez: the echoes, pulse p from sum_{q < p} nscale ntr_q nf_q npos_q, laid out (scale, repetition, frequency, position)
 *     row-major; all three NULL = not downloaded.
 *   fx / fy / fz: m after the last repetition in the layout of mbfir_bloch_batch's mode-0 outputs; all three NULL = not downloaded.
 * One upload, two launches, one download: the first launch sweeps the period's samples once per (pulse, scale, distinct gain, 256
 * points) and leaves the 24 doubles of (A, B, A_e, B_e) per point in a device workspace; the second walks the repetitions, one
 * workgroup per (pulse, scale, 256 points).  No atomics: a result's bits depend only on its own pulse, scale, point and train, and
 * the first n echoes of a train are those of the train cut after n repetitions.
 * mbfir_bloch_prop_batch is the first launch alone, at gain 1: after scales it takes echo (npulse) and returns a / ae (9 doubles,
 * column-major: entry (i, j) at i + 3 j) and b / be (3 doubles, at meq = 1) of every (scale, frequency, position), block (s, f, k)
 * of pulse p at 9 (or 3) times O_p + (s nf_p + f) npos_p + k with O_p = sum_{q < p} nscale nf_q npos_q.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_batch (a train table, echo, meq or, for
 * mbfir_bloch_prop_batch, an output NULL is a required array NULL); further MBFIR_E_ARG cases, each with its reason in
 * mbfir_last_error and no device work done: ntr < 1; roff or goff inconsistent with ntr; echo outside [0, ntime]; a gain index
 * outside [0, ngain); a gain, cosine, sine or meq that is not finite; m0, the echo planes or the final planes only partly given, or
 * neither output wanted; a workspace, output or workgroup count that overflows.  A refused call leaves the context usable.  A NULL
 * context returns MBFIR_E_ARG. */
int mbfir_bloch_train_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                            const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                            const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                            const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                            const int* ntr, const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                            const long* goff, const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                            const double* m0y, const double* m0z, double* ex, double* ey, double* ez, double* fx, double* fy,
                            double* fz);
int mbfir_bloch_prop_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                           const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                           const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                           const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                           const int* echo, double* a, double* b, double* ae, double* be);
/* ---- Adjoint of the pulse train with respect to b1 and the initial magnetisation ----------------------------------------------------
 * The vector-Jacobian product of mbfir_bloch_train_batch's echoes and final state: for the loss
 *     L = sum_k <ce_k, echo_k> + <cf, m_N>
 * the gradient dL/dRe b1 + i dL/dIm b1 of the period's samples, summed over the points, the scales and the repetitions (repetition k
 * plays gains[k] exp(i phi_k) b1: the chain rule through that product is included), and dL/dm0.  It takes
 * mbfir_bloch_train_batch's arguments through demod and m0x / m0y / m0z, then
 *   cex / cey / cez: the cotangents of the echoes, laid out as ex / ey / ez (with demod != 0: of the demodulated echoes); all
 *     three NULL = none.
 *   cfx / cfy / cfz: the cotangents of the final state, laid out as fx / fy / fz; all three NULL = none.  Not both triples NULL.
 *   g_re / g_im: one entry per sample of every pulse, laid out as b1_re / b1_im.
 *   gmx / gmy / gmz: dL/dm0 of every (scale, frequency, position) in the layout of the final planes; all three NULL = not wanted.
 *     dL/dm0 depends neither on m0 nor on meq, and has the same bits for any of them.
 * One upload, four launches, one download: the forward call's propagator launch; the repetitions walked forwards (a checkpoint
 * before every eighth) and backwards, which leaves the cotangents of the 24 doubles of (A, B, A_e, B_e) per (scale, distinct gain,
 * point) in a device workspace; the period's samples swept forwards and backwards once per (pulse, scale, distinct gain, 64
 * points), the four columns of [A | B] on the four wavefronts of a workgroup; and the fold over chunks and combinations.  No
 * atomics: a pulse's gradient bits depend only on the pulse, its grids, its train, its cotangents and the scale list.  gr, tp,
 * t1, t2, df, the positions and meq are not differentiated (the gains and the phases: mbfir_bloch_train_vjp_sched_batch).
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_batch; further MBFIR_E_ARG cases, each with
 * its reason in mbfir_last_error and no device work done: a cotangent triple or gmx / gmy / gmz only partly given; both cotangent
 * triples NULL; g_re or g_im NULL; a partial, checkpoint, workspace or workgroup count that overflows.  A refused call leaves the
 * context usable.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_train_vjp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                const double* cex, const double* cey, const double* cez, const double* cfx, const double* cfy,
                                const double* cfz, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz);
/* ---- Adjoint of the pulse train with respect to b1, the gradient waveform and the off-resonance --------------------------------------
 * mbfir_bloch_train_vjp_batch plus, for the same loss, dL/dgx, dL/dgy, dL/dgz of the period's samples and dL/ddf.  gr and df enter
 * a period only through a sample's precession angle about z, which neither the RF phase nor the gain of a repetition touches, so
 * the repetitions are walked exactly as mbfir_bloch_train_vjp_batch walks them.  It takes that call's arguments in order, then
 *   ggx / ggy / ggz: one double per sample of every pulse, laid out as gx / gy / gz, in the units of the waveform, summed over the
 *     points, the scales, the gains and the repetitions without a factor (scale and gain multiply b1, not gr); all three required.
 *     A NULL gx / gy / gz is differentiated at zero; a component is exactly zero where no position has that axis.
 *   gdf: dL/ddf of every (scale, frequency, position) in the layout of the final planes, summed over the repetitions; the caller
 *     sums over whatever shares an off-resonance.  NULL = not wanted.
 * g_re / g_im equal mbfir_bloch_train_vjp_batch's to rounding (not promised to the bit); gmx / gmy / gmz have its bits.  One upload,
 * four launches (five with gdf), one download: the propagator launch and the walk of the repetitions as in
 * mbfir_bloch_train_vjp_batch; the period's samples swept forwards and backwards once per (pulse, scale, distinct gain, 64 points),
 * which leaves five partials per (workgroup, sample) and, with gdf, one double per (scale, distinct gain, point); the folds over
 * chunks and combinations.  No atomics: the bits of every result depend only on the pulse, its grids, its train, its cotangents
 * and the scale list, and not on whether gdf or gm* is wanted.  tp, t1, t2, the positions, meq and the scales are not
 * differentiated.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_vjp_batch, in its order; then a NULL ggx / ggy /
 * ggz and a partial, workspace or workgroup count that overflows.  Each names bloch_train_vjp_gr_batch in mbfir_last_error and no
 * device work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_train_vjp_gr_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                   const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                   const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                   const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                   int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                   const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                   const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                   const double* cex, const double* cey, const double* cez, const double* cfx, const double* cfy,
                                   const double* cfz, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz, double* ggx,
                                   double* ggy, double* ggz, double* gdf);
/* ---- Adjoint of the pulse train with respect to its schedule: the gain and the RF phase of every repetition ------------------------
 * For the loss of mbfir_bloch_train_vjp_batch, L = sum_k <ce_k, echo_k> + <cf, m_N>, the gradients dL/dgains[k] and dL/dphi_k of
 * every repetition k (repetition k plays gains[k] exp(i phi_k) b1), both summed over the scales and the points, and dL/dm0.  It
 * takes mbfir_bloch_train_vjp_batch's arguments through cfz, then
 *   ggain / gphi: one entry per repetition of every pulse, laid out as cosphi; either NULL = not wanted, not both.  The gradient
 *     is per repetition: repetitions that share a gain value share their planes, and each still has its own dL/dgains[k].
 *     dL/dphi_k is the derivative with respect to the angle phi_k of which the table holds (cos phi_k, sin phi_k), the two moved
 *     together along the circle; it is not a derivative with respect to the table's entries.
 *   gmx / gmy / gmz: dL/dm0 as mbfir_bloch_train_vjp_batch returns it, with its bits; all three NULL = not wanted.
 * A gain of exactly 0 is an ordinary repetition with a finite derivative: d amplitude / d gain is the scale, and nothing is divided
 * by a gain.  One upload, three launches and the fold, one download: the forward call's propagator launch; the tangent of the
 * period along its own b1 once per (pulse, scale, distinct gain, 64 points), which leaves the derivative of the 24 doubles of (A, B,
 * A_e, B_e) in the gain in a device workspace (skipped when ggain is NULL); the repetitions walked forwards (a checkpoint before
 * every eighth) and backwards, which contracts the multiplier with those derivatives and with the generator of the z-rotations
 * and leaves one partial per (scale, 256 points, repetition); and the fold over chunks and scales.  There is no reverse sweep
 * over the period's samples.  No atomics: a pulse's gradient bits depend only on the pulse, its grids, its train, its cotangents and
 * the scale list, and not on which of ggain, gphi and gm* are wanted.  b1, gr, tp, t1, t2, df, the positions and meq are not
 * differentiated here.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_batch; further MBFIR_E_ARG cases, each with
 * its reason in mbfir_last_error and no device work done: both ggain and gphi NULL; a cotangent triple or gmx / gmy / gmz only
 * partly given; both cotangent triples NULL; a partial, checkpoint, workspace or workgroup count that overflows.  A refused call
 * leaves the context usable.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_train_vjp_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                      const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                      const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                      const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                      const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                      const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                      const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                      const double* m0y, const double* m0z, const double* cex, const double* cey, const double* cez,
                                      const double* cfx, const double* cfy, const double* cfz, double* ggain, double* gphi,
                                      double* gmx, double* gmy, double* gmz);
/* ---- Tangent of the pulse train with respect to b1 and the initial magnetisation ----------------------------------------------------
 * The Jacobian-vector product of mbfir_bloch_train_batch's echoes and final state: d/de of both at (b1 + e v, m0 + e dm0), e = 0,
 * for ndir directions per pulse (repetition k plays gains[k] exp(i phi_k) (b1 + e v): the chain rule through that product is
 * included).  It takes mbfir_bloch_train_batch's arguments through demod and m0x / m0y / m0z, then
 *   ndir: the directions per pulse, at least 1.
 *   v_re / v_im: direction k of pulse p at ndir toff[p] + k n_p + t, as mbfir_bloch_jvp_batch's.
 *   dm0x / dm0y / dm0z: the m0 directions, pulse p from ndir times its final-plane offset, (direction, scale, frequency, position)
 *     row-major; all three NULL = zero.
 *   ex / ey / ez, fx / fy / fz: the echoes and the final state with mbfir_bloch_train_batch's bits; either triple all NULL = not
 *     downloaded.
 *   dex / dey / dez: the tangent echoes, pulse p from ndir times its echo offset, (direction, scale, repetition, frequency,
 *     position) row-major (with demod != 0: of the demodulated echoes); all three NULL = not wanted.
 *   dfx / dfy / dfz: the tangent of the final state, laid out as dm0; all three NULL = not wanted.  Not both tangent triples NULL.
 * One upload, three launches, one download: the forward call's propagator launch; the period's samples swept once per (pulse,
 * scale, distinct gain, 64 points, group of mbfir_test_bloch_train_jvp_group(0) directions), which leaves the tangents of the 24
 * doubles of (A, B, A_e, B_e) per direction in a device workspace; and the repetitions, per (scale, 256 points, group of
 * mbfir_test_bloch_train_jvp_group(1) directions).  No atomics and no reduction: a tangent's bits depend only on its pulse, scale,
 * point, train and direction.  The gains, the phases, gr, tp, t1, t2, df, the positions and meq are not differentiated.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_batch; further MBFIR_E_ARG cases, each with
 * its reason in mbfir_last_error and no device work done: v_re or v_im NULL; a triple only partly given; both tangent triples NULL;
 * ndir < 1; ndir times the samples, the echoes or the workspace, or a workgroup count, that overflows.  A refused call leaves the
 * context usable.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_train_jvp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z, int ndir,
                                const double* v_re, const double* v_im, const double* dm0x, const double* dm0y, const double* dm0z,
                                double* ex, double* ey, double* ez, double* fx, double* fy, double* fz, double* dex, double* dey,
                                double* dez, double* dfx, double* dfy, double* dfz);
/* mbfir_test_bloch_train_jvp_group (host only): the directions one workgroup of the call above carries, in the period's kernel
 * (which = 0) and in the repetitions' kernel (which != 0); compile-time constants. */
int mbfir_test_bloch_train_jvp_group(int which);
/* ---- Tangent of the pulse train with respect to its schedule: the gain and the RF phase of every repetition ------------------------
 * The Jacobian-vector product of mbfir_bloch_train_batch's echoes and final state: d/de of both at (gains + e dgain, phi + e dphi,
 * m0 + e dm0), e = 0, for ndir directions per pulse (repetition k plays gains[k] exp(i phi_k) b1).  It takes
 * mbfir_bloch_train_jvp_batch's arguments through m0x / m0y / m0z and ndir, then
 *   dgain / dphi: the directions of the gains and of the phases (per radian, of the angle phi_k of which the table holds the cosine
 *     and the sine), direction k of pulse p at ndir roff[p] + k ntr_p + repetition; either NULL = that part does not move.  A
 *     direction is per repetition: repetitions that share a gain value still move separately.
 *   dm0x / dm0y / dm0z, ex .. fz, dex .. dfz: as mbfir_bloch_train_jvp_batch's.
 * With the ntr unit directions of the gains followed by the ntr of the phases one call returns the whole Jacobian of the echoes in
 * the schedule.  A gain of exactly 0 is an ordinary repetition: nothing is divided by a gain.  One upload, three launches (two
 * when dgain is NULL), one download: the forward call's propagator launch; the tangent of the period along its own b1 once per
 * (pulse, scale, distinct gain, 64 points), as mbfir_bloch_train_vjp_sched_batch runs it, whatever ndir is: the workspace is twice
 * the forward call's; and the repetitions, per (scale, 256 points, group of mbfir_test_bloch_train_sched_jvp_group() directions).
 * There is no sweep over the period's samples per direction.  No atomics and no reduction: a tangent's bits depend only on its
 * pulse, scale, point, train and direction, not on ndir, on its place among the directions or on which of dgain, dphi and dm0 are
 * given (a NULL part is a part of zeros).  b1, gr, tp, t1, t2, df, the positions and meq are not differentiated here.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_batch; further MBFIR_E_ARG cases, each with
 * its reason in mbfir_last_error and no device work done: a triple only partly given; dgain, dphi and the dm0 triple all NULL; both
 * tangent triples NULL; ndir < 1; ndir times the repetitions or the echoes, the workspace, or a workgroup count, that overflows.  A
 * refused call leaves the context usable.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_train_jvp_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                      const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                      const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                      const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                      const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                      const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                      const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                      const double* m0y, const double* m0z, int ndir, const double* dgain, const double* dphi,
                                      const double* dm0x, const double* dm0y, const double* dm0z, double* ex, double* ey, double* ez,
                                      double* fx, double* fy, double* fz, double* dex, double* dey, double* dez, double* dfx,
                                      double* dfy, double* dfz);
/* mbfir_test_bloch_train_sched_jvp_group (host only): the directions one workgroup of the call above carries; a compile-time
 * constant. */
int mbfir_test_bloch_train_sched_jvp_group(void);

/* ---- Fused least-squares and Gauss-Newton products of the pulse train -------------------------------------------------------------
 * For the loss, per pulse,
 *   L = 1/2 sum_s sum_k rw_k sum_points sum_c w_c (echo_{k,c} - t_c)^2 + 1/2 sum_s sum_points sum_c wf_c (m_{N,c} - tf_c)^2
 * with echo and m_N what mbfir_bloch_train_batch returns under the same demod, mbfir_bloch_train_lsq_batch returns L, its gradient
 * dL/dRe b1 + i dL/dIm b1 of the period's samples (mbfir_bloch_train_vjp_batch's conventions for scales and gains) and on request
 * dL/dm0; mbfir_bloch_train_gn_batch returns H v = J' W J v for ndir directions of the period's b1, J the Jacobian of (echoes, final
 * state) in b1 and W the weights, rw included.  Neither the echoes nor their cotangents ever leave the device.  Both take
 * mbfir_bloch_train_batch's arguments through demod and m0x / m0y / m0z, then
 *   ebcast: 0 = the echo planes below lie as the echoes do (S x ntr x nf x npos per pulse); 1 = they lie as the final planes do
 *           (S x nf x npos per pulse) and are used at every repetition;
 *   wx / wy / wz, tx / ty / tz (lsq) or wx / wy / wz (gn): the echo weights (>= 0, finite) and targets; all NULL = no echo term;
 *   rw: one factor >= 0 per repetition, laid out as cosphi (pulse p from roff[p]); NULL = ones;
 *   wfx .. tfz (lsq) or wfx / wfy / wfz (gn): the final weights and targets, laid out as the final planes; all NULL = no final term;
 *   lsq: loss (npulse), g_re / g_im (the gradient per b1 sample), gmx / gmy / gmz (dL/dm0, the final planes' layout; all NULL = not
 *        wanted);
 *   gn:  ndir >= 1, v_re / v_im (direction k of pulse p at ndir toff[p] + k ntime_p, as mbfir_bloch_train_jvp_batch takes them),
 *        h_re / h_im (the products, the same layout).
 * At least one of the two terms must be present.  No atomics: a pulse's loss, gradient and products depend only on the pulse, its
 * grids, its train, its planes and the scale list, and a direction's product depends neither on ndir nor on its place among the
 * directions.  Targets equal to mbfir_bloch_train_batch's own output give L = 0 and a gradient of exact zeros.  The gains, the
 * phases, gr, tp, t1, t2, df, the positions, meq and the scales are not differentiated; m0 is not a variable of gn.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_batch; further MBFIR_E_ARG cases, each with a
 * message beginning "bloch_train_lsq_batch:" / "bloch_train_gn_batch:": ebcast outside {0, 1}, a partly given sextuple or triple,
 * both terms absent, a NULL output or direction plane, ndir < 1, a negative or non-finite weight or rw, sizes that overflow.
 * A NULL ctx returns MBFIR_E_ARG. */
int mbfir_bloch_train_lsq_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                                const double* wz, const double* tx, const double* ty, const double* tz, const double* rw,
                                const double* wfx, const double* wfy, const double* wfz, const double* tfx, const double* tfy,
                                const double* tfz, double* loss, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz);
int mbfir_bloch_train_gn_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                               const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                               int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                               const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                               const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                               const double* wz, const double* rw, const double* wfx, const double* wfy, const double* wfz, int ndir,
                               const double* v_re, const double* v_im, double* h_re, double* h_im);
/* ---- Fused least-squares and Gauss-Newton products of the pulse train's schedule ----------------------------------------------------
 * The loss L of the two calls above with the gain and the RF phase of every repetition as the variable (repetition k plays
 * gains[k] exp(i phi_k) b1).  mbfir_bloch_train_lsq_sched_batch takes mbfir_bloch_train_lsq_batch's arguments through wfx .. tfz,
 * then the outputs
 *   loss (npulse); ggain / gphi: dL/dgains[k] and dL/dphi_k (per radian) of every repetition, laid out as cosphi (roff[npulse]
 *     doubles each; either NULL = not wanted, not both), what mbfir_bloch_train_vjp_sched_batch returns at the cotangents
 *     ce_k = rw_k w (echo_k - t), cf = wf (m_N - tf); gmx / gmy / gmz: dL/dm0 in the final planes' layout (all NULL = not wanted).
 * mbfir_bloch_train_gn_sched_batch takes mbfir_bloch_train_gn_batch's arguments through wfx / wfy / wfz (weights without targets),
 * then
 *   ndir >= 1; dgain / dphi: the directions, laid out as mbfir_bloch_train_jvp_sched_batch takes them (direction k of pulse p at
 *     ndir roff[p] + k ntr_p; either NULL = zeros, not both); hgain / hphi: the two halves of H v = J' W J v in the same layout
 *     (either NULL = not wanted, not both), J the Jacobian of (echoes, final state) in (gains, phases), W the weights, rw included.
 * Neither the echoes, their tangents nor their cotangents leave the device: what comes back is 2 ntr numbers per pulse and
 * direction.  One upload, three launches and a fold, one download; the period is swept once more per (scale, distinct gain) only
 * when a gains direction or a gains output is asked for, and the workspace is twice the forward call's whatever ndir is.  With
 * the 2 ntr unit directions one gn call returns the dense normal matrix of the schedule, rows as directions.  No atomics: a
 * pulse's loss, gradient and products depend only on the pulse, its grids, its train, its planes and the scale list; a
 * direction's product depends neither on ndir, nor on its place among the directions, nor on whether an all-zero half was passed
 * as NULL; a wanted half does not depend on whether the other was asked for.  Targets equal to mbfir_bloch_train_batch's own
 * output give L = 0 and gradients of exact zeros.  m0 is not a variable of gn; b1, gr, tp, t1, t2, df, the positions, meq and the
 * scales are not differentiated.
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_train_batch; further MBFIR_E_ARG cases, each with a
 * message beginning "bloch_train_lsq_sched_batch:" / "bloch_train_gn_sched_batch:" and no device work done: ebcast outside {0, 1}, a
 * partly given sextuple or triple, both terms absent, both outputs NULL, both direction parts NULL, ndir < 1, sizes that overflow
 * (the workspace, and the partials, checkpoints and workgroups times ndir), a negative or non-finite weight or rw.  A refused call
 * leaves the context usable.  A NULL ctx returns MBFIR_E_ARG. */
int mbfir_bloch_train_lsq_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                      const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                      const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                      const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                      const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                      const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                      const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                      const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                                      const double* wz, const double* tx, const double* ty, const double* tz, const double* rw,
                                      const double* wfx, const double* wfy, const double* wfz, const double* tfx, const double* tfy,
                                      const double* tfz, double* loss, double* ggain, double* gphi, double* gmx, double* gmy,
                                      double* gmz);
int mbfir_bloch_train_gn_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                     const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                     const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                     const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                                     const double* wz, const double* rw, const double* wfx, const double* wfy, const double* wfz,
                                     int ndir, const double* dgain, const double* dphi, double* hgain, double* hphi);
/* ---- Adjoint of mbfir_bloch_batch's steady state with respect to b1, the gradient waveform and the off-resonance -------------------
 * mbfir_bloch_ss_vjp_batch with four more outputs after its own 31 arguments.  dM = (I - A)^-1 dF at m0 = M holds for every
 * parameter of the period, so these are mbfir_bloch_vjp_gr_batch's outputs on the sweep started from m0 = M with the end cotangent
 * (I - A)^-T c, fused into one kernel that starts with mode 1's own sweep:
 *   ggx / ggy / ggz: one entry per sample of every pulse, laid out as gx / gy / gz: dL/dgx, dL/dgy, dL/dgz, summed over the points
 *     of the pulse and over the scales without a factor (a scale multiplies b1, not the gradient).  All three are required; a NULL
 *     input plane gx / gy / gz (an axis no pulse plays) is differentiated at zero and its gradient is returned all the same.
 *   gdf: dL/ddf of every (scale, frequency, position), S x nf x npos per pulse in the layout of the cotangents; the caller sums
 *     over whatever shares an off-resonance.  NULL = not wanted: it is then neither formed nor downloaded.
 * There is no m0 and no dL/dm0.  g_re / g_im are those of mbfir_bloch_ss_vjp_batch to rounding (the sums run over other sub-groups
 * of the same order), not promised to the bit; mx / my / mz receive M with mode 1's bits.  tp, t1, t2, the positions and the scales
 * are not differentiated.  The error grows with kappa = ||(I - A)^-1|| as mbfir_bloch_ss_vjp_batch's does, dL/ddf's with its
 * square; there is no guard on det(I - A).  The launch shape, staging and checkpoints are mbfir_bloch_ss_vjp_batch's; one upload,
 * two launches (the three sweeps with one partial per workgroup, sample and component; then the fold of mbfir_bloch_vjp_gr_batch),
 * one download; no atomics, so the bits of every result depend only on the pulse, its grids, its cotangents and the scale list.
 * Argument checks and MBFIR_E_ARG messages as mbfir_bloch_ss_vjp_batch's (a cotangent or gradient plane NULL; mx / my / mz only
 * partly given; a partial or checkpoint count that overflows), and one more case: a NULL ggx, ggy or ggz.  Each names
 * bloch_ss_vjp_gr_batch in mbfir_last_error and no device work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_ss_vjp_gr_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const double* cmx, const double* cmy, const double* cmz,
                                double* g_re, double* g_im, double* mx, double* my, double* mz, double* ggx, double* ggy,
                                double* ggz, double* gdf);
/* ---- Least-squares products of mbfir_bloch_batch ----------------------------------------------------------------------------------
 * For the end point (mx, my, mz) of mbfir_bloch_batch (mode 0), relaxation included, weights (wx, wy, wz) >= 0 and targets (tx, ty,
 * tz) per output entry, the loss of a pulse is L = 1/2 sum w_c (m_c - t_c)^2 over c = x, y, z, its points and its scales, and J =
 * dm / db1 is the Jacobian of the end point with respect to the b1 samples (real-linear, as in mbfir_bloch_jvp_batch).  The end
 * point is its own profile: there is no profile argument.  The forward call's input arguments up to nscale and scales come first
 * (no mode), then m0x / m0y / m0z as mbfir_bloch_vjp_batch takes them (all three NULL = [0 0 1] everywhere), then wx / wy / wz
 * (and tx / ty / tz), laid out as the mode-0 outputs.
 *   lsq: loss[npulse] receives L per pulse, g_re / g_im (laid out as b1) the gradient J' W (m - t) = dL/dRe b1 + i dL/dIm b1.
 *   gn:  ndir >= 1 directions per pulse in v_re / v_im, laid out as mbfir_bloch_jvp_batch lays them out; h_re / h_im receive the
 *        Gauss-Newton products sum_s s J_s' W_s J_s (s v), pulse p from ndir toff[p], direction-major.
 * Each is one upload, one sweep launch (one workgroup per forward workgroup, and for gn per direction: mbfir_bloch_vjp_batch's two
 * sweeps with the cotangent w (m - t), or w dm of a tangent carried through the forward sweep, formed at the point) plus a fold,
 * and one download of the n (ndir n) complex results per pulse and the losses: nothing of point size comes back; the partials and
 * the checkpoints stay on the device.  No atomics: a pulse's g, L and H v bits depend only on the pulse, its grids, its weights,
 * target or direction, m0 and the scale list, not on the batch, its order or ndir.  A point of weight 0 contributes exact zeros,
 * and so does scale 0 to g and H v.  dL/dm0 and m0 directions are not part of these calls.  The argument checks and their
 * MBFIR_E_ARG messages are those of mbfir_bloch_batch, then in this order, each with its reason in mbfir_last_error: a weight,
 * target, direction or output plane NULL; m0x / m0y / m0z only partly given; a negative or non-finite weight; ndir < 1; partials,
 * checkpoints or a workgroup count that overflow.  No device work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_lsq_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                          const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                          const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                          const double* m0x, const double* m0y, const double* m0z, const double* wx, const double* wy,
                          const double* wz, const double* tx, const double* ty, const double* tz, double* loss, double* g_re,
                          double* g_im);
int mbfir_bloch_gn_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                         const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                         const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                         const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                         const double* m0x, const double* m0y, const double* m0z, const double* wx, const double* wy,
                         const double* wz, int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im);
/* ---- Least-squares products of the steady state of mbfir_bloch_batch ----------------------------------------------------------------
 * For the steady state M = (mx, my, mz) of mbfir_bloch_batch (mode 1), weights (wx, wy, wz) >= 0 and targets (tx, ty, tz) per output
 * entry, the loss of a pulse is L = 1/2 sum w_c (M_c - t_c)^2 over c = x, y, z, its points and its scales, and J = dM / db1 is the
 * Jacobian of the steady state with respect to the b1 samples (real-linear, as in mbfir_bloch_ss_jvp_batch).  The forward call's
 * input arguments up to nscale and scales come first (no mode, and no m0: the steady state does not depend on it), then wx / wy / wz
 * (and tx / ty / tz), laid out as the mode-1 outputs.
 *   lsq: loss[npulse] receives L per pulse, g_re / g_im (laid out as b1) the gradient sum_s s J_s' W_s (M_s - t_s) = dL/dRe b1 + i
 *        dL/dIm b1; mx / my / mz (all three NULL: not wanted) receive M with mbfir_bloch_batch's bits.  The residual is formed from
 *        that M: targets equal to mode 1's own output give L = 0 and g = 0 exactly.
 *   gn:  ndir >= 1 directions per pulse in v_re / v_im, laid out as mbfir_bloch_jvp_batch lays them out; h_re / h_im receive the
 *        Gauss-Newton products sum_s s J_s' W_s J_s (s v), pulse p from ndir toff[p], direction-major.
 * Each is one upload, one sweep launch (one workgroup per forward workgroup, and for gn per direction) plus a fold, and one download
 * of the n (ndir n) complex results per pulse and the losses: nothing of point size comes back unless M is asked for.  No atomics:
 * a pulse's L, g and H v bits depend only on the pulse, its grids, its weights, target or direction and the scale list, not on the
 * batch, its order or ndir.  A point of weight 0 contributes exact zeros, and so does scale 0 to g and H v.  No guard on det(I - A).
 * The argument checks and their MBFIR_E_ARG messages are those of mbfir_bloch_batch at mode 1, then in this order, each with its
 * reason in mbfir_last_error: a weight, target, direction or output plane NULL; mx / my / mz only partly given; a negative or
 * non-finite weight; ndir < 1; partials, checkpoints, inverse planes or a workgroup count that overflow.  No device work is done
 * before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_ss_lsq_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* wx, const double* wy, const double* wz, const double* tx,
                             const double* ty, const double* tz, double* loss, double* g_re, double* g_im, double* mx, double* my,
                             double* mz);
int mbfir_bloch_ss_gn_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* wx, const double* wy, const double* wz, int ndir, const double* v_re,
                            const double* v_im, double* h_re, double* h_im);
/* ---- Tangents of mbfir_abr_batch / mbfir_abr2_batch with respect to the rf samples ----------------------------------------------
 * The Jacobian-vector product of the forward call, in both models: the forward call's inputs, then ndir >= 1 directions for every
 * pulse in v_re / v_im, direction-major within a pulse (sample m of direction k of pulse p at ndir roff[p] + k n_p + m), then the
 * forward call's four output planes and four more for the tangents.  (da, db) is the first-order change of (a, b) when rf moves
 * along the direction: d/dt (a, b)(rf + t v) at t = 0, real-linear in v (scale s contributes the tangent along s v at s rf).  a /
 * b: laid out as the forward call lays them out, with its bits; the four may be NULL together, and the primal is then not
 * downloaded.  da / db (re, im planes): pulse p starts at ndir times its forward offset and is laid out (direction, scale, point)
 * row-major, the point index as in the forward call.  g / gx / gy, the grids and the scales are not differentiated.  One upload,
 * one launch (one workgroup per forward workgroup and group of mbfir_test_jvp_group() directions, which share each sample's
 * trigonometry), one download; no atomics, and a tangent's bits depend only on its pulse, scale, point and direction: not on the
 * batch, its order, ndir or the direction's place among the others.  The argument checks and their MBFIR_E_ARG messages are those of
 * the forward calls (a v, da or db plane NULL, or some but not all of a / b NULL, is a required array NULL), then ndir < 1, then a
 * direction array, tangent output or workgroup count that overflows; no device work is done before they pass. */
int mbfir_abr_jvp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                        int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int ndir,
                        const double* v_re, const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im,
                        double* da_re, double* da_im, double* db_re, double* db_im);
int mbfir_abr2_jvp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                         const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                         const double* y, int nscale, const double* scales, int mode, int ndir, const double* v_re,
                         const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im, double* da_re, double* da_im,
                         double* db_re, double* db_im);
/* ---- Least-squares products of mbfir_abr_batch / mbfir_abr2_batch ---------------------------------------------------------------
 * For a profile f(a, b) of the forward call's outputs, a real weight w >= 0 and a target t per output entry, the loss of a pulse is
 * L = 1/2 sum w |f - t|^2 over its points and scales, and J = df / drf is the Jacobian of the profile with respect to the rf samples
 * (real-linear, as in the tangent calls).  profile: 0 ex f = 2 conj(a) b, 1 se f = i b^2, 2 inv (sat) f = 1 - 2 |b|^2, 3 st
 * f = i a^2.  The forward call's inputs come first, mode included; w (and t_re / t_im) are laid out as the forward call lays out a.
 *   lsq: loss[npulse] receives L per pulse, g_re / g_im the gradient J^H W (f - t) = dL / d Re rf + i dL / d Im rf per rf sample.
 *        t_im may be NULL (a real target); for profile 2, whose f is real, t_im is not read.
 *   gn:  ndir >= 1 directions per pulse in v_re / v_im, laid out as mbfir_abr_jvp_batch lays them out; h_re / h_im receive the
 *        Gauss-Newton products J^H W J v, pulse p from ndir roff[p], direction-major.
 * Each is one upload, one sweep launch (one workgroup per forward workgroup, and for gn per direction) plus a fold, and one
 * download of the n (ndir n) complex results per pulse and the losses: nothing of point size comes back.  No atomics: a pulse's
 * g, L and H v bits depend only on the pulse, its grid, its weights, target or direction and the scale list, not on the batch, its
 * order or ndir.  A point of weight 0 contributes exact zeros, and so does scale 0 to g and H v.  The argument checks and their
 * MBFIR_E_ARG messages are those of the forward calls, then in this order: w, t_re, v_re, v_im or an output NULL ("a required array
 * is null"); profile out of range; a negative or non-finite weight; ndir < 1; partials or a workgroup count that overflow.  No
 * device work is done before they pass. */
int mbfir_abr_lsq_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                        int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int profile,
                        const double* w, const double* t_re, const double* t_im, double* loss, double* g_re, double* g_im);
int mbfir_abr2_lsq_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                         const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                         const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                         const double* t_re, const double* t_im, double* loss, double* g_re, double* g_im);
int mbfir_abr_gn_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                       int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int profile,
                       const double* w, int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im);
int mbfir_abr2_gn_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                        const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                        const double* y, int nscale, const double* scales, int mode, int profile, const double* w, int ndir,
                        const double* v_re, const double* v_im, double* h_re, double* h_im);
/* mbfir_abr_lm_step_batch / mbfir_abr2_lm_step_batch: one damped Gauss-Newton (Levenberg-Marquardt) step per pulse, solved on the
 * device: conjugate gradients on (H + mu[p] I) d = b from d = 0 in the real inner product <u, v> = sum Re(conj(u) v), H = J^H W J
 * as in mbfir_abr_gn_batch, at most cg iterations, while <r, r> > rtol <b, b>.  The arguments up to w are those of mbfir_abr_gn_batch
 * / mbfir_abr2_gn_batch; b_re, b_im are laid out as rf is.  With t_re (and t_im; NULL for a real target) the loss and gradient of
 * mbfir_abr_lsq_batch at rf + d are returned too; t_re and t_im both NULL: solve only, and loss, g_re, g_im may be NULL.
 * Outputs per pulse: d, ncg (iterations done), rr (the last <r, r>), gg (<b, b>), status (0: the tolerance was reached, 1: the cap
 * cg was reached, 2: breakdown, <p, (H + mu) p> not finite or not > 0; d, rr and ncg are then those before that iteration).
 * One upload, a chain of launches (two per CG iteration), one download; the host reads nothing in between, so cg is also a launch
 * count: all 2 cg launches are queued whatever rtol stops, the workgroups of a pulse that has stopped returning at once.  A pulse's outputs
 * depend only on the pulse, its grid, weights, target, b, mu, cg, rtol and the scale list: not on the batch, its order, or when its
 * neighbours stop.  The checks are those of mbfir_abr_gn_batch at ndir = 1 in their order, then: b, mu or a required output NULL
 * ("a required array is null"); a negative or non-finite mu; cg < 0; a negative or NaN rtol; sections that overflow.  No device
 * work is done before they pass. */
int mbfir_abr_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                            int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int profile,
                            const double* w, const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                            const double* t_re, const double* t_im, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                            int* status, double* loss, double* g_re, double* g_im);
int mbfir_abr2_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                             const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                             const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                             const double* b_re, const double* b_im, const double* mu, int cg, double rtol, const double* t_re,
                             const double* t_im, double* d_re, double* d_im, int* ncg, double* rr, double* gg, int* status,
                             double* loss, double* g_re, double* g_im);
/* mbfir_bloch_lm_step_batch: the step above for the Bloch model with relaxation: conjugate gradients on (H + mu[p] I) d = b from
 * d = 0 in the real inner product <u, v> = sum Re(conj(u) v), H = sum_s s J_s' W_s J_s (s .) as in mbfir_bloch_gn_batch, at most cg
 * iterations, while <r, r> > rtol <b, b>.  The arguments up to wx, wy, wz are those of mbfir_bloch_gn_batch; b_re, b_im are laid out
 * as b1 is.  With tx, ty, tz the loss and gradient of mbfir_bloch_lsq_batch at b1 + d (one IEEE addition per part) are returned
 * too, with that call's bits; all three NULL: solve only, and loss, g_re, g_im may be NULL.  Outputs per pulse: d, ncg (iterations
 * done), rr (the last <r, r>), gg (<b, b>), status (0: the tolerance was reached, 1: the cap cg was reached, 2: breakdown,
 * <p, (H + mu) p> not finite or not > 0; d, rr and ncg are then those before that iteration).  H p has the bits of
 * mbfir_bloch_gn_batch on the same p.  One upload, a chain of launches (two per CG iteration), one download; the host reads nothing
 * in between, so cg is also a launch count: all 2 cg launches are queued whatever rtol stops, the workgroups of a pulse that has
 * stopped returning at once.  The partials and the checkpoints of one direction are allocated once and serve every iteration and
 * the trial; they, r, H p and the trial's input rows stay on the device.  A pulse's outputs depend only on the pulse, its grids,
 * weights, targets, m0, b, mu, cg, rtol and the scale list: not on the batch, its order, or when its neighbours stop.  The checks
 * are those of mbfir_bloch_gn_batch at ndir = 1 in their order and with their messages, then: b, mu or a required output NULL ("a
 * required array is null"); tx, ty, tz only partly given; a negative or non-finite mu; cg < 0; a negative or NaN rtol; sections or
 * a workgroup count that overflow.  No device work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                              const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                              const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                              const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                              int nscale, const double* scales, const double* m0x, const double* m0y, const double* m0z,
                              const double* wx, const double* wy, const double* wz, const double* b_re, const double* b_im,
                              const double* mu, int cg, double rtol, const double* tx, const double* ty, const double* tz,
                              double* d_re, double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss, double* g_re,
                              double* g_im);
/* mbfir_bloch_ss_lm_step_batch: the step above for the steady state of the period (mbfir_bloch_batch's mode 1): conjugate gradients
 * on (H + mu[p] I) d = b from d = 0, H = sum_s s J_s' W_s J_s (s .) as in mbfir_bloch_ss_gn_batch at the call's b1, weights and
 * scales, at most cg iterations, while <r, r> > rtol <b, b>.  The arguments up to wx, wy, wz are those of mbfir_bloch_ss_gn_batch
 * (there is no m0); b_re, b_im are laid out as b1 is.  With tx, ty, tz the loss and gradient of mbfir_bloch_ss_lsq_batch at b1 + d
 * (one IEEE addition per part) are returned too, with that call's bits; all three NULL: solve only, and loss, g_re, g_im may be
 * NULL.  Outputs per pulse as for mbfir_bloch_lm_step_batch: d, ncg, rr, gg, status (0: the tolerance was reached, 1: the cap cg
 * was reached, 2: breakdown).  H p has the bits of mbfir_bloch_ss_gn_batch on the same p.  b1 is fixed within the solve, so
 * (I - A)^-1 and M of a pulse are computed once per call, not once per iteration.  One upload, a chain of launches (one, then two
 * per CG iteration), one download; the host reads nothing in between, so cg is also a launch count.  The partials and the
 * checkpoints of one direction serve every iteration and the trial; they, r, H p, (I - A)^-1, M and the trial's input rows stay
 * on the device.  No guard on det(I - A).  A pulse's outputs depend only on the pulse, its grids, weights, targets, b, mu, cg, rtol
 * and the scale list: not on the batch, its order, or when its neighbours stop.  The checks are those of mbfir_bloch_batch at mode
 * 1 and of mbfir_bloch_ss_gn_batch at ndir = 1 in their order and with their messages, then: b, mu or a required output NULL ("a
 * required array is null"); tx, ty, tz only partly given; a negative or non-finite mu; cg < 0; a negative or NaN rtol; sections,
 * planes or a workgroup count that overflow.  No device work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_ss_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                 const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                 const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                 const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                 const double* dz, int nscale, const double* scales, const double* wx, const double* wy,
                                 const double* wz, const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                                 const double* tx, const double* ty, const double* tz, double* d_re, double* d_im, int* ncg,
                                 double* rr, double* gg, int* status, double* loss, double* g_re, double* g_im);
/* Magnitude targets: the six calls mbfir_bloch_lsq_batch, mbfir_bloch_gn_batch, mbfir_bloch_lm_step_batch,
 * mbfir_bloch_ss_lsq_batch, mbfir_bloch_ss_gn_batch and mbfir_bloch_ss_lm_step_batch each have a twin that fits the transverse
 * magnitude |Mxy| and mz instead of the vector (mx, my, mz).  With m the end point (mode 0) or the steady state (mode 1) of a point,
 *     rho = sqrt(mx mx + my my)   (each product, the sum and the root rounded once: np.sqrt(mx * mx + my * my) on the forward
 *                                  call's output has its bits)
 *     u   = (mx, my) / rho, and (0, 0) where rho = 0
 *     L   = 1/2 sum w_xy (rho - t_xy)^2 + w_z (mz - t_z)^2
 *     g   = J' c,      c = (w_xy (rho - t_xy) u_x, w_xy (rho - t_xy) u_y, w_z (mz - t_z))
 *     H v = J' U' W U J v:  c = (w_xy (u . dm_xy) u_x, w_xy (u . dm_xy) u_y, w_z dm_z),  dm = J v
 * A twin takes its component call's arguments with wx, wy, wz replaced by the pair wxy, wz and tx, ty, tz by the pair txy, tz, the
 * planes laid out as before (O entries each); every other argument, the outputs, the launches, the transfers and the guarantees
 * on the bits are the component call's, and so are the argument checks, their order and their messages ("only partly given"
 * refers to the pair: "txy and tz are given together or not at all").  rho = 0 is not an error: the transverse term then adds
 * 1/2 w_xy t_xy^2 to L and exact zeros to g and H v.  A negative t_xy is accepted.  Fitting |Mxy| alone is w_z = 0.  L and g are
 * those of the component call at the target (t_xy u_x, t_xy u_y, t_z) with the weights (w_xy, w_xy, w_z); H is not the component
 * call's at any weights: it drops the curvature across u. */
int mbfir_bloch_lsq_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                              const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                              const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                              const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                              int nscale, const double* scales, const double* m0x, const double* m0y, const double* m0z,
                              const double* wxy, const double* wz, const double* txy, const double* tz, double* loss, double* g_re,
                              double* g_im);
int mbfir_bloch_gn_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                             const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                             int nscale, const double* scales, const double* m0x, const double* m0y, const double* m0z,
                             const double* wxy, const double* wz, int ndir, const double* v_re, const double* v_im, double* h_re,
                             double* h_im);
int mbfir_bloch_ss_lsq_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                 const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                 const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                 const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                 const double* dz, int nscale, const double* scales, const double* wxy, const double* wz,
                                 const double* txy, const double* tz, double* loss, double* g_re, double* g_im, double* mx,
                                 double* my, double* mz);
int mbfir_bloch_ss_gn_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                const double* dz, int nscale, const double* scales, const double* wxy, const double* wz, int ndir,
                                const double* v_re, const double* v_im, double* h_re, double* h_im);
int mbfir_bloch_lm_step_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                  const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                  const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                  const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                  const double* dz, int nscale, const double* scales, const double* m0x, const double* m0y,
                                  const double* m0z, const double* wxy, const double* wz, const double* b_re, const double* b_im,
                                  const double* mu, int cg, double rtol, const double* txy, const double* tz, double* d_re,
                                  double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss, double* g_re,
                                  double* g_im);
int mbfir_bloch_ss_lm_step_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const double* wxy, const double* wz,
                                     const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                                     const double* txy, const double* tz, double* d_re, double* d_im, int* ncg, double* rr,
                                     double* gg, int* status, double* loss, double* g_re, double* g_im);
/* mbfir_bloch_train_lm_step_batch: the step above for the echoes of a pulse train (mbfir_bloch_train_batch): conjugate
 * gradients on (H + mu[p] I) d = b from d = 0, H = J' W J as in mbfir_bloch_train_gn_batch at the call's b1, train, weights, rw and
 * scales (echo term, final term, the scales' and gains' chain rule), at most cg iterations, while <r, r> > rtol <b, b>.  The
 * arguments up to wfx, wfy, wfz are those of mbfir_bloch_train_gn_batch; b_re, b_im are laid out as b1 is.  tx, ty, tz: the echo
 * targets, laid out as the echo weights are under ebcast; tfx, tfy, tfz: the final targets.  With targets the loss and gradient of
 * mbfir_bloch_train_lsq_batch at b1 + d (one IEEE addition per part) are returned too, with that call's bits; all six NULL: solve
 * only, and loss, g_re, g_im may be NULL.  Outputs per pulse as for mbfir_bloch_lm_step_batch: d, ncg, rr, gg, status (0: the
 * tolerance was reached, 1: the cap cg was reached, 2: breakdown).  H p has the bits of mbfir_bloch_train_gn_batch on the same p.
 * b1 is fixed within the solve, so the propagators' planes and the checkpoints of the period adjoint's forward half are computed
 * once per call.  One upload, a chain of launches (three, then a memset and four per CG iteration, six and a memset for the
 * trial), one download; the host reads nothing in between, so cg is also a launch count.  The tangent planes, the cotangent planes,
 * the partials and the checkpoints of one direction serve every iteration and the trial; they, r, H p, the primal planes and the
 * trial's input rows stay on the device.  A pulse's outputs depend only on the pulse, its grids, its train, weights, targets, m0, b,
 * mu, cg, rtol and the scale list: not on the batch, its order, or when its neighbours stop.  The checks are those of
 * mbfir_bloch_train_batch and of mbfir_bloch_train_gn_batch at ndir = 1 (ebcast, the weights, the sizes) in their order and with
 * their messages, then: b, mu or a required output NULL ("a required array is null"); a negative or non-finite mu; cg < 0; a
 * negative or NaN rtol; sections that overflow; then, with a message beginning "bloch_train_lm_step_batch:", a target triple only
 * partly given, a target for a term that has no weights, or, when a target is given, none for a term that has weights.  No device
 * work is done before they pass.  A NULL context returns MBFIR_E_ARG. */
int mbfir_bloch_train_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                    const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                    const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                    const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                    const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                    const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                    const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                    const double* m0z, int ebcast, const double* wx, const double* wy, const double* wz,
                                    const double* rw, const double* wfx, const double* wfy, const double* wfz, const double* b_re,
                                    const double* b_im, const double* mu, int cg, double rtol, const double* tx, const double* ty,
                                    const double* tz, const double* tfx, const double* tfy, const double* tfz, double* d_re,
                                    double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss, double* g_re,
                                    double* g_im);
/* mbfir_bloch_train_lm_step_sched_batch: the Levenberg-Marquardt step of the train's schedule, the gain and the RF phase of every
 * repetition.  One call evaluates and solves at the same schedule, so the propagators of a schedule are computed once:
 *   1. with targets, loss / ggain / gphi: L, dL/dgains and dL/dphases at the call's schedule, with the bits of
 *      mbfir_bloch_train_lsq_sched_batch;
 *   2. conjugate gradients on (H + mu[p] I) d = b from d = 0, H = J' W J restricted to the varied halves as
 *      mbfir_bloch_train_gn_sched_batch applies it at that schedule, at most cg iterations, while <r, r> > rtol <b, b>.
 * There is no trial at schedule + d: a trial has other gains and tables, which the host stages; evaluating the trial with the next
 * call solves the next step at the same time.  The arguments through tfz are those of mbfir_bloch_train_lsq_sched_batch; all six
 * target planes may be NULL (solve only; loss, ggain, gphi may then be NULL).  bgain / bphi: the right-hand side, laid out as cosphi;
 * both NULL with targets: b = -g of 1., negated exactly and left on the device; given: used, and 1. is still returned.  dgain / dphi:
 * the step, laid out as cosphi; either NULL marks that half as not varied (not both): its direction is zeros, its product is never
 * read, its b and g must be NULL, and without the gains the period's tangent is not launched.  ncg, rr, gg, status per pulse as for
 * mbfir_bloch_train_lm_step_batch (0: the tolerance was reached, 1: the cap cg was reached, 2: breakdown, a <p, (H + mu I) p> that
 * is not finite or not > 0).  cg = 0 with targets is mbfir_bloch_train_lsq_sched_batch and d = 0.  The inner product runs over the
 * varied halves by a fixed tree; no atomics.  H p has the bits of mbfir_bloch_train_gn_sched_batch on the same p.  One upload, a
 * chain of launches (up to five, then two per CG iteration), one download; the host reads nothing in between.  A pulse's outputs
 * depend only on the pulse, its grids, its train, weights, targets, m0, b, mu, cg, rtol and the scale list: not on the batch, its
 * order, or when its neighbours stop.  The checks are those of mbfir_bloch_train_batch, then those the two calls above share at
 * ndir = 1 (ebcast, the weights, both terms absent, both halves NULL, the sizes at two checkpointed states).  Targets are optional
 * here, so the weights are checked in mbfir_bloch_train_gn_sched_batch's wording ("the echo weights are given together or not at
 * all", "the final weights ...") and two of mbfir_bloch_train_lsq_sched_batch's messages cannot occur: "the echo / final weights and
 * targets are given together or not at all" (the target messages below take its place) and "the loss plane is null" (a NULL loss
 * with targets is "a required array is null"); "both halves NULL" reads "neither the gains nor the phases vary: dgain and dphi are
 * both null".  Then: mu or a required output NULL ("a required array is null"); a negative or non-finite mu ("a damping mu is
 * negative or not finite", as in mbfir_bloch_train_lm_step_batch); cg < 0; a negative or NaN rtol; sections that overflow; a b or g for a half that does
 * not vary; a target triple only partly given, a target for a term that has no weights, or, when a target is given, none for a term
 * that has weights; b given for one varied half only; neither targets nor b.  No device work is done before they pass.  A NULL
 * context returns MBFIR_E_ARG. */
int mbfir_bloch_train_lm_step_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                          const double* gx, const double* gy, const double* gz, const long* tsoff,
                                          const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                          const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                          const double* dy, const double* dz, int nscale, const double* scales, const int* ntr,
                                          const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                                          const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                                          const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wx,
                                          const double* wy, const double* wz, const double* tx, const double* ty, const double* tz,
                                          const double* rw, const double* wfx, const double* wfy, const double* wfz, const double* tfx,
                                          const double* tfy, const double* tfz, const double* bgain, const double* bphi,
                                          const double* mu, int cg, double rtol, double* dgain, double* dphi, int* ncg, double* rr,
                                          double* gg, int* status, double* loss, double* ggain, double* gphi);
/* Magnitude targets for the pulse train: the six train calls mbfir_bloch_train_lsq_batch, mbfir_bloch_train_gn_batch,
 * mbfir_bloch_train_lm_step_batch, mbfir_bloch_train_lsq_sched_batch, mbfir_bloch_train_gn_sched_batch and
 * mbfir_bloch_train_lm_step_sched_batch each have a twin that fits the echo amplitude |Mxy| and the z component of every echo, and of
 * the final state, instead of the vectors.  The formulas are those of the magnitude twins above, applied once per echo
 * and once at m_N.  With e echo k as mbfir_bloch_train_batch returns it under the call's demod, or m_N,
 *     rho = sqrt(ex ex + ey ey)   (each product, the sum and the root rounded once: np.sqrt(ex * ex + ey * ey) on the forward
 *                                  call's output has its bits)
 *     u   = (ex, ey) / rho, and (0, 0) where rho = 0
 *     L   = 1/2 sum_s sum_k rw_k sum_points [w_xy (rho_k - t_xy)^2 + w_z (e_kz - t_z)^2]
 *         + 1/2 sum_s sum_points [wf_xy (rho_N - tf_xy)^2 + wf_z (m_Nz - tf_z)^2]
 *     lsq: ce_k = rw_k (w_xy (rho_k - t_xy) u_x, w_xy (rho_k - t_xy) u_y, w_z (e_kz - t_z)), cf likewise with wf, tf
 *     gn:  ce_k = rw_k (w_xy (u . de_xy) u_x, w_xy (u . de_xy) u_y, w_z de_z), cf likewise with dm_N
 * A twin takes its component call's arguments with every weight triple replaced by a pair (wxy, wz) and every target triple by a
 * pair (txy, tz), for the echo term and for the final term, the planes laid out as before (ebcast as before); one call fits
 * magnitudes in both terms.  Every other argument, the outputs, the launches, the transfers, the guarantees on the bits and the
 * argument checks, their order and their messages are the component call's ("only partly given" refers to the pair).  rho = 0 is not
 * an error: the transverse term then adds 1/2 rw_k w_xy t_xy^2 to L and exact zeros to the gradients and to H v.  A negative t_xy
 * is accepted.  H drops the curvature of rho across u. */
int mbfir_bloch_train_lsq_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                    const double* gx, const double* gy, const double* gz, const long* tsoff,
                                    const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                    const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                    const double* dy, const double* dz, int nscale, const double* scales, const int* ntr,
                                    const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                                    const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                                    const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wxy,
                                    const double* wz, const double* txy, const double* tz, const double* rw, const double* wfxy,
                                    const double* wfz, const double* tfxy, const double* tfz, double* loss, double* g_re,
                                    double* g_im, double* gmx, double* gmy, double* gmz);
int mbfir_bloch_train_gn_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                   const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                   const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                   const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                   const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                   const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                   const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                   const double* m0y, const double* m0z, int ebcast, const double* wxy, const double* wz,
                                   const double* rw, const double* wfxy, const double* wfz, int ndir, const double* v_re,
                                   const double* v_im, double* h_re, double* h_im);
int mbfir_bloch_train_lm_step_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                        const double* gx, const double* gy, const double* gz, const long* tsoff,
                                        const double* tsteps, const double* t1, const double* t2, const double* gamma,
                                        int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                                        const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                                        const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                                        const int* gidx, const long* goff, const double* gains, const int* echo,
                                        const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                        int ebcast, const double* wxy, const double* wz, const double* rw, const double* wfxy,
                                        const double* wfz, const double* b_re, const double* b_im, const double* mu, int cg,
                                        double rtol, const double* txy, const double* tz, const double* tfxy, const double* tfz,
                                        double* d_re, double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss,
                                        double* g_re, double* g_im);
int mbfir_bloch_train_lsq_sched_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                          const double* gx, const double* gy, const double* gz, const long* tsoff,
                                          const double* tsteps, const double* t1, const double* t2, const double* gamma,
                                          int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                                          const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                                          const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                                          const int* gidx, const long* goff, const double* gains, const int* echo,
                                          const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                          int ebcast, const double* wxy, const double* wz, const double* txy, const double* tz,
                                          const double* rw, const double* wfxy, const double* wfz, const double* tfxy,
                                          const double* tfz, double* loss, double* ggain, double* gphi, double* gmx, double* gmy,
                                          double* gmz);
int mbfir_bloch_train_gn_sched_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                         const double* gx, const double* gy, const double* gz, const long* tsoff,
                                         const double* tsteps, const double* t1, const double* t2, const double* gamma,
                                         int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                                         const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                                         const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                                         const int* gidx, const long* goff, const double* gains, const int* echo,
                                         const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                         int ebcast, const double* wxy, const double* wz, const double* rw, const double* wfxy,
                                         const double* wfz, int ndir, const double* dgain, const double* dphi, double* hgain,
                                         double* hphi);
int mbfir_bloch_train_lm_step_sched_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re,
                                              const double* b1_im, const double* gx, const double* gy, const double* gz,
                                              const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                                              const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                                              const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                                              const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                              const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                              const int* echo, const double* meq, int demod, const double* m0x,
                                              const double* m0y, const double* m0z, int ebcast, const double* wxy,
                                              const double* wz, const double* txy, const double* tz, const double* rw,
                                              const double* wfxy, const double* wfz, const double* tfxy, const double* tfz,
                                              const double* bgain, const double* bphi, const double* mu, int cg, double rtol,
                                              double* dgain, double* dphi, int* ncg, double* rr, double* gg, int* status,
                                              double* loss, double* ggain, double* gphi);
/* mbfir_test_jvp_group (host only): the directions one workgroup of the two calls above carries (a compile-time constant). */
int mbfir_test_jvp_group(void);
/* mbfir_test_sim_blocks (host only): the workgroup table of the three calls above for pulses of ntime[p] samples and npoint[p]
 *   points ((frequency, position) pairs, positions, or nx ny points) at nscale scales: 4 ints (pulse, scale, chunk, 0) per workgroup in launch
 *   order into out (may be NULL).  Returns the number of workgroups; -1 for npulse or nscale < 1, an ntime or npoint < 1, or a
 *   table of more than 2^31 - 1 workgroups. */
long mbfir_test_sim_blocks(int npulse, const int* ntime, const long* npoint, int nscale, int* out);

/* ---- Root-flip search for the smallest peak (fir_flip_zero.m:56-102, rf_tools/mex5/minpeakrf.c) -----------------------
 * Scores a whole candidate set of one beta polynomial on the device and keeps the best.  Candidate c has the n coefficients of
 *     c0(x) * prod_{j < nz} (x - r_j),   r_j = zf[j] if factor j is flipped in c, else z[j]
 * (c0: the n - nz coefficients of the roots that never flip, leading first; the factors are multiplied on in the order j = 0, 1, ..
 * as the host fir_flip_zero does), then scaled:
 *   scale_rule 0: sum(beta) = s_re + i s_im                                       (fir_flip_zero.m:83)
 *   scale_rule 1: beta / max_k |FFT_nn(beta)_k| * bsf, nn = next power of two >= n, bsf = s_re in [0, 1]   (npoly.code.c, minpeakrf.c)
 * and scored:
 *   criterion 0: max_k |beta_k|
 *   criterion 1: max_k |rf_k|, rf = ab2rf(b2a(beta), beta) as mbfir_b2rf computes it (b2a.m:15-32 with its 8 n padding and clip,
 *                ab2rf.m:14-29) -- not b2a.code.c, which minpeakrf.c calls (power-of-two padding, conjugate convention)
 * Candidates: masks != NULL: explicit, ceil(nz / 32) words per candidate, bit j of word j / 32 set = factor j flipped (nz <= 1023);
 *   masks == NULL: c = 0 .. ncand-1 enumerated on the device (ncand <= 2^24): factor j flipped iff bit (enum_bits[j] >> 1) of c
 *   equals enum_bits[j] & 1 (every source bit < 24); enum_bits == NULL is fir_flip_zero.m's combination_2power (:153-160): ncand must
 *   be 2^nz and factor j is flipped iff bit (nz - 1 - j) of c is 0.
 * Winner: the smallest peak; exactly equal peaks go to the lowest index, or the highest with tie_high = 1 (minpeakrf.c's `<=`); a
 *   candidate with a non-finite peak never wins.  *winner receives its index, *winner_peak its peak, beta_re / beta_im (n each,
 *   optional) its scaled coefficients, peaks (ncand, optional) every candidate's peak (inf where it is not finite).
 * Limits: 2 <= n <= 1024 (minpeakrf.c's MAXN), 0 <= nz <= n - 1, ncand >= 1, else MBFIR_E_ARG.  Returns MBFIR_NUMERICAL (winner = -1)
 * when no candidate has a finite peak. */
int mbfir_flip_search(mbfir_ctx* ctx, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re, const double* z_im,
                      const double* zf_re, const double* zf_im, long ncand, const unsigned* masks, const int* enum_bits,
                      int scale_rule, double s_re, double s_im, int criterion, int tie_high, double* peaks, double* beta_re,
                      double* beta_im, long* winner, double* winner_peak);
/* mbfir_test_flip_stages (test hook): mbfir_flip_search under two overrides, then every stage of selected candidates.
 * 1. The search exactly as mbfir_flip_search launches it (one host body serves both): twiddles, the scoring launch, the arg-min over
 *    the workgroups' bests, the pick launch.  Arguments up to tie_high, peaks (required here), beta_re / beta_im (required), winner
 *    and winner_peak are mbfir_flip_search's.  force_mode: -1 the mode a search chooses, or 0 (working set and twiddles in LDS),
 *    1 (twiddles from global memory), 2 (everything in the per-workgroup global scratch); a mode whose LDS does not fit the device is
 *    MBFIR_E_ARG with a message, before any launch.  max_blocks: 0 as a search chooses, else a cap on the scoring launch's workgroups
 *    (candidates beyond it are reached by the grid stride).  blk_p / blk_i (ncand each; report[2] are written): each workgroup's best
 *    peak and its index (-1: none finite), the input of the arg-min.
 * 2. One more scoring launch (same mode, threads and LDS) over the nsel candidates sel[] (0 <= nsel <= 1024, each < ncand; repeats
 *    allowed) through the instantiation that also stores the stages.  Block s of each array belongs to sel[s]; complex values are
 *    interleaved (re, im):
 *      st_beta  n complex     the candidate after the build and the scale rule
 *      st_bf    8n            |fft(beta, 8n)| after the clip scale (times 1 / (1e-8 + max) when max >= 1)
 *      st_xl    8n            log(sqrt(1 - bf^2))
 *      st_xlfp  4n + 1 complex  fft(xl)(0 : 4n) windowed (x 2 except at 0 and 4n)
 *      st_afa   8n complex    exp(ifft(xlfp))
 *      st_a     n complex     alpha, a = fft(afa)(0 : n-1) / 8n reversed
 *      st_theta n             theta[i - 1] = atan2(|s_i|, c_i) of recursion step i = n .. 1 (|rf_i| = 2 theta_i)
 *      st_peak  1             the candidate's peak as this launch scored it
 *    With criterion 0 only st_beta and st_peak are written.  Nothing is written outside these sizes.
 * report (8 longs): mode used, threads per workgroup, workgroups of the search's scoring launch, dynamic LDS bytes, scratch stride
 *    (double2 per workgroup), the device's LDS limit per workgroup as read, nn, mask words per candidate.
 * Returns as mbfir_flip_search (MBFIR_NUMERICAL with winner -1 when no candidate is finite: the blocks are still written). */
int mbfir_test_flip_stages(mbfir_ctx* ctx, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re,
                           const double* z_im, const double* zf_re, const double* zf_im, long ncand, const unsigned* masks,
                           const int* enum_bits, int scale_rule, double s_re, double s_im, int criterion, int tie_high, int force_mode,
                           int max_blocks, int nsel, const long* sel, double* peaks, double* blk_p, long* blk_i, double* beta_re,
                           double* beta_im, long* winner, double* winner_peak, double* st_beta, double* st_bf, double* st_xl,
                           double* st_xlfp, double* st_afa, double* st_a, double* st_theta, double* st_peak, long* report);

/* ---- Conventional SLR filters: Parks-McClellan and fmp (rf_tools/dzlp.m, dzmp.m, fmp.m) ----------------------------------------
 * mbfir_remez_batch: `h = remez(numtaps - 1, edges, desired, weight)` as dzlp.m:13 and dzmp.m:16 call it, for njobs independent
 *   designs in one launch (one workgroup each).  Real, symmetric, linear-phase filters only: type I (odd numtaps) and type II (even),
 *   3 <= numtaps <= 2047.  edges: 2 nband band edges in [0, 1] (1 = Nyquist, MATLAB's convention), ascending, bands disjoint;
 *   desired: the amplitude at both edges of each band (linear in between); weight: one positive weight per band; 1 <= nband <= 64.
 *   type must be MBFIR_REMEZ_BANDPASS: Hilbert transformers and differentiators (antisymmetric taps) are rejected with MBFIR_E_ARG.
 *   Grid: McClellan-Parks-Rabiner, density points per cosine term (opts->grid_density, 0 = 16), the grid rule of
 *   scipy.signal.remez with the bands in Nyquist units; type II leaves omega = pi off the grid.  The exchange stops when the extremal
 *   set no longer changes, or after opts->maxiter iterations (0 = 25).  Out: h (numtaps), ext (optional, the L + 1 final extremal
 *   frequencies, L = (numtaps + 1) / 2 or numtaps / 2), status (MBFIR_REMEZ_*), iterations, delta (the weighted ripple of the last
 *   iterate, signed).  MBFIR_REMEZ_MAXITER keeps the last iterate; it is never reported as converged.  Returns 0 when every design
 *   ran (whatever its status), MBFIR_E_ARG naming the first bad job, MBFIR_E_HIP.
 * mbfir_fmp: `hmp = fmp(h)` (rf_tools/fmp.m:12-23): the minimum-phase factor of an equiripple linear-phase filter of odd length
 *   l <= 2047 (h_im may be NULL), (l + 1) / 2 complex taps out.  Even l is MBFIR_E_ARG (the reference prints and returns). */
#define MBFIR_REMEZ_BANDPASS 0
#define MBFIR_REMEZ_CONVERGED 0
#define MBFIR_REMEZ_MAXITER 1
#define MBFIR_REMEZ_FAILED 2
typedef struct mbfir_remez_job {
    int numtaps;
    int nband;
    int type;              /* MBFIR_REMEZ_BANDPASS */
    const double* edges;   /* 2 nband */
    const double* desired; /* 2 nband */
    const double* weight;  /* nband */
    double* h;             /* out: numtaps */
    double* ext;           /* out, optional: L + 1 */
    int status;            /* out */
    int iterations;        /* out */
    double delta;          /* out */
} mbfir_remez_job;
typedef struct mbfir_remez_opts {
    int grid_density;      /* 0 -> 16 */
    int maxiter;           /* 0 -> 25 */
} mbfir_remez_opts;
int mbfir_remez_batch(mbfir_ctx* ctx, mbfir_remez_job* jobs, int njobs, const mbfir_remez_opts* opts);
int mbfir_fmp(mbfir_ctx* ctx, int l, const double* h_re, const double* h_im, double* out_re, double* out_im);

/* Device kernel test hooks (need a GPU; host arrays in, host arrays out):
 *  mbfir_test_gram: T = A' diag(dk) A for nw weight vectors; A is m x nt row-major,
 *     d is nw x m, out is nw x nt x nt (full symmetric).
 *  mbfir_test_chol: M = inv(chol(H)) for SPD H (n x n); out_l = L, out_m = L^-1 (row-major, lower).
 *  mbfir_test_specfact: x(2n-1) -> taps (n) through the device fmp2/mag2mp.
 *  mbfir_test_mfma_peak: measured fp64 MFMA rate, TFLOP/s (bench.py roofline peak).            */
int mbfir_test_gram(mbfir_ctx* ctx, int m, int nt, int nw, const double* A, const double* d, double* out);
int mbfir_test_chol(mbfir_ctx* ctx, int n, const double* H, double* out_l, double* out_m);
/*  mbfir_test_chol_lanes: the same for `nlanes` matrices factorised TOGETHER, the way a lock-step batch does it (lane index a
 *  grid dimension / the single-launch form); H, out_l, out_m hold nlanes consecutive n x n blocks; mask (nlanes ints or NULL):
 *  lanes with mask 0 are switched off (their outputs stay untouched).  form: -1 = the default of chol_inv_launch for this lane
 *  count, otherwise the value of MBFIR_CHOL_SPLIT to use. */
int mbfir_test_chol_lanes(mbfir_ctx* ctx, int n, int nlanes, int form, const int* mask, const double* H, double* out_l, double* out_m);
int mbfir_test_specfact(mbfir_ctx* ctx, int n, const double* x, double* h_re, double* h_im);
/*  mbfir_test_specfact_stages (test hook): the tap extraction's kernels through the instantiations that also store what the chain
 *  overwrites in place -- the same arithmetic, launched as production launches it.
 *    kind 0: k_specfact on nlanes (1 .. 64) inputs in ONE launch with a lane stride, as a lock-step unit of one order is factorised;
 *            n = the order (1 .. 4096), in_re = nlanes blocks of 2n - 1 reals (the designers' x), in_im ignored.
 *    kind 1: k_fmp on one filter; n = its odd length (<= 2047), in_re / in_im its taps (in_im may be NULL), nlanes = 1.
 *  Everything lives in one device arena of nlanes lanes of `stride` doubles, filled with `fill` before the inputs go in and copied
 *  back whole into raw (nlanes * stride doubles).  A lane holds eight blocks, each followed by at least `guard` doubles that nothing
 *  may write (rounded up so that every block starts on 16 bytes); `extra` more doubles end the lane.  Complex blocks are interleaved
 *  (re, im) and in the kernel's own storage order, lp = 8 * 2^ceil(log2(l)) the transform length:
 *      0 in     2n - 1 reals (kind 0) / n complex (kind 1)
 *      1 work   3 lp complex: B0, B1, B2 as the kernel leaves them
 *      2 h      the taps: n complex (kind 0), (n + 1) / 2 complex (kind 1)
 *      3 hpf    lp complex: B0 after the first transform (bin k of the transform of fftshift(hp))
 *      4 xl     lp reals: log(sqrt(|hpf - lift|)), entry i from bin (i + lp / 2) mod lp
 *      5 xlfp   lp complex: the transform of xl after the window (x 2 on 1 .. lp/2 - 1, 0 above lp/2)
 *      6 a      lp complex: exp(ifft(xlfp))
 *      7 lift   1 real: what is subtracted from real(hpf) (kind 1: 1.000001 min real(hpf); kind 0: 0)
 *  layout (18 longs, always written): lp, stride, the eight block offsets within a lane, the eight block sizes (all in doubles).
 *  With raw NULL only layout is written and no device work is done, so a caller can size raw.  Bad arguments: MBFIR_E_ARG. */
int mbfir_test_specfact_stages(mbfir_ctx* ctx, int kind, int n, int nlanes, const double* in_re, const double* in_im, int guard,
                               double fill, long extra, long* layout, double* raw);
/*  mbfir_test_unit_ops: the operators of ONE lock-step unit -- the njobs designs of `jobs` as its lanes, a single design as a unit of
 *  one -- at an iterate the caller chooses.  The unit is set up by the stages a solve runs (switches read from the environment, lanes,
 *  plan, arena, masks, seed tables) and scaled as an iteration's head scales it; every product then goes through the solve's own
 *  launch code, so the kernels, grids, pairings and templates are the ones a solve of this unit would launch.  Per lane b (host
 *  arrays of njobs blocks; nv = 1 or 2 vectors per block; ldx >= the unit's largest N = n_unknowns, ldr >= its largest R = n_rows,
 *  ldh = N rounded up to 64; entries past a lane's own N / R are ignored):
 *    in:  v (nv x ldx, x-space), u and sub (nv x ldr, row space; sub may be NULL = 0), s and z (ldr each: a strictly interior
 *         pair of the lane's cone -- l orthant rows, n_q3 cones of three rows, then the big cone), mask (njobs ints or NULL: a lane
 *         with 0 is switched off, as a finished design is in a solve);
 *    in / out: gv = G v and wgv = W^-2 G v - sub (nv x ldr), gtu = G'u (nv x ldx), H (ldh x ldh, row-major: the LOWER triangle of
 *         G'W^-2 G as the normal-matrix build leaves it ahead of the factorisation, padding included; the lattice path writes
 *         the lower 64 x 64 tiles only).  All four go to the device before the launches and come back after them: what a masked
 *         lane's blocks held on entry they hold on exit.
 *    report (16 longs): [0] lattice path, [1] passes that ran one thread per pair of lanes, [2] the build took its one-pass
 *         branch, [3] D1 lattice points, [4] evaluation segments, [5] folded entries, [6] runs (chunks), [7] chunks per block,
 *         [8] np = ldh, [9] folded entries of lane 0 with one side empty, [10] segment length, [11] heterogeneous unit (per-lane
 *         dimensions), [12] one seed table serves the unit, [13] G v passes, [14] G'v passes, [15] lanes.  tmin: the lattice origin.
 *  opts: grid_m and dense_trig as for a solve.  Row-sharded units and units on the extended-precision path (opts.ddkkt >= 0 for
 *  fir_qp_cvx) are MBFIR_E_ARG.  The context stays usable for solves. */
int mbfir_test_unit_ops(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int nv, int ldx, int ldr, int ldh,
                        const double* v, const double* u, const double* sub, const double* s, const double* z, const int* mask,
                        double* gv, double* gtu, double* wgv, double* H, long* report, double* tmin);
/*  mbfir_test_unit_cone: the cone stages of ONE iteration of a lock-step unit -- the njobs designs of `jobs` as its lanes, a single
 *  design as a unit of one -- at an iterate the caller chooses.  The unit is set up as for mbfir_test_unit_ops.  Everything the three
 *  KKT solves of an iteration would have produced is an INPUT, uploaded into the buffers the solves write; the hook then launches the
 *  stages an iteration launches between its solves, in its order: NT scaling; predictor tail (dtau_a, dkappa_a, W^-1 ds_a, W dz_a,
 *  step maxima); combined right-hand side (alpha_a, sigma, bx, lam \ (...), bz, W^-2 bz); combined tail (dtau, dkappa, ds, dz, step
 *  maxima); then either the update (corrector = 0) or the corrector right-hand side (alpha_0, bz_k, W^-2 bz_k) and the corrector tail
 *  (candidate sums, its dtau_c, dkappa_c, ds_k, dz_k, the pick, the update along the direction picked); last the initial point's cone
 *  shift of one more vector.  form: 0 = the kernels a solve on one rank launches (MBFIR_FUSE and MBFIR_CORR_BIG read from the
 *  environment), 1 = the two-phase folding kernels of a row-sharded solve (k_scal_dtau / k_scal_step phases 0 and 1, the all-reduce
 *  between them being the identity).  ldx >= the unit's largest N, ldr >= its largest R, ldw = 4 max(n_q3, 1); rows are ordered as
 *  the program's: l orthant rows, n_q3 cones of three rows, then the big cone; entries past a lane's own N / R are ignored.  Per
 *  lane b (host arrays of njobs blocks):
 *    in_r (13 + 1 rows of ldr): [0] s, [1] z (a strictly interior pair), [2] rz, [3..4] bz2 (the two right-hand sides whose W^-2
 *         products the scaling fuses), [5] z1, [6] z2, [7] g1 = G x1, [8] g2 = G x2 (batch solve), [9] zc, [10] gc (combined solve),
 *         [11] kz, [12] kg (corrector solve), [13] the vector of the cone shift;
 *    in_x (6 rows of ldx): [0] x, [1] rx, [2] x1, [3] x2, [4] xc, [5] kx;
 *    in_sc (8): tau, kappa, mu, S_RT (the residual of the tau equation), S_SIGMAX (cap on sigma), S_DRES, S_NRMC (||c||), S_RNC
 *         (residual norm of the corrector solve);
 *    mask (njobs ints or NULL): a lane with 0 is switched off, as a finished design is in a solve;
 *    in / out -- out_r (22 rows of ldr): [0] dl = z/s, [1] wl = sqrt(s/z) (orthant rows only), [2] lam, [3..4] W^-2 bz2 (orthant and
 *         3-row cones), [5] the big cone's w (w0, w1; `big` entries), [6] W^-1 ds_a, [7] W dz_a, [8] lds, [9] bz of the combined
 *         system, [10] its W^-2 bz (orthant and 3-row cones), [11] ds, [12] dz, [13] bz_k, [14] its W^-2 (orthant and 3-row cones),
 *         [15] z2 + kz, [16] g2 + kg, [17] ds_k, [18] dz_k, [19] s and [20] z after the update, [21] the shifted vector;
 *         out_x (3 rows of ldx): [0] bx of the combined system, [1] xc + kx, [2] x after the update;
 *         out_w3 (ldw): (eta, w0, w1, w2) per 3-row cone;
 *         out_sc (7 snapshots of 24, taken after: scaling, predictor tail, combined right-hand side, combined tail, corrector
 *         right-hand side, update / corrector tail, shift): [0] eta of the big cone, [1] tau, [2] kappa, [3] sigma, [4] alpha,
 *         [5] alpha_a, [6] dtau, [7] dkappa, [8] dtau_a, [9] dkappa_a, [10] S_TMAX, [11] tau and [12] kappa as the fused update
 *         reads them, [13] alpha_0, [14] dtau_c, [15] dkappa_c, [16] S_PICK, [17] S_NCORR, [18] S_NPICK, [19] w0 of the big cone,
 *         [20] mu, [21..23] the mailbox RB[0..2].
 *         Every out block goes to the device as the caller filled it, right before the stage that writes it, and comes back right
 *         after that stage: entries no kernel writes (rows past the ones named above, padding) and ALL blocks of a masked lane hold
 *         on exit what they held on entry; so do the blocks and snapshots of stages that did not run (corrector = 0: out_r
 *         [13..18], out_x [1], snapshot 4).  The blocks a kernel updates IN PLACE (out_r [15], [16], [19], [20], [21], out_x [1], [2])
 *         hold the lane's input on a live lane when their stage starts, so their entries past the lane's own N / R return the
 *         input's padding; on a masked lane they too hold the caller's block.  out_sc of a masked lane is not written.
 *    report (16 longs): [0] cone blocks, [1] l, [2] n_q3, [3] big, [4] N, [5] R (the unit's largest), [6] heterogeneous unit,
 *         [7] lanes, [8] MBFIR_FUSE, [9] MBFIR_CORR_BIG, [10] form, [11] rows of step maxima the affine and [12] the combined
 *         direction folded, [13] blocks of the update.
 *  Row-sharded units and units on the extended-precision path (opts.ddkkt >= 0 for fir_qp_cvx) are MBFIR_E_ARG with a message, as
 *  is a bad argument.  The context stays usable for solves. */
int mbfir_test_unit_cone(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int form, int corrector, int ldx, int ldr,
                         int ldw, const int* mask, const double* in_r, const double* in_x, const double* in_sc, double* out_r, double* out_x,
                         double* out_w3, double* out_sc, long* report);
/*  mbfir_test_unit_kkt: the residual kernels of an iterate and the plain KKT solve [0 G'; G -W^2][dx; dz] = [bx; bz] of ONE lock-step
 *  unit, group of launches by group of launches.  The unit is set up as for mbfir_test_unit_ops.  In this order:
 *  (1) the residual kernels at the caller's (x, s, z, tau, kappa): form 0 as a solve on one rank launches them, form 1 the two-phase
 *      form of a row-sharded solve (the all-reduce between the phases being the identity; the mailbox then sits behind G'z);
 *  (2) mode 0: the caller's right-hand sides go into the buffers of the batch solve (nv = 2) or the combined solve (nv = 1) -- bx = bz =
 *      NULL (nv = 2) keeps the two the residual kernels just wrote, (-c, -rx) and (h, s - rz) --, then the NT scaling and the build and
 *      factorisation of H; then kkt_solve with the lanes' own sweep counts nsweep[b] in 0 .. 8 under the sweep masks.  wbz_ready (nv = 2):
 *      the entry of an iteration's solves, W^-2 bz from the scaling's fused product and k_big_winv2; otherwise the winv2 entry.
 *      two: the sweep's update in the two launches of a row-sharded solve.
 *      mode 1: the initial point itself (unit scaling, build, k_init_rhs, the solve with nv = 2, the copies and the cone shifts).
 *  Per lane b (host arrays of njobs blocks; ldx >= the unit's largest N, ldr >= its largest R, ldh = np, ldw = 4 max(n_q3, 1)):
 *    s, z (ldr), x (ldx), tau_kappa (2), bx (nv x ldx), bz (nv x ldr), nsweep, mask (0: the lane is switched off);
 *    in / out -- res_r (3 rows of ldr): rz, bz2[0], bz2[1]; res_x (4 rows of ldx): G'z, rx, bx2[0], bx2[1]; res_sc (24): S_RT, S_MU,
 *         S_PCOST, S_DCOST, S_GAP, S_RELGAP, S_PRES, S_DRES, S_PINF, S_DINF, S_CX, S_HZ, S_SZ, S_CHOLFIX, then (out only) tau, kappa,
 *         ||h||, ||c||, the degree, then the mailbox (5);
 *         M (np x np): the inverse factor; flag: the pivot-replacement counter;
 *         out_x (46 blocks of 2 x ldx): [0] G'W^-2 bz, [1] dx after the Cholesky solve, [2] G'dz, [3] r = bx - G'dz, [4 + 2 s], [5 + 2 s]
 *         p and z of the s-th start (s = 0: before sweep 0; z only where the unfused form writes it), [20 + 3 q .. 22 + 3 q] Hp, dx, r of
 *         sweep q, [44] dx and [45] r as the solve leaves them;
 *         out_r (37 blocks of 2 x ldr): [0] W^-2 bz, [1] G dx, [2] dz after the Cholesky solve, [3 + 4 q .. 6 + 4 q] Gp, W^-2 Gp, gdx, dz
 *         of sweep q, [35] gdx and [36] dz as the solve leaves them;
 *         out_sc (18 snapshots of 13: after the residual of the Cholesky solve, after start s (8), after sweep q (8), at the end): the
 *         solve's nine norm slots n_0 .. n_8, S_CG_RZ[2], S_CG_ALPHA[2];
 *         init_r (7 rows of ldr; mode 1): dl, wl, the big cone's w, s, z, bz2[0], bz2[1]; init_x (3 rows of ldx): x, bx2[0], bx2[1];
 *         init_w3 (ldw).
 *         Every block goes to the device as the caller filled it right before the launches that write it and comes back right after
 *         them: a masked lane returns every block as it was, rows past a lane's own N / R and the blocks of sweeps a lane does not run
 *         hold the caller's values, as do the norm slots past the lane's count.  Blocks updated in place (dx, r, gdx, dz of a sweep,
 *         p of a restart) are copied back for the lanes that run the sweep.
 *    report (24 longs): [0] one-pass M'(M b), [1] MBFIR_FUSE, [2] form, [3] N, [4] R, [5] np, [6] big, [7] lanes, [8] heterogeneous,
 *         [9] lattice path, [10] workgroups of k_gt_finish, [11] nv, [12] two, [13] wbz_ready, [14] mode, [15] largest sweep count,
 *         [16] l, [17] n_q3, [18] row blocks of the residual kernel, [19] z is written, [20] G v and [21] G'v passes.
 *  Row-sharded units and units on the extended-precision path are MBFIR_E_ARG with a message, as is a bad argument.  The context stays
 *  usable for solves. */
int mbfir_test_unit_kkt(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int mode, int form, int two, int wbz_ready,
                        int nv, int ldx, int ldr, int ldh, int ldw, const int* mask, const int* nsweep, const double* s, const double* z,
                        const double* x, const double* tau_kappa, const double* bx, const double* bz, double* res_r, double* res_x,
                        double* res_sc, double* M, long* flag, double* out_x, double* out_r, double* out_sc, double* init_r, double* init_x,
                        double* init_w3, long* report);
/*  mbfir_test_unit_ddkkt: the extended-precision path of an iteration (opts.ddkkt on) of ONE lock-step unit at the caller's iterate,
 *  stage by stage.  The unit is set up as for mbfir_test_unit_ops.  In this order, as the head of an iteration and its solves launch
 *  them: the NT scaling of (s, z); the selection of every live lane's strong set (eigen data, cap, strong set, its fixed order; the cap
 *  raised x 100 and the selection repeated where a set does not fit -- the one host synchronisation); the lanes' mode masks; the capped
 *  normal matrix with the strong rows U and its factorisation in the solve's own form (capacitance form by default, MBFIR_DDFORM=dd
 *  the double-double one; a single design pads to MBFIR_TEST_CAP_KP); then (solve != 0) the solve of the caller's nv = 1 or 2
 *  right-hand sides: the refinement passes of the extended-precision solve on the lanes with a non-empty strong set, the plain solve
 *  with opts.refine sweeps on the others.
 *  Per lane b (host arrays of njobs blocks; ldx >= the unit's largest N, ldr >= its largest R, ldh = np, ldw = 4 max(n_q3, 1), ldu: the
 *  rows of U, Yt, Zt, S, Ms the caller has room for, 64 .. 3072):
 *    in:  s, z (ldr), bx (nv x ldx), bz (nv x ldr), mask (0: the lane is switched off);
 *    in / out, every live lane -- sel_r (4 rows of ldr): dl, dlc, the big cone's w, its what; sel_q (18 ldw / 4): w3 (4 per cone), e3 (8
 *         per cone: lam_p, lam_0, lam_m, what), m3c (6 per cone); sel_sc (16): eb[0 .. 7], S_ETAB, the lane's final cap factor;
 *         sel_part (ldp rows of 2): the partial rows (sum log typical weight, count) the selection folds, the big cone's row first, then
 *         one per 256 orthant rows and 3-row cones -- the first min(ldp, rows) of them, the number of rows in lane_rep[3];
 *         sel_i (ldr + 3 ldw / 4 + 3 ints): slotl, slot3, slotb, kcnt; strong_i (3 x 3072 ints): skind, sidx, sdir and strong_x (3072): sX,
 *         over the lane's count; H (np x np): the normal matrix ahead of the factorisation; U (ldu x np): rows 0 .. min(kp, ldu) - 1,
 *         sent to the device as the caller filled them before the rows are formed; M and Hf (np x np): the buffers M and H as the solve
 *         leaves them (capacitance form: M the inverse factor; double-double form: Hf, M the high and low parts of the factor); flag;
 *         end_x (2 x ldx): dx; end_r (2 blocks of 2 x ldr): dz, gdx; out_sc row 3: the norm slots at the end;
 *    in / out, the lanes in the extended-precision mode -- Yt, Zt (ldu x np), S (ahead of its factorisation), Ms (ldu x ldu): the
 *         capacitance form's, or all four NULL; per pass p < 3, blocks of two vectors:
 *         out_x (9 of ldx): [0] G'dz, [1] r1 = bx - G'dz, [2] G'W_w^-2 r2, [3], [4] the right-hand side of the normal-equation solve
 *         (double-double form: high, low; capacitance form: [4] rhs_w), [5] y (capacitance form), [6], [7] the solve's result (high;
 *         low in the double-double form), [8] dx after the pass;
 *         out_r (6 of ldr): [0] r2, [1] W_w^-2 r2, [2] G Bh, [3] W_w^-2 (G Bh - r2), [4] dz and [5] gdx after the pass;
 *         out_k (3 of 3072): [0] t = e'r2 per strong slot, [1] U y - t (capacitance form), [2] zeta;
 *         out_sc rows 0 .. 2 (9): the solve's norm slots after r1 of the pass.
 *         Every block goes to the device as the caller filled it right before the launches that write it and comes back right after.
 *    lane_rep (4 longs): [0] 0 switched off, 1 extended-precision mode, 2 plain mode, [1] the strong count, [2] selections run, [3] partial rows.
 *    report (16 longs): [0] kp, [1] capacitance form, [2] passes, [3] lanes, [4] N, [5] R, [6] np, [7] l, [8] n_q3, [9] big, [10] the
 *         largest strong count, [11] selections run, [12] nv, [13] solve, [14] heterogeneous, [15] sweeps of the plain mode.
 *  MBFIR_E_ARG with a message, before anything is launched: a bad lane count, leading dimensions that do not fit, nv outside 1 .. 2, the
 *  double-double form with more than one lane, a row-sharded context, a unit not on the extended-precision path. */
int mbfir_test_unit_ddkkt(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int nv, int solve, int ldx, int ldr, int ldh,
                          int ldw, int ldu, int ldp, const int* mask, const double* s, const double* z, const double* bx, const double* bz, double* sel_r,
                          double* sel_q, double* sel_sc, double* sel_part, int* sel_i, int* strong_i, double* strong_x, double* H, double* U, double* M, double* Hf,
                          double* Yt, double* Zt, double* S, double* Ms, long* flag, double* out_x, double* out_r, double* out_k, double* out_sc,
                          double* end_x, double* end_r, long* lane_rep, long* report);
/*  mbfir_test_fold: the host-side analysis of a frequency grid w[m] for the lattice kernels (no GPU, no context): pairs
 *  +w / -w (fold != 0), cuts the folded list into equally spaced runs.  out[6]: lattice usable, folded entries, pairs,
 *  runs, longest run, self-check failures (must be 0).  (Own addition; nothing in the reference corresponds.) */
int mbfir_test_fold(const double* w, int m, int fold, long* out);
/*  mbfir_test_ddsolve: x = (H + U' diag(X) U)^-1 b through the double-double kernels of the extended-precision
 *     KKT solve; H n x n, U k x n (row-major), b and x as (hi, lo) pairs of nrhs x n arrays, nrhs <= 2;
 *     nfix receives the number of replaced pivots; Lh / Ll (optional, n x n) the Cholesky factor.            */
int mbfir_test_ddsolve(mbfir_ctx* ctx, int n, int k, const double* H, const double* U, const double* X, int nrhs,
                       const double* bh, const double* bl, double* xh, double* xl, int* nfix, double* Lh, double* Ll);
/*  mbfir_test_ddstages: the same double-double kernels stage by stage.  H, U, X, b as for mbfir_test_ddsolve, padded to np = n rounded up
 *  to 64 (identity past n, zero coupling); pivtol the pivot rule's threshold; form the triangular-solve kernel: 0 the single
 *  workgroup (no flags), 1 one workgroup per 32-row block, 2 the 64-row blocks with the inverses of the diagonal blocks; nsolve >= 1
 *  solves on ONE flag array with the epochs 1 .. nsolve, each from a fresh copy of b.  The launches are a solve's own, in order: the
 *  rank-k update, the factorisation (the block inverses for form 2 only), the solves.  Read back after each group, full padded size:
 *    Hh, Hl (np x np) the updated matrix; d0 (np); Lh, Ll (np x np) the same buffers after the factorisation (the factor in the lower
 *    triangle); Lth, Ltl (np x np) its transpose; ri (2 x np: high words, low words) the reciprocal diagonal; dinv (2 x np / 64 x 64 x 64:
 *    high words, low words) the block inverses; xh, xl (nsolve x 2 x np) the solutions; counter (2 ints): the pivot counter after the
 *    factorisation and after the last solve (replaced pivots + 2^20 per lost hand-off).
 *  Hl, d0, Lth, Ltl, ri, dinv and the rows nrhs .. 1 of every solution go to the device as the caller filled them and come back after
 *  the launches: what no launch writes holds on exit what it held on entry.  A bad argument is MBFIR_E_ARG with a message, before
 *  anything is launched. */
int mbfir_test_ddstages(mbfir_ctx* ctx, int n, int k, const double* H, const double* U, const double* X, int nrhs, const double* bh,
                        const double* bl, double pivtol, int form, int nsolve, double* Hh, double* Hl, double* d0, double* Lh, double* Ll,
                        double* Lth, double* Ltl, double* ri, double* dinv, double* xh, double* xl, int* counter);
/*  mbfir_test_capsolve: the capacitance form of the extended-precision KKT solve (capkkt.hip) stage by stage -- for nlanes
 *  independent problems (H_w + U' diag(X) U) dx = (a + b) + U' diag(X) t, laid out as a lock-step unit lays its lanes out, exactly the
 *  launches a solve issues: the factorisation of H_w (M = L^-1), Yt = U M', Zt = Yt M, S = Yt Yt' + X^-1, the factorisation of S
 *  (Ms), the sum of the pivot counters; then one pass of the solve: rhs_w = a + b, y = M'(M rhs_w), w = U y - t, zeta = Ms'(Ms w),
 *  dx = y - Zt' zeta.  One problem runs as a single design does, several as a unit (launches sized to kp, a lane's own count read
 *  from its arena).  np = n rounded up to 64.  Per lane (host arrays of nlanes blocks):
 *    in:  k (nlanes ints, 1 <= k[b] <= kp), kp (multiple of 64, <= 1024), H (n x n, SPD), U (kp x n; rows from k[b] on are ignored:
 *         the device holds zero rows there), X (kp; entries from k[b] on ignored), a, b (nrhs x n), t (nrhs x kp; entries from k[b]
 *         on ignored), nrhs 1 or 2, mask (nlanes ints or NULL: a lane with 0 is switched off), hsolve_form: y by the one-pass
 *         kernel (1; np <= 1024), by the pair of triangular GEMVs (0), or as a solve of this size would choose (-1);
 *    in / out: M (np x np), Yt, Zt (kp x np), S, Ms (kp x kp), rhs_w, y, dx (nrhs x np), w, zeta (nrhs x kp), flag (nlanes ints:
 *         replaced pivots of both factorisations).  They go to the device as the caller filled them and come back after the
 *         launches: what a masked lane's blocks held on entry they hold on exit.
 *  Before the launches the hook writes NaN where the kernels claim not to read: the 64 x 64 tiles of M, S and Ms strictly above the
 *  diagonal (they come back as NaN) and their mirror images in the stored transpose, the ignored entries of X and t, the padding of
 *  a and b, the split-K slab and the other scratch vectors.  A bad argument is MBFIR_E_ARG with a message, before anything is
 *  launched. */
int mbfir_test_capsolve(mbfir_ctx* ctx, int n, int nlanes, const int* k, int kp, int nrhs, int hsolve_form, const int* mask,
                        const double* H, const double* U, const double* X, const double* a, const double* b, const double* t,
                        double* M, double* Yt, double* Zt, double* S, double* Ms, double* rhs_w, double* y, double* w,
                        double* zeta, double* dx, int* flag);
int mbfir_test_mfma_peak(mbfir_ctx* ctx, double* tflops_f64_mfma, double* tflops_f64_valu);
/* Device time (ms per call, HIP events, averaged over reps) of the Cholesky+inverse phase on a random SPD
 * n x n matrix, and of the Gram launches on a random m x nt matrix -- kernel tuning aid. */
int mbfir_test_time_kernels(mbfir_ctx* ctx, int n, int m, int nt, int reps, double* ms_chol, double* ms_gram);

#ifdef __cplusplus
}
#endif
#endif
