// Device-resident primal-dual interior-point solver for the structured conic program of
// program.h:   min c'z  s.t.  G z + s = h,  s in R_+^l x Q_3^nq3 x Q_big.
//
// Algorithm (identical, step for step, to the test oracle oracle/conic_ipm.py so the two agree to
// rounding): homogeneous self-dual embedding, Nesterov-Todd scaling, Mehrotra predictor-corrector
// (step fraction 0.99, sigma = min((1-alpha_aff)^3, 0.25)), KKT systems reduced to the normal equations
//   (G' W^-2 G) dx = bx + G' W^-2 bz ,  dz = W^-2 (G dx - bz)
// with dz kept explicit and corrected incrementally (CG sweeps on the exact operator; their number follows a
// controller whose target is max(1e-11 ||c||, 0.1 ||rx||)) so the dual equation G'dz = bx holds as far as the
// iterate's own residual makes it worth.
//
// Per iteration on the GPU (K numbers as in SURVEY 8a / DESIGN 4):
//   K1  G v   : lattice mode: trigonometric polynomial per FOLDED frequency (+w and -w share the recurrence:
//               cosine and sine sums apart, C + S | C - S) (k_trig_eval) + row gather; dense mode: A1 * [v, P'v] (k_amulti, HBM-bound)
//   K3  G' v  : per-frequency aggregation folded to (p(+w) + p(-w), p(+w) - p(-w)) (k_freq_fold), trigonometric
//               moments per column (k_trig_moments, k_gt_finish); dense mode: A1' * [p1, p2] (k_atmulti)
//   K6  NT scaling, per-frequency 2x2 weight blocks (k_scaling, k_freq_blocks)
//   K2  normal matrix: lattice mode from the moments of the weight vectors (Toeplitz + Hankel,
//       k_assemble_H_lat); dense mode T_k = A1' D_k A1 on the fp64 matrix cores (gram.hip); plus the
//       sparse identity-row / border / big-cone terms
//   K4  Cholesky + triangular inverse (chol.hip); every solve = two triangular GEMVs, refined by
//       preconditioned CG on the exact operator
//   K5  step length: closed form per cone, block max-reductions, scalars stay on the device
// One host synchronisation per iteration (termination test on 24 doubles per design).
//
// Lock-step batches ("lanes", solve_lanes): B designs of one shape share every launch -- blockIdx.z (Cholesky:
// a 1-D grid ordered by block kind) is the design, all device buffers of lane b sit b * lane_bytes after lane 0's, every kernel starts with the
// LANES(...) prologue (mask test + pointer shift); per-lane status, sweep counts and masks live on the host.
// Extended-precision KKT solve (ddkkt.inc + ddlin.hip): double-double accumulation / factorisation of the strongly
// weighted part of the normal matrix for nearly active cones (fir_qp_cvx, and the retry of any numerical failure).
// Row-sharded solves: reductions are ncclAllReduce calls on the solver stream (run-time bound RCCL) or a host hook.
#include "dev_common.h"
#include <functional>
#include <mutex>
#include <thread>
#include "cone_dev.h"
#include "dd_dev.h"
#include "program.h"
#include "solver.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

// RCCL is bound at run time (dlopen): a process that has torch loaded shares torch's librccl, and the library
// still loads on a machine without RCCL (the CPU-side tests bind every symbol of include/mbfir.h).
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace mbfir {

struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string err;
};
static void rccl_bind(RcclApi& api);
static RcclApi& rccl() {
    // bound once per process; two contexts may call mbfir_comm_init from different host threads at the same moment
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] { rccl_bind(api); });
    return api;
}
static void rccl_bind(RcclApi& api) {
    void* h = nullptr;
    // one RCCL per process: a copy that is already loaded (torch's, when the host is Python) is preferred -- by the
    // path the host names in MBFIR_RCCL_PATH, then by the usual names -- before a fresh one is opened
    const char* hinted = std::getenv("MBFIR_RCCL_PATH");
    if (hinted && *hinted) {
        h = dlopen(hinted, RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen(hinted, RTLD_NOW | RTLD_GLOBAL);
    }
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) {
        if (h) break;
        h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);          // already in the process?
    }
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) {
        if (h) break;
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) { api.err = "librccl not found"; return; }
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(h, "ncclAllReduce"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce;
    if (!api.ok) api.err = "librccl lacks the expected symbols";
}

enum {
    S_TAU = 0, S_KAPPA, S_MU, S_SIGMA, S_ALPHA, S_ALPHA_A, S_DTAU, S_DKAP, S_DTAU_A, S_DKAP_A,
    S_RT, S_PCOST, S_DCOST, S_GAP, S_RELGAP, S_PRES, S_DRES, S_PINF, S_DINF, S_CX, S_HZ, S_SZ,
    S_DEN, S_ETAB, S_NRMH, S_NRMC, S_DEG, S_DKC, S_WB0, S_TMAX, S_BAD,
    S_CHOLFIX /* pivots the last factorisation replaced (copied from the counter so that one D2H copy serves the host) */,
    S_TAU0 /* tau, kappa of the iterate the step is taken from: k_update's blocks read these while block 0 publishes the new ones */, S_KAP0,
    // centrality corrector (round 6): step of the uncorrected direction, dtau / dkappa of the corrected one, 1 when the corrected
    // direction is the one taken, and the lane's counts (corrector solves, corrected directions taken)
    S_ALPHA0, S_DTAU_C, S_DKAP_C, S_PICK, S_NCORR, S_NPICK,
    S_RNA = 40 /* 9 residual norms, batch solve */, S_RNB = 49 /* 9 residual norms, combined solve */,
    S_CG_RZ = 58 /* 2 */, S_CG_ALPHA = 60 /* 2 */, S_CG_BETA = 62 /* 2 */,
    S_RNC = 64 /* 9 residual norms, corrector solve */,
    S_DTAU0 = 73 /* dtau, dkappa of the uncorrected direction as k_dir_post (mode 1) left them: k_update_pick's blocks read these while block 0 publishes the picked ones */, S_DKAP0 = 74,
    S_SIGMAX = 76 /* the cap on Mehrotra's sigma of this solve: SIGMA_MAX, or SIGMA_MAX_CORR where the centrality corrector runs */, S_COUNT = 80
};
constexpr double STEP = 0.99;
constexpr double SIGMA_MAX = 0.25;   // cap of Mehrotra's centring parameter (oracle/conic_ipm.py SIGMA_MAX)
constexpr double SIGMA_MAX_CORR = 0.05;      // ... where a centrality corrector follows the direction (oracle/conic_ipm.py SIGMA_MAX_CORR)
// one centrality corrector per iteration on the orthant rows (oracle/conic_ipm.py CORR_*)
constexpr double CORR_DELTA = 0.5, CORR_BMIN = 0.1, CORR_BMAX = 10.0, CORR_ACCEPT = 1.01, CORR_ETA = 1.0;
// end game: an iterate that meets the stopping rule is kept and the iteration goes on until the gap measures are POLISH times below
// the tolerances, at most POLISH_MAX more iterations (oracle/conic_ipm.py POLISH*)
constexpr double POLISH = 1e-2;
constexpr int POLISH_MAX = 3, POLISH_SWEEPS = 1;     // (POLISH_SWEEPS: refinement sweeps on top of the controller's count during the final approach and the end game)
constexpr double POLISH_APPROACH = 30.0;              // ... the final approach: a gap measure within this factor of its tolerance (oracle/conic_ipm.py)
constexpr int NPART = 1024;   // max blocks contributing to a reduction
constexpr int SCAL_T = 256;   // threads of the one-workgroup-per-design folding kernels (a 1024-thread block has to wait for a
                              // whole CU when other units share the chip)
constexpr int MAX_SWEEPS = 8;
// kkt_solve's optional observer (test_unit_kkt): the groups of launches it is called after, in their order
enum { KKT_ST_WBZ = 0, KKT_ST_GTWBZ, KKT_ST_HSOLVE, KKT_ST_GDX, KKT_ST_RESID, KKT_ST_START, KKT_ST_GP, KKT_ST_HP, KKT_ST_STEP, KKT_ST_RESTART };
struct KktObserver {
    std::function<void(int, int)> fn;
    bool two_launch_cg = false;
    void operator()(int stage, int sweep) const { fn(stage, sweep); }
};
// kkt_solve_dd's optional observer (test_unit_ddkkt; the same struct, called with the group and the pass): the groups of launches of
// one pass in their order.  DD_ST_Y .. DD_ST_ZETAC: the capacitance form alone; DD_ST_ZETA: the double-double form alone
enum { DD_ST_R1 = 0, DD_ST_R2, DD_ST_WBZ, DD_ST_GTW, DD_ST_RHS, DD_ST_Y, DD_ST_CAPW, DD_ST_ZETAC, DD_ST_SOLVE, DD_ST_GBH, DD_ST_WBZ2, DD_ST_ZETA,
       DD_ST_ACCUM };
// the scalar slots: the auto-numbered ones end before the first norm block, each norm block holds n_0 .. n_MAX_SWEEPS
static_assert(S_NPICK < S_RNA, "scalar slots: the auto-numbered slots run into S_RNA");
static_assert(S_RNA + MAX_SWEEPS + 1 <= S_RNB && S_RNB + MAX_SWEEPS + 1 <= S_CG_RZ && S_RNC + MAX_SWEEPS + 1 <= S_SIGMAX,
              "scalar slots: a block of residual norms overlaps the next slot");
static_assert(S_RNC + MAX_SWEEPS + 1 <= S_DTAU0 && S_DTAU0 < S_DKAP0 && S_DKAP0 < S_SIGMAX, "scalar slots: S_DTAU0 / S_DKAP0 overlap their neighbours");
static_assert(S_RNA < S_COUNT && S_RNB < S_COUNT && S_CG_BETA + 2 <= S_COUNT && S_RNC < S_COUNT && S_DKAP0 < S_COUNT && S_SIGMAX < S_COUNT,
              "scalar slots: S_COUNT too small");
constexpr int CAP_KMAX = 1024;   // strong directions the capacitance form of the extended-precision solve takes (S is CAP_KMAX^2; the one-pass M'(M b) goes to np = 1024)
constexpr int MAX_LANES = 64, MASK_ROWS = MAX_SWEEPS + 4;
constexpr int ROW_BEST = MAX_SWEEPS + 1;      // mask rows: 0 live, 1 .. MAX_SWEEPS sweep q, then: lanes with a new best iterate,
constexpr int ROW_DD = MAX_SWEEPS + 2;        // live lanes whose iteration runs the extended-precision solve,
constexpr int ROW_PL = MAX_SWEEPS + 3;        // live lanes whose iteration runs the plain one (lock-step units with opts.ddkkt: round 5)
constexpr int WALL_ITERS = 3;
constexpr double REFTOL = 1e-11, REFETA = 1e-1 /* forcing term of the refinement, oracle/conic_ipm.py */, INACC_FEAS = 1e-6, INACC_GAP = 1.22e-4 /* CVX's reduced tolerance eps^(1/4) */;

// ------------------------------------------------------------------------------------------------
// device-side problem description
// (round 5: a unit may also hold designs of different ORDERS -- the probes of a min-order search: the dimensions that move with the
//  order follow the six that move with the band edges)
struct LaneDims { int Mf, R, l, nyrows, nfold, nchunk, Nt, N, nq3, big, D1, seg, useg, Mown /* dense path: the lane's own padded row count */; double tmin /* the lane's lattice origin */; };
static_assert(sizeof(LaneDims) == 64, "LaneDims: 14 ints + one double");
struct DProg {
    int Nt, Ne, N, Mf, R, l, nq3, big, quad;
    int ld, Mpad, LDV, Rp, np;
    int Mown;                         // dense path: the lane's own padded row count (the split partials a fold adds; = Mpad unless dims)
    const double *w, *col_tau, *col_scale, *psign, *c;
    const int *col_kind, *pcol;
    const int *freq, *col;
    const double *alpha, *beta, *ey, *h;
    const int *f_ptr, *f_rows;        // frequency -> rows
    const int *c_ptr, *c_rows;        // column   -> identity rows
    const int *yrows; int nyrows;     // rows with a non-zero ey
    // Row-sharded solves: rep[r] = 1 for the rows every rank holds (no frequency: identity rows, spike / per-tap cones, the big
    // cone; program.h); own = 1 on the rank whose copy of them counts in the sums over the rows (rank 0; 1 when not sharded)
    const int* rep; int own;
    __device__ __forceinline__ double row_weight(int r) const { return (own || !rep[r]) ? 1.0 : 0.0; }
    // Lattice ("matrix-free") mode: every trig column is scale * cos|sin(w (tmin + m)) with m on an
    // integer lattice 0..D1-1 and the frequency grid splits into chunks of equally spaced points, so
    // A1 is never formed: products with A1 / A1' and the Gram matrices A1' D A1 come from rotation
    // recurrences (see "lattice kernels" below).  useg = number of partial sums k_rows_G adds up.
    int trig, D1, LDL, seg, useg, nchunk, LDM;
    double tmin;
    const int *lat;                   // Nt: lattice index of column j
    const int *lat_col, *lat_qcol;    // 2*D1 [kind][m]: column there (or -1); source column of P'v there
    const double *lat_scale, *lat_qscale;
    const int *ch_start, *ch_count;   // nchunk: runs of the FOLDED frequency list (analyse_lattice)
    const int *fold_pos, *fold_neg;   // nfold: frequency index at +wf[k] / -wf[k], or -1
    const double* wf; int nfold;
    int cgrp;                         // chunks per block of k_trig_moments (<= CGRP)
    int seeds_shared;                 // all lanes of the unit have the same grid and lattice: they read lane 0's seed tables
    const double *ch_w0, *ch_dw;
    // rotation seeds, tabulated once per design (a sincos costs as much as ~40 recurrence steps):
    const double4* seed_tau;          // [nchunk][D1]   (cos, sin)(w0 t), (cos, sin)(dw t), t = tmin + m
    const double4* seed_h;            // [nchunk][3 D1 - 1]  same for the difference | sum progressions of the H moments
    const double4* seed_eval;         // [useg][Mpad]   (cos, sin)(wf_k (tmin + sg seg)), (cos, sin)(wf_k), k < nfold
    // Lock-step batch ("lanes"): B designs of identical shape advance together, blockIdx.z = lane.  Every device
    // buffer of lane b -- program arrays and work vectors alike -- sits lane_bytes after the same buffer of lane
    // b-1 (one arena, identical layout per lane), so a kernel shifts all its pointers by blockIdx.z * lane_bytes.
    // mask (not shifted; nlanes ints) switches lanes off: finished designs, refinement sweeps a lane does not need.
    size_t lane_bytes;
    const int* mask;
    // Lock-step units with the extended-precision solve (round 5): the lanes switch to it one by one (each when ITS strong set is
    // non-empty, as in its single solve), so the kernels that build the normal matrix take the capped weights (D.dlc, D.m3c) on
    // the lanes flagged in dd_lane (not lane-shifted) and the plain ones (dl_plain, lane-shifted; w3 on the fly) on the others
    const int* dd_lane;
    const double* dl_plain;
    __device__ __forceinline__ bool plain_weights() const { return dd_lane && !dd_lane[blockIdx.z]; }
    // Heterogeneous units (round 4): lanes of one designer and order whose band edges differ have different grids, row
    // counts and chunk lists.  Every array and launch is then sized to the unit's MAXIMA (one arena layout for all lanes,
    // shorter arrays zero-padded) and the kernel prologue replaces the dimensions that differ by the block's lane's own
    // (dims, not lane-shifted, nlanes entries; null when all lanes have the same dimensions): a lane then does exactly
    // the arithmetic of its single solve -- blocks past its own extent contribute neutral partials (sums 0, maxima -1e300).
    const LaneDims* dims;
    __device__ __forceinline__ void load_dims(int lane) {
        const LaneDims d = dims[lane];
        Mf = d.Mf; R = d.R; l = d.l; nyrows = d.nyrows; nfold = d.nfold; nchunk = d.nchunk;
        // ... and the lane's own order: unknowns, cone counts, lattice extent and its segments.  The STRIDES (ld, LDV, Rp, np, LDM,
        // Mpad) stay the unit's: a shorter lane's vectors and matrices sit in the same layout, padded -- H by identity rows and
        // columns, which the factorisation passes through untouched (the same blocks see the same arithmetic as in the lane's
        // single solve at its own np; the padding blocks factorise to the identity)
        Nt = d.Nt; N = d.N; nq3 = d.nq3; big = d.big; D1 = d.D1; seg = d.seg; useg = d.useg; Mown = d.Mown;
        // ... and its lattice origin (round 6: the centred delays of fir_qprog_phs / fir_qp_cvx start at -(n - 1) / 2; the origin enters the
        // seed tables alone -- k_build_seeds_m / _e --, which every lane of such a unit builds for itself)
        tmin = d.tmin;
    }
    template <class T>
    __device__ __forceinline__ static void sh(const T*& p, size_t off) { p = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p) + off); }
    __device__ __forceinline__ void shift(size_t off) {
        sh(w, off); sh(col_tau, off); sh(col_scale, off); sh(psign, off); sh(c, off); sh(col_kind, off); sh(pcol, off);
        sh(freq, off); sh(col, off); sh(alpha, off); sh(beta, off); sh(ey, off); sh(h, off);
        sh(f_ptr, off); sh(f_rows, off); sh(c_ptr, off); sh(c_rows, off); sh(yrows, off); sh(rep, off);
        sh(lat, off); sh(lat_col, off); sh(lat_qcol, off); sh(lat_scale, off); sh(lat_qscale, off);
        sh(ch_start, off); sh(ch_count, off); sh(ch_w0, off); sh(ch_dw, off); sh(fold_pos, off); sh(fold_neg, off); sh(wf, off);
        if (!seeds_shared) { sh(seed_tau, off); sh(seed_h, off); sh(seed_eval, off); }
        if (dl_plain) sh(dl_plain, off);
    }
};
// Kernel prologue: leave if the lane is masked off, then move the program and the listed pointer arguments to
// the block's lane (null pointers stay null).
template <class... Ptr>
__device__ __forceinline__ void lane_shift(size_t off, Ptr&... p) {
    ((p = p ? (Ptr)((const char*)p + off) : p), ...);
}
#define LANES(P, ...)                                                \
    if ((P).mask && !(P).mask[blockIdx.z]) return;                    \
    if ((P).dims) (P).load_dims(blockIdx.z);                          \
    if (blockIdx.z) {                                                 \
        const size_t loff_ = (size_t)blockIdx.z * (P).lane_bytes;     \
        (P).shift(loff_);                                             \
        lane_shift(loff_, __VA_ARGS__);                               \
    }
#define LANES_RAW(lane_bytes, mask, ...)                              \
    if ((mask) && !(mask)[blockIdx.z]) return;                        \
    if (blockIdx.z) lane_shift((size_t)blockIdx.z * (lane_bytes), __VA_ARGS__);
inline dim3 lane_grid(dim3 g, int nlanes) { g.z = nlanes; return g; }

// ------------------------------------------------------------------------------------------------
// trig matrix
__global__ void k_build_A1(DProg P, double* __restrict__ A1) {
    LANES(P, A1);
    int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= P.Nt || i >= P.Mf) return;
    double sn, cs;
    sincos(P.w[i] * P.col_tau[j], &sn, &cs);
    A1[(long)i * P.ld + j] = P.col_scale[j] * (P.col_kind[j] ? sn : cs);
}

// XX = [v ; P'v]  (second half only when quad)
template <int NV>
__global__ void k_make_xx(DProg P, const double* __restrict__ v, double* __restrict__ XX) {
    LANES(P, v, XX);
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P.Nt) return;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double val = v[(long)q * P.LDV + j];
        XX[(long)q * P.LDV + j] = val;
        if (P.quad) XX[(long)(NV + q) * P.LDV + P.pcol[j]] = P.psign[j] * val;
    }
}

// K1: U[v][i] = sum_j A1[i][j] XX[v][j]; one wave per frequency row, 16-byte loads.
template <int NVV>
__global__ __launch_bounds__(256) void k_amulti(const double* __restrict__ A1, int ld, int Mf,
                                                const double* __restrict__ XX, int ldv,
                                                double* __restrict__ UU, int Mpad, size_t lane_bytes, const int* __restrict__ lane_mask,
                                                const LaneDims* __restrict__ dims) {
    LANES_RAW(lane_bytes, lane_mask, A1, XX, UU);
    if (dims) Mf = dims[blockIdx.z].Mf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wv;
    if (row >= Mf) return;
    const double* a = A1 + (long)row * ld;
    double acc[NVV];
#pragma unroll
    for (int v = 0; v < NVV; ++v) acc[v] = 0;
#pragma unroll 8
    for (int j = 2 * lane; j < ld; j += 128) {
        double2 t = *reinterpret_cast<const double2*>(a + j);
#pragma unroll
        for (int v = 0; v < NVV; ++v) {
            double2 xv = *reinterpret_cast<const double2*>(XX + (long)v * ldv + j);
            acc[v] += t.x * xv.x + t.y * xv.y;
        }
    }
#pragma unroll
    for (int v = 0; v < NVV; ++v) {
        double s = wave_sum(acc[v]);
        if (lane == 0) UU[(long)v * Mpad + row] = s;
    }
}

// one row of G v from the per-frequency products
template <int NV>
__device__ __forceinline__ double row_value(const DProg& P, const double* __restrict__ UU, const double* __restrict__ X,
                                            int r, int v) {
    const int f = P.freq[r], cl = P.col[r];
    const double al = P.alpha[r], be = P.beta[r];
    double val = 0;
    if (f >= 0) {
        const int NVV = P.quad ? 2 * NV : NV;
        double u1 = 0, u2 = 0;
        for (int sg = 0; sg < P.useg; ++sg) {
            u1 += UU[((long)sg * NVV + v) * P.Mpad + f];
            if (P.quad) u2 += UU[((long)sg * NVV + NV + v) * P.Mpad + f];
        }
        val = al * u1 + be * u2;
    } else if (cl >= 0) {
        val = al * X[(long)v * P.LDV + cl];
    }
    for (int e = 0; e < P.Ne; ++e) val += P.ey[3 * r + e] * X[(long)v * P.LDV + P.Nt + e];
    return val;
}
// rows of G v from the per-frequency products
template <int NV>
__global__ void k_rows_G(DProg P, const double* __restrict__ UU, const double* __restrict__ X,
                         double* __restrict__ out) {
    LANES(P, UU, X, out);
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.R) return;
    const int f = P.freq[r], cl = P.col[r];
    const double al = P.alpha[r], be = P.beta[r];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double val = 0;
        if (f >= 0) {
            const int NVV = P.quad ? 2 * NV : NV;
            double u1 = 0, u2 = 0;
            for (int sg = 0; sg < P.useg; ++sg) {
                u1 += UU[((long)sg * NVV + v) * P.Mpad + f];
                if (P.quad) u2 += UU[((long)sg * NVV + NV + v) * P.Mpad + f];
            }
            val = al * u1 + be * u2;
        } else if (cl >= 0) {
            val = al * X[(long)v * P.LDV + cl];
        }
        for (int e = 0; e < P.Ne; ++e) val += P.ey[3 * r + e] * X[(long)v * P.LDV + P.Nt + e];
        out[(long)v * P.Rp + r] = val;
    }
}

// K3: G'v.  Two launches:
//  k_atmulti<NVV, AGG>: partial[split][v][j] = sum_{i in split} A1[i][j] PP[v][i].  Block = 64 x 4
//     threads: 4 waves share 128 columns and interleave the AT_ROWS rows of the split (128: 1040 workgroups at the headline
//     size, 22.7 us per pass; 256 rows -- two workgroups per CU in ONE round -- took 32.7 us, 64 rows 24.2); with AGG the
//     per-frequency operands p1[i] = sum_{rows at i} alpha_r val_r, p2[i] = sum beta_r val_r are
//     formed in LDS first from the CSR map (each of the ld/128 column blocks redoes that cheap walk),
//     otherwise they are read from the array PP (border products of the H assembly).
//  k_gt_finish<NV>: folds the split partials (fixed order), applies the quadrature permutation,
//     adds the identity rows and the y block.
constexpr int AT_ROWS = 128;
template <int NVV, bool AGG>
__global__ __launch_bounds__(256) void k_atmulti(DProg P, const double* __restrict__ A1, const double* __restrict__ src,
                                                 double* __restrict__ partial) {
    LANES(P, A1, src, partial);
    __shared__ double sh[4][NVV][128];
    __shared__ double pp[NVV][AT_ROWS];
    const int lane = threadIdx.x, wq = threadIdx.y, tid = wq * 64 + lane;
    const int col0 = blockIdx.x * 128 + 2 * lane, split = blockIdx.y;
    const int ld = P.ld, Mpad = P.Mpad;
    const int r0 = split * AT_ROWS, r1 = min(r0 + AT_ROWS, Mpad);
    if (tid < AT_ROWS) {
        const int i = r0 + tid;                        // one frequency row per thread
        if (AGG) {
            constexpr int NV = NVV;                    // upper bound; the real NV is NVV or NVV/2
            const int nv = P.quad ? NVV / 2 : NVV;
            double p1[NV], p2[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) p1[v] = p2[v] = 0;
            if (i < P.Mf)
                for (int q = P.f_ptr[i]; q < P.f_ptr[i + 1]; ++q) {
                    const int r = P.f_rows[q];
                    const double al = P.alpha[r], be = P.beta[r];
#pragma unroll
                    for (int v = 0; v < NV; ++v)
                        if (v < nv) {
                            const double x = src[(long)v * P.Rp + r];
                            p1[v] += al * x;
                            p2[v] += be * x;
                        }
                }
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (v < nv) {
                    pp[v][tid] = p1[v];
                    if (P.quad) pp[nv + v][tid] = p2[v];
                }
        } else {
#pragma unroll
            for (int v = 0; v < NVV; ++v) pp[v][tid] = i < Mpad ? src[(long)v * Mpad + i] : 0.0;
        }
    }
    __syncthreads();
    double2 acc[NVV];
#pragma unroll
    for (int v = 0; v < NVV; ++v) acc[v] = make_double2(0, 0);
#pragma unroll 16
    for (int i = r0 + wq; i < r1; i += 4) {
        double2 t = *reinterpret_cast<const double2*>(A1 + (long)i * ld + col0);
#pragma unroll
        for (int v = 0; v < NVV; ++v) {
            const double p = pp[v][i - r0];
            acc[v].x += t.x * p;
            acc[v].y += t.y * p;
        }
    }
#pragma unroll
    for (int v = 0; v < NVV; ++v) {
        sh[wq][v][2 * lane] = acc[v].x;
        sh[wq][v][2 * lane + 1] = acc[v].y;
    }
    __syncthreads();
    for (int e = tid; e < NVV * 128; e += 256) {
        int v = e >> 7, cc = e & 127;
        double t = sh[0][v][cc] + sh[1][v][cc] + sh[2][v][cc] + sh[3][v][cc];
        partial[((long)split * NVV + v) * ld + blockIdx.x * 128 + cc] = t;
    }
}

// fold the split partials: TT[v][j] = sum_s partial[s][v][j].  Block = FPC columns x 16 split groups: 256 threads like k_gt_finish (a
// 1024-thread block waits for a whole CU once other units share the chip); the 16 per-group sums and the sum over them keep their order.
// dims != null (heterogeneous unit, lattice partials): the lane folds its OWN cdiv(nchunk, cgrp) partials -- the grouping of
// the unrolled sums below depends on the count, and the lane's result has to be that of its single solve bit for bit
constexpr int FPC = 16;
__global__ __launch_bounds__(FPC * 16) void k_fold_partials(const double* __restrict__ partial, int nsplit, int nvv, int ld,
                                                        int ldo, double* __restrict__ TT, size_t lane_bytes, const int* lane_mask,
                                                        const LaneDims* __restrict__ dims, int cgrp, int vtrim = 1 << 30, int jtrim = 0) {
    LANES_RAW(lane_bytes, lane_mask, partial, TT);
    if (dims) nsplit = cgrp > 0 ? (dims[blockIdx.z].nchunk + cgrp - 1) / cgrp : (dims[blockIdx.z].Mown - cgrp - 1) / -cgrp;     // (cgrp < 0: dense path, -cgrp rows per split)
    // (the H-build's border moments: the rows from vtrim on are read at the columns below jtrim = D1 alone, and the moment kernel's blocks
    //  past D1 have not written their partials -- trim_border --, so nothing is folded or stored there)
    if (dims && vtrim < nvv) jtrim = dims[blockIdx.z].D1;
    __shared__ double sh[16][FPC + 1];
    const int c = threadIdx.x, sg = threadIdx.y, j = blockIdx.x * FPC + c, v = blockIdx.y;
    if (v >= vtrim && blockIdx.x * FPC >= jtrim) return;
    const bool on = j < ld && (v < vtrim || j < jtrim);   // (the block that straddles jtrim leaves out its columns past it)
    double t = 0;
    if (on) {
        const double* p = partial + (long)v * ld + j;
        const long ss = (long)nvv * ld;
        int s = sg;
        for (; s + 48 < nsplit; s += 64) {
            const double a0 = p[s * ss], a1 = p[(s + 16) * ss], a2 = p[(s + 32) * ss], a3 = p[(s + 48) * ss];
            t += (a0 + a1) + (a2 + a3);
        }
        for (; s < nsplit; s += 16) t += p[s * ss];
    }
    sh[sg][c] = t;
    __syncthreads();
    if (sg == 0 && on) {
        double a = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) a += sh[q][c];
        TT[(long)v * ldo + j] = a;
    }
}

// Block x < nblk_cols: 32 columns x 8 split groups -> out[v][j] (4 loads in flight per thread);
// the last block forms the y block.
constexpr int GTC = 32, GTG = 8;       // 256 threads: a 1024-thread block waits for a whole CU once other units share the chip
// rn_bx != null (round 5, one launch less per KKT solve): the LAST workgroup of the lane to finish also forms the residual
// r = bx - G'v and its norm -- k_resid_norm's sums with 256 threads, in its order -- (rn_cnt: one int per lane, zero between launches).
struct GtResid { const double* bx; double* r; double* Sc; int slot; int* cnt; };
template <int NV>
__device__ __forceinline__ void gt_resid_tail(const DProg& P, const GtResid& F, const double* __restrict__ t, double* red) {
    // The hand-over between workgroups WITHOUT a device-wide fence: __threadfence() writes back and invalidates the XCD's whole L2
    // on this chip (the eight L2s are not coherent with each other) -- with four units in flight that cost 12 % of the batch.  The
    // values handed over are stored write-through and loaded past the caches instead (agent-scope relaxed atomics: sc1), the
    // stores are drained (s_waitcnt vmcnt(0)) before the counter moves.
    __shared__ int s_last;
    const int tid = threadIdx.y * GTC + threadIdx.x;
    // (every storing wave drains its write-through stores before the barrier behind which ONE lane moves the counter: a
    //  workgroup-scope release fence does NOT emit the s_waitcnt vmcnt(0) this needs -- found by the lock-step fuzz: 1 of 720
    //  jobs differed in the last bits from run to run until the wait was explicit)
    drain_stores();
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(F.cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    double m = 0;
    for (int v = 0; v < NV; ++v) {
        double a = 0;
        for (int j = tid; j < P.N; j += GTC * GTG) {
            const long o = (long)v * P.LDV + j;
            const double r = F.bx[o] - __hip_atomic_load(t + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            F.r[o] = r;
            a += r * r;
        }
        // (block_sum for a 32 x 8 block: waves are 64 consecutive threads of the x-fastest order)
        a = wave_sum(a);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = a;
        __syncthreads();
        if (tid == 0) {
            double s = 0;
            for (int w = 0; w < GTC * GTG / 64; ++w) s += red[w];
            red[16] = s;
        }
        __syncthreads();
        m = fmax(m, sqrt(red[16]));
    }
    if (tid == 0) { F.Sc[F.slot] = m; __hip_atomic_store(F.cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}
template <int NV>
__global__ __launch_bounds__(GTC * GTG) void k_gt_finish(DProg P, const double* __restrict__ partial, int nsplit,
                                                    const double* __restrict__ val, double* __restrict__ out, GtResid F) {
    LANES(P, partial, val, out, F.bx, F.r, F.Sc, F.cnt);
    if (P.dims) nsplit = P.trig ? (P.nchunk + P.cgrp - 1) / P.cgrp : (P.Mown + AT_ROWS - 1) / AT_ROWS;      // the lane's own partial count (see k_fold_partials)
    __shared__ double sh[2 * NV][GTG][GTC + 1];
    __shared__ double red[17];
    const int c = threadIdx.x, sg = threadIdx.y;
    const int NVV = P.quad ? 2 * NV : NV;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {
        // y block of G'v:  out[v][Nt+e] = sum_r ey[r][e] val[v][r]
        const int tid = sg * GTC + c;
        for (int v = 0; v < NV; ++v)
            for (int e = 0; e < P.Ne; ++e) {
                double a = 0;
                for (int q = tid; q < P.nyrows; q += GTC * GTG) {
                    const int r = P.yrows[q];
                    a += P.row_weight(r) * (P.ey[3 * r + e] * val[(long)v * P.Rp + r]);      // (replicated rows: once over the ranks)
                }
                a = wave_sum(a);
                __syncthreads();
                if ((tid & 63) == 0) red[tid >> 6] = a;
                __syncthreads();
                if (tid == 0) {
                    double t = 0;
                    for (int w = 0; w < GTC * GTG / 64; ++w) t += red[w];
                    if (F.bx) __hip_atomic_store(out + (long)v * P.LDV + P.Nt + e, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else out[(long)v * P.LDV + P.Nt + e] = t;
                }
            }
        if (F.bx) gt_resid_tail<NV>(P, F, out, red);
        return;
    }
    const int j = blockIdx.x * GTC + c;
    const bool ok = j < P.Nt;
    const int pj = (ok && P.quad) ? P.pcol[j] : 0;
    // dense: partial[s][vv][column]; lattice: partial[chunk][vv][kind][m], scaled here
    long o1 = j, o2 = pj, st1 = P.ld;
    double f1 = 1.0, f2 = 1.0;
    if (P.trig && ok) {
        o1 = (long)P.col_kind[j] * P.LDM + P.lat[j]; o2 = (long)P.col_kind[pj] * P.LDM + P.lat[pj];
        st1 = 2L * P.LDM;
        f1 = P.col_scale[j]; f2 = P.col_scale[pj];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double t1 = 0, t2 = 0;
        if (ok) {
            const double* p1 = partial + (long)v * st1 + o1;
            const double* p2 = partial + (long)(NV + v) * st1 + o2;
            const long ss = (long)NVV * st1;
            int s = sg;
            for (; s + 3 * GTG < nsplit; s += 4 * GTG) {
                const double a0 = p1[s * ss], a1 = p1[(s + GTG) * ss], a2 = p1[(s + 2 * GTG) * ss], a3 = p1[(s + 3 * GTG) * ss];
                t1 += (a0 + a1) + (a2 + a3);
                if (P.quad) {
                    const double b0 = p2[s * ss], b1 = p2[(s + GTG) * ss], b2 = p2[(s + 2 * GTG) * ss], b3 = p2[(s + 3 * GTG) * ss];
                    t2 += (b0 + b1) + (b2 + b3);
                }
            }
            for (; s < nsplit; s += GTG) {
                t1 += p1[s * ss];
                if (P.quad) t2 += p2[s * ss];
            }
        }
        sh[v][sg][c] = f1 * t1;
        sh[NV + v][sg][c] = f2 * t2;
    }
    __syncthreads();
    if (sg == 0 && ok) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double t1 = 0, t2 = 0;
#pragma unroll
            for (int q = 0; q < GTG; ++q) { t1 += sh[v][q][c]; t2 += sh[NV + v][q][c]; }
            double g = t1 + (P.quad ? P.psign[j] * t2 : 0.0);
            if (P.own)                                               // identity rows are replicated rows: summed over the ranks once
            for (int q = P.c_ptr[j]; q < P.c_ptr[j + 1]; ++q) {
                const int r = P.c_rows[q];
                g += P.alpha[r] * val[(long)v * P.Rp + r];
            }
            if (F.bx) __hip_atomic_store(out + (long)v * P.LDV + j, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else out[(long)v * P.LDV + j] = g;
        }
    }
    if (F.bx) gt_resid_tail<NV>(P, F, out, red);
}

// ------------------------------------------------------------------------------------------------
// lattice kernels (DProg::trig): the trig matrix is never stored.
//  * cos/sin(w t) along a unit-step progression of t (fixed frequency) or along an equally spaced
//    run of frequencies (fixed t) follow from one sincos seed by the rotation recurrence
//    (c, s) <- (c cd - s sd, s cd + c sd); runs are at most 128 steps, so the recurrence error stays
//    at a few 1e-14, the level at which cos(w * tau) is defined in double anyway.
//  * Gram matrices: sum_i d_i trig(w_i ta) trig(w_i tb) = 1/2 [mom(ta - tb) +- mom(ta + tb)] with
//    the moments g(t) = sum_i d_i cos(w_i t), s(t) = sum_i d_i sin(w_i t) on two unit-step
//    progressions (differences, sums): O(Mf N) instead of the O(Mf N^2) of a dense A1' D A1.
constexpr int CHK = 64;       // (folded) frequencies per chunk at most

// K1 (lattice): UU[sg][vv][i] = sum_{m in segment sg} XL[vv][cos][m] cos(w_i t_m) + XL[vv][sin][m] sin(w_i t_m),
// XL = the lattice coefficients of A1 * [v ; P'v] (column scale * entry of v, or of P'v), formed here in
// LDS for the block's segment; one thread per (FOLDED frequency, segment): the cosine and the sine sums are kept
// apart, C + S is the response at +wf and C - S the one at -wf; the coefficient reads are wave-uniform.
constexpr int SEGMAX = 128;
template <int NV>
__global__ __launch_bounds__(256) void k_trig_eval(DProg P, const double* __restrict__ vin, double* __restrict__ UU) {
    LANES(P, vin, UU);
    constexpr int NVVMAX = 2 * NV;
    __shared__ double2 cf[NVVMAX][SEGMAX];                // (cos, sin) coefficient pairs
    const int k = blockIdx.x * 256 + threadIdx.x, sg = blockIdx.y;
    const int m0 = sg * P.seg, m1 = min(m0 + P.seg, P.D1);
    const int NVV = P.quad ? 2 * NV : NV;
    for (int e = threadIdx.x; e < 2 * (m1 - m0); e += 256) {
        const int kind = e & 1, m = m0 + (e >> 1), le = kind * P.D1 + m;
        const int j = P.lat_col[le], qj = P.quad ? P.lat_qcol[le] : -1;
        const double sc = P.lat_scale[le], qs = P.quad ? P.lat_qscale[le] : 0.0;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const double c1 = j >= 0 ? sc * vin[(long)q * P.LDV + j] : 0.0;
            if (kind) cf[q][e >> 1].y = c1; else cf[q][e >> 1].x = c1;
            if (P.quad) {
                const double c2 = qj >= 0 ? qs * vin[(long)q * P.LDV + qj] : 0.0;
                if (kind) cf[NV + q][e >> 1].y = c2; else cf[NV + q][e >> 1].x = c2;
            }
        }
    }
    __syncthreads();
    if (k >= P.nfold) return;
    const double4 sd4 = P.seed_eval[(long)sg * P.Mpad + k];
    double c = sd4.x, s = sd4.y;
    const double cw = sd4.z, sw = sd4.w;
    double ac[NVVMAX], as[NVVMAX];
#pragma unroll
    for (int v = 0; v < NVVMAX; ++v) ac[v] = as[v] = 0;
#pragma unroll 8
    for (int m = 0; m < m1 - m0; ++m) {
#pragma unroll
        for (int v = 0; v < NVVMAX; ++v)
            if (v < NVV) { const double2 x = cf[v][m]; ac[v] += x.x * c; as[v] += x.y * s; }
        const double cn = c * cw - s * sw;
        s = s * cw + c * sw;
        c = cn;
    }
    const int ip = P.fold_pos[k], in = P.fold_neg[k];
#pragma unroll
    for (int v = 0; v < NVVMAX; ++v)
        if (v < NVV) {
            double* u = UU + ((long)sg * NVV + v) * P.Mpad;
            if (ip >= 0) u[ip] = ac[v] + as[v];
            if (in >= 0) u[in] = ac[v] - as[v];
        }
}

// One step of the rotation recurrence (c, s) <- (c cd - s sd, s cd + c sd) for the PAIRED kernels, with the fused products spelt out.
// k_trig_eval and k_trig_moments leave the fusing to the compiler's contraction, which rounds one product of each sum on its own and
// lets the other ride in the FMA -- and picked differently in the two: s cd fused in k_trig_eval (SFUSE = 0), c sd in k_trig_moments
// (SFUSE = 1).  Which product is fused decides the last bit, and a single solve always runs the unpaired kernels, so each paired kernel
// copies its twin's form here.  This is a copy, not a shared definition: if a compiler contracts the unpaired kernels otherwise,
// tests/test_lanepair_gpu.py (unit against single solves, bitwise) fails and SFUSE has to follow.
// (k_trig_moments itself now calls rotate<1> too: its body is instantiated twice per kernel -- all operands, and the full-length
//  ones alone where the border moments are not read -- and the two have to round alike.)
template <int SFUSE>
__device__ __forceinline__ void rotate(double& c, double& s, double cd, double sd) {
    const double cn = fma(c, cd, -(s * sd));
    s = SFUSE ? fma(c, sd, s * cd) : fma(s, cd, c * sd);
    c = cn;
}
// Lane pairs (k_trig_eval_pair, k_trig_moments_pair): the lanes of a lock-step unit that share grid and lattice (DProg::seeds_shared, no dims)
// run the SAME (c, s) chains, so one block serves lanes 2z and 2z + 1 and every thread runs its chain once for both: operands,
// LDS staging, accumulators and the order of each lane's accumulating FMAs stay the lane's own (results bit-identical to the unpaired kernels'),
// the program tables that are equal across the pair (ch_*, fold_*, lat_*, seeds) are read from the pair's first lane.  A pair with
// one lane masked off (or absent: odd lane count) runs the live lane alone (NL = 1) and touches nothing of the other.
// Prologue: live[] per lane of the pair, P moved to the pair's first lane; returns false when both lanes are off.
__device__ __forceinline__ bool pair_prologue(DProg& P, int nlanes, bool (&live)[2], size_t& off0) {
    const int l0 = 2 * blockIdx.z;
    live[0] = !P.mask || P.mask[l0];
    live[1] = l0 + 1 < nlanes && (!P.mask || P.mask[l0 + 1]);
    off0 = (size_t)l0 * P.lane_bytes;
    if (!live[0] && !live[1]) return false;
    if (l0) P.shift(off0);
    return true;
}
template <class T>
__device__ __forceinline__ T* byte_shift(T* p, size_t off) { return (T*)((const char*)p + off); }
// acc += x_LANE y with x_LANE the x of lane LANE of the thread's row of 16 lanes: the broadcast rides in the FMA (v_fmac_f64_dpp row_newbcast), the
// same fused operation as acc = fma(x, y, acc).  Every lane of the row has to be active (a disabled source lane leaves acc as it was).
// The s_nop in front of a block's first step covers the two wait states between a vector write of x and a DPP read, which the
// compiler does not see through an asm statement.
template <int LANE>
__device__ __forceinline__ void fmac_row(double& acc, double x, double y) {
    if constexpr (LANE == 0) asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(y));
    else asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(y), "n"(LANE));
}
// Steps I ... 15 of a block of 16 lattice points of trig_eval_sum: lane r of every row of 16 holds the coefficients of point r
template <int NVVMAX, int NL, int NVC, int I>
__device__ __forceinline__ void eval_steps16(const double2 (&x)[NL][NVVMAX], double (&ac)[NL][NVVMAX], double (&as)[NL][NVVMAX], double& c, double& s, double cw, double sw) {
    if constexpr (I < 16) {
#pragma unroll
        for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int v = 0; v < NVC; ++v) { fmac_row<I>(ac[L][v], x[L][v].x, c); fmac_row<I>(as[L][v], x[L][v].y, s); }
        rotate<0>(c, s, cw, sw);
        eval_steps16<NVVMAX, NL, NVC, I + 1>(x, ac, as, c, s, cw, sw);
    }
}
// trig_eval_sum for a pair with the vector count known (NVC > 0), in blocks of 16 points: one read per block and image instead of sixteen wave-uniform
// ones, the points' coefficients by row broadcast (every lane of the wave active; cf zero from n to the end of its last block: fma(0, c, a) = a)
template <int NVVMAX, int NL, int NVC>
__device__ __forceinline__ void trig_eval_sum_rows(const double2 (*cf)[NVVMAX][SEGMAX], int n, const double4 sd4, double (&ac)[NL][NVVMAX], double (&as)[NL][NVVMAX]) {
    double c = sd4.x, s = sd4.y;
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
    for (int v = 0; v < NVVMAX; ++v) ac[L][v] = as[L][v] = 0;
    for (int m0 = 0; m0 < n; m0 += 16) {
        double2 x[NL][NVVMAX];
#pragma unroll
        for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int v = 0; v < NVC; ++v) x[L][v] = cf[L][v][m0 + (threadIdx.x & 15)];
        eval_steps16<NVVMAX, NL, NVC, 0>(x, ac, as, c, s, sd4.z, sd4.w);
    }
}
// the sums of trig_eval_lanes over the segment's n lattice points: NVC vectors (0: the run-time count NVV), one (c, s) chain for all NL lanes
template <int NVVMAX, int NL, int NVC>
__device__ __forceinline__ void trig_eval_sum(const double2 (*cf)[NVVMAX][SEGMAX], int n, int NVV, const double4 sd4, double (&ac)[NL][NVVMAX], double (&as)[NL][NVVMAX]) {
    double c = sd4.x, s = sd4.y;
    const double cw = sd4.z, sw = sd4.w;
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
    for (int v = 0; v < NVVMAX; ++v) ac[L][v] = as[L][v] = 0;
#pragma unroll (NVVMAX == 2 ? 8 / NL : 8)              // (one vector per lane: the body under the 64-register bound; else k_trig_eval's)
    for (int m = 0; m < n; ++m) {
#pragma unroll
        for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int v = 0; v < NVVMAX; ++v)
            if (NVC ? v < NVC : v < NVV) { const double2 x = cf[L][v][m]; ac[L][v] += x.x * c; as[L][v] += x.y * s; }
        rotate<0>(c, s, cw, sw);
    }
}
// k_trig_eval's work for NL lanes in one block (vin[L], UU[L]: the lanes' own vectors; cf[L]: the lanes' own LDS images)
template <int NV, int NL>
__device__ __forceinline__ void trig_eval_lanes(const DProg& P, const double* const (&vin)[NL], double* const (&UU)[NL], double2 (*cf)[2 * NV][SEGMAX]) {
    constexpr int NVVMAX = 2 * NV;
    const int k = blockIdx.x * 256 + threadIdx.x, sg = blockIdx.y;
    const int m0 = sg * P.seg, m1 = min(m0 + P.seg, P.D1);
    const int NVV = P.quad ? 2 * NV : NV;
    for (int e = threadIdx.x; e < 2 * (m1 - m0); e += 256) {
        const int kind = e & 1, m = m0 + (e >> 1), le = kind * P.D1 + m;
        const int j = P.lat_col[le], qj = P.quad ? P.lat_qcol[le] : -1;
        const double sc = P.lat_scale[le], qs = P.quad ? P.lat_qscale[le] : 0.0;
#pragma unroll
        for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const double c1 = j >= 0 ? sc * vin[L][(long)q * P.LDV + j] : 0.0;
            if (kind) cf[L][q][e >> 1].y = c1; else cf[L][q][e >> 1].x = c1;
            if (P.quad) {
                const double c2 = qj >= 0 ? qs * vin[L][(long)q * P.LDV + qj] : 0.0;
                if (kind) cf[L][NV + q][e >> 1].y = c2; else cf[L][NV + q][e >> 1].x = c2;
            }
        }
    }
    constexpr bool ROWB = NL == 2;                        // (the one-lane body keeps the run-time vector count and k_trig_eval's loop)
    if (ROWB)                                             // (the row-broadcast sums run whole blocks of 16 points: zeros behind the segment's last one)
        for (int e = 2 * (m1 - m0) + threadIdx.x; e < 2 * ((m1 - m0 + 15) & ~15); e += 256)
#pragma unroll
            for (int L = 0; L < NL; ++L)
#pragma unroll
            for (int v = 0; v < 2 * NV; ++v) { if (e & 1) cf[L][v][e >> 1].y = 0.0; else cf[L][v][e >> 1].x = 0.0; }
    __syncthreads();
    // (a pair keeps every lane of a wave that has a frequency: its sums take their coefficients from the lanes of a row; a frequency past the end runs on zero seeds)
    if ((ROWB ? k - (int)(threadIdx.x & 63) : k) >= P.nfold) return;
    const double4 sd4 = k < P.nfold ? P.seed_eval[(long)sg * P.Mpad + k] : make_double4(0.0, 0.0, 0.0, 0.0);
    double ac[NL][NVVMAX], as[NL][NVVMAX];
    // (a pair takes the vector count out of the loop: with two lanes' reads in flight the per-vector branches cost registers)
    if constexpr (!ROWB) trig_eval_sum<NVVMAX, NL, 0>(cf, m1 - m0, NVV, sd4, ac, as);
    else if (P.quad) trig_eval_sum_rows<NVVMAX, NL, NVVMAX>(cf, m1 - m0, sd4, ac, as);
    else trig_eval_sum_rows<NVVMAX, NL, NV>(cf, m1 - m0, sd4, ac, as);
    if (k >= P.nfold) return;
    const int ip = P.fold_pos[k], in = P.fold_neg[k];
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
    for (int v = 0; v < NVVMAX; ++v)
        if (v < NVV) {
            double* u = UU[L] + ((long)sg * NVV + v) * P.Mpad;
            if (ip >= 0) u[ip] = ac[L][v] + as[L][v];
            if (in >= 0) u[in] = ac[L][v] - as[L][v];
        }
}
// ... for the lanes 2z and 2z + 1 of a unit of nlanes (launch bounds: one vector per lane the waves per SIMD k_trig_eval gets; two vectors per lane
// 4: the blocks of 16 points of both of its bodies, the four-vector one's sixteen coefficient registers included, take 128 registers; no spills --
// DESIGN.md section 4)
template <int NV>
__global__ __launch_bounds__(256, NV == 1 ? 8 : 4) void k_trig_eval_pair(DProg P, const double* __restrict__ vin, double* __restrict__ UU, int nlanes) {
    __shared__ double2 cf[2][2 * NV][SEGMAX];
    bool live[2];
    size_t off0;
    if (!pair_prologue(P, nlanes, live, off0)) return;
    const bool both = live[0] && live[1];
    const size_t off1 = (both || !live[0]) ? P.lane_bytes : 0;                 // both: the pair's second lane; else: the live one
    if (both) {
        const double* const v2[2] = {byte_shift(vin, off0), byte_shift(vin, off0 + off1)};
        double* const u2[2] = {byte_shift(UU, off0), byte_shift(UU, off0 + off1)};
        trig_eval_lanes<NV, 2>(P, v2, u2, cf);
    } else {
        const double* const v1[1] = {byte_shift(vin, off0 + off1)};
        double* const u1[1] = {byte_shift(UU, off0 + off1)};
        trig_eval_lanes<NV, 1>(P, v1, u1, cf);
    }
}

// seed tables for the recurrences below (once per design)
// (the progressions start at ka * tmin and kb * tmin: the LANE's origin)
__global__ void k_build_seeds_m(DProg P, double ka, int na, double kb, int nb, double4* __restrict__ seeds) {
    LANES(P, seeds);
    if (P.dims) { na = P.D1; nb = nb ? 2 * P.D1 - 1 : 0; }      // (the launch carries the unit's largest extent: the lane's own)
    const double t0a = ka * P.tmin, t0b = kb * P.tmin;
    const int m = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
    if (m >= na + nb || ch >= P.nchunk) return;
    const double t = m < na ? t0a + m : t0b + (m - na);
    double s, c, sd, cd;
    sincos(P.ch_w0[ch] * t, &s, &c);
    sincos(P.ch_dw[ch] * t, &sd, &cd);
    seeds[(long)ch * (na + nb) + m] = make_double4(c, s, cd, sd);
}
__global__ void k_build_seeds_e(DProg P, double4* __restrict__ seeds) {
    LANES(P, seeds);
    const int i = blockIdx.x * blockDim.x + threadIdx.x, sg = blockIdx.y;
    if (i >= P.nfold) return;
    const double w = P.wf[i];
    double s, c, sw, cw;
    sincos(w * (P.tmin + sg * P.seg), &s, &c);
    sincos(w, &sw, &cw);
    seeds[(long)sg * P.Mpad + i] = make_double4(c, s, cw, sw);
}

// K3 / K2 (lattice): partial[group][v][0|1][m] = sum over the CGRP chunks of the group, sum_{k in chunk}
// pe_v[k] cos(wf_k t_m) | po_v[k] sin(wf_k t_m), t_m on up to two unit-step progressions (na points, then nb points;
// the seeds table knows them), with pe = p(+wf) + p(-wf), po = p(+wf) - p(-wf) over the folded frequency list.
// Block = 256 moment points x one group of CGRP chunks: every thread runs the recurrence of its point through the
// group's chunks one after the other (fixed order), so the operands of a chunk group are staged -- with AGG:
// aggregated from the row vector through the CSR map (p1 = sum alpha_r val_r, p2 = sum beta_r val_r over the rows at
// that frequency); otherwise read from the per-frequency array src[v][Mpad] -- once per 256 points, and the fold
// kernels see nchunk / CGRP partials.
constexpr int CGRP = 4;
constexpr int MPTS = 256;     // moment points per block
template <int NV, bool AGG>
__device__ __forceinline__ void freq_operands(const DProg& P, const double* __restrict__ src, int i, double (&out)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) out[v] = 0;
    if (i < 0) return;
    if (AGG) {
        const int nv = P.quad ? NV / 2 : NV;
        for (int qq = P.f_ptr[i]; qq < P.f_ptr[i + 1]; ++qq) {
            const int r = P.f_rows[qq];
            const double al = P.alpha[r], be = P.beta[r];
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (v < nv) {
                    const double x = src[(long)v * P.Rp + r];
                    out[v] += al * x;
                    if (P.quad) out[nv + v] += be * x;
                }
        }
    } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) out[v] = src[(long)v * P.Mpad + i];
    }
}
// (pe, po) of every folded frequency, one thread each: the serial gathers through the CSR map happen once here, not
// once per block of the moment kernel
template <int NV, bool AGG>
__global__ __launch_bounds__(256) void k_freq_fold(DProg P, const double* __restrict__ src, double2* __restrict__ out) {
    LANES(P, src, out);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.nfold) return;
    double a[NV], b[NV];
    freq_operands<NV, AGG>(P, src, P.fold_pos[k], a);
    freq_operands<NV, AGG>(P, src, P.fold_neg[k], b);
#pragma unroll
    for (int v = 0; v < NV; ++v) out[(long)v * P.Mpad + k] = make_double2(a[v] + b[v], a[v] - b[v]);
}
// FOLD (round 5: one launch less per G'v): the folded operands are formed HERE from the row vector `rows` -- what k_freq_fold<NV, true>
// would have written to src (same sums, same order) -- by every block for the 256 frequencies of its chunk group.
// Border moments only where they are read (the H-build's one-pass form: `nfull` full-length operands in front, the border operands
// behind them, all on the progressions (na = D1, nb = 2 D1 - 1)): k_assemble_H_lat reads the border moments at the points m < D1 alone
// -- the two-pass form runs them over (D1, 0) --, so a block whose points all lie at m >= na runs the body with the first NVA = nfull
// operands: it stages, accumulates and stores those, every one by the instructions and in the order of the full body (the operands
// share the (c, s) chains and nothing else), in the partial layout of the launch's NV.  The block that straddles na does all operands.
// The border rows of `partial` keep stale words at m >= na past those blocks; k_fold_partials folds those rows over the columns m < na alone.
template <int NV>
__device__ __forceinline__ bool trim_border(int nfull, int na) { return NV > 1 && nfull == 1 && int(blockIdx.x) * MPTS >= na; }
template <int NV, int NVA, bool FOLD>
__device__ __forceinline__ void trig_moments_body(const DProg& P, const double2* __restrict__ src, const double4* __restrict__ seeds, int na, int nb,
                                                  double* __restrict__ partial, const double* __restrict__ rows, double2 (*pp)[CGRP][CHK]) {
    static_assert(NVA == NV || !FOLD, "trig_moments_body: the trimmed form is the H-build's");
    const int tid = threadIdx.x;
    const int ch0 = blockIdx.y * P.cgrp;
    for (int e = tid; e < P.cgrp * CHK; e += 256) {       // stage the operands of the group's chunks
        const int cc = e / CHK, q = e - cc * CHK, ch = ch0 + cc;
        const bool live = ch < P.nchunk && q < P.ch_count[ch < P.nchunk ? ch : 0];
        const int k = live ? P.ch_start[ch] + q : 0;
        if constexpr (FOLD) {
            double a[NV], b[NV];
            freq_operands<NV, true>(P, rows, live ? P.fold_pos[k] : -1, a);
            freq_operands<NV, true>(P, rows, live ? P.fold_neg[k] : -1, b);
#pragma unroll
            for (int v = 0; v < NVA; ++v) pp[v][cc][q] = make_double2(a[v] + b[v], a[v] - b[v]);
        } else {
#pragma unroll
        for (int v = 0; v < NVA; ++v) pp[v][cc][q] = live ? src[(long)v * P.Mpad + k] : make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    const int m = blockIdx.x * MPTS + tid;
    if (m >= na + nb) return;
    double ag[NVA], as[NVA];
#pragma unroll
    for (int v = 0; v < NVA; ++v) ag[v] = as[v] = 0;
    // two chunks at a time: their recurrences are independent chains, which is what keeps the fp64 pipe busy with the
    // two or three waves per SIMD this grid has (operands past a chunk's end are staged as zeros)
    for (int cl = 0; cl < P.cgrp; cl += 2) {
        const int cha = ch0 + cl, chb = cha + 1;
        if (cha >= P.nchunk) break;
        const bool two = cl + 1 < P.cgrp && chb < P.nchunk;
        const double4 sa = seeds[(long)cha * (na + nb) + m];
        const double4 sb = two ? seeds[(long)chb * (na + nb) + m] : make_double4(0.0, 0.0, 0.0, 0.0);
        double c0 = sa.x, s0 = sa.y, c1 = sb.x, s1 = sb.y;
        const int cnt = max(P.ch_count[cha], two ? P.ch_count[chb] : 0);
        const int clb = two ? cl + 1 : cl;                  // (a lone last chunk pairs with itself at zero weight: sb = 0)
#pragma unroll 4
        for (int q = 0; q < cnt; ++q) {
#pragma unroll
            for (int v = 0; v < NVA; ++v) {
                const double2 pa = pp[v][cl][q], pb = pp[v][clb][q];
                ag[v] += pa.x * c0; as[v] += pa.y * s0;
                ag[v] += pb.x * c1; as[v] += pb.y * s1;
            }
            // (the form the compiler's contraction gave this recurrence, spelt out since the body has two instantiations per kernel:
            //  the trimmed blocks' chains must round as the others' do)
            rotate<1>(c0, s0, sa.z, sa.w);
            rotate<1>(c1, s1, sb.z, sb.w);
        }
    }
#pragma unroll
    for (int v = 0; v < NVA; ++v) {
        partial[(((long)blockIdx.y * NV + v) * 2) * P.LDM + m] = ag[v];
        partial[(((long)blockIdx.y * NV + v) * 2 + 1) * P.LDM + m] = as[v];
    }
}

template <int NV, bool FOLD = false>
__global__ __launch_bounds__(256) void k_trig_moments(DProg P, const double2* __restrict__ src, const double4* __restrict__ seeds,
                                                      int na, int nb, double* __restrict__ partial, const double* __restrict__ rows = nullptr,
                                                      int nfull = NV) {
    if (!P.seeds_shared && blockIdx.z) seeds = reinterpret_cast<const double4*>(reinterpret_cast<const char*>(seeds) + (size_t)blockIdx.z * P.lane_bytes);
    LANES(P, src, partial, rows);
    if (P.dims) { na = P.D1; nb = nb ? 2 * P.D1 - 1 : 0; }      // (the launch carries the unit's largest extent: the lane's own)
    __shared__ double2 pp[NV][CGRP][CHK];                 // (pe, po)
    if constexpr (!FOLD && NV > 1) {
        if (trim_border<NV>(nfull, na)) { trig_moments_body<NV, 1, FOLD>(P, src, seeds, na, nb, partial, rows, pp); return; }
    }
    trig_moments_body<NV, NV, FOLD>(P, src, seeds, na, nb, partial, rows, pp);
}

// a product and a sum rounded on their own, whatever -ffp-contract says
__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_rounded(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
// The operands of one folded frequency (kp: its +w entry, kn: its -w entry; -1: none) for the NL lanes of a block: out[L][0] / out[L][1] are what
// freq_operands<NV, true> gives lane L for kp / kn -- every sum over its own rows in the same qq order -- but the 2 NL gather chains
// f_ptr -> f_rows -> alpha / beta / row run side by side: all index loads of a step, then all row loads, then the sums (a chain past its
// end reads entry 0 and adds nothing).  One after the other, as four calls of freq_operands run them, they are 4 x 4 dependent loads in front of the barrier.
// Like the rotation (rotate<>), the sums are a COPY of what the compiler made of freq_operands in k_trig_moments<NV, true>, read off its ISA:
// the first operand accumulates by FMA, out[0] = fma(alpha, x0, out[0]); the second one (NV = 2: beta x0 of a quad program, alpha x1 otherwise --
// the compiler selects between the two products, so neither rides in an FMA) adds a product that is rounded first.  With one row per
// frequency the two forms agree (the sum starts at 0); with several (the half-planes of fir_qprog_phs) they differ in the last bit.
template <int NV, int NL>
__device__ __forceinline__ void freq_operands_lanes(const DProg* const (&PL)[NL], const double* const (&rows)[NL], int kp, int kn, double (&out)[NL][2][NV]) {
    static_assert(NV <= 2, "freq_operands_lanes: the sums are spelt out for one and two operands");
    constexpr int NS = 2 * NL;                            // chain z: lane z / 2, sign z % 2
    const bool quad = PL[0]->quad;
    const int nv = quad ? NV / 2 : NV;
    int q0[NS], cnt[NS], nmax = 0;
#pragma unroll
    for (int z = 0; z < NS; ++z) {
        const int i = (z & 1) ? kn : kp;
        const int* fp = PL[z >> 1]->f_ptr;
        q0[z] = i >= 0 ? fp[i] : 0;
        cnt[z] = i >= 0 ? fp[i + 1] - q0[z] : 0;
        nmax = max(nmax, cnt[z]);
#pragma unroll
        for (int v = 0; v < NV; ++v) out[z >> 1][z & 1][v] = 0;
    }
    if (nv == 0) return;                                  // (one operand of a quad program: freq_operands adds nothing either)
    for (int t = 0; t < nmax; ++t) {
        int r[NS];
#pragma unroll
        for (int z = 0; z < NS; ++z) r[z] = PL[z >> 1]->f_rows[t < cnt[z] ? q0[z] + t : 0];
        double al[NS], be[NS], x[NS][NV];
#pragma unroll
        for (int z = 0; z < NS; ++z) {
            const DProg& Q = *PL[z >> 1];
            al[z] = Q.alpha[r[z]]; be[z] = Q.beta[r[z]];
#pragma unroll
            for (int v = 0; v < NV; ++v) x[z][v] = v < nv ? rows[z >> 1][(long)v * Q.Rp + r[z]] : 0.0;
        }
#pragma unroll
        for (int z = 0; z < NS; ++z) {
            const bool on = t < cnt[z];
            double (&o)[NV] = out[z >> 1][z & 1];
            const double a0 = fma(al[z], x[z][0], o[0]);
            o[0] = on ? a0 : o[0];
            if constexpr (NV == 2) {
                const double p = quad ? mul_rounded(be[z], x[z][0]) : mul_rounded(al[z], x[z][1]);
                const double a1 = add_rounded(o[1], p);
                o[1] = on ? a1 : o[1];
            }
        }
    }
}
// Steps I ... 15 of a block of 16 steps of trig_moments_lanes' loop: lane r of every row of 16 holds the operands of step r (pa: the first chunk's,
// pb: the second one's); per lane and vector the four FMAs of a step in the loop's order, then the two rotations.
template <int NV, int NL, int I>
__device__ __forceinline__ void moment_steps16(const double2 (&pa)[NL][NV], const double2 (&pb)[NL][NV], double (&ag)[NL][NV], double (&as)[NL][NV],
                                               double& c0, double& s0, double& c1, double& s1, const double4& sa, const double4& sb) {
    if constexpr (I < 16) {
#pragma unroll
        for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            fmac_row<I>(ag[L][v], pa[L][v].x, c0); fmac_row<I>(as[L][v], pa[L][v].y, s0);
            fmac_row<I>(ag[L][v], pb[L][v].x, c1); fmac_row<I>(as[L][v], pb[L][v].y, s1);
        }
        rotate<1>(c0, s0, sa.z, sa.w);
        rotate<1>(c1, s1, sb.z, sb.w);
        moment_steps16<NV, NL, I + 1>(pa, pb, ag, as, c0, s0, c1, s1, sa, sb);
    }
}
// k_trig_moments<NV, FOLD>'s work for NL lanes in one block (lane pairs, see k_trig_eval_pair): P holds the tables the lanes share, PL[L] the lane's own
// program (alpha, beta, f_ptr, f_rows), rows[L] (FOLD) or src[L] (the lane's folded operands PPf) / partial[L] its vectors, pp[L] its LDS image; one
// (c, s) chain per chunk serves all NL lanes.  The seeds of the first two chunks are loaded in front of the staging, so they arrive while the operands
// are gathered; the next two chunks' travel during the loop before.  With one or two operands per lane the loop reads each operand from LDS in ONE lane
// per row of 16 and hands it to the others inside the FMA (moment_steps16): read by every thread, the wave-uniform reads held the CU's one LDS pipe as
// long as the FMAs held its four fp64 pipes, and the two did not overlap.
// (NVA: the operands the block works on, the first NVA of the layout's NV -- see trim_border)
template <int NV, int NL, bool FOLD, int NVA = NV>
__device__ __forceinline__ void trig_moments_lanes(const DProg& P, const DProg* const (&PL)[NL], const double2* const (&src)[NL], const double4* __restrict__ seeds, int na, int nb,
                                                   double* const (&partial)[NL], const double* const (&rows)[NL], double2 (*pp)[NV][CGRP][CHK]) {
    static_assert(NVA == NV || !FOLD, "trig_moments_lanes: the trimmed form is the H-build's");
    const int tid = threadIdx.x;
    const int ch0 = blockIdx.y * P.cgrp;
    const int m = blockIdx.x * MPTS + tid;
    const auto seed = [&](int cc) {                       // (zero without the chunk: a lone last chunk pairs with zero weight)
        return (m < na + nb && cc < P.cgrp && ch0 + cc < P.nchunk) ? seeds[(long)(ch0 + cc) * (na + nb) + m] : make_double4(0.0, 0.0, 0.0, 0.0);
    };
    double4 sa = seed(0), sb = seed(1);
    for (int e = tid; e < P.cgrp * CHK; e += 256) {       // stage the operands of the group's chunks
        const int cc = e / CHK, q = e - cc * CHK, ch = ch0 + cc;
        const bool live = ch < P.nchunk && q < P.ch_count[ch < P.nchunk ? ch : 0];
        const int k = live ? P.ch_start[ch] + q : 0;
        if constexpr (FOLD) {
            double ab[NL][2][NV];
            freq_operands_lanes<NV, NL>(PL, rows, live ? P.fold_pos[k] : -1, live ? P.fold_neg[k] : -1, ab);
#pragma unroll
            for (int L = 0; L < NL; ++L)
#pragma unroll
            for (int v = 0; v < NV; ++v) pp[L][v][cc][q] = make_double2(ab[L][0][v] + ab[L][1][v], ab[L][0][v] - ab[L][1][v]);
        } else {
#pragma unroll
            for (int L = 0; L < NL; ++L)
#pragma unroll
            for (int v = 0; v < NVA; ++v) pp[L][v][cc][q] = live ? src[L][(long)v * P.Mpad + k] : make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    // ROWB (one or two operands per lane): the loop takes its operands from the lanes of the thread's row instead of reading every one of them
    // in every thread, so a wave with a point to compute keeps all its lanes (a point past the end runs on zero seeds and stores nothing)
    constexpr bool ROWB = NV <= 2;
    if ((ROWB ? m - (tid & 63) : m) >= na + nb) return;
    double ag[NL][NVA], as[NL][NVA];
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
    for (int v = 0; v < NVA; ++v) ag[L][v] = as[L][v] = 0;
    // two chunks at a time: their recurrences are independent chains, which is what keeps the fp64 pipe busy with the
    // two or three waves per SIMD this grid has (operands past a chunk's end are staged as zeros)
    for (int cl = 0; cl < P.cgrp; cl += 2) {
        const int cha = ch0 + cl, chb = cha + 1;
        if (cha >= P.nchunk) break;
        const bool two = cl + 1 < P.cgrp && chb < P.nchunk;
        const double4 na4 = seed(cl + 2), nb4 = seed(cl + 3);
        double c0 = sa.x, s0 = sa.y, c1 = sb.x, s1 = sb.y;
        const int cnt = max(P.ch_count[cha], two ? P.ch_count[chb] : 0);
        const int clb = two ? cl + 1 : cl;                  // (a lone last chunk pairs with itself at zero weight: sb = 0)
        if constexpr (ROWB) {
            // blocks of 16 steps: lane r of a row loads the operands of step q0 + r (one read per block and image where the plain loop below
            // has sixteen wave-uniform ones), the steps take them by row broadcast.  The last block runs past cnt on operands staged
            // as zeros, like the shorter chunk of the two: fma(0, c, a) = a.
            for (int q0 = 0; q0 < cnt; q0 += 16) {
                double2 pa[NL][NVA], pb[NL][NVA];
#pragma unroll
                for (int L = 0; L < NL; ++L)
#pragma unroll
                for (int v = 0; v < NVA; ++v) { pa[L][v] = pp[L][v][cl][q0 + (tid & 15)]; pb[L][v] = pp[L][v][clb][q0 + (tid & 15)]; }
                moment_steps16<NVA, NL, 0>(pa, pb, ag, as, c0, s0, c1, s1, sa, sb);
            }
        } else {
#pragma unroll (NV * NL > 4 ? 2 : 4)
        for (int q = 0; q < cnt; ++q) {
#pragma unroll
            for (int L = 0; L < NL; ++L)
#pragma unroll
            for (int v = 0; v < NVA; ++v) {
                const double2 pa = pp[L][v][cl][q], pb = pp[L][v][clb][q];
                ag[L][v] += pa.x * c0; as[L][v] += pa.y * s0;
                ag[L][v] += pb.x * c1; as[L][v] += pb.y * s1;
            }
            rotate<1>(c0, s0, sa.z, sa.w);
            rotate<1>(c1, s1, sb.z, sb.w);
        }
        }
        sa = na4; sb = nb4;
    }
    if (m >= na + nb) return;
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
    for (int v = 0; v < NVA; ++v) {
        partial[L][(((long)blockIdx.y * NV + v) * 2) * P.LDM + m] = ag[L][v];
        partial[L][(((long)blockIdx.y * NV + v) * 2 + 1) * P.LDM + m] = as[L][v];
    }
}
// ... for the lanes 2z and 2z + 1 of a unit of nlanes with seeds_shared and without dims (seeds: the unit's one table; na, nb: every lane's).
// FOLD: the G'v form, operands gathered from `rows` (one or two operands: with four the registers allow fewer waves per SIMD than
// k_trig_moments<4, true> gets); else the H-build form, operands from the lanes' `src` (PPf), both progressions.  DESIGN.md section 4.
template <int NV, bool FOLD = true>
__global__ __launch_bounds__(256, 4) void k_trig_moments_pair(DProg P, const double2* __restrict__ src, const double4* __restrict__ seeds, int na, int nb,
                                                                       double* __restrict__ partial, const double* __restrict__ rows, int nlanes,
                                                                       int nfull = NV) {
    static_assert(!FOLD || NV <= 2, "k_trig_moments_pair: G'v of one or two operands");
    __shared__ double2 pp[2][NV][CGRP][CHK];
    bool live[2];
    size_t off0;
    if (!pair_prologue(P, nlanes, live, off0)) return;
    const bool both = live[0] && live[1];
    const size_t off1 = (both || !live[0]) ? P.lane_bytes : 0;                 // both: the pair's second lane; else: the live one
    DProg Q = P;
    Q.shift(off1);
    if (both) {
        const DProg* const p2[2] = {&P, &Q};
        const double2* const s2[2] = {FOLD ? nullptr : byte_shift(src, off0), FOLD ? nullptr : byte_shift(src, off0 + off1)};
        double* const o2[2] = {byte_shift(partial, off0), byte_shift(partial, off0 + off1)};
        const double* const r2[2] = {FOLD ? byte_shift(rows, off0) : nullptr, FOLD ? byte_shift(rows, off0 + off1) : nullptr};
        if constexpr (!FOLD && NV > 1) {
            if (trim_border<NV>(nfull, na)) { trig_moments_lanes<NV, 2, FOLD, 1>(P, p2, s2, seeds, na, nb, o2, r2, pp); return; }
        }
        trig_moments_lanes<NV, 2, FOLD>(P, p2, s2, seeds, na, nb, o2, r2, pp);
    } else {
        const DProg* const p1[1] = {&Q};
        const double2* const s1[1] = {FOLD ? nullptr : byte_shift(src, off0 + off1)};
        double* const o1[1] = {byte_shift(partial, off0 + off1)};
        const double* const r1[1] = {FOLD ? byte_shift(rows, off0 + off1) : nullptr};
        if constexpr (!FOLD && NV > 1) {
            if (trim_border<NV>(nfull, na)) { trig_moments_lanes<NV, 1, FOLD, 1>(P, p1, s1, seeds, na, nb, o1, r1, pp); return; }
        }
        trig_moments_lanes<NV, 1, FOLD>(P, p1, s1, seeds, na, nb, o1, r1, pp);
    }
}

// ------------------------------------------------------------------------------------------------
// reductions: every block writes NC partial values; scalar kernels fold them in a fixed order
template <int NC>
__device__ __forceinline__ void block_partials(double vals[NC], double* __restrict__ part, bool is_max) {
    __shared__ double sh[17];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double s = is_max ? block_max(vals[c], sh) : block_sum(vals[c], sh);
        if (threadIdx.x == 0) part[(long)blockIdx.x * NC + c] = s;
    }
}
__device__ __forceinline__ double fold_partials(const double* part, int nb, int nc, int c, bool is_max, double* sh) {
    double a = is_max ? -1e300 : 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        double v = part[(long)b * nc + c];
        a = is_max ? fmax(a, v) : a + v;
    }
    return is_max ? block_max(a, sh) : block_sum(a, sh);
}
// K block reductions in ONE barrier sequence (the prologues of the cone kernels ran one block_sum / block_max after the other): column k
// goes through the wave tree and then over the waves in their order exactly as in block_sum / block_max -- thread k does the walk
// thread 0 does there --, so every result has the bits of its own call.  sh: K rows of 17 doubles; results valid in every thread
template <int K>
__device__ __forceinline__ void block_reduce_k(double (&v)[K], bool is_max, double (*sh)[17]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = is_max ? wave_max(v[k]) : wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[k][wv] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double* q = sh[threadIdx.x];
        double t = is_max ? q[0] : 0.0 + q[0];
        for (int i = 1; i < nw; ++i) t = is_max ? fmax(t, q[i]) : t + q[i];
        q[16] = t;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k][16];
}
// fold_partials of the K columns c0 .. c0 + K - 1 in one pass over the partial rows (each thread walks its rows in fold_partials' order)
template <int K>
__device__ __forceinline__ void fold_partials_k(const double* part, int nb, int nc, int c0, bool is_max, double (&a)[K], double (*sh)[17]) {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = is_max ? -1e300 : 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double v = part[(long)b * nc + c0 + k];
            a[k] = is_max ? fmax(a[k], v) : a[k] + v;
        }
    }
    block_reduce_k<K>(a, is_max, sh);
}
// the step to the boundary from the folded maxima (k_scal_step's arithmetic, shared by the kernels that form it themselves)
__device__ __forceinline__ double step_bound(double ts, double tz, double tau, double kap, double dtau, double dkap) {
    return fmax(0.0, fmax(fmax(ts, tz), fmax(-dtau / tau, -dkap / kap)));
}

// ------------------------------------------------------------------------------------------------
// big cone (one workgroup).  Vectors are slices at offset ob of the R-space vectors.
struct BigW {
    double eta, w0;
};
__device__ __forceinline__ double big_dot(const double* a, const double* b, int n, double* sh) {
    double t = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) t += a[i] * b[i];
    return block_sum(t, sh);
}

// scaling of the big cone: wbb (w0 in [0], w1 in [1..]), eta -> Sc[S_ETAB]; lam = W z
__global__ __launch_bounds__(1024) void k_big_scaling(DProg P, const double* __restrict__ s,
                                                      const double* __restrict__ z, double* __restrict__ wbb,
                                                      double* __restrict__ lam, double* __restrict__ Sc) {
    LANES(P, s, z, wbb, lam, Sc);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;                       // (the lane's own row count: heterogeneous units)
    s += ob; z += ob; lam += ob;
    const int big = P.big, n1 = big - 1;
    double ns = sqrt(big_dot(s + 1, s + 1, n1, sh)), nz = sqrt(big_dot(z + 1, z + 1, n1, sh));
    double a = sqrt(jres(s[0], ns)), b = sqrt(jres(z[0], nz));
    double sz1 = big_dot(s + 1, z + 1, n1, sh);
    double gamma = sqrt((1.0 + (s[0] * z[0] + sz1) / (a * b)) / 2.0);
    double w0 = (s[0] / a + z[0] / b) / (2 * gamma);
    double eta = sqrt(a / b);
    for (int i = threadIdx.x; i < n1; i += blockDim.x) wbb[1 + i] = (s[1 + i] / a - z[1 + i] / b) / (2 * gamma);
    if (threadIdx.x == 0) { wbb[0] = w0; Sc[S_ETAB] = eta; Sc[S_WB0] = w0; }
    __syncthreads();
    // lam = W z
    double dot = big_dot(wbb + 1, z + 1, n1, sh);
    double f = z[0] + dot / (1 + w0);
    for (int i = threadIdx.x; i < n1; i += blockDim.x) lam[1 + i] = (z[1 + i] + f * wbb[1 + i]) * eta;
    if (threadIdx.x == 0) lam[0] = (w0 * z[0] + dot) * eta;
}

// out = W u / W^-1 u for the big cone (device function; all threads of the block participate)
__device__ __forceinline__ void big_apply(int big, const double* wbb, double eta, const double* u, double* out,
                                          bool inverse, double* sh) {
    const int n1 = big - 1;
    const double w0 = wbb[0], u0 = u[0];
    double dot = big_dot(wbb + 1, u + 1, n1, sh);
    if (inverse) {
        double f = -u0 + dot / (1 + w0);
        for (int i = threadIdx.x; i < n1; i += blockDim.x) out[1 + i] = (u[1 + i] + f * wbb[1 + i]) / eta;
        __syncthreads();
        if (threadIdx.x == 0) out[0] = (w0 * u0 - dot) / eta;
    } else {
        double f = u0 + dot / (1 + w0);
        for (int i = threadIdx.x; i < n1; i += blockDim.x) out[1 + i] = (u[1 + i] + f * wbb[1 + i]) * eta;
        __syncthreads();
        if (threadIdx.x == 0) out[0] = (w0 * u0 + dot) * eta;
    }
    __syncthreads();
}
// out (op)= W^-2 v : mode 0: out = W^-2 v - sub (sub may be null) ; mode 1: out += W^-2 v
__device__ __forceinline__ void big_inv2(int big, const double* wbb, double eta, const double* v, const double* sub,
                                         double* out, int mode, double* sh) {
    const int n1 = big - 1;
    const double u0 = wbb[0], e2 = 1.0 / (eta * eta), v0 = v[0];
    double uv = u0 * v0 - big_dot(wbb + 1, v + 1, n1, sh);          // (Jw)'v
    for (int i = threadIdx.x; i < n1; i += blockDim.x) {
        double t = (2 * (-wbb[1 + i]) * uv + v[1 + i]) * e2;
        if (mode == 0) out[1 + i] = t - (sub ? sub[1 + i] : 0.0);
        else out[1 + i] += t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = (2 * u0 * uv - v0) * e2;
        if (mode == 0) out[0] = t - (sub ? sub[0] : 0.0);
        else out[0] += t;
    }
    __syncthreads();
}
// max-step term ||rho1|| - rho0 for direction d relative to lam
__device__ __forceinline__ double big_step(int big, const double* lam, const double* d, double* sh) {
    const int n1 = big - 1;
    double nl = sqrt(big_dot(lam + 1, lam + 1, n1, sh));
    double a = sqrt(jres(lam[0], nl));
    double lb0 = lam[0] / a;
    double dot = big_dot(lam + 1, d + 1, n1, sh) / a;                 // lbar1'd1
    double rho0 = (lb0 * d[0] - dot) / a;
    double f = -d[0] + dot / (1 + lb0);
    double t = 0;
    for (int i = threadIdx.x; i < n1; i += blockDim.x) {
        double r = (d[1 + i] + f * lam[1 + i] / a) / a;
        t += r * r;
    }
    t = block_sum(t, sh);
    return sqrt(t) - rho0;
}

// ------------------------------------------------------------------------------------------------
// K6 scaling for LP rows and Q3 cones (thread per cone); lam = W z
// NT scaling of the LP rows and Q3 cones; with bz2 != null also wbz2 = W^-2 bz2 for the two right-hand
// sides of the batch solve that follows (saves the separate k_winv2 pass)
__global__ void k_scaling(DProg P, const double* __restrict__ s, const double* __restrict__ z,
                          double* __restrict__ dl, double* __restrict__ wl, double* __restrict__ w3,
                          double* __restrict__ lam, const double* __restrict__ bz2, double* __restrict__ wbz2) {
    LANES(P, s, z, dl, wl, w3, lam, bz2, wbz2);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.l) {
        double sv = s[t], zv = z[t];
        const double dd = zv / sv;
        dl[t] = dd;
        wl[t] = sqrt(sv / zv);
        lam[t] = sqrt(sv * zv);
        if (bz2) { wbz2[t] = dd * bz2[t]; wbz2[P.Rp + t] = dd * bz2[P.Rp + t]; }
    } else if (t < P.l + P.nq3) {
        int c = t - P.l, r = P.l + 3 * c;
        double ss[3] = {s[r], s[r + 1], s[r + 2]}, zz[3] = {z[r], z[r + 1], z[r + 2]}, ll[3];
        Soc3 W = soc3_scaling(ss, zz);
        soc3_apply(W, zz, ll, false);
        w3[4 * c] = W.eta; w3[4 * c + 1] = W.w0; w3[4 * c + 2] = W.w1; w3[4 * c + 3] = W.w2;
        lam[r] = ll[0]; lam[r + 1] = ll[1]; lam[r + 2] = ll[2];
        if (bz2)
            for (int v = 0; v < 2; ++v) {
                const long o = (long)v * P.Rp + r;
                double vv[3] = {bz2[o], bz2[o + 1], bz2[o + 2]}, rr[3];
                soc3_inv2_apply(W, vv, rr);
                wbz2[o] = rr[0]; wbz2[o + 1] = rr[1]; wbz2[o + 2] = rr[2];
            }
    }
}
__device__ __forceinline__ Soc3 load_w3(const double* w3, int c) {
    Soc3 W;
    W.eta = w3[4 * c]; W.w0 = w3[4 * c + 1]; W.w1 = w3[4 * c + 2]; W.w2 = w3[4 * c + 3];
    return W;
}

// out = W^-2 in - sub  (mode 0)   or   out += W^-2 in  (mode 1), LP rows + Q3 cones
template <int NV>
__global__ void k_winv2(DProg P, const double* __restrict__ dl, const double* __restrict__ w3,
                        const double* __restrict__ in, const double* __restrict__ sub, double* __restrict__ out,
                        int mode) {
    LANES(P, dl, w3, in, sub, out);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.l) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            long o = (long)v * P.Rp + t;
            double val = dl[t] * in[o];
            if (mode == 0) out[o] = val - (sub ? sub[o] : 0.0);
            else out[o] += val;
        }
    } else if (t < P.l + P.nq3) {
        int c = t - P.l;
        Soc3 W = load_w3(w3, c);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            long o = (long)v * P.Rp + P.l + 3 * c;
            double vv[3] = {in[o], in[o + 1], in[o + 2]}, rr[3];
            soc3_inv2_apply(W, vv, rr);
            for (int a = 0; a < 3; ++a) {
                if (mode == 0) out[o + a] = rr[a] - (sub ? sub[o + a] : 0.0);
                else out[o + a] += rr[a];
            }
        }
    }
}
// rows of G v AND out = W^-2 (G v) - sub in one pass (programs without a big cone): one thread per
// LP row / Q3 cone
template <int NV>
__global__ void k_rows_winv2(DProg P, const double* __restrict__ UU, const double* __restrict__ X,
                             const double* __restrict__ dl, const double* __restrict__ w3,
                             const double* __restrict__ sub, double* __restrict__ gout, double* __restrict__ out) {
    LANES(P, UU, X, dl, w3, sub, gout, out);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.l) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const long o = (long)v * P.Rp + t;
            const double gv = row_value<NV>(P, UU, X, t, v);
            gout[o] = gv;
            out[o] = dl[t] * gv - (sub ? sub[o] : 0.0);
        }
    } else if (t < P.l + P.nq3) {
        const int c = t - P.l;
        const Soc3 W = load_w3(w3, c);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const long o = (long)v * P.Rp + P.l + 3 * c;
            double vv[3], rr[3];
            for (int a = 0; a < 3; ++a) { vv[a] = row_value<NV>(P, UU, X, P.l + 3 * c + a, v); gout[o + a] = vv[a]; }
            soc3_inv2_apply(W, vv, rr);
            for (int a = 0; a < 3; ++a) out[o + a] = rr[a] - (sub ? sub[o + a] : 0.0);
        }
    }
}
template <int NV>
__global__ __launch_bounds__(1024) void k_big_winv2(DProg P, const double* __restrict__ wbb,
                                                    const double* __restrict__ Sc, const double* __restrict__ in,
                                                    const double* __restrict__ sub, double* __restrict__ out, int mode) {
    LANES(P, wbb, Sc, in, sub, out);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;
    for (int v = 0; v < NV; ++v) {
        long o = (long)v * P.Rp + ob;
        big_inv2(P.big, wbb, Sc[S_ETAB], in + o, sub ? sub + o : nullptr, out + o, mode, sh);
    }
}

// ------------------------------------------------------------------------------------------------
// residuals
// rows: rz = Gx + s - h tau ; bz batch: [0] = h (constant system), [1] = s - rz (affine)
// UU != null: the rows of G x are formed here from the per-frequency products (no k_rows_G pass)
__global__ __launch_bounds__(256) void k_resid_rows(DProg P, const double* __restrict__ Gx, const double* __restrict__ s,
                                                    const double* __restrict__ z, const double* __restrict__ Sc,
                                                    double* __restrict__ rz, double* __restrict__ bz2,
                                                    double* __restrict__ part, const double* __restrict__ UU,
                                                    const double* __restrict__ X) {
    LANES(P, Gx, s, z, Sc, rz, bz2, part, UU, X);
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    double v[4] = {0, 0, 0, 0};
    if (r < P.R) {
        double tau = Sc[S_TAU], gx = UU ? row_value<1>(P, UU, X, r, 0) : Gx[r], sv = s[r], zv = z[r], hv = P.h[r];
        double res = gx + sv - hv * tau;
        rz[r] = res;
        bz2[r] = hv;
        bz2[P.Rp + r] = sv - res;
        const double wr = P.row_weight(r);
        v[0] = wr * (res * res); v[1] = wr * (sv * zv); v[2] = wr * (hv * zv); v[3] = wr * ((gx + sv) * (gx + sv));
    }
    block_partials<4>(v, part, false);
}
// One workgroup: columns rx = G'z + c tau, bx batch [0] = -c, [1] = -rx, the N-space sums, the fold of
// the row partials and all residual / gap / certificate scalars.
// phase 0: fold the local row sums into RB (then the host all-reduces RB over the row shards);
// phase 1: take the row sums from RB and finish; phase 2: both in one launch (single GPU).
__global__ __launch_bounds__(1024) void k_scal_resid(DProg P, double* __restrict__ Sc, const double* __restrict__ GTz,
                                                     const double* __restrict__ x, double* __restrict__ rx,
                                                     double* __restrict__ bx2, const double* __restrict__ partR, int nbR,
                                                     double* __restrict__ RB, int phase, const int* __restrict__ flag) {
    LANES(P, Sc, GTz, x, rx, bx2, partR, RB, flag);
    __shared__ double sh[17];
    double rz2, sz, hz, gxs2;
    if (phase != 1) {
        rz2 = fold_partials(partR, nbR, 4, 0, false, sh);
        sz = fold_partials(partR, nbR, 4, 1, false, sh);
        hz = fold_partials(partR, nbR, 4, 2, false, sh);
        gxs2 = fold_partials(partR, nbR, 4, 3, false, sh);
        if (phase == 0) {
            // (row-sharded: the fifth slot carries this rank's pivot-replacement count -- every rank factorises the same H itself,
            //  and the wall exit / the NUMERICAL verdict branch on that count: summed over the ranks with the row sums, every rank
            //  sees the SAME number whatever its own factorisation said, so the ranks cannot part ways in front of a collective)
            if (threadIdx.x == 0) { RB[0] = rz2; RB[1] = sz; RB[2] = hz; RB[3] = gxs2; RB[4] = flag ? double(flag[0]) : 0.0; }
            return;
        }
    } else {
        rz2 = RB[0]; sz = RB[1]; hz = RB[2]; gxs2 = RB[3];
    }
    const double tau0 = Sc[S_TAU];
    double a0 = 0, a1 = 0, a2 = 0;
    for (int j = threadIdx.x; j < P.N; j += blockDim.x) {
        double g = GTz[j], cv = P.c[j];
        double res = g + cv * tau0;
        rx[j] = res;
        bx2[j] = -cv;
        bx2[P.LDV + j] = -res;
        a0 += res * res; a1 += cv * x[j]; a2 += g * g;
    }
    double rx2 = block_sum(a0, sh);
    double cx = block_sum(a1, sh);
    double gtz2 = block_sum(a2, sh);
    if (threadIdx.x == 0) {
        double tau = Sc[S_TAU], kap = Sc[S_KAPPA];
        Sc[S_RT] = kap + cx + hz;
        Sc[S_MU] = (sz + kap * tau) / (Sc[S_DEG] + 1.0);
        Sc[S_CX] = cx; Sc[S_HZ] = hz; Sc[S_SZ] = sz;
        double pcost = cx / tau, dcost = -hz / tau, gap = sz / (tau * tau);
        Sc[S_PCOST] = pcost; Sc[S_DCOST] = dcost; Sc[S_GAP] = gap;
        Sc[S_PRES] = sqrt(rz2) / tau / Sc[S_NRMH];
        Sc[S_DRES] = sqrt(rx2) / tau / Sc[S_NRMC];
        double den = fmax(fabs(pcost), fabs(dcost));
        Sc[S_RELGAP] = den > 0 ? gap / den : 1e300;
        Sc[S_PINF] = hz < 0 ? sqrt(gtz2) / (-hz) : 1e300;
        Sc[S_DINF] = cx < 0 ? sqrt(gxs2) / (-cx) : 1e300;
        Sc[S_CHOLFIX] = phase == 1 ? RB[4] : (flag ? double(flag[0]) : 0.0);
    }
}

// ------------------------------------------------------------------------------------------------
// N-space helpers
// ---- single-workgroup N-space kernels (N <= a few thousand: one launch does reduce + update) ----
// r[v] = bx[v] - t[v] ; Sc[slot] = max_v ||r_v||_2
template <int NV>
__global__ __launch_bounds__(1024) void k_resid_norm(DProg P, const double* __restrict__ bx, const double* __restrict__ t,
                                                     double* __restrict__ out, double* __restrict__ Sc, int slot) {
    LANES(P, bx, t, out, Sc);
    __shared__ double sh[17];
    double m = 0;
    for (int v = 0; v < NV; ++v) {
        double a = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) {
            long o = (long)v * P.LDV + j;
            double r = bx[o] - t[o];
            out[o] = r;
            a += r * r;
        }
        m = fmax(m, sqrt(block_sum(a, sh)));
    }
    if (threadIdx.x == 0) Sc[slot] = m;
}
// CG: rz_new = r'z ; beta = first ? 0 : rz_new / rz ; rz = rz_new ; p = z + beta p
template <int NV>
__global__ __launch_bounds__(1024) void k_cg_start(DProg P, double* __restrict__ Sc, const double* __restrict__ r,
                                                   const double* __restrict__ z, double* __restrict__ p, int first) {
    LANES(P, Sc, r, z, p);
    __shared__ double sh[17];
    for (int v = 0; v < NV; ++v) {
        double a = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) a += r[(long)v * P.LDV + j] * z[(long)v * P.LDV + j];
        const double rz_new = block_sum(a, sh);
        const double rz_old = Sc[S_CG_RZ + v];
        const double beta = first ? 0.0 : (rz_old > 0 ? rz_new / rz_old : 0.0);
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) {
            long o = (long)v * P.LDV + j;
            p[o] = first ? z[o] : z[o] + beta * p[o];
        }
        __syncthreads();
        if (threadIdx.x == 0) Sc[S_CG_RZ + v] = rz_new;
    }
}
// The same behind the one-pass z = M'M r (round 5: one launch instead of k_hsolve_fold + k_cg_start): 1024 threads add the
// HS_PARTS partial vectors of k_hsolve in k_hsolve_fold's order (thread (w, t) the entry j = t + 256 w), then the first 256 do
// k_cg_start's sums -- thread t over its four entries in w order, the block sum of 256 threads -- with z from LDS: the same bits.
// One workgroup per vector (grid (NV, 1, lanes), vector v = blockIdx.x: the vectors share nothing -- their own partials, p, r and
// S_CG_RZ + v --, so two workgroups do side by side what one did one after the other); a grid of one workgroup does all NV.
template <int NV>
__global__ __launch_bounds__(1024) void k_fold_cg_start(DProg P, double* __restrict__ Sc, const double* __restrict__ r,
                                                        const double* __restrict__ part, double* __restrict__ p, int first) {
    LANES(P, Sc, r, part, p);
    __shared__ double zs[1024];
    __shared__ double sh[17];
    const int t = threadIdx.x;
    const bool act = t < SCAL_T;                              // (the 768 others only keep the barriers company)
    const int lane = t & 63, wv = t >> 6;
    const int v0 = gridDim.x > 1 ? blockIdx.x : 0, v1 = gridDim.x > 1 ? blockIdx.x + 1 : NV;
    for (int v = v0; v < v1; ++v) {
        double x[HS_PARTS];
#pragma unroll
        for (int g = 0; g < HS_PARTS; ++g) x[g] = t < P.np ? part[((long)g * NV + v) * P.np + t] : 0.0;
        double s = 0;
#pragma unroll
        for (int g = 0; g < HS_PARTS; ++g) s += x[g];
        zs[t] = s;                                            // (a grid of one: the barrier that ends the vector before has freed zs)
        __syncthreads();
        double a = 0;
        if (act) for (int j = t; j < P.N; j += SCAL_T) a += r[(long)v * P.LDV + j] * zs[j];
        a = wave_sum(a);                                      // block_sum of the first 256 threads
        __syncthreads();
        if (act && lane == 0) sh[wv] = a;
        __syncthreads();
        if (t == 0) { double q = 0; for (int i = 0; i < SCAL_T / 64; ++i) q += sh[i]; sh[16] = q; }
        __syncthreads();
        const double rz_new = sh[16];
        const double rz_old = Sc[S_CG_RZ + v];
        const double beta = first ? 0.0 : (rz_old > 0 ? rz_new / rz_old : 0.0);
        if (act) for (int j = t; j < P.N; j += SCAL_T) {
            const long o = (long)v * P.LDV + j;
            p[o] = first ? zs[j] : zs[j] + beta * p[o];
        }
        __syncthreads();
        if (t == 0) Sc[S_CG_RZ + v] = rz_new;
    }
}
// CG: alpha = rz / p'Hp (0 if p'Hp <= 0) ; dx += alpha p ; r -= alpha Hp ; Sc[slot] = max_v ||r_v||
template <int NV>
__global__ __launch_bounds__(1024) void k_cg_step(DProg P, double* __restrict__ Sc, const double* __restrict__ p,
                                                  const double* __restrict__ Hp, double* __restrict__ dx,
                                                  double* __restrict__ r, int slot) {
    LANES(P, Sc, p, Hp, dx, r);
    __shared__ double sh[17];
    double m = 0;
    for (int v = 0; v < NV; ++v) {
        double a = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) a += p[(long)v * P.LDV + j] * Hp[(long)v * P.LDV + j];
        const double pHp = block_sum(a, sh);
        const double al = pHp > 0 ? Sc[S_CG_RZ + v] / pHp : 0.0;
        double rr2 = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) {
            long o = (long)v * P.LDV + j;
            dx[o] += al * p[o];
            double rr = r[o] - al * Hp[o];
            r[o] = rr;
            rr2 += rr * rr;
        }
        m = fmax(m, sqrt(block_sum(rr2, sh)));
        if (threadIdx.x == 0) Sc[S_CG_ALPHA + v] = al;
    }
    if (threadIdx.x == 0) Sc[slot] = m;
}
// ---- preconditioned conjugate gradients on (G' W^-2 G) dx = rhs: R-space update -------------------
// gdx += alpha Gp ; dz += alpha Wp
template <int NV>
__global__ void k_cg_update_r(DProg P, const double* __restrict__ Sc, const double* __restrict__ Gp,
                              const double* __restrict__ Wp, double* __restrict__ gdx, double* __restrict__ dz) {
    LANES(P, Sc, Gp, Wp, gdx, dz);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P.R) return;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        long o = (long)q * P.Rp + t;
        double al = Sc[S_CG_ALPHA + q];
        gdx[o] += al * Gp[o];
        dz[o] += al * Wp[o];
    }
}
// CG step and R-space update in one launch (unsharded solves): every block forms alpha = rz / p'Hp itself
// (N is small), updates its slice of gdx / dz, and block 0 also does dx += alpha p, r -= alpha Hp and the
// residual norm.
template <int NV>
__global__ __launch_bounds__(256) void k_cg_step_update(DProg P, double* __restrict__ Sc, const double* __restrict__ p,
                                                        const double* __restrict__ Hp, double* __restrict__ dx,
                                                        double* __restrict__ r, int slot, const double* __restrict__ Gp,
                                                        const double* __restrict__ Wp, double* __restrict__ gdx,
                                                        double* __restrict__ dz) {
    LANES(P, Sc, p, Hp, dx, r, Gp, Wp, gdx, dz);
    __shared__ double sh[17];
    double al[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double a = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) a += p[(long)v * P.LDV + j] * Hp[(long)v * P.LDV + j];
        const double pHp = block_sum(a, sh);
        al[v] = pHp > 0 ? Sc[S_CG_RZ + v] / pHp : 0.0;
    }
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.R) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const long o = (long)q * P.Rp + t;
            gdx[o] += al[q] * Gp[o];
            dz[o] += al[q] * Wp[o];
        }
    }
    if (blockIdx.x != 0) return;
    double m = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double rr2 = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) {
            const long o = (long)v * P.LDV + j;
            dx[o] += al[v] * p[o];
            const double rr = r[o] - al[v] * Hp[o];
            r[o] = rr;
            rr2 += rr * rr;
        }
        m = fmax(m, sqrt(block_sum(rr2, sh)));
        if (threadIdx.x == 0) Sc[S_CG_ALPHA + v] = al[v];
    }
    if (threadIdx.x == 0) Sc[slot] = m;
}
// dots needed for dtau: c'x1, c'x2 (N space) ; h'z1, h'z2, ||W z1||^2 (R space)
// ADD (the corrector's tail, one-phase, programs without a big cone: one launch less): k_corr_add comes first -- the candidate
// xk = x2c + xk, zk = z2c + zk, gk = g2c + gk is formed in place, every thread its own LP row or its cone's three rows (these are all
// the rows there are without a big cone), the N-space vector by a grid-stride loop -- and the sums take the new zk as z2
template <bool ADD>
__global__ __launch_bounds__(256) void k_dots_r(DProg P, const double* __restrict__ wl, const double* __restrict__ w3,
                                                const double* __restrict__ z1, const double* __restrict__ z2,
                                                double* __restrict__ part, const double* __restrict__ x2c,
                                                const double* __restrict__ z2c, const double* __restrict__ g2c,
                                                double* __restrict__ xk, double* __restrict__ zk, double* __restrict__ gk) {
    LANES(P, wl, w3, z1, z2, part, x2c, z2c, g2c, xk, zk, gk);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    double v[3] = {0, 0, 0};
    if (ADD) for (int j = t; j < P.N; j += gridDim.x * blockDim.x) xk[j] = x2c[j] + xk[j];
    if (t < P.l) {
        double zt;
        if (ADD) { zt = z2c[t] + zk[t]; zk[t] = zt; gk[t] = g2c[t] + gk[t]; } else zt = z2[t];
        v[0] = P.h[t] * z1[t]; v[1] = P.h[t] * zt;
        double wz = wl[t] * z1[t];
        v[2] = wz * wz;
        if (!P.own && P.rep[t]) v[0] = v[1] = v[2] = 0.0;
    } else if (t < P.l + P.nq3) {
        int c = t - P.l, r = P.l + 3 * c;
        Soc3 W = load_w3(w3, c);
        double zz[3] = {z1[r], z1[r + 1], z1[r + 2]}, wz[3], zt[3];
        for (int a = 0; a < 3; ++a) {
            if (ADD) { zt[a] = z2c[r + a] + zk[r + a]; zk[r + a] = zt[a]; gk[r + a] = g2c[r + a] + gk[r + a]; } else zt[a] = z2[r + a];
        }
        soc3_apply(W, zz, wz, false);
        for (int a = 0; a < 3; ++a) { v[0] += P.h[r + a] * z1[r + a]; v[1] += P.h[r + a] * zt[a]; v[2] += wz[a] * wz[a]; }
        if (!P.own && P.rep[r]) v[0] = v[1] = v[2] = 0.0;
    }
    // (programs with the big cone: its partial row comes FIRST, the block partials behind it -- positions that do not move with the
    //  number of blocks, so a lane of a heterogeneous unit folds exactly what its single solve folds)
    block_partials<3>(v, part + (P.big ? 3 : 0), false);
}
// big-cone contribution to the same three sums (written as one extra partial row)
__global__ __launch_bounds__(1024) void k_big_dots(DProg P, const double* __restrict__ wbb, const double* __restrict__ Sc,
                                                   const double* __restrict__ z1, const double* __restrict__ z2,
                                                   double* __restrict__ scratch, double* __restrict__ part_row) {
    LANES(P, wbb, Sc, z1, z2, scratch, part_row);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;
    double a = big_dot(P.h + ob, z1 + ob, P.big, sh);
    double b = big_dot(P.h + ob, z2 + ob, P.big, sh);
    big_apply(P.big, wbb, Sc[S_ETAB], z1 + ob, scratch, false, sh);
    double c = big_dot(scratch, scratch, P.big, sh);
    if (threadIdx.x == 0) { const double wo = P.own ? 1.0 : 0.0; part_row[0] = wo * a; part_row[1] = wo * b; part_row[2] = wo * c; }   // (the big cone is replicated)
}

// dtau for the affine (mode 0) or the combined (mode 1) direction.  One workgroup: the N-space dots
// c'x1, c'x2 are formed here, the R-space sums come as block partials.
__global__ __launch_bounds__(1024) void k_scal_dtau(DProg P, double* __restrict__ Sc, const double* __restrict__ x1,
                                                    const double* __restrict__ x2, const double* __restrict__ partR,
                                                    int nbR, int mode, double* __restrict__ RB, int phase) {
    LANES(P, Sc, x1, x2, partR, RB);
    __shared__ double sh[17];
    double hz1, hz2, wz1;
    if (phase != 1) {
        hz1 = fold_partials(partR, nbR, 3, 0, false, sh);
        hz2 = fold_partials(partR, nbR, 3, 1, false, sh);
        wz1 = fold_partials(partR, nbR, 3, 2, false, sh);
        if (phase == 0) {
            if (threadIdx.x == 0) { RB[0] = hz1; RB[1] = hz2; RB[2] = wz1; }
            return;
        }
    } else {
        hz1 = RB[0]; hz2 = RB[1]; wz1 = RB[2];
    }
    double a1 = 0, a2 = 0;
    for (int j = threadIdx.x; j < P.N; j += blockDim.x) { a1 += P.c[j] * x1[j]; a2 += P.c[j] * x2[j]; }
    double cx1 = block_sum(a1, sh);
    double cx2 = block_sum(a2, sh);
    if (threadIdx.x == 0) {
        double tau = Sc[S_TAU], kap = Sc[S_KAPPA];
        double den = kap / tau + wz1;
        (void)cx1; (void)hz1;
        if (mode == 0) {
            double dkc = -kap * tau, bt = -Sc[S_RT];
            Sc[S_DTAU_A] = (dkc / tau - bt + cx2 + hz2) / den;
            Sc[S_DKAP_A] = (dkc - kap * Sc[S_DTAU_A]) / tau;
        } else {                                          // (mode 3: the corrected direction -- same system, its own slots)
            double sigma = Sc[S_SIGMA];
            double dkc = sigma * Sc[S_MU] - kap * tau - Sc[S_DKAP_A] * Sc[S_DTAU_A];
            double bt = -(1 - sigma) * Sc[S_RT];
            const double dt = (dkc / tau - bt + cx2 + hz2) / den;
            Sc[mode == 3 ? S_DTAU_C : S_DTAU] = dt;
            Sc[mode == 3 ? S_DKAP_C : S_DKAP] = (dkc - kap * dt) / tau;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Direction in the scaled space (affine: mode 0, combined: mode 1).
//   dz = z2 + dtau z1
//   ds = -(1-sigma) rz - G x2 - dtau (G x1 - h)      (primal equation, so the primal residual
//                                                      contracts by exactly 1 - alpha (1-sigma))
//   wdz = W dz ; dss = W^-1 ds
// mode 0 stores dssa, wdza (Mehrotra corrector); mode 1 stores ds, dz.  Emits the step maxima.
__global__ __launch_bounds__(256) void k_dir_post(DProg P, const double* __restrict__ wl, const double* __restrict__ w3,
                                                  const double* __restrict__ lam, const double* __restrict__ z1,
                                                  const double* __restrict__ z2, const double* __restrict__ g1,
                                                  const double* __restrict__ g2, const double* __restrict__ rz,
                                                  double* __restrict__ Sc, double* __restrict__ outA,
                                                  double* __restrict__ outB, double* __restrict__ part, int mode,
                                                  const double* __restrict__ dpart, int ndp, const double* __restrict__ x2) {
    LANES(P, wl, w3, lam, z1, z2, g1, g2, rz, Sc, outA, outB, part, dpart, x2);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    double dtau;
    if (dpart) {
        // fused k_scal_dtau (unsharded solves): every block folds the k_dots_r partials and the N-space dot
        // c'x2 itself, block 0 publishes dtau / dkappa
        __shared__ double sh[17];
        const double hz2 = fold_partials(dpart, ndp, 3, 1, false, sh);
        const double wz1 = fold_partials(dpart, ndp, 3, 2, false, sh);
        double a2 = 0;
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) a2 += P.c[j] * x2[j];
        const double cx2 = block_sum(a2, sh);
        const double tau = Sc[S_TAU], kap = Sc[S_KAPPA], den = kap / tau + wz1;
        double dkc, bt;
        if (mode == 0) { dkc = -kap * tau; bt = -Sc[S_RT]; }
        else {
            const double sigma = Sc[S_SIGMA];
            dkc = sigma * Sc[S_MU] - kap * tau - Sc[S_DKAP_A] * Sc[S_DTAU_A];
            bt = -(1 - sigma) * Sc[S_RT];
        }
        dtau = (dkc / tau - bt + cx2 + hz2) / den;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const double dkap = (dkc - kap * dtau) / tau;
            Sc[mode == 0 ? S_DTAU_A : mode == 3 ? S_DTAU_C : S_DTAU] = dtau;
            Sc[mode == 0 ? S_DKAP_A : mode == 3 ? S_DKAP_C : S_DKAP] = dkap;
            if (mode == 1) { Sc[S_TAU0] = tau; Sc[S_KAP0] = kap; Sc[S_DTAU0] = dtau; Sc[S_DKAP0] = dkap; }
        }
    } else {
        dtau = mode == 0 ? Sc[S_DTAU_A] : mode == 3 ? Sc[S_DTAU_C] : Sc[S_DTAU];
    }
    const double oms = mode == 0 ? 1.0 : 1.0 - Sc[S_SIGMA];
    double v[2] = {-1e300, -1e300};
    if (t < P.l) {
        double dz = z2[t] + dtau * z1[t], l = lam[t];
        double ds = -oms * rz[t] - g2[t] - dtau * (g1[t] - P.h[t]);
        double wdz = wl[t] * dz, dss = ds / wl[t];
        if (mode == 0) { outA[t] = dss; outB[t] = wdz; } else { outA[t] = ds; outB[t] = dz; }
        v[0] = -dss / l; v[1] = -wdz / l;
    } else if (t < P.l + P.nq3) {
        int c = t - P.l, r = P.l + 3 * c;
        Soc3 W = load_w3(w3, c);
        double dz[3], ds[3], wdz[3], dss[3], ll[3];
        for (int a = 0; a < 3; ++a) {
            dz[a] = z2[r + a] + dtau * z1[r + a];
            ds[a] = -oms * rz[r + a] - g2[r + a] - dtau * (g1[r + a] - P.h[r + a]);
            ll[a] = lam[r + a];
        }
        soc3_apply(W, dz, wdz, false);
        soc3_apply(W, ds, dss, true);
        for (int a = 0; a < 3; ++a) {
            if (mode == 0) { outA[r + a] = dss[a]; outB[r + a] = wdz[a]; } else { outA[r + a] = ds[a]; outB[r + a] = dz[a]; }
        }
        v[0] = soc3_step(ll, dss); v[1] = soc3_step(ll, wdz);
    }
    block_partials<2>(v, part + (P.big ? 2 : 0), true);
}
__global__ __launch_bounds__(1024) void k_big_dir_post(DProg P, const double* __restrict__ wbb, const double* __restrict__ lam,
                                                       const double* __restrict__ z1, const double* __restrict__ z2,
                                                       const double* __restrict__ g1, const double* __restrict__ g2,
                                                       const double* __restrict__ rz, const double* __restrict__ Sc,
                                                       double* __restrict__ outA, double* __restrict__ outB,
                                                       double* __restrict__ scratch, double* __restrict__ part_row, int mode) {
    LANES(P, wbb, lam, z1, z2, g1, g2, rz, Sc, outA, outB, scratch, part_row);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;
    const double dtau = mode == 0 ? Sc[S_DTAU_A] : mode == 3 ? Sc[S_DTAU_C] : Sc[S_DTAU];
    const double oms = mode == 0 ? 1.0 : 1.0 - Sc[S_SIGMA];
    double* dzv = scratch;                 // big
    double* dsv = scratch + P.big;         // big
    double* wdz = scratch + 2 * P.big;     // big
    double* dss = scratch + 3 * P.big;     // big
    for (int i = threadIdx.x; i < P.big; i += blockDim.x) {
        dzv[i] = z2[ob + i] + dtau * z1[ob + i];
        dsv[i] = -oms * rz[ob + i] - g2[ob + i] - dtau * (g1[ob + i] - P.h[ob + i]);
    }
    __syncthreads();
    big_apply(P.big, wbb, Sc[S_ETAB], dzv, wdz, false, sh);
    big_apply(P.big, wbb, Sc[S_ETAB], dsv, dss, true, sh);
    for (int i = threadIdx.x; i < P.big; i += blockDim.x) {
        if (mode == 0) { outA[ob + i] = dss[i]; outB[ob + i] = wdz[i]; } else { outA[ob + i] = dsv[i]; outB[ob + i] = dzv[i]; }
    }
    __syncthreads();
    double a = big_step(P.big, lam + ob, dss, sh);
    double b = big_step(P.big, lam + ob, wdz, sh);
    if (threadIdx.x == 0) { part_row[0] = a; part_row[1] = b; }
}
// step length + sigma (mode 0, affine) or final alpha and tau/kappa update (mode 1)
__global__ __launch_bounds__(1024) void k_scal_step(DProg P, double* __restrict__ Sc, const double* __restrict__ part, int nb,
                                                    int mode, const double* __restrict__ rx, double* __restrict__ bxc,
                                                    double* __restrict__ RB, int phase) {
    LANES(P, Sc, part, rx, bxc, RB);
    __shared__ double sh[17];
    double ts, tz;
    if (phase != 1) {
        ts = fold_partials(part, nb, 2, 0, true, sh);
        tz = fold_partials(part, nb, 2, 1, true, sh);
        if (phase == 0) {
            if (threadIdx.x == 0) { RB[0] = ts; RB[1] = tz; }
            return;
        }
    } else {
        ts = RB[0]; tz = RB[1];
    }
    if (threadIdx.x == 0) {
        double tau = Sc[S_TAU], kap = Sc[S_KAPPA];
        double dtau = mode == 0 ? Sc[S_DTAU_A] : mode >= 3 ? Sc[S_DTAU_C] : Sc[S_DTAU];
        double dkap = mode == 0 ? Sc[S_DKAP_A] : mode >= 3 ? Sc[S_DKAP_C] : Sc[S_DKAP];
        double t = fmax(0.0, fmax(fmax(ts, tz), fmax(-dtau / tau, -dkap / kap)));
        Sc[S_TMAX] = t;
        if (mode == 0) {
            double a = t == 0.0 ? 1.0 : fmin(1.0, 1.0 / t);
            Sc[S_ALPHA_A] = a;
            Sc[S_SIGMA] = fmin((1 - a) * (1 - a) * (1 - a), Sc[S_SIGMAX]);
            sh[16] = Sc[S_SIGMA];
        } else if (mode == 2) {                           // the uncorrected direction's step, kept for the corrector: nothing moves yet
            Sc[S_ALPHA0] = t == 0.0 ? 1.0 : fmin(1.0, STEP / t);
        } else {
            double a = t == 0.0 ? 1.0 : fmin(1.0, STEP / t);
            if (mode >= 3) {                              // corrected against uncorrected direction (oracle/conic_ipm.py CORR_ACCEPT; mode 4, the form
                                                          // without the residual guard, is no longer passed by the host: its term stays for the NOTE below)
                // (its solve ran without refinement sweeps; what it leaves of the dual equation, ||G'dzk|| in S_RNC, must not exceed
                //  CORR_ETA times the iterate's own ||rx|| = dres tau ||c|| -- or the absolute floor of the refinement)
                const double a0 = Sc[S_ALPHA0];
                const double tolk = fmax(REFTOL * Sc[S_NRMC], CORR_ETA * Sc[S_DRES] * tau * Sc[S_NRMC]);
                // NOTE (ROCm 7.2 / gfx950): written as `a >= ... && Sc[S_RNC] <= tolk` alone, this select was MISCOMPILED -- the backend emitted
                // v_cmp_le_f64 vcc, ... ; s_cselect_b32 s12, 0x3ff00000, 0 with no SCC definition in between (s_cselect reads SCC, v_cmp
                // writes VCC), so S_PICK held a stale condition while S_ALPHA / S_NPICK followed the real one: the update then took the
                // corrected direction's step along the uncorrected direction.  tools/scan_scc.py finds that shape in the generated
                // assembly; tests/test_host_cpu.py runs it over every device source of the package.
                const bool pick = a >= CORR_ACCEPT * a0 && (mode == 4 || Sc[S_RNC] <= tolk);
                Sc[S_PICK] = pick ? 1.0 : 0.0;
                Sc[S_NCORR] += 1.0;
                if (pick) { Sc[S_DTAU] = dtau; Sc[S_DKAP] = dkap; Sc[S_NPICK] += 1.0; }
                else { a = a0; dtau = Sc[S_DTAU]; dkap = Sc[S_DKAP]; }
            }
            Sc[S_ALPHA] = a;
            Sc[S_TAU] = tau + a * dtau;
            Sc[S_KAPPA] = kap + a * dkap;
        }
    }
    if (mode == 0) {                                     // bx of the combined system: -(1 - sigma) rx
        __syncthreads();
        const double oms = 1.0 - sh[16];
        for (int j = threadIdx.x; j < P.N; j += blockDim.x) bxc[j] = -oms * rx[j];
    }
}

// combined right-hand side: ds_c = sigma mu e - lam o lam - dssa o wdza ; lds = lam \ ds_c ;
// bz = -(1-sigma) rz - W lds ;  (bx = -(1-sigma) rx is formed by k_scal_step)
// spart != null (unsharded solves): the affine step length and sigma (k_scal_step, mode 0) are formed here
// by every block from the k_dir_post partials, block 0 publishes them and bx = -(1-sigma) rx.
// wbz != null: also wbz = W^-2 bz (saves the k_winv2 pass of the solve that follows).
__global__ __launch_bounds__(256) void k_comb_rhs(DProg P, const double* __restrict__ wl, const double* __restrict__ w3,
                           const double* __restrict__ lam, const double* __restrict__ dssa,
                           const double* __restrict__ wdza, const double* __restrict__ rz,
                           double* __restrict__ Sc, double* __restrict__ lds, double* __restrict__ bz,
                           const double* __restrict__ spart, int nsp, const double* __restrict__ rx,
                           double* __restrict__ bxc, const double* __restrict__ dl, double* __restrict__ wbz) {
    LANES(P, wl, w3, lam, dssa, wdza, rz, Sc, lds, bz, spart, rx, bxc, dl, wbz);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    double sigma;
    if (spart) {
        __shared__ double sh[2][17];
        double tm[2];
        fold_partials_k<2>(spart, nsp, 2, 0, true, tm, sh);      // (both maxima in one pass and one barrier sequence)
        const double tau = Sc[S_TAU], kap = Sc[S_KAPPA];
        const double tt = step_bound(tm[0], tm[1], tau, kap, Sc[S_DTAU_A], Sc[S_DKAP_A]);
        const double a = tt == 0.0 ? 1.0 : fmin(1.0, 1.0 / tt);
        sigma = fmin((1 - a) * (1 - a) * (1 - a), Sc[S_SIGMAX]);
        if (blockIdx.x == 0) {
            if (threadIdx.x == 0) { Sc[S_TMAX] = tt; Sc[S_ALPHA_A] = a; Sc[S_SIGMA] = sigma; }
            for (int j = threadIdx.x; j < P.N; j += blockDim.x) bxc[j] = -(1.0 - sigma) * rx[j];
        }
    } else {
        sigma = Sc[S_SIGMA];
    }
    const double smu = sigma * Sc[S_MU];
    if (t < P.l) {
        double l = lam[t];
        double dsc = smu - l * l - dssa[t] * wdza[t];
        double q = dsc / l;
        lds[t] = q;
        const double b = -(1 - sigma) * rz[t] - wl[t] * q;
        bz[t] = b;
        if (wbz) wbz[t] = dl[t] * b;
    } else if (t < P.l + P.nq3) {
        int c = t - P.l, r = P.l + 3 * c;
        Soc3 W = load_w3(w3, c);
        double ll[3] = {lam[r], lam[r + 1], lam[r + 2]}, a3[3] = {dssa[r], dssa[r + 1], dssa[r + 2]},
               b3[3] = {wdza[r], wdza[r + 1], wdza[r + 2]}, p1[3], p2[3], dsc[3], q[3], wq[3];
        soc3_prod(ll, ll, p1);
        soc3_prod(a3, b3, p2);
        dsc[0] = smu - p1[0] - p2[0]; dsc[1] = -p1[1] - p2[1]; dsc[2] = -p1[2] - p2[2];
        soc3_div(ll, dsc, q);
        soc3_apply(W, q, wq, false);
        double bb[3], wb[3];
        for (int a = 0; a < 3; ++a) { lds[r + a] = q[a]; bb[a] = -(1 - sigma) * rz[r + a] - wq[a]; bz[r + a] = bb[a]; }
        if (wbz) {
            soc3_inv2_apply(W, bb, wb);
            for (int a = 0; a < 3; ++a) wbz[r + a] = wb[a];
        }
    }
}
__global__ __launch_bounds__(1024) void k_big_comb_rhs(DProg P, const double* __restrict__ wbb, const double* __restrict__ lam,
                                                       const double* __restrict__ dssa, const double* __restrict__ wdza,
                                                       const double* __restrict__ rz, const double* __restrict__ Sc,
                                                       double* __restrict__ lds, double* __restrict__ bz,
                                                       double* __restrict__ scratch) {
    LANES(P, wbb, lam, dssa, wdza, rz, Sc, lds, bz, scratch);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;
    const int n1 = P.big - 1;
    const double sigma = Sc[S_SIGMA], smu = sigma * Sc[S_MU];
    const double* L = lam + ob;
    const double* A = dssa + ob;
    const double* B = wdza + ob;
    double ll = big_dot(L, L, P.big, sh), ab = big_dot(A, B, P.big, sh);
    double l0 = L[0], a0 = A[0], b0 = B[0];
    // dsc = sigma mu e - lam o lam - dssa o wdza  -> scratch
    for (int i = threadIdx.x; i < n1; i += blockDim.x)
        scratch[1 + i] = -(2 * l0 * L[1 + i]) - (a0 * B[1 + i] + b0 * A[1 + i]);
    if (threadIdx.x == 0) scratch[0] = smu - ll - ab;
    __syncthreads();
    // q = lam \ dsc  -> lds
    double nl = sqrt(big_dot(L + 1, L + 1, n1, sh));
    double a = jres(l0, nl);
    double ld = big_dot(L + 1, scratch + 1, n1, sh);
    double q0 = (l0 * scratch[0] - ld) / a;
    for (int i = threadIdx.x; i < n1; i += blockDim.x) lds[ob + 1 + i] = (scratch[1 + i] - q0 * L[1 + i]) / l0;
    if (threadIdx.x == 0) lds[ob] = q0;
    __syncthreads();
    // bz = -(1-sigma) rz - W q
    big_apply(P.big, wbb, Sc[S_ETAB], lds + ob, scratch, false, sh);
    for (int i = threadIdx.x; i < P.big; i += blockDim.x) bz[ob + i] = -(1 - sigma) * rz[ob + i] - scratch[i];
}
// x += alpha (x2 + dtau x1) ; s += alpha ds ; z += alpha dz
// part != null (round 5: one launch less): the step length is formed HERE -- k_scal_step's fold of the k_dir_post partials and its
// scalar arithmetic (mode 1), by every block for itself; block 0 publishes alpha and the new tau, kappa (the blocks read the old
// ones from the snapshot k_dir_post left: S_TAU0, S_KAP0)
__global__ __launch_bounds__(256) void k_update(DProg P, double* __restrict__ Sc, const double* __restrict__ x1,
                         const double* __restrict__ x2, double* __restrict__ x, const double* __restrict__ ds,
                         const double* __restrict__ dz, double* __restrict__ s, double* __restrict__ z,
                         const double* __restrict__ part, int nb) {
    LANES(P, Sc, x1, x2, x, ds, dz, s, z, part);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (part) {
        __shared__ double sh[17];
        const double ts = fold_partials(part, nb, 2, 0, true, sh), tz = fold_partials(part, nb, 2, 1, true, sh);
        const double tau = Sc[S_TAU0], kap = Sc[S_KAP0], dtau = Sc[S_DTAU], dkap = Sc[S_DKAP];
        const double tm = fmax(0.0, fmax(fmax(ts, tz), fmax(-dtau / tau, -dkap / kap)));
        const double a = tm == 0.0 ? 1.0 : fmin(1.0, STEP / tm);
        if (blockIdx.x == 0 && threadIdx.x == 0) { Sc[S_TMAX] = tm; Sc[S_ALPHA] = a; Sc[S_TAU] = tau + a * dtau; Sc[S_KAPPA] = kap + a * dkap; }
        if (t < P.N) x[t] += a * (x2[t] + dtau * x1[t]);
        if (t < P.R) { s[t] += a * ds[t]; z[t] += a * dz[t]; }
        return;
    }
    const double a = Sc[S_ALPHA], dtau = Sc[S_DTAU];
    if (t < P.N) x[t] += a * (x2[t] + dtau * x1[t]);
    if (t < P.R) { s[t] += a * ds[t]; z[t] += a * dz[t]; }
}
// the same after a centrality corrector: k_scal_step (mode 3) has chosen between the two directions (S_PICK), set alpha, dtau
// and moved tau, kappa
// part != null (one-phase, sw.fuse: one launch less): the pick and the step are formed HERE -- k_scal_step's fold of the corrected
// direction's maxima and its scalar arithmetic (mode 3), by every block for itself; block 0 publishes what mode 3 publishes.  What block 0
// overwrites the blocks read from the snapshots k_dir_post (mode 1) left: tau, kappa in S_TAU0 / S_KAP0, the uncorrected dtau, dkappa in
// S_DTAU0 / S_DKAP0 (nothing has moved tau or kappa since).  The pick is ONE value, pickd, behind a barrier the optimiser cannot see
// through: the step, dtau, the direction moved along and the stored S_PICK / S_NPICK all come from it and cannot disagree (see the NOTE
// at k_scal_step)
__global__ __launch_bounds__(256) void k_update_pick(DProg P, double* __restrict__ Sc, const double* __restrict__ x1,
                         const double* __restrict__ x2, const double* __restrict__ x2k, double* __restrict__ x,
                         const double* __restrict__ ds, const double* __restrict__ dz, const double* __restrict__ dsk,
                         const double* __restrict__ dzk, double* __restrict__ s, double* __restrict__ z,
                         const double* __restrict__ part, int nb) {
    LANES(P, Sc, x1, x2, x2k, x, ds, dz, dsk, dzk, s, z, part);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (part) {
        __shared__ double sh[2][17];
        double tm[2];
        fold_partials_k<2>(part, nb, 2, 0, true, tm, sh);
        const double tau = Sc[S_TAU0], kap = Sc[S_KAP0], dtauc = Sc[S_DTAU_C], dkapc = Sc[S_DKAP_C];
        const double tt = step_bound(tm[0], tm[1], tau, kap, dtauc, dkapc);
        const double ac = tt == 0.0 ? 1.0 : fmin(1.0, STEP / tt);
        const double a0 = Sc[S_ALPHA0];
        const double tolk = fmax(REFTOL * Sc[S_NRMC], CORR_ETA * Sc[S_DRES] * tau * Sc[S_NRMC]);
        double pickd = (ac >= CORR_ACCEPT * a0 && Sc[S_RNC] <= tolk) ? 1.0 : 0.0;
        asm volatile("" : "+v"(pickd));
        const bool pick = pickd != 0.0;
        const double a = pick ? ac : a0, dtau = pick ? dtauc : Sc[S_DTAU0], dkap = pick ? dkapc : Sc[S_DKAP0];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            Sc[S_TMAX] = tt; Sc[S_PICK] = pickd; Sc[S_NCORR] += 1.0;
            if (pick) { Sc[S_DTAU] = dtau; Sc[S_DKAP] = dkap; Sc[S_NPICK] += pickd; }
            Sc[S_ALPHA] = a; Sc[S_TAU] = tau + a * dtau; Sc[S_KAPPA] = kap + a * dkap;
        }
        if (t < P.N) x[t] += a * ((pick ? x2k[t] : x2[t]) + dtau * x1[t]);
        if (t < P.R) { s[t] += a * (pick ? dsk[t] : ds[t]); z[t] += a * (pick ? dzk[t] : dz[t]); }
        return;
    }
    const double a = Sc[S_ALPHA], dtau = Sc[S_DTAU];
    const bool pick = Sc[S_PICK] != 0.0;
    if (t < P.N) x[t] += a * ((pick ? x2k[t] : x2[t]) + dtau * x1[t]);
    if (t < P.R) { s[t] += a * (pick ? dsk[t] : ds[t]); z[t] += a * (pick ? dzk[t] : dz[t]); }
}
// Centrality corrector, right-hand side (oracle/conic_ipm.py solve(): CORR_*).  (ds, dz) is the predictor-corrector direction,
// S_ALPHA0 its step.  On the orthant rows the products at the trial step  at = min(1, alpha0 + CORR_DELTA),
//   v = (lam + at W^-1 ds)(lam + at W dz),
// are projected onto [CORR_BMIN, CORR_BMAX] sigma mu; t = projection - v, bounded below by -CORR_BMAX sigma mu;
//   bz = -W (lam \ t),  wbz = W^-2 bz;   the 3-row cones get zeros (their products are left alone).
// The big cone (k_big_corr_rhs): the same for the two eigenvalues v0 +- ||v1|| of the Jordan product
// v = (lam + at W^-1 ds) o (lam + at W dz) (corr_target), except on the extended-precision path.
__device__ __forceinline__ void corr_target(double e1, double e2, double mut, double& d1, double& d2) {
    d1 = fmax(fmin(fmax(e1, CORR_BMIN * mut), CORR_BMAX * mut) - e1, -CORR_BMAX * mut);
    d2 = fmax(fmin(fmax(e2, CORR_BMIN * mut), CORR_BMAX * mut) - e2, -CORR_BMAX * mut);
}
__global__ __launch_bounds__(256) void k_corr_rhs(DProg P, const double* __restrict__ wl, const double* __restrict__ dl,
                                                  const double* __restrict__ lam, const double* __restrict__ ds,
                                                  const double* __restrict__ dz, double* __restrict__ Sc,
                                                  double* __restrict__ bz, double* __restrict__ wbz,
                                                  const double* __restrict__ part, int nb) {
    LANES(P, wl, dl, lam, ds, dz, Sc, bz, wbz, part);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    // part != null (one-phase, sw.fuse: one launch less): the trial step is formed HERE -- k_scal_step's fold of the k_dir_post maxima and
    // its scalar arithmetic (mode 2), by every block for itself (none of the scalars it reads is written in this kernel); block 0
    // publishes S_TMAX and S_ALPHA0, which k_big_corr_rhs reads behind this kernel
    double alpha0;
    if (part) {
        __shared__ double sh[2][17];
        double tm[2];
        fold_partials_k<2>(part, nb, 2, 0, true, tm, sh);
        const double tt = step_bound(tm[0], tm[1], Sc[S_TAU], Sc[S_KAPPA], Sc[S_DTAU], Sc[S_DKAP]);
        alpha0 = tt == 0.0 ? 1.0 : fmin(1.0, STEP / tt);
        if (blockIdx.x == 0 && threadIdx.x == 0) { Sc[S_TMAX] = tt; Sc[S_ALPHA0] = alpha0; }
    } else {
        alpha0 = Sc[S_ALPHA0];
    }
    if (t < P.l) {
        const double at = fmin(1.0, alpha0 + CORR_DELTA), mut = Sc[S_SIGMA] * Sc[S_MU];
        const double l = lam[t], w = wl[t];
        const double dss = ds[t] / w, wdz = w * dz[t];
        const double v = (l + at * dss) * (l + at * wdz);
        double tt = fmin(fmax(v, CORR_BMIN * mut), CORR_BMAX * mut) - v;
        tt = fmax(tt, -CORR_BMAX * mut);
        const double b = -w * (tt / l);
        bz[t] = b; wbz[t] = dl[t] * b;
    } else if (t < P.l + P.nq3) {
        const int r = P.l + 3 * (t - P.l);
        for (int a = 0; a < 3; ++a) { bz[r + a] = 0.0; wbz[r + a] = 0.0; }
    }
}
// ... the big cone's rows (one workgroup; W^-2 bz of these rows is formed by k_big_winv2 in the solve that follows)
__global__ __launch_bounds__(1024) void k_big_corr_rhs(DProg P, const double* __restrict__ wbb, const double* __restrict__ lam,
                                                       const double* __restrict__ ds, const double* __restrict__ dz,
                                                       const double* __restrict__ Sc, double* __restrict__ bz,
                                                       double* __restrict__ scratch, int on, const int* __restrict__ dd_mask) {
    LANES(P, wbb, lam, ds, dz, Sc, bz, scratch);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;
    const int big = P.big, n1 = big - 1;
    if (!on || (dd_mask && dd_mask[blockIdx.z])) {       // extended-precision path: the cone is left alone
        for (int i = threadIdx.x; i < big; i += blockDim.x) bz[ob + i] = 0.0;
        return;
    }
    const double at = fmin(1.0, Sc[S_ALPHA0] + CORR_DELTA), mut = Sc[S_SIGMA] * Sc[S_MU];
    const double* L = lam + ob;
    double* u = scratch;                   // lam + at W^-1 ds
    double* w = scratch + big;             // lam + at W dz
    double* v = scratch + 2 * big;         // their Jordan product, then the target t, then W (lam \ t)
    double* q = scratch + 3 * big;         // lam \ t
    big_apply(big, wbb, Sc[S_ETAB], ds + ob, u, true, sh);
    big_apply(big, wbb, Sc[S_ETAB], dz + ob, w, false, sh);
    for (int i = threadIdx.x; i < big; i += blockDim.x) { u[i] = L[i] + at * u[i]; w[i] = L[i] + at * w[i]; }
    __syncthreads();
    const double v0 = big_dot(u, w, big, sh), u0 = u[0], w0 = w[0];
    for (int i = threadIdx.x; i < n1; i += blockDim.x) v[1 + i] = u0 * w[1 + i] + w0 * u[1 + i];
    __syncthreads();
    const double nv = sqrt(big_dot(v + 1, v + 1, n1, sh));
    double d1, d2;
    corr_target(v0 + nv, v0 - nv, mut, d1, d2);
    const double f = 0.5 * (d1 - d2) / (nv > 0 ? nv : 1.0), t0 = 0.5 * (d1 + d2);
    for (int i = threadIdx.x; i < n1; i += blockDim.x) v[1 + i] *= f;
    __syncthreads();
    // q = lam \ t
    const double l0 = L[0], nl = sqrt(big_dot(L + 1, L + 1, n1, sh)), a = jres(l0, nl), ld = big_dot(L + 1, v + 1, n1, sh);
    const double q0 = (l0 * t0 - ld) / a;
    for (int i = threadIdx.x; i < n1; i += blockDim.x) q[1 + i] = (v[1 + i] - q0 * L[1 + i]) / l0;
    if (threadIdx.x == 0) q[0] = q0;
    __syncthreads();
    big_apply(big, wbb, Sc[S_ETAB], q, v, false, sh);
    for (int i = threadIdx.x; i < big; i += blockDim.x) bz[ob + i] = -v[i];
}
// candidate = predictor-corrector solution + corrector solution, in place in the corrector's arrays
__global__ __launch_bounds__(256) void k_corr_add(DProg P, const double* __restrict__ x2, const double* __restrict__ z2,
                                                  const double* __restrict__ g2, double* __restrict__ xk, double* __restrict__ zk,
                                                  double* __restrict__ gk) {
    LANES(P, x2, z2, g2, xk, zk, gk);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.N) xk[t] = x2[t] + xk[t];
    if (t < P.R) { zk[t] = z2[t] + zk[t]; gk[t] = g2[t] + gk[t]; }
}

// ------------------------------------------------------------------------------------------------
// H assembly
// per-frequency 2x2 weight block [D11 D12; D12 D22] and border vectors B1[e], B2[e]
// m3c != null: the (capped, eigen-form) 3x3 blocks of the extended-precision solve replace soc3_inv2(w3)
__device__ __forceinline__ void load_m3(const double* __restrict__ w3, const double* __restrict__ m3c, int c, double m[6]) {
    if (m3c) { for (int q = 0; q < 6; ++q) m[q] = m3c[6L * c + q]; }
    else soc3_inv2(load_w3(w3, c), m);
}
// per-frequency blocks of the normal matrix: v[0] = d11, (quad: v[1] = d12, v[2] = d22), then the border values
// b1[e] (quad: then b2[e]) -- the order of the Dw | BB arrays
__device__ __forceinline__ void freq_block_at(const DProg& P, const double* __restrict__ dl, const double* __restrict__ w3,
                                              const double* __restrict__ m3c, int i, double (&v)[9]) {
    double d11 = 0, d12 = 0, d22 = 0, b1[3] = {0, 0, 0}, b2[3] = {0, 0, 0};
    if (i >= 0)
    for (int q = P.f_ptr[i]; q < P.f_ptr[i + 1]; ++q) {
        int r = P.f_rows[q];
        if (r < P.l) {
            double d = dl[r], al = P.alpha[r], be = P.beta[r];
            d11 += d * al * al; d12 += d * al * be; d22 += d * be * be;
            for (int e = 0; e < P.Ne; ++e) { b1[e] += d * al * P.ey[3 * r + e]; b2[e] += d * be * P.ey[3 * r + e]; }
        } else {
            int c = (r - P.l) / 3, a = (r - P.l) - 3 * c;
            if (a != 1) continue;                       // a cone is handled once, at its first trig row
            int r0 = P.l + 3 * c;
            double m[6];
            load_m3(w3, m3c, c, m);
            double al[3] = {0, P.alpha[r0 + 1], P.alpha[r0 + 2]}, be[3] = {0, P.beta[r0 + 1], P.beta[r0 + 2]};
            for (int p = 1; p < 3; ++p)
                for (int s = 1; s < 3; ++s) {
                    double mm = sym3(m, p, s);
                    d11 += mm * al[p] * al[s]; d12 += mm * al[p] * be[s]; d22 += mm * be[p] * be[s];
                }
            for (int e = 0; e < P.Ne; ++e) {
                for (int p = 1; p < 3; ++p) {
                    double t = 0;
                    for (int s = 0; s < 3; ++s) t += sym3(m, p, s) * P.ey[3 * (r0 + s) + e];
                    b1[e] += al[p] * t; b2[e] += be[p] * t;
                }
            }
        }
    }
    int o = 0;
    v[o++] = d11;
    if (P.quad) { v[o++] = d12; v[o++] = d22; }
    for (int e = 0; e < P.Ne; ++e) v[o++] = b1[e];
    if (P.quad) for (int e = 0; e < P.Ne; ++e) v[o++] = b2[e];
}
__global__ void k_freq_blocks(DProg P, const double* __restrict__ dl, const double* __restrict__ w3,
                              double* __restrict__ Dw, double* __restrict__ BB, const double* __restrict__ m3c) {
    LANES(P, dl, w3, Dw, BB, m3c);
    if (P.plain_weights()) { dl = P.dl_plain; m3c = nullptr; }
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.Mf) return;
    double v[9];
    freq_block_at(P, dl, w3, m3c, i, v);
    int o = 0;
    Dw[i] = v[o++];
    if (P.quad) { Dw[P.Mpad + i] = v[o++]; Dw[2L * P.Mpad + i] = v[o++]; }
    for (int e = 0; e < P.Ne; ++e) BB[(long)e * P.Mpad + i] = v[o++];
    if (P.quad) for (int e = 0; e < P.Ne; ++e) BB[(long)(P.Ne + e) * P.Mpad + i] = v[o++];
}
// the same for the lattice path, straight into the folded operands of the moment kernel: one thread per folded
// frequency, (pe, po) of the nv = nwv + nvb vectors (k_freq_blocks + k_freq_fold in one launch)
__global__ __launch_bounds__(256) void k_freq_blocks_fold(DProg P, const double* __restrict__ dl, const double* __restrict__ w3,
                                                          const double* __restrict__ m3c, int nv, double2* __restrict__ out) {
    LANES(P, dl, w3, m3c, out);
    if (P.plain_weights()) { dl = P.dl_plain; m3c = nullptr; }
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.nfold) return;
    double a[9], b[9];
    freq_block_at(P, dl, w3, m3c, P.fold_pos[k], a);
    freq_block_at(P, dl, w3, m3c, P.fold_neg[k], b);
    for (int v = 0; v < nv; ++v) out[(long)v * P.Mpad + k] = make_double2(a[v] + b[v], a[v] - b[v]);
}

// H (np x np) from the Gram matrices and the border products.  TT[v][j] = (A1' BB[v])[j].
__global__ void k_assemble_H(DProg P, const double* __restrict__ T, const double* __restrict__ TT,
                             double* __restrict__ H, double pad_diag) {
    LANES(P, T, TT, H);
    int k = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (k >= P.np || j >= P.np) return;
    double v = 0;
    const long ld = P.ld, ld2 = ld * ld;
    if (j < P.Nt && k < P.Nt) {
        v = T[j * ld + k];
        if (P.quad) {
            int pj = P.pcol[j], pk = P.pcol[k];
            double sj = P.psign[j], sk = P.psign[k];
            v += sj * sk * T[2 * ld2 + pj * ld + pk] + sk * T[ld2 + j * ld + pk] + sj * T[ld2 + pj * ld + k];
        }
    } else if (j < P.N && k < P.N) {
        int jj = j < k ? j : k, kk = j < k ? k : j;       // jj < Nt <= kk  or both >= Nt
        if (jj < P.Nt) {
            int e = kk - P.Nt;
            v = TT[(long)e * P.LDV + jj];
            if (P.quad) v += P.psign[jj] * TT[(long)(P.Ne + e) * P.LDV + P.pcol[jj]];
        }
    } else if (j == k) {
        v = pad_diag;                                     // padding (1 on one shard, 0 on the others: H is summed)
    }
    H[(long)j * P.np + k] = v;
}
// Lattice mode: the same H from the moments.  Mom[w][0|1][.] = g_w | s_w on the difference progression
// (t = 0 .. D1-1, index m) followed by the sum progression (t = 2 tmin + m', index D1 + m');
// MomB[e][0|1][m] are the border moments on the column progression t = tmin + m.
__device__ __forceinline__ double lat_T(const DProg& P, const double* __restrict__ Mw, int j, int k) {
    const int mj = P.lat[j], mk = P.lat[k], kj = P.col_kind[j], kk = P.col_kind[k];
    const int d = mj - mk, ad = d < 0 ? -d : d, si = P.D1 + mj + mk;
    const double* G = Mw;
    const double* S = Mw + P.LDM;
    double v;
    if (kj == 0 && kk == 0) v = G[ad] + G[si];
    else if (kj == 1 && kk == 1) v = G[ad] - G[si];
    else {
        const double sdv = d < 0 ? -S[ad] : S[ad];       // s(tau_j - tau_k)
        v = kj == 0 ? S[si] - sdv : S[si] + sdv;
    }
    return 0.5 * v * P.col_scale[j] * P.col_scale[k];
}
// mode 1: slot = flag (rank 0), mode 0: slot = 0 (the others), mode 2: flag = slot after the all-reduce
__global__ void k_flag_share(int* flag, double* slot, int mode) {
    if (mode == 2) flag[0] = int(slot[0] + 0.5);
    else slot[0] = mode == 1 ? double(flag[0]) : 0.0;
}
__global__ void k_assemble_H_lat(DProg P, const double* __restrict__ Mom, const double* __restrict__ MomB,
                                 double* __restrict__ H, double pad_diag) {
    LANES(P, Mom, MomB, H);
    // grid: (lower 64 x 64 tiles, 16 row quads of a tile): the factorisations read the lower tiles only, so only those are
    // formed -- a block is 4 rows x 64 columns of one tile, every thread has work and a row segment is one 512-byte store
    int ti = int((sqrt(8.0 * blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= int(blockIdx.x)) ++ti;
    while (ti * (ti + 1) / 2 > int(blockIdx.x)) --ti;
    const int tk = int(blockIdx.x) - ti * (ti + 1) / 2;
    const int j = 64 * ti + 4 * blockIdx.y + (threadIdx.x >> 6), k = 64 * tk + (threadIdx.x & 63);
    if (k >= P.np || j >= P.np) return;
    double v = 0;
    const long mw = 2L * P.LDM;
    if (j < P.Nt && k < P.Nt) {
        v = lat_T(P, Mom, j, k);
        if (P.quad) {
            int pj = P.pcol[j], pk = P.pcol[k];
            double sj = P.psign[j], sk = P.psign[k];
            v += sj * sk * lat_T(P, Mom + 2 * mw, pj, pk) + sk * lat_T(P, Mom + mw, j, pk) + sj * lat_T(P, Mom + mw, pj, k);
        }
    } else if (j < P.N && k < P.N) {
        int jj = j < k ? j : k, kk = j < k ? k : j;       // jj < Nt <= kk  or both >= Nt
        if (jj < P.Nt) {
            int e = kk - P.Nt;
            v = P.col_scale[jj] * MomB[((long)e * 2 + P.col_kind[jj]) * P.LDM + P.lat[jj]];
            if (P.quad) {
                int pq = P.pcol[jj];
                v += P.psign[jj] * P.col_scale[pq] * MomB[((long)(P.Ne + e) * 2 + P.col_kind[pq]) * P.LDM + P.lat[pq]];
            }
        }
    } else if (j == k) {
        v = pad_diag;
    }
    H[(long)j * P.np + k] = v;
}
// identity rows: thread j owns row j of H (and the mirrored border entries)
// wsum: the result is summed over the ranks of a row-sharded solve afterwards (replicated rows then count on the owner only)
__device__ __forceinline__ void h_yy_block(const DProg& P, const double* __restrict__ dl, const double* __restrict__ w3,
                                           double* __restrict__ H, long ld, long base, const double* __restrict__ m3c, bool wsum);
// yy_too: one more block at the end of the grid adds the y-y block (k_H_yy's work; 256 threads)
__global__ __launch_bounds__(256) void k_H_identity(DProg P, const double* __restrict__ dl, const double* __restrict__ w3,
                                                    double* __restrict__ H, const double* __restrict__ m3c, int yy_too, int summed) {
    LANES(P, dl, w3, H, m3c);
    if (P.plain_weights()) { dl = P.dl_plain; m3c = nullptr; }
    // summed: the matrix is summed over the ranks afterwards (dense row-sharded path): the y-y block weights the replicated
    // rows, and the identity rows -- all of them replicated -- are added by the owner only
    if (yy_too && blockIdx.x == gridDim.x - 1) { h_yy_block(P, dl, w3, H, (long)P.np, (long)P.Nt, m3c, summed != 0); return; }
    if (summed && !P.own) return;
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P.Nt) return;
    const long np = P.np;
    for (int q = P.c_ptr[j]; q < P.c_ptr[j + 1]; ++q) {
        int r = P.c_rows[q];
        double al = P.alpha[r];
        if (r < P.l) {
            double d = dl[r];
            H[j * np + j] += d * al * al;
            for (int e = 0; e < P.Ne; ++e) {
                double t = d * al * P.ey[3 * r + e];
                H[j * np + P.Nt + e] += t;
                H[(P.Nt + e) * np + j] += t;
            }
        } else if (r < P.l + 3 * P.nq3) {
            int c = (r - P.l) / 3, a = (r - P.l) - 3 * c, r0 = P.l + 3 * c;
            double m[6];
            load_m3(w3, m3c, c, m);
            for (int b = 0; b < 3; ++b) {
                double mm = sym3(m, a, b);
                int cb = P.col[r0 + b];
                if (cb >= 0) H[j * np + cb] += al * P.alpha[r0 + b] * mm;
                for (int e = 0; e < P.Ne; ++e) {
                    double t = al * mm * P.ey[3 * (r0 + b) + e];
                    H[j * np + P.Nt + e] += t;
                    H[(P.Nt + e) * np + j] += t;
                }
            }
        }
    }
}
// y-y block: sum over rows with a non-zero ey (LP rows and Q3 cones); one block
// out[(base + e) * ld + base + f] += ... : (H, np, Nt), or a 3 x 3 scratch (ld 3, base 0) that the lead-factor mode all-reduces
__device__ __forceinline__ void h_yy_block(const DProg& P, const double* __restrict__ dl, const double* __restrict__ w3,
                                           double* __restrict__ H, long ld, long base, const double* __restrict__ m3c, bool wsum) {
    __shared__ double sh[17];
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = threadIdx.x; q < P.nyrows; q += blockDim.x) {
        int r = P.yrows[q];
        if (wsum && !P.own && P.rep[r]) continue;            // summed over the ranks afterwards: replicated rows once
        if (r < P.l) {
            double d = dl[r];
            for (int e = 0; e < P.Ne; ++e)
                for (int f = 0; f < P.Ne; ++f) acc[3 * e + f] += d * P.ey[3 * r + e] * P.ey[3 * r + f];
        } else if (r < P.l + 3 * P.nq3) {
            int c = (r - P.l) / 3, a = (r - P.l) - 3 * c, r0 = P.l + 3 * c;
            double m[6];
            load_m3(w3, m3c, c, m);
            for (int b = 0; b < 3; ++b)
                for (int e = 0; e < P.Ne; ++e)
                    for (int f = 0; f < P.Ne; ++f)
                        acc[3 * e + f] += P.ey[3 * r + e] * sym3(m, a, b) * P.ey[3 * (r0 + b) + f];
        }
    }
    for (int e = 0; e < P.Ne; ++e)
        for (int f = 0; f < P.Ne; ++f) {
            double t = block_sum(acc[3 * e + f], sh);
            if (threadIdx.x == 0) H[(base + e) * ld + base + f] += t;
        }
}
__global__ __launch_bounds__(256) void k_H_yy(DProg P, const double* __restrict__ dl, const double* __restrict__ w3,
                                              double* __restrict__ H, long ld, long base, const double* __restrict__ m3c) {
    LANES(P, dl, w3, H, m3c);
    h_yy_block(P, dl, w3, H, ld, base, m3c, true);
}
// Dense row-sharded solves: the ranks' normal matrices are summed as their PACKED LOWER TRIANGLE (the 64 x 64 tiles (i, j <= i), one
// after the other: nblk (nblk + 1) / 2 x 4096 doubles instead of np^2 -- the factorisation never reads a tile above the diagonal)
__global__ __launch_bounds__(256) void k_pack_tril(const double* __restrict__ H, int np, double* __restrict__ out, int unpack) {
    const int t = blockIdx.x;
    int ti = int((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((long)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
    while ((long)ti * (ti + 1) / 2 > t) --ti;
    const int tj = t - ti * (ti + 1) / 2;
    double* Hw = const_cast<double*>(H);
    for (int e = threadIdx.x; e < 64 * 32; e += 256) {
        const int r = e >> 5, c2 = 2 * (e & 31);
        double2* tile = reinterpret_cast<double2*>(out + (long)t * 4096 + r * 64 + c2);
        double2* mat = reinterpret_cast<double2*>(Hw + ((long)ti * 64 + r) * np + (long)tj * 64 + c2);
        if (unpack) *mat = *tile; else *tile = *mat;
    }
}
__global__ void k_zero3(double* __restrict__ a, long na, double* __restrict__ b, long nb, double* __restrict__ c, long nc, size_t lane_bytes, const int* lane_mask) {
    LANES_RAW(lane_bytes, lane_mask, a, b, c);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) a[i] = 0.0;
    if (i < nb) b[i] = 0.0;
    if (i < nc) c[i] = 0.0;
}
__global__ void k_H_yy_add(DProg P, const double* __restrict__ yy, double* __restrict__ H) {
    LANES(P, yy, H);
    const int e = threadIdx.x / 3, f = threadIdx.x % 3;
    if (threadIdx.x < 9 && e < P.Ne && f < P.Ne) H[(long)(P.Nt + e) * P.np + P.Nt + f] += yy[3 * e + f];
}
// big cone: q = G_b'(J wbar)  then  H += eta^-2 (2 q q' - G_b' J G_b)
__global__ void k_big_q(DProg P, const double* __restrict__ wbb, double* __restrict__ qv, double* __restrict__ qd) {
    LANES(P, wbb, qv, qd);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    const long ob = P.l + 3L * P.nq3;
    if (t >= P.big) return;
    int r = int(ob) + t;
    double u = t == 0 ? wbb[0] : -wbb[t];
    if (P.col[r] >= 0) {                                    // one identity row per column in the big cone
        qv[P.col[r]] = P.alpha[r] * u;
        if (t > 0) qd[P.col[r]] = P.alpha[r] * P.alpha[r];
    }
    if (t == 0)
        for (int e = 0; e < P.Ne; ++e) qv[P.Nt + e] = P.ey[3 * r + e] * u;
}
__global__ void k_H_big(DProg P, const double* __restrict__ qv, const double* __restrict__ qd,
                        const double* __restrict__ Sc, double* __restrict__ H) {
    LANES(P, qv, qd, Sc, H);
    int k = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (k >= P.N || j >= P.N) return;
    const double e2 = 1.0 / (Sc[S_ETAB] * Sc[S_ETAB]);
    const long ob = P.l + 3L * P.nq3;
    double v = 2 * qv[j] * qv[k];
    if (j == k && j < P.Nt) v += qd[j];                      // - G_b' J G_b on the x block: + alpha_k^2 e e'
    if (j >= P.Nt && k >= P.Nt) v -= P.ey[3 * ob + (j - P.Nt)] * P.ey[3 * ob + (k - P.Nt)];
    H[(long)j * P.np + k] += e2 * v;
}

// initial point helpers -----------------------------------------------------------------------
// cone "distance outside" (max over cones of -(interior distance)) and ||v||^2
__global__ __launch_bounds__(256) void k_cone_resid(DProg P, const double* __restrict__ v, double* __restrict__ part) {
    LANES(P, v, part);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    double a[2] = {-1e300, 0};
    if (t < P.l) { a[0] = -v[t]; a[1] = P.row_weight(t) * (v[t] * v[t]); }
    else if (t < P.l + P.nq3) {
        int r = P.l + 3 * (t - P.l);
        a[0] = sqrt(v[r + 1] * v[r + 1] + v[r + 2] * v[r + 2]) - v[r];
        a[1] = P.row_weight(r) * (v[r] * v[r] + v[r + 1] * v[r + 1] + v[r + 2] * v[r + 2]);
    }
    __shared__ double sh[17];
    double m = block_max(a[0], sh), s = block_sum(a[1], sh);
    if (threadIdx.x == 0) { const long row = blockIdx.x + (P.big ? 1 : 0); part[2L * row] = m; part[2L * row + 1] = s; }   // (big cone's row first)
}
__global__ __launch_bounds__(1024) void k_big_cone_resid(DProg P, const double* __restrict__ v, double* __restrict__ part_row) {
    LANES(P, v, part_row);
    __shared__ double sh[17];
    const long ob = P.l + 3L * P.nq3;
    double n1 = big_dot(v + ob + 1, v + ob + 1, P.big - 1, sh);
    if (threadIdx.x == 0) { part_row[0] = sqrt(n1) - v[ob]; part_row[1] = P.own ? n1 + v[ob] * v[ob] : 0.0; }
}
// fold the cone-residual partials: RB[0] = max (distance outside), RB[1] = sum ||v||^2
__global__ __launch_bounds__(256) void k_cone_fold(const double* __restrict__ part, int nb, double* __restrict__ RB, size_t lane_bytes, const int* lane_mask) {
    LANES_RAW(lane_bytes, lane_mask, part, RB);
    __shared__ double sh[17];
    double tmax = fold_partials(part, nb, 2, 0, true, sh);
    double n2 = fold_partials(part, nb, 2, 1, false, sh);
    if (threadIdx.x == 0) { RB[0] = tmax; RB[1] = n2; }
}
// v += (1 + t) e  when  t >= -1e-8 max(1, ||v||)
__global__ __launch_bounds__(256) void k_cone_shift(DProg P, double* __restrict__ v, const double* __restrict__ RB) {
    LANES(P, v, RB);
    const double tmax = RB[0], nrm = sqrt(RB[1]);
    if (!(tmax >= -1e-8 * fmax(1.0, nrm))) return;
    const double add = 1.0 + tmax;
    const long ncones = (long)P.l + P.nq3 + (P.big ? 1 : 0);
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < ncones; t += (long)gridDim.x * blockDim.x) {
        long r = t < P.l ? t : (t < P.l + P.nq3 ? P.l + 3 * (t - P.l) : P.l + 3L * P.nq3);
        v[r] += add;
    }
}
__global__ void k_neg_copy_r(DProg P, const double* __restrict__ a, double* __restrict__ out, double sgn) {
    LANES(P, a, out);
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < P.R) out[r] = sgn * a[r];
}
__global__ void k_init_rhs(DProg P, double* __restrict__ bx2, double* __restrict__ bz2) {
    LANES(P, bx2, bz2);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.N) { bx2[t] = 0.0; bx2[P.LDV + t] = -P.c[t]; }
    if (t < P.R) { bz2[t] = P.h[t]; bz2[P.Rp + t] = 0.0; }
}
// H for the initial point (W = I): weights d=1 for LP rows, M = I for cones
__global__ void k_unit_scaling(DProg P, double* __restrict__ dl, double* __restrict__ wl, double* __restrict__ w3,
                               double* __restrict__ wbb, double* __restrict__ Sc) {
    LANES(P, dl, wl, w3, wbb, Sc);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P.l) { dl[t] = 1.0; wl[t] = 1.0; }
    if (t < P.nq3) { w3[4 * t] = 1.0; w3[4 * t + 1] = 1.0; w3[4 * t + 2] = 0.0; w3[4 * t + 3] = 0.0; }
    if (t < P.big) wbb[t] = t == 0 ? 1.0 : 0.0;
    if (t == 0) { Sc[S_ETAB] = 1.0; Sc[S_WB0] = 1.0; }
}
__global__ void k_finish_x(DProg P, const double* __restrict__ x, const double* __restrict__ Sc, double* __restrict__ out) {
    LANES(P, x, Sc, out);
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < P.N) out[j] = x[j] / Sc[S_TAU];
}
#include "ddkkt.inc"

// ================================================================================================
// host driver
// ================================================================================================
// The MBFIR_* switches of the solver's host code and of its factorisation, read from the environment once per call of solve_lanes,
// shape_key, max_lanes and the factorisation's test hooks (tests change them between solves in one process).  Each default is the
// behaviour with the switch unset.
struct SolveSwitches {
    bool corrector = true;       // CORRECTOR=0: no centrality corrector (programs without orthant rows never run it)
    bool corr_big = true;        // CORR_BIG=0: the corrector corrects the orthant rows alone and leaves the big cone's products alone
    int test_cap_kp = 0;         // TEST_CAP_KP (test hook): a single design pads its capacitance matrix S as a unit's largest lane would
    int ar_chunks = 0;           // AR_CHUNKS (>= 1; 0: the build's own choice): collectives of a dense row-sharded build
    int ar_overlap = 1;          // AR_OVERLAP: 1 the chunked all-reduce overlapped with the Gram product, 0 the assembled H summed, 2 (diagnostic) the chunked form without shards
    int cgrp = 4;                // CGRP (1 .. CGRP): chunks per block of the moment kernels
    int ddform = -1;             // DDFORM: -1 unset (opts.dd_form decides), 0 "dd" the double-double form, 1 any other value the capacitance form
    bool dd_blockinv = true;     // DD_BLOCKINV=0: substitution instead of the inverses of the dd factor's diagonal blocks
    bool hsolve = true;          // HSOLVE=0: the preconditioner as two triangular GEMVs instead of one pass over M
    bool fuse = true;            // FUSE=0: folds, residual norm, CG start and step length as launches of their own instead of inside their neighbours
                                 // (the corrector's trial step, candidate sum and pick included; the H-build's border moments over all points)
    bool speculate = true;       // SPECULATE=0: the head of the next iteration goes out after the host's verdicts, not before
    bool trace_host = false;     // TRACE_HOST (set): report where the host thread spends the solve
    int fold = -1;               // FOLD: -1 unset (fold unless the extended-precision solve is on), 0 / 1 every frequency on its own / +w and -w paired
    int chol_split = -1;         // CHOL_SPLIT: the factorisation's form (chol_inv_launch); -1 unset: its own choice per call
    bool poison = false;         // POISON=1 (test switch): NaN in the factorisation's diagonal-block images before every build
    int test_lose_flag = -1;     // TEST_LOSE_FLAG=k (test hook of chol.hip): the diagonal block of panel step k does not raise its flag; -1 none
    bool lanepair = true;        // LANEPAIR=0: every lane of a unit runs the lattice recurrences of G'v and G v itself instead of one thread per pair of lanes
};
static SolveSwitches read_switches() {
    SolveSwitches w;
    auto flag = [](const char* name, bool& v) { if (const char* ev = std::getenv(name)) v = std::atoi(ev) != 0; };
    auto number = [](const char* name, int& v) { if (const char* ev = std::getenv(name)) v = std::atoi(ev); };
    flag("MBFIR_CORRECTOR", w.corrector); flag("MBFIR_CORR_BIG", w.corr_big); flag("MBFIR_DD_BLOCKINV", w.dd_blockinv);
    flag("MBFIR_HSOLVE", w.hsolve); flag("MBFIR_FUSE", w.fuse); flag("MBFIR_SPECULATE", w.speculate); flag("MBFIR_POISON", w.poison);
    flag("MBFIR_LANEPAIR", w.lanepair);
    number("MBFIR_TEST_CAP_KP", w.test_cap_kp); number("MBFIR_AR_OVERLAP", w.ar_overlap);
    number("MBFIR_CHOL_SPLIT", w.chol_split); number("MBFIR_TEST_LOSE_FLAG", w.test_lose_flag);
    if (const char* ev = std::getenv("MBFIR_CGRP")) w.cgrp = std::max(1, std::min(CGRP, std::atoi(ev)));
    if (const char* ev = std::getenv("MBFIR_AR_CHUNKS")) w.ar_chunks = std::max(1, std::atoi(ev));
    if (const char* ev = std::getenv("MBFIR_DDFORM")) w.ddform = std::strcmp(ev, "dd") != 0 ? 1 : 0;
    if (const char* ev = std::getenv("MBFIR_FOLD")) w.fold = std::atoi(ev) != 0;
    w.trace_host = std::getenv("MBFIR_TRACE_HOST") != nullptr;
    return w;
}

// Host analysis for the lattice mode (DProg::trig): column delays on one unit-step lattice, at most
// one column per (kind, lattice point), and a frequency grid made of equally spaced runs.
struct LatticeInfo {
    bool ok = false;
    double tmin = 0;
    int D1 = 0;
    std::vector<int> lat, lat_col, lat_qcol, ch_start, ch_count;
    std::vector<double> lat_scale, lat_qscale, ch_w0, ch_dw;
    // folded frequency list (see analyse_lattice): entry k stands for +wf[k] (frequency index fold_pos[k], or -1) and
    // -wf[k] (fold_neg[k], or -1); the chunks index this list
    std::vector<int> fold_pos, fold_neg;
    std::vector<double> wf;
};
// CHUNK_LEN: longest run of frequencies one recurrence covers between two exact sincos seeds.
// fold: pair the frequencies +w / -w of a grid that is symmetric about 0 (linspace(-pi, pi, m) is, to 2 ulp): the two
// share cos(w t) and differ in the sign of sin(w t), so every recurrence of the lattice kernels serves both -- the
// moment sums take p(+w) + p(-w) on the cosine and p(+w) - p(-w) on the sine, a row response is C + S at +w and C - S
// at -w.  A frequency without a partner (band edges, one-sided grids) is an entry with one side empty.
constexpr int CHUNK_LEN = 64;
static_assert(CHUNK_LEN <= CHK, "a chunk holds at most CHK frequencies");
static LatticeInfo analyse_lattice(const TrigProgram& Q, bool fold) {
    LatticeInfo L;
    const int Nt = Q.Nt, Mf = Q.Mf;
    if (Nt <= 0 || Mf <= 0) return L;
    double tmin = Q.col_tau[0];
    for (double t : Q.col_tau) tmin = std::min(tmin, t);
    L.lat.resize(Nt);
    int D1 = 0;
    for (int j = 0; j < Nt; ++j) {
        const double m = Q.col_tau[j] - tmin;
        const long mi = std::lround(m);
        if (std::fabs(m - double(mi)) > 1e-9 || mi > 8L * Nt + 64) return L;
        L.lat[j] = int(mi);
        D1 = std::max(D1, int(mi) + 1);
    }
    L.lat_col.assign(2 * D1, -1); L.lat_qcol.assign(2 * D1, -1);
    L.lat_scale.assign(2 * D1, 0.0); L.lat_qscale.assign(2 * D1, 0.0);
    for (int j = 0; j < Nt; ++j) {
        const int e = Q.col_kind[j] * D1 + L.lat[j];
        if (L.lat_col[e] >= 0) return L;
        L.lat_col[e] = j; L.lat_scale[e] = Q.col_scale[j];
    }
    if (Q.quad)
        for (int j0 = 0; j0 < Nt; ++j0) {
            if (Q.psign[j0] == 0.0) continue;
            const int jp = Q.pcol[j0];
            if (jp < 0 || jp >= Nt) return L;
            const int e = Q.col_kind[jp] * D1 + L.lat[jp];
            if (L.lat_qcol[e] >= 0) return L;
            L.lat_qcol[e] = j0; L.lat_qscale[e] = Q.col_scale[jp] * Q.psign[j0];
        }
    double wmax = 1.0;
    for (double w : Q.w) wmax = std::max(wmax, std::fabs(w));
    const double tol = 2 * 2.2204460492503131e-16 * wmax;
    // ---- the folded list ---------------------------------------------------------------------------------------
    if (fold) {
        std::vector<int> order(Mf);
        for (int i = 0; i < Mf; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::fabs(Q.w[a]) < std::fabs(Q.w[b]); });
        for (int q = 0; q < Mf; ++q) {
            const int i = order[q];
            const bool neg = Q.w[i] < 0.0;
            const double aw = std::fabs(Q.w[i]);
            if (!L.wf.empty() && aw - L.wf.back() <= tol && (neg ? L.fold_neg.back() < 0 : L.fold_pos.back() < 0)) {
                (neg ? L.fold_neg : L.fold_pos).back() = i;
                L.wf.back() = 0.5 * (L.wf.back() + aw);       // the pair's common |w|: each side within 1 ulp of its own
            } else {
                L.wf.push_back(aw); L.fold_pos.push_back(neg ? -1 : i); L.fold_neg.push_back(neg ? i : -1);
            }
        }
    } else {                                                  // every frequency on its own, in the program's order, signs kept
        L.wf = Q.w;
        L.fold_pos.resize(Mf); L.fold_neg.assign(Mf, -1);
        for (int i = 0; i < Mf; ++i) L.fold_pos[i] = i;
    }
    const int Nf = int(L.wf.size());
    const std::vector<double>& W = L.wf;
    // Longest run from i (at most CHUNK_LEN points) that lies on the straight line through its END POINTS to within
    // `tol`: a linspace run passes at full length (every point is within half an ulp of the exact line), where a step
    // estimated from the first two points drifts out of tolerance after ~30 points.  Shrink by halves on failure.
    for (int i = 0; i < Nf;) {
        int cnt = std::min(CHUNK_LEN, Nf - i);
        double dwf = 0.0;
        for (;;) {
            dwf = cnt > 1 ? (W[i + cnt - 1] - W[i]) / (cnt - 1) : 0.0;
            bool ok = true;
            for (int q = 1; q + 1 < cnt && ok; ++q) ok = std::fabs(W[i + q] - (W[i] + q * dwf)) <= tol;
            if (ok || cnt <= 2) break;
            cnt = std::max(2, cnt / 2);
        }
        if (cnt == 2 && i + 2 < Nf && std::fabs(W[i + 2] - (W[i] + 2 * dwf)) > tol && std::fabs(dwf) > 0 &&
            (i + 3 >= Nf || std::fabs((W[i + 2] - W[i + 1]) - (W[i + 3] - W[i + 2])) <= tol))
            cnt = 1;                                       // an isolated point (a band edge) ahead of the next run
        if (cnt <= 1) { cnt = 1; dwf = 0.0; }
        L.ch_start.push_back(i); L.ch_count.push_back(cnt); L.ch_w0.push_back(W[i]); L.ch_dw.push_back(dwf);
        i += cnt;
    }
    if ((long)L.ch_start.size() > Mf / 8 + 64) return L;       // grid too irregular: the dense path is the better one
    L.tmin = tmin; L.D1 = D1; L.ok = true;
    return L;
}

__global__ __launch_bounds__(256) void k_zero_lanes(double2* __restrict__ p, size_t n16, size_t lane_bytes) {
    p = reinterpret_cast<double2*>(reinterpret_cast<char*>(p) + (size_t)blockIdx.y * lane_bytes);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n16; e += (size_t)gridDim.x * 256) p[e] = make_double2(0.0, 0.0);
}

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool measuring = false;      // first pass: only add up the sizes
    void reset() { off = 0; }
    template <class T>
    T* get(size_t n) {
        size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
        if (!measuring && off + bytes > cap) throw HipError("device arena exhausted");
        T* p = reinterpret_cast<T*>(base + off);
        off += bytes;
        return p;
    }
};

static double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// Two programs can share a lock-step batch when every array the device holds for them has the same length and
// the scalar structure the kernels are launched with is the same: dimensions, lattice extent and chunk count.
// index structures + lattice analysis of one program, kept with the program (TrigProgram::prep) so that the batch
// front end can compute them in its parallel assembly threads and the solve does not repeat them
struct LanePrep {
    bool fold = true, dense = false;
    std::vector<int> f_ptr, f_rows, c_ptr, c_rows, yrows, rep;
    LatticeInfo Lt;
};
// Host-side description of one lane (one design of a lock-step batch)
struct LaneHost {
    const TrigProgram* Q = nullptr;
    TrigProgram local;                       // the row shard (sharded solves have one lane)
    std::shared_ptr<const LanePrep> prep;    // its index structures (lane_prep)
    LatticeInfo Lt;                          // its lattice analysis (a row-sharded solve may drop it: dense path on every rank)
    double nrm_h = 1, nrm_c = 1, degree = 0;
    // IPM state
    int status = ST_MAXIT, nsweep = 0 /* sweeps the iteration's solves run */, nsweep_ctl = 0 /* ... of which the controller asks for (the rest: POLISH_SWEEPS) */, wall = 0;
    bool live = true, have_best = false;
    double best_merit = 1e300, rx_prev = 0;
    SolveInfo info, best_info;
    // end game (oracle/conic_ipm.py POLISH): the first iteration whose iterate met the stopping rule, the best such iterate's merit and report
    // (its x / tau is in xbest: once an iterate has met the rule the reduced-accuracy candidate that buffer held is of no use)
    int first_opt = -1;
    double opt_merit = 1e300;
    SolveInfo opt_info;
    // extended-precision path: strong directions of the current iteration (0: the plain solve), iterations on it, its largest set
    int dd_k = 0, dd_iters = 0, dd_kmax = 0;
};

static void index_structures(const TrigProgram& Q, LanePrep& L) {
    const int R = Q.R, Nt = Q.Nt, Mf = Q.Mf;
    L.f_ptr.assign(Mf + 1, 0); L.c_ptr.assign(Nt + 1, 0); L.f_rows.clear(); L.c_rows.clear(); L.yrows.clear();
    for (int r = 0; r < R; ++r) {
        if (Q.freq[r] >= 0) L.f_ptr[Q.freq[r] + 1]++;
        if (Q.col[r] >= 0) L.c_ptr[Q.col[r] + 1]++;
        if (Q.ey[3 * r] != 0 || Q.ey[3 * r + 1] != 0 || Q.ey[3 * r + 2] != 0) L.yrows.push_back(r);
        if (Q.freq[r] >= 0 && r >= Q.l) {
            int a = (r - Q.l) % 3;
            if (r >= Q.l + 3 * Q.nq3 || a == 0) throw HipError("unsupported cone layout (trig row at cone position 0 / in big cone)");
        }
    }
    for (int i = 0; i < Mf; ++i) L.f_ptr[i + 1] += L.f_ptr[i];
    for (int j = 0; j < Nt; ++j) L.c_ptr[j + 1] += L.c_ptr[j];
    L.f_rows.resize(L.f_ptr[Mf]); L.c_rows.resize(L.c_ptr[Nt]);
    std::vector<int> fp(L.f_ptr.begin(), L.f_ptr.end() - 1), cp(L.c_ptr.begin(), L.c_ptr.end() - 1);
    for (int r = 0; r < R; ++r) {
        if (Q.freq[r] >= 0) L.f_rows[fp[Q.freq[r]]++] = r;
        if (Q.col[r] >= 0) L.c_rows[cp[Q.col[r]]++] = r;
    }
}

static std::shared_ptr<LanePrep> lane_prep(const TrigProgram& Q, const SolveOpts& o, const SolveSwitches& sw) {
    const bool fold = o.ddkkt_theta <= 0, dense = o.dense_trig != 0;
    if (Q.prep) {
        auto have = std::static_pointer_cast<LanePrep>(Q.prep);
        if (have->fold == fold && have->dense == dense) return have;
    }
    auto pr = std::make_shared<LanePrep>();
    pr->fold = fold; pr->dense = dense;
    index_structures(Q, *pr);
    pr->rep = replicated_rows(Q);
    if (!dense) pr->Lt = analyse_lattice(Q, sw.fold < 0 ? fold : sw.fold != 0);
    Q.prep = pr;
    return pr;
}

// what unit planning hands on to the arena layout and the driver
struct UnitPlan {
    int n_max = 0, lp = 0;                   // the unit's largest order and its spectral-factorisation length
    bool use_dd = false;                     // the extended-precision KKT solve is on
    std::vector<std::vector<int>> tiles;     // every lane's Gram tile table (lane 0's chunk tables behind it)
};

// The verdict on one live lane after iteration `it` (mirrors oracle/conic_ipm.py): the refinement-sweep controller, the stopping
// rule and the end game, the infeasibility tests, the reduced-accuracy candidate, max_iter and the numerical wall.  hs: the lane's
// scalar row.  Updates the lane's host state (a lane that finishes is no longer live); returns whether the lane has a new best
// iterate (xbest is then to take its x / tau -- also on a lane that this very iteration retires).
static bool lane_verdict(LaneHost& L, const double* hs, const SolveOpts& o, int it) {
    SolveInfo& info = L.info;
    if (it > 0 && L.dd_k == 0) {                      // (iterations on the extended-precision path keep the count)
        // refinement-sweep controller (mirrors oracle/conic_ipm.py next_sweeps): the norms were
        // measured before each sweep of the two KKT solves of the previous iteration
        const double tol = std::max(REFTOL * hs[S_NRMC], REFETA * L.rx_prev);   // ||rx|| of the iteration the norms belong to
        int need = 0;
        bool unconverged = false;
        for (int slot : {int(S_RNA), int(S_RNB)}) {        // (the corrector's solve runs without sweeps and reports no norms)
            int k = -1;
            for (int q = 0; q <= std::min(L.nsweep, MAX_SWEEPS); ++q)      // n_0 .. n_nsweep
                if (hs[slot + q] <= tol) { k = q; break; }
            if (k < 0) unconverged = true;
            else need = std::max(need, k);
        }
        L.nsweep_ctl = unconverged ? std::min(MAX_SWEEPS, L.nsweep + 1) : need;
    }
    L.rx_prev = hs[S_DRES] * hs[S_TAU] * hs[S_NRMC];
    info.iters = it; info.pcost = hs[S_PCOST]; info.dcost = hs[S_DCOST]; info.gap = hs[S_GAP];
    info.relgap = hs[S_RELGAP]; info.pres = hs[S_PRES]; info.dres = hs[S_DRES];
    info.correctors = int(hs[S_NCORR]); info.correctors_taken = int(hs[S_NPICK]);
    bool best = false;
    auto finish = [&](int status) { L.status = status; L.live = false; return best; };
    const bool finite = std::isfinite(hs[S_PRES]) && std::isfinite(hs[S_DRES]) && std::isfinite(hs[S_GAP]) && hs[S_TAU] > 0;
    if (finite && hs[S_PRES] <= o.feastol && hs[S_DRES] <= o.feastol && (hs[S_GAP] <= o.abstol || hs[S_RELGAP] <= o.reltol)) {
        // end game (mirrors oracle/conic_ipm.py): the iterate meets the stopping rule -- keep the best such iterate (xbest) and
        // go on until the gap measures are POLISH times below the tolerances or POLISH_MAX more iterations have passed; the
        // best iterate is the answer however the end game ends
        const double merit_o = std::min(hs[S_RELGAP] / o.reltol, hs[S_GAP] / std::max(o.abstol, 1e-300));
        if (L.first_opt < 0 || merit_o < L.opt_merit) {
            L.opt_merit = merit_o; L.opt_info = info;
            best = true;
        }
        if (L.first_opt < 0) L.first_opt = it;
        if (hs[S_GAP] <= POLISH * o.abstol || hs[S_RELGAP] <= POLISH * o.reltol) return finish(ST_OPTIMAL);
    }
    if (L.first_opt >= 0 && it >= L.first_opt + POLISH_MAX) return finish(ST_OPTIMAL);      // (whether or not this iterate still meets the rule)
    {   // what this iteration's solves run: the controller's count, POLISH_SWEEPS more in the final approach and the end game
        const bool approach = finite && (hs[S_GAP] <= POLISH_APPROACH * o.abstol || hs[S_RELGAP] <= POLISH_APPROACH * o.reltol);
        L.nsweep = std::min(MAX_SWEEPS, L.nsweep_ctl + ((approach || L.first_opt >= 0) ? POLISH_SWEEPS : 0));
    }
    if (!finite) return finish(ST_NUMERICAL);
    const bool collapsed = hs[S_KAPPA] / hs[S_TAU] >= 1e6;
    if (L.first_opt < 0 && (hs[S_PINF] <= o.feastol || (collapsed && hs[S_PINF] <= 1e-5))) return finish(ST_PRIMAL_INFEASIBLE);
    if (L.first_opt < 0 && (hs[S_DINF] <= o.feastol || (collapsed && hs[S_DINF] <= 1e-5))) return finish(ST_DUAL_INFEASIBLE);
    if (L.first_opt < 0 && hs[S_PRES] <= INACC_FEAS && hs[S_DRES] <= INACC_FEAS) {
        // best iterate for the reduced-accuracy exit: residuals within the reduced tolerance,
        // smallest gap measure (mirrors oracle/conic_ipm.py)
        double merit = std::min(hs[S_RELGAP], hs[S_GAP] / std::max(o.abstol, 1e-300) * o.reltol);
        if (merit < L.best_merit) {
            L.best_merit = merit; L.best_info = info; L.have_best = true;
            best = true;
        }
    }
    if (it == o.max_iter) return finish(ST_MAXIT);
    // numerical wall (mirrors oracle/conic_ipm.py): the last factorisation replaced pivots and the
    // residuals are out of the reduced-accuracy range, three iterations in a row
    L.wall = (int(hs[S_CHOLFIX]) > 0 && (hs[S_PRES] > INACC_FEAS || hs[S_DRES] > INACC_FEAS)) ? L.wall + 1 : 0;
    if (L.wall >= WALL_ITERS) return finish(ST_NUMERICAL);
    return best;
}

struct Solver::Impl {
    int device = 0;
    hipStream_t st = nullptr;
    // row sharding (one process per GPU): reductions over the shards go through this hook
    int shard_rank = 0, shard_size = 1;
    int (*ar_fn)(void*, long, int, void*) = nullptr;
    void* ar_user = nullptr;
    double* RB = nullptr;        // 16 doubles: reduction mailbox
    // RCCL communicator of this context (mbfir_comm_init): the sharded solve's reductions are ncclAllReduce calls
    // enqueued on the solver stream -- no host synchronisation, no callback.  Without one the hook is used.
    ncclComm_t comm = nullptr;
    int comm_size = 0, comm_rank = 0;
    long n_collectives = 0;      // issued by the current solve
    double collective_bytes = 0; // ... and the bytes they carried
    long n_pair = 0;             // ... and how many lattice passes ran the paired kernels (k_trig_eval_pair: every G v, the residual's included; k_trig_moments_pair: G'v, H-build moments)
    long n_gv = 0, n_gtv = 0;    // passes over the frequency rows of the current solve: G v (apply_G / apply_G_winv2, the residual's row response), G'v (apply_GT)
    void allreduce(double* buf, long count, int op, hipStream_t on = nullptr) {
        if (shard_size <= 1) return;
        if (!on) on = st;
        ++n_collectives;
        collective_bytes += 8.0 * double(count);
        if (comm) {
            ncclResult_t r = rccl().AllReduce(buf, buf, size_t(count), ncclDouble, op == 1 ? ncclMax : ncclSum, comm, on);
            if (r != ncclSuccess) throw HipError(std::string("ncclAllReduce: ") + (rccl().GetErrorString ? rccl().GetErrorString(r) : "failed"));
            return;
        }
        MBFIR_HIP(hipStreamSynchronize(on));
        if (!ar_fn || ar_fn(buf, count, op, ar_user) != 0) throw HipError("all-reduce hook failed");
    }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Arena ar;
    double* hostSc = nullptr;    // pinned, S_COUNT per lane
    int* hostFlag = nullptr;     // pinned, 4 per lane
    // lock-step batch: nlanes designs of identical shape in one arena, lane b at + b * lane_bytes (see DProg)
    int nlanes = 1, nlanes_last = 1;
    bool taps_valid = false;     // hout holds the taps of the last unit's solutions (specfact_last)
    int lane_n[64] = {};         // taps of the lanes of the last unit (they differ when the unit held designs of different orders)
    long chol_launch_count = 0;  // k_chol_step launches of the current solve
    size_t lane_bytes = 0;
    bool lane_live[64] = {};     // host copy of mask row 0 (the dense Gram products are launched per lane)
    bool fused_hsolve = false;   // x = M'(M b) in one pass over M (np <= 1024, no extended-precision solve): no stored transpose
    int* maskT = nullptr;        // device, MASK_ROWS x MAX_LANES ints: row 0 = live lanes, rows 1..MAX_SWEEPS = lanes that
                                 // still need CG sweep q, row MAX_SWEEPS + 1 = scratch (lanes with a new best iterate)
    int* hostMask = nullptr;     // pinned twin
    LaneDims* dimsT = nullptr;   // device, MAX_LANES entries: the lanes' own dimensions in a heterogeneous unit (DProg::dims)
    LaneDims* hostDims = nullptr;   // pinned twin
    const int* mask_row(int r) const { return nlanes > 1 ? maskT + (size_t)r * MAX_LANES : nullptr; }
    std::string err;

    // per-solve device pointers
    DProg P{};
    GramPlan gp;                 // the unit's sizes: ld, the largest Mpad and slab of its lanes
    std::vector<GramPlan> gps;   // ... and every lane's own plan (dense path)
    int nsplit_at = 0;
    double *A1, *T, *slab, *H, *M, *Mt, *W1, *Sc;
    int *tile_ij, *flag;
    double *x, *s, *z, *lam, *dl, *wl, *w3, *wbb;
    double *XX, *UU, *PP, *partial, *TT, *TT2, *Dw, *BB, *qv;
    double2* PPf = nullptr;      // (pe, po) per folded frequency (k_freq_fold)
    double *Mom, *MomB;            // lattice mode: H moments, border moments
    double *tmpN, *tmpN2, *rhsN, *yN, *tmpR, *wbz, *pN, *wpR;
    double *bx2, *bz2, *dx2, *dz2, *gdx2, *gdxc, *xbest, *rx, *rz, *GTz, *Gx;
    double *dssa, *wdza, *lds, *bxc, *bzc, *dxc, *dzc, *ds, *dz, *scratch;
    double *kbx, *kbz, *kx, *kz, *kg, *kds, *kdz;        // centrality corrector: right-hand side (kbx stays zero), solution / candidate, its direction
    SolveSwitches sw;            // the switches of the current solve (read once at its start: none is read in a per-iteration path)
    // dense row-sharded builds of a program with ONE weight matrix (fir_ap_cvx, fir_linprog): the Gram product goes in sw.ar_chunks
    // launches and the all-reduce of chunk c's packed tiles runs on st2 while chunk c + 1 is computed; the small
    // ingredients (border products, y-y block) follow in one collective and every rank assembles and factorises the same H.
    // MBFIR_AR_OVERLAP=0: the assembled H is summed instead (packed lower triangle, after the build; the only form for programs
    // with three weight matrices, whose T is 3 x the size of H); =2 (diagnostic): the chunked form without shards, collectives skipped
    bool ar_overlap = false;
    std::vector<GramChunk> gchunks;
    const int* chunk_tab = nullptr;
    double* Tp = nullptr;
    hipStream_t st2 = nullptr;
    std::vector<hipEvent_t> ovev;            // 2 per chunk: chunk folded (st), chunk summed (st2)
    double *partR, *partR2, *partN, *xout, *hout, *sfwork;
    int nbR = 0, nbN = 0, nbC = 0;
    // extended-precision KKT solve (ddkkt.inc): H = H_w + U'XU and its Cholesky factor in double-double.
    // The dd factor reuses the buffers of the double-precision inverse: Hl = M, L' = (Mt, W1).
    DDev D{};
    double *ddB = nullptr, *ddtS = nullptr, *ddzeta = nullptr, *ddri = nullptr, *ddd0 = nullptr;
    double* ddinv = nullptr;     // inverses of the 64 x 64 diagonal blocks of the dd factor (k_dd_blockinv); nullptr (MBFIR_DD_BLOCKINV=0): substitution
    int* ddflags = nullptr;      // block flags of k_dd_trsv_mw / k_dd_trsv_bi; dd_epoch: the value the current call waits for
    int dd_epoch = 0;
    // capacitance form of that solve (capkkt.hip; the default): Yt = U M', Zt = Yt M (k x np each), S = Yt Yt' + X^-1 and its
    // inverse Cholesky factor Ms (kp x kp, kp = k rounded up to 64, at most CAP_KMAX), W1s / flagS the workspace and pivot
    // counter of that factorisation, capw the right-hand side of the S solve
    bool cap_form = true;
    int dd_passes = 2;           // refinement passes on the augmented system around the extended-precision solve (<= 8: the norm slots)
    double *capYt = nullptr, *capZt = nullptr, *capS = nullptr, *capMs = nullptr, *capW1 = nullptr, *capw = nullptr, *capPart = nullptr;
    int* capflag = nullptr;
    int dd_k = 0;                 // strong directions of the current iteration (0: plain double-precision solve)

    void ensure_arena(size_t bytes) {
        if (bytes <= ar.cap) { ar.reset(); return; }
        if (ar.base) MBFIR_HIP(hipFree(ar.base));
        ar.base = nullptr; ar.cap = 0;
        if (hipMalloc(&ar.base, bytes) != hipSuccess) {
            (void)hipGetLastError();
            ar.base = nullptr;
            throw ResourceError("arena of " + std::to_string(bytes >> 20) + " MiB not available on the device");
        }
        ar.cap = bytes;
        ar.reset();
    }
    // one array per lane, all of the same length (the lanes share one arena layout); get(b) returns lane b's vector
    // The arrays are gathered in a pinned host image of the lanes' program region and go to the device in ONE copy per
    // lane (flush_uploads): ~35 arrays x 8 lanes as separate pageable copies cost ~10 ms per unit with the stream idle.
    char* stage = nullptr;       // pinned
    // Program arrays go to the device in ONE pinned copy per lane: upload() writes every array straight into the lane's image
    // of the arena region [stage_lo, stage_hi) -- whose extent the measuring pass of the layout has recorded (meas_lo, meas_hi)
    // -- and flush_uploads() sends the images.  (Round 2 staged [array][lane] and re-packed to [lane][array]: three passes over
    // 32 MB of host memory per unit of 16 headline designs, 6-9 ms with the GPU idle at the start of every batch.)
    size_t stage_cap = 0, stage_lo = 0, stage_hi = 0;      // byte range of the arena (lane 0) the staged arrays cover
    size_t meas_lo = 0, meas_hi = 0;                       // the same range as the measuring pass saw it
    template <class T, class F>
    T* upload(F get) {
        // (heterogeneous units: the array is as long as the longest lane's; a shorter lane's tail is zero-filled)
        size_t n0 = 0;
        for (int b = 0; b < nlanes; ++b) n0 = std::max(n0, get(b).size());
        T* p = ar.get<T>(std::max<size_t>(n0, 1));
        const size_t off = size_t(reinterpret_cast<char*>(p) - ar.base), bytes = n0 * sizeof(T);
        if (ar.measuring) {
            if (meas_hi == meas_lo) meas_lo = meas_hi = off;
            meas_hi = std::max(meas_hi, off + std::max<size_t>(bytes, sizeof(T)));
            return p;
        }
        if (stage_hi == stage_lo) {                           // first array of this layout pass
            stage_lo = stage_hi = off;
            if (off != meas_lo) throw HipError("upload: the layout differs from its measuring pass");
        }
        if (off < stage_hi || off + bytes > meas_hi) throw HipError("upload: arrays out of order");
        pend.push_back({off, bytes, stage_hi, [get](int b, size_t& nb) -> const void* { nb = get(b).size() * sizeof(T); return get(b).data(); }});
        stage_hi = off + bytes;
        return p;
    }
    struct Pend { size_t off, bytes, prev_end; std::function<const void*(int, size_t&)> src; };
    std::vector<Pend> pend;
    void flush_uploads() {
        if (pend.empty()) return;
        const size_t region = meas_hi - meas_lo, need = region * nlanes;
        if (need > stage_cap) {
            if (stage) hipHostFree(stage);
            stage_cap = std::max(need * 2, size_t(1) << 22);
            MBFIR_HIP(hipHostMalloc(reinterpret_cast<void**>(&stage), stage_cap));
        }
        // lane images filled and sent by a few threads: 32 MB for a unit of 16 headline designs, 2.5 ms on one core with
        // the stream idle -- at the start of a batch that is time the slowest unit does not get back
        const int nth = need >= (size_t(4) << 20) ? std::min(nlanes, 4) : 1;
        std::vector<hipError_t> rc(nth, hipSuccess);
        auto fill = [&](int t) {
            if (t > 0) rc[t] = hipSetDevice(device);
            for (int b = t; b < nlanes && rc[t] == hipSuccess; b += nth) {
                char* img = stage + region * b;
                for (const Pend& q : pend) {
                    if (q.off > q.prev_end) std::memset(img + (q.prev_end - stage_lo), 0, q.off - q.prev_end);      // alignment gap before the array
                    if (q.bytes) {
                        size_t nb = 0;
                        const void* src = q.src(b, nb);
                        if (nb > q.bytes) nb = q.bytes;
                        if (nb) std::memcpy(img + (q.off - stage_lo), src, nb);
                        if (nb < q.bytes) std::memset(img + (q.off - stage_lo) + nb, 0, q.bytes - nb);
                    }
                }
                const size_t filled = stage_hi - stage_lo;
                if (region > filled) std::memset(img + filled, 0, region - filled);
                rc[t] = hipMemcpyAsync(ar.base + stage_lo + (size_t)b * lane_bytes, img, region, hipMemcpyHostToDevice, st);
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nth; ++t) th.emplace_back(fill, t);
        fill(0);
        for (auto& t : th) t.join();
        for (hipError_t e : rc) MBFIR_HIP(e);
        pend.clear();
        stage_lo = stage_hi = 0;
    }
    // the same stretch of every lane
    void memset_lanes(void* p, size_t bytes) {
        // own kernel: the runtime's pitched 2-D fill runs at ~0.6 TB/s (1.7 ms per unit of 8 headline designs, 4.8 ms
        // with four units in flight), this one at the HBM write rate
        if ((bytes & 15) == 0 && (reinterpret_cast<size_t>(p) & 15) == 0 && (lane_bytes & 15) == 0)
            hipLaunchKernelGGL(k_zero_lanes, dim3(std::min<size_t>(2048, cdiv((long)(bytes / 16), 256)), nlanes), dim3(256), 0, st,
                               reinterpret_cast<double2*>(p), bytes / 16, lane_bytes);
        else if (nlanes > 1) hipMemset2DAsync(p, lane_bytes, 0, bytes, nlanes, st);
        else hipMemsetAsync(p, 0, bytes, st);
    }
    void copy_lanes(void* dst, const void* src, size_t bytes) {
        if (nlanes > 1) MBFIR_HIP(hipMemcpy2DAsync(dst, lane_bytes, src, lane_bytes, bytes, nlanes, hipMemcpyDeviceToDevice, st));
        else MBFIR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    }

    // ---- operators ----
    // one thread runs the lattice recurrences of two lanes (k_trig_eval_pair: G v; k_trig_moments_pair: G'v and the H-build's moments): the lanes of the unit share
    // grid and lattice, have the same extents, and the solve is neither sharded nor on the extended-precision path
    bool lane_pairs() const { return sw.lanepair && nlanes >= 2 && P.seeds_shared && !P.dims && shard_size == 1 && !dd_unit; }
    template <int NV>
    void trig_eval(const double* v) {
        const dim3 g(cdiv(P.nfold, 256), P.useg);
        if (lane_pairs()) {
            ++n_pair;
            hipLaunchKernelGGL(k_trig_eval_pair<NV>, lane_grid(g, cdiv(nlanes, 2)), dim3(256), 0, st, P, v, UU, nlanes);
        } else hipLaunchKernelGGL(k_trig_eval<NV>, lane_grid(g, nlanes), dim3(256), 0, st, P, v, UU);
    }
    template <int NV>
    void apply_G(const double* v, double* out) {
        const int NVV = P.quad ? 2 * NV : NV;
        ++n_gv;
        if (P.trig) {
            trig_eval<NV>(v);
            hipLaunchKernelGGL(k_rows_G<NV>, lane_grid(dim3(cdiv(P.R, 256)), nlanes), dim3(256), 0, st, P, UU, v, out);
            return;
        }
        const double* xx = v;
        if (P.quad) {
            hipLaunchKernelGGL(k_make_xx<NV>, lane_grid(dim3(cdiv(P.Nt, 256)), nlanes), dim3(256), 0, st, P, v, XX);
            xx = XX;
        }
        dim3 g(cdiv(P.Mf, 4));
        if (NVV == 1) hipLaunchKernelGGL(k_amulti<1>, lane_grid(g, nlanes), dim3(256), 0, st, A1, P.ld, P.Mf, xx, P.LDV, UU, P.Mpad, lane_bytes, P.mask, P.dims);
        else if (NVV == 2) hipLaunchKernelGGL(k_amulti<2>, lane_grid(g, nlanes), dim3(256), 0, st, A1, P.ld, P.Mf, xx, P.LDV, UU, P.Mpad, lane_bytes, P.mask, P.dims);
        else hipLaunchKernelGGL(k_amulti<4>, lane_grid(g, nlanes), dim3(256), 0, st, A1, P.ld, P.Mf, xx, P.LDV, UU, P.Mpad, lane_bytes, P.mask, P.dims);
        hipLaunchKernelGGL(k_rows_G<NV>, lane_grid(dim3(cdiv(P.R, 256)), nlanes), dim3(256), 0, st, P, UU, v, out);
    }
    // gout = G v and wout = W^-2 gout - sub; one kernel less than apply_G + winv2 on the lattice path
    // without a big cone
    template <int NV>
    void apply_G_winv2(const double* v, double* gout, const double* sub, double* wout) {
        if (P.trig && !P.big) {
            ++n_gv;
            trig_eval<NV>(v);
            hipLaunchKernelGGL(k_rows_winv2<NV>, lane_grid(dim3(cdiv(P.l + P.nq3, 256)), nlanes), dim3(256), 0, st, P, UU, v, dl, w3, sub, gout, wout);
            return;
        }
        apply_G<NV>(v, gout);
        winv2<NV>(gout, sub, wout, 0);
    }
    // border products of the H assembly: partial = A1' * BB (BB is a per-frequency array)
    // lattice mode: moments of per-frequency arrays on the progressions (t0a, na), (t0b, nb)
    // pp == nullptr: the folded operands are in PPf already (k_freq_blocks_fold)
    // nfull (0: all): the operands in front that are read over the whole of (na, nb); those behind are read at the points m < na alone and the
    // blocks past na leave them out (trim_border); k_fold_partials folds their rows over the columns below na alone, `out` keeps stale words past them
    void moments_array(int nv, const double* pp, const double4* seeds, int na, int nb, double* out, int nfull = 0) {
        if (nfull <= 0) nfull = nv;
        dim3 g(cdiv(na + nb, MPTS), cdiv(P.nchunk, P.cgrp)), b(256), gf(cdiv(P.nfold, 256));
        const bool pair = lane_pairs();                    // (the H-build's moment pass: k_trig_moments_pair<NV, false>)
        if (pair) ++n_pair;
        switch (nv) {
#define MOM_CASE(NVX)                                                                                                          \
            case NVX:                                                                                                          \
                if (pp) hipLaunchKernelGGL((k_freq_fold<NVX, false>), lane_grid(gf, nlanes), b, 0, st, P, pp, PPf);            \
                if (pair) hipLaunchKernelGGL((k_trig_moments_pair<NVX, false>), lane_grid(g, cdiv(nlanes, 2)), b, 0, st, P, PPf, seeds, na, nb, partial, (const double*)nullptr, nlanes, nfull); \
                else hipLaunchKernelGGL((k_trig_moments<NVX>), lane_grid(g, nlanes), b, 0, st, P, PPf, seeds, na, nb, partial, (const double*)nullptr, nfull); \
                break;
            MOM_CASE(1) MOM_CASE(2) MOM_CASE(3) MOM_CASE(4) MOM_CASE(6)
#undef MOM_CASE
            default: throw HipError("moments: unsupported vector count");
        }
        hipLaunchKernelGGL(k_fold_partials, lane_grid(dim3(cdiv(P.LDM, FPC), 2 * nv), nlanes), dim3(FPC, 16), 0, st, partial, cdiv(P.nchunk, P.cgrp), 2 * nv, P.LDM, P.LDM, out, lane_bytes, P.mask, P.dims, P.cgrp,
                           nfull < nv ? 2 * nfull : 1 << 30, na);
    }
    void atmulti_array(int nvv, const double* pp) {
        dim3 g(P.ld / 128, nsplit_at), b(64, 4);
        switch (nvv) {
            case 1: hipLaunchKernelGGL((k_atmulti<1, false>), lane_grid(g, nlanes), b, 0, st, P, A1, pp, partial); break;
            case 2: hipLaunchKernelGGL((k_atmulti<2, false>), lane_grid(g, nlanes), b, 0, st, P, A1, pp, partial); break;
            case 3: hipLaunchKernelGGL((k_atmulti<3, false>), lane_grid(g, nlanes), b, 0, st, P, A1, pp, partial); break;
            case 4: hipLaunchKernelGGL((k_atmulti<4, false>), lane_grid(g, nlanes), b, 0, st, P, A1, pp, partial); break;
            case 6: hipLaunchKernelGGL((k_atmulti<6, false>), lane_grid(g, nlanes), b, 0, st, P, A1, pp, partial); break;
            default: throw HipError("atmulti: unsupported vector count");
        }
    }
    // tail: that many scalars directly behind the NV * LDV entries of `out` ride in the same all-reduce (row-sharded solves: a
    // scalar mailbox packed into the vector reduction that follows it -- one latency-bound collective less)
    // rn_bx != null: the residual r = rn_bx - G'v and its norm (Sc[rn_slot]) ride in k_gt_finish (unsharded solves)
    template <int NV>
    void apply_GT(const double* val, double* out, int tail = 0, const double* rn_bx = nullptr, double* rn_r = nullptr, int rn_slot = 0) {
        ++n_gtv;
        if (P.trig) {
            dim3 g(cdiv(P.D1, MPTS), cdiv(P.nchunk, P.cgrp)), b(256);
            const dim3 gf(cdiv(P.nfold, 256));
            // (pairs up to two operands: with four, the paired kernel's registers allow fewer waves than the unpaired one's -- DESIGN.md section 4)
            constexpr bool PAIR1 = NV <= 2, PAIR2 = 2 * NV <= 2;
            if (sw.fuse && lane_pairs() && (P.quad ? PAIR2 : PAIR1)) {
                const dim3 g2 = lane_grid(g, cdiv(nlanes, 2));
                ++n_pair;
                if constexpr (PAIR2) if (P.quad) hipLaunchKernelGGL(k_trig_moments_pair<2 * NV>, g2, b, 0, st, P, (const double2*)nullptr, P.seed_tau, P.D1, 0, partial, val, nlanes);
                if constexpr (PAIR1) if (!P.quad) hipLaunchKernelGGL(k_trig_moments_pair<NV>, g2, b, 0, st, P, (const double2*)nullptr, P.seed_tau, P.D1, 0, partial, val, nlanes);
            } else if (sw.fuse) {
                if (P.quad) hipLaunchKernelGGL((k_trig_moments<2 * NV, true>), lane_grid(g, nlanes), b, 0, st, P, (const double2*)nullptr, P.seed_tau, P.D1, 0, partial, val);
                else hipLaunchKernelGGL((k_trig_moments<NV, true>), lane_grid(g, nlanes), b, 0, st, P, (const double2*)nullptr, P.seed_tau, P.D1, 0, partial, val);
            } else if (P.quad) {
                hipLaunchKernelGGL((k_freq_fold<2 * NV, true>), lane_grid(gf, nlanes), b, 0, st, P, val, PPf);
                hipLaunchKernelGGL((k_trig_moments<2 * NV>), lane_grid(g, nlanes), b, 0, st, P, PPf, P.seed_tau, P.D1, 0, partial);
            } else {
                hipLaunchKernelGGL((k_freq_fold<NV, true>), lane_grid(gf, nlanes), b, 0, st, P, val, PPf);
                hipLaunchKernelGGL((k_trig_moments<NV>), lane_grid(g, nlanes), b, 0, st, P, PPf, P.seed_tau, P.D1, 0, partial);
            }
        } else {
            dim3 g(P.ld / 128, nsplit_at), b(64, 4);
            if (P.quad) hipLaunchKernelGGL((k_atmulti<2 * NV, true>), lane_grid(g, nlanes), b, 0, st, P, A1, val, partial);
            else hipLaunchKernelGGL((k_atmulti<NV, true>), lane_grid(g, nlanes), b, 0, st, P, A1, val, partial);
        }
        hipLaunchKernelGGL(k_gt_finish<NV>, lane_grid(dim3(cdiv(P.Nt, GTC) + 1), nlanes), dim3(GTC, GTG), 0, st, P, partial, P.trig ? cdiv(P.nchunk, P.cgrp) : nsplit_at, val, out,
                           GtResid{rn_bx, rn_r, Sc, rn_slot, gt_cnt});
        allreduce(out, (long)NV * P.LDV + tail, 0);       // sum the shards' G'v (N-space vectors are replicated)
    }
    template <int NV>
    void winv2(const double* in, const double* sub, double* out, int mode) {
        hipLaunchKernelGGL(k_winv2<NV>, lane_grid(dim3(cdiv(P.l + P.nq3, 256)), nlanes), dim3(256), 0, st, P, dl, w3, in, sub, out, mode);
        if (P.big) hipLaunchKernelGGL(k_big_winv2<NV>, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, wbb, Sc, in, sub, out, mode);
    }
    // Row-sharded solves on the lattice path: the normal matrix is a linear function of ~100 KB of trigonometric
    // moments, so the ranks all-reduce the MOMENTS (and the 3 x 3 y-y block); every rank holds the non-frequency rows
    // (replicated, program.h) and their scaling, so EVERY rank assembles and factorises the same H itself (round 4;
    // before, rank 0 alone did and shared each preconditioner application M'(M b) through a collective -- ~6 latency-bound
    // all-reduces per iteration): the factors are bit-identical across the ranks (same moments, same deterministic
    // assembly and factorisation), the solves with them are local.
    bool lead_factor() const { return shard_size > 1 && P.trig; }
    // (launch fusions of round 5, sw.fuse: results are bit-identical either way -- tests/test_switches_gpu.py)
    int* gt_cnt = nullptr;       // workgroups of the current k_gt_finish that are done (per lane; GtResid)
    // out = M' M (rhs + rhs2)
    template <int NV>
    void hsolve(const double* rhs, double* out, const double* rhs2 = nullptr) {
        if (fused_hsolve) {
            // one pass over the inverse factor (chol.hip k_hsolve); its partial vectors borrow the moment kernels'
            // partial buffer, which is idle between a G'v product and the next
            hsolve_launch(M, P.np, rhs, rhs2, out, partial, NV, P.LDV, st, nlanes, lane_bytes, P.mask);
        } else {
            trigemv_launch(M, P.np, 0, rhs, yN, NV, P.LDV, st, rhs2, nlanes, lane_bytes, P.mask);
            trigemv_launch(Mt, P.np, 1, yN, out, NV, P.LDV, st, nullptr, nlanes, lane_bytes, P.mask);
        }
    }
    // [0 G'; G -W^2][dx; dz] = [bx; bz]; gdx = G dx.  The Cholesky solve is refined by `nsweep`
    // iterations of preconditioned CG on (G' W^-2 G) dx = rhs with the operator applied exactly
    // through G (K1 + K3 passes) and M'M as preconditioner; dz and gdx are carried along, so the
    // dual equation G'dz = bx ends at the CG residual.  Residual norms n_0 (after the Cholesky solve)
    // .. n_nsweep go to Sc[slot ..] for the sweep controller.  Mirrors oracle/conic_ipm.py kkt_solve.
    // obs (test_unit_kkt; null in every solve): called on the host after each group of launches below with the group's number
    // (KKT_ST_*) and the sweep; obs->two_launch_cg runs the sweep's update in the row-sharded form on one rank
    template <int NV>
    void kkt_solve(const double* bx, const double* bz, double* dx, double* dz, double* gdx, int nsweep, int slot,
                   bool wbz_ready = false, const KktObserver* obs = nullptr) {
        // lock-step batch: nsweep is the largest count over the live lanes; mask row q switches off the lanes that
        // need fewer than q sweeps
        const dim3 gR = lane_grid(dim3(cdiv(P.R, 256)), nlanes), g1 = lane_grid(dim3(1), nlanes), b256(256);
        if (!wbz_ready) winv2<NV>(bz, nullptr, wbz, 0);
        else if (P.big) hipLaunchKernelGGL(k_big_winv2<NV>, g1, dim3(1024), 0, st, P, wbb, Sc, bz, nullptr, wbz, 0);
        if (obs) (*obs)(KKT_ST_WBZ, 0);
        apply_GT<NV>(wbz, tmpN);
        if (obs) (*obs)(KKT_ST_GTWBZ, 0);
        hsolve<NV>(bx, dx, tmpN);                                                           // M'M (bx + G' W^-2 bz)
        if (obs) (*obs)(KKT_ST_HSOLVE, 0);
        apply_G_winv2<NV>(dx, gdx, wbz, dz);
        if (obs) (*obs)(KKT_ST_GDX, 0);
        double* r = rhsN;
        if (sw.fuse && shard_size <= 1) apply_GT<NV>(dz, tmpN, 0, bx, r, slot);                       // G'dz ; r = bx - G'dz ; n_0
        else {
        apply_GT<NV>(dz, tmpN);
        hipLaunchKernelGGL(k_resid_norm<NV>, g1, dim3(SCAL_T), 0, st, P, bx, tmpN, r, Sc, slot);      // r = bx - G'dz ; n_0
        }
        if (obs) (*obs)(KKT_ST_RESID, 0);
        if (nsweep <= 0) return;
        const int* live = P.mask;
        P.mask = mask_row(1);
        // z = M'M r and the start of the sweep (rz, beta, p): the partial vectors of the one-pass product are added by the kernel
        // that starts the sweep (sw.fuse; otherwise k_hsolve_fold writes z and k_cg_start reads it)
        auto z_and_start = [&](int first) {
            if (sw.fuse && fused_hsolve) {
                hsolve_launch(M, P.np, r, nullptr, tmpN2, partial, NV, P.LDV, st, nlanes, lane_bytes, P.mask, false);
                // (one workgroup per vector; the row-sharded form keeps the one workgroup it had)
                hipLaunchKernelGGL(k_fold_cg_start<NV>, lane_grid(dim3(shard_size <= 1 ? NV : 1), nlanes), dim3(1024), 0, st, P, Sc, r, partial, pN, first);
            } else {
                hsolve<NV>(r, tmpN2);
                hipLaunchKernelGGL(k_cg_start<NV>, g1, dim3(SCAL_T), 0, st, P, Sc, r, tmpN2, pN, first);
            }
        };
        z_and_start(1);
        if (obs) (*obs)(KKT_ST_START, 0);
        const bool one_launch = shard_size == 1 && !(obs && obs->two_launch_cg);
        for (int it = 0; it < nsweep; ++it) {
            P.mask = mask_row(it + 1);
            apply_G_winv2<NV>(pN, tmpR, nullptr, wpR);                                      // G p, W^-2 G p
            if (obs) (*obs)(KKT_ST_GP, it);
            apply_GT<NV>(wpR, tmpN);                                                        // H p
            if (obs) (*obs)(KKT_ST_HP, it);
            if (one_launch) {
                hipLaunchKernelGGL(k_cg_step_update<NV>, gR, b256, 0, st, P, Sc, pN, tmpN, dx, r, slot + it + 1, tmpR, wpR, gdx, dz);
            } else {
                hipLaunchKernelGGL(k_cg_step<NV>, g1, dim3(SCAL_T), 0, st, P, Sc, pN, tmpN, dx, r, slot + it + 1);   // alpha, dx, r, n_{it+1}
                hipLaunchKernelGGL(k_cg_update_r<NV>, gR, b256, 0, st, P, Sc, tmpR, wpR, gdx, dz);
            }
            if (obs) (*obs)(KKT_ST_STEP, it);
            if (it + 1 < nsweep) { P.mask = mask_row(it + 2); z_and_start(0); if (obs) (*obs)(KKT_ST_RESTART, it); }
        }
        P.mask = live;
    }
    // Extended-precision solve, step 1 (after the NT scaling): eigen data, cap, strong set.  Returns the number of
    // strong eigen-directions (0: nothing above the cap, the plain solve is exact enough).  One host
    // synchronisation (the count decides which solve runs).
    // Lock-step units (round 5): every live lane selects ITS strong set (its own cap, its own count); ks[b] <- the lane's count,
    // thetas[b] the lane's cap factor (raised x 100 for a lane whose set does not fit, as in its single solve).  Returns the largest.
    // the selection's first step (k_dd_prep, and the big cone's row 0): returns the partial rows k_dd_select folds
    int dd_prep_launch() {
        hipLaunchKernelGGL(k_dd_prep, lane_grid(dim3(std::max(nbC, 1)), nlanes), dim3(256), 0, st, P, dl, w3, D, partR);
        if (P.big) hipLaunchKernelGGL(k_dd_prep_big, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, wbb, Sc, D, partR);      // (row 0: see k_dd_prep)
        return std::max(nbC, 1) + (P.big ? 1 : 0);
    }
    int dd_prepare_lanes(const double theta0, int* ks, const bool* live) {
        const int nb = std::max(nbC, 1), nbp = dd_prep_launch();
        for (int b = 0; b < nlanes; ++b) hostTheta[b] = theta0;
        const int kmax_fit = cap_form ? CAP_KMAX : DD_KMAX;
        for (int attempt = 0; attempt < 8; ++attempt) {
            if (attempt > 0) memset_lanes(D.kcnt, sizeof(int));
            MBFIR_HIP(hipMemcpyAsync(ddtheta, hostTheta, sizeof(double) * nlanes, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_dd_select, lane_grid(dim3(nb), nlanes), dim3(256), 0, st, P, dl, D, partR, nbp, theta0, (const double*)ddtheta);
            hipLaunchKernelGGL(k_dd_order, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, D);
            MBFIR_HIP(hipMemcpy2DAsync(hostFlag + MAX_LANES, sizeof(int), D.kcnt, lane_bytes, sizeof(int), nlanes, hipMemcpyDeviceToHost, st));
            MBFIR_HIP(hipStreamSynchronize(st));
            bool fits = true;
            int kmax = 0;
            for (int b = 0; b < nlanes; ++b) {
                ks[b] = live[b] ? hostFlag[MAX_LANES + b] : 0;
                if (ks[b] > kmax_fit) { fits = false; hostTheta[b] *= 100.0; }
                kmax = std::max(kmax, ks[b]);
            }
            dd_attempts = attempt + 1;
            if (fits) return kmax;
        }
        throw HipError("extended-precision solve: strong set does not fit");
    }
    double hostTheta[MAX_LANES];        // the lanes' cap factors as the last selection used them
    int dd_attempts = 0;                // ... and the number of selections it took
    double* ddtheta = nullptr;          // the lanes' cap factors (lane 0's arena; read unshifted)
    bool dd_unit = false;               // a lock-step unit on the extended-precision path (some of its lanes, some iterations)
    int dd_kp = 0;                      // ... the largest strong set of this iteration, rounded up to 64 (the unit's S is dd_kp x dd_kp)
    int dd_prepare(double theta) {
        const int nb = std::max(nbC, 1), nbp = dd_prep_launch();
        for (int attempt = 0; attempt < 8; ++attempt) {
            if (attempt > 0) hipMemsetAsync(D.kcnt, 0, sizeof(int), st);        // (the first attempt's counter was cleared by k_dd_prep)
            hipLaunchKernelGGL(k_dd_select, lane_grid(dim3(nb), nlanes), dim3(256), 0, st, P, dl, D, partR, nbp, theta, (const double*)nullptr);
            hipLaunchKernelGGL(k_dd_order, dim3(1), dim3(1024), 0, st, P, D);
            MBFIR_HIP(hipMemcpyAsync(hostFlag + 1, D.kcnt, sizeof(int), hipMemcpyDeviceToHost, st));
            MBFIR_HIP(hipStreamSynchronize(st));
            hostTheta[0] = theta; dd_attempts = attempt + 1;  // (test_unit_ddkkt reports them)
            if (hostFlag[1] <= (cap_form ? CAP_KMAX : DD_KMAX)) return hostFlag[1];
            theta *= 100.0;                                   // more strong directions than U has rows (or than S takes): raise the cap
        }
        throw HipError("extended-precision solve: strong set does not fit");
    }
    // [0 G'; G -W^2][dx; dz] = [bx; bz] by iterative refinement around the double-double normal-equation solve
    // (mirrors oracle/conic_ipm.py kkt_solve_dd, nref = 2).  Residual norms ||bx - G'dz|| before each pass go
    // to Sc[slot ..].
    // obs (test_unit_ddkkt; null in every solve): called on the host after each group of launches below with the group's number
    // (DD_ST_*) and the pass
    template <int NV>
    void kkt_solve_dd(const double* bx, const double* bz, double* dx, double* dz, double* gdx, int slot, const KktObserver* obs = nullptr) {
        const dim3 gC(std::max(nbC, 1)), b256(256);
        // (lock-step units: the launches carry the unit's largest strong set, every lane reads its own count from its arena)
        const int k = dd_unit ? dd_kp : dd_k;
        const int* kcnt = dd_unit ? D.kcnt : nullptr;
        double *Bh = ddB, *Bl = ddB + 2L * P.LDV;
        // (one launch instead of three memsets: the trace of BASELINE config 3's batch held 10 348 fill kernels)
        hipLaunchKernelGGL(k_zero3, lane_grid(dim3(cdiv(NV * std::max<long>(P.LDV, P.Rp), 256)), nlanes), dim3(256), 0, st, dx, long(NV) * P.LDV, dz, long(NV) * P.Rp, gdx, long(NV) * P.Rp,
                           lane_bytes, P.mask);
        for (int it = 0; it < dd_passes; ++it) {
            apply_GT<NV>(dz, tmpN);
            hipLaunchKernelGGL(k_resid_norm<NV>, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, bx, tmpN, rhsN, Sc, slot + it);   // r1 = bx - G'dz
            if (obs) (*obs)(DD_ST_R1, it);
            hipLaunchKernelGGL(k_dd_r2<NV>, lane_grid(gC, nlanes), b256, 0, st, P, D, dl, bz, gdx, dz, tmpR, ddtS);                  // r2, t
            if (P.big) hipLaunchKernelGGL(k_dd_r2_big<NV>, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, D, bz, gdx, dz, tmpR, ddtS, scratch);
            if (obs) (*obs)(DD_ST_R2, it);
            hipLaunchKernelGGL(k_dd_winv2c<NV>, lane_grid(gC, nlanes), b256, 0, st, P, D, tmpR, (const double*)nullptr, wbz);
            if (P.big) hipLaunchKernelGGL(k_dd_winv2c_big<NV>, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, D, tmpR, (const double*)nullptr, wbz, scratch);
            if (obs) (*obs)(DD_ST_WBZ, it);
            apply_GT<NV>(wbz, tmpN2);
            if (obs) (*obs)(DD_ST_GTW, it);
            if (cap_form) {
                // y = H_w^-1 rhs_w ; zeta = S^-1 (U y - t) ; dx = y - Zt' zeta   (all double; zeta are the strong directions'
                // multipliers X (U dx - t) themselves)
                int kp = int(round_up(k, 64));
                if (!dd_unit) kp = std::max(kp, sw.test_cap_kp);                                 // test hook: pad S as a unit's largest lane would
                cap_add_launch(rhsN, tmpN2, Bl, P.N, P.np, P.LDV, NV, st, nlanes, lane_bytes, P.mask);                       // rhs_w
                if (obs) (*obs)(DD_ST_RHS, it);
                double* yv = tmpN2;                                                              // (free from here on; yN is hsolve's own intermediate)
                hsolve<NV>(Bl, yv);                                                              // y
                if (obs) (*obs)(DD_ST_Y, it);
                cap_uy_launch(D.U, k, kp, P.N, P.np, yv, P.LDV, ddtS, capw, DD_KMAX, NV, st, nlanes, lane_bytes, P.mask, kcnt);
                if (obs) (*obs)(DD_ST_CAPW, it);
                hsolve_launch(capMs, kp, capw, nullptr, ddzeta, partial, NV, DD_KMAX, st, nlanes, lane_bytes, P.mask);       // zeta
                if (obs) (*obs)(DD_ST_ZETAC, it);
                cap_dx_launch(capZt, k, P.N, P.np, ddzeta, DD_KMAX, yv, Bh, P.LDV, NV, st, nlanes, lane_bytes, P.mask, kcnt);      // the correction of this pass
            } else {
            hipLaunchKernelGGL(k_dd_rhs<NV>, lane_grid(dim3(cdiv(P.np, 16)), nlanes), b256, 0, st, P, D, k, rhsN, tmpN2, ddtS, Bh, Bl);
            if (obs) (*obs)(DD_ST_RHS, it);
            dd_trsv_launch(H, M, Mt, W1, ddri, ddri + P.np, P.np, Bh, Bl, NV, P.LDV, st, ddflags, ++dd_epoch, flag, ddinv);
            }
            if (obs) (*obs)(DD_ST_SOLVE, it);
            apply_G<NV>(Bh, wpR);
            if (obs) (*obs)(DD_ST_GBH, it);
            hipLaunchKernelGGL(k_dd_winv2c<NV>, lane_grid(gC, nlanes), b256, 0, st, P, D, wpR, tmpR, wbz);
            if (P.big) hipLaunchKernelGGL(k_dd_winv2c_big<NV>, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, D, wpR, tmpR, wbz, scratch);
            if (obs) (*obs)(DD_ST_WBZ2, it);
            if (!cap_form) hipLaunchKernelGGL(k_dd_zeta<NV>, lane_grid(dim3(k), nlanes), dim3(64), 0, st, P, D, Bh, Bl, ddtS, ddzeta);
            if (obs && !cap_form) (*obs)(DD_ST_ZETA, it);
            hipLaunchKernelGGL(k_dd_accum<NV>, lane_grid(gC, nlanes), b256, 0, st, P, D, wbz, wpR, ddzeta, dz, gdx);
            if (P.big) hipLaunchKernelGGL(k_dd_accum_big<NV>, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, D, wbz, wpR, ddzeta, dz, gdx);
            hipLaunchKernelGGL(k_dd_accum_x<NV>, lane_grid(dim3(nbN), nlanes), b256, 0, st, P, Bh, dx);
            if (obs) (*obs)(DD_ST_ACCUM, it);
        }
    }
    // H = G' W^-2 G from the current scaling, then Cholesky + inverse.  Timing events are pooled
    // and read once at the end of the solve, so measuring does not serialise the host.
    bool timing = true;
    std::vector<hipEvent_t> evpool;
    size_t evused = 0;
    std::vector<hipEvent_t> capev;       // (begin, end) pairs around the capacitance form's products
    size_t capev_used = 0;
    double cap_flop_sum = 0;
    hipEvent_t next_cap_event() {
        if (capev_used == capev.size()) {
            hipEvent_t e;
            MBFIR_HIP(hipEventCreate(&e));
            capev.push_back(e);
        }
        return capev[capev_used++];
    }
    hipEvent_t next_event() {
        if (evused == evpool.size()) {
            hipEvent_t e;
            MBFIR_HIP(hipEventCreate(&e));
            evpool.push_back(e);
        }
        return evpool[evused++];
    }
    // ddk > 0: this iteration runs the extended-precision solve -- H_w from the capped weights (D.dlc, D.m3c),
    // then H = H_w + U'XU and its Cholesky factor in double-double
    double* H_keep = nullptr;    // test_unit_ops: where build_H copies the lanes' H (np x np each, one after the other) ahead of the factorisation
    bool h_one_pass = false;     // the last build_H took its one_pass branch
    double* capS_keep = nullptr; // test_unit_ddkkt: where build_H copies the lanes' capacitance matrices (kp x kp each) ahead of their factorisation
    void build_H(int ddk = 0) {
        double* yy_sum = nullptr;
        const double* dlw = ddk > 0 ? D.dlc : dl;
        const double* m3c = ddk > 0 ? D.m3c : nullptr;
        // (lock-step unit with lanes in both modes: the kernels pick per lane -- DProg::plain_weights)
        const int* live_mask = P.mask;
        P.dd_lane = (dd_unit && ddk > 0) ? mask_row(ROW_DD) : nullptr;
        P.dl_plain = P.dd_lane ? dl : nullptr;
        const int nwv = P.quad ? 3 : 1, nvb = P.quad ? 2 * P.Ne : P.Ne;
        const bool one_pass = P.trig && P.Ne > 0 && P.tmin == 0.0 && nwv + nvb <= 4;
        h_one_pass = one_pass;
        if (!one_pass) hipLaunchKernelGGL(k_freq_blocks, lane_grid(dim3(cdiv(P.Mf, 256)), nlanes), dim3(256), 0, st, P, dlw, w3, Dw, BB, m3c);
        hipEvent_t g0 = timing ? next_event() : nullptr, g1 = timing ? next_event() : nullptr;
        if (P.trig) {
            if (g0) hipEventRecord(g0, st);
            const double* momb = MomB;
            if (one_pass) {
                // delays start at 0: the border moments sit on the difference progression, one moment launch does both,
                // and the per-frequency blocks go straight into its folded operands (no Dw / BB round trip)
                hipLaunchKernelGGL(k_freq_blocks_fold, lane_grid(dim3(cdiv(P.nfold, 256)), nlanes), dim3(256), 0, st, P, dlw, w3, m3c, nwv + nvb, PPf);
                // (the border operands, behind the nwv weight operands, only where k_assemble_H_lat reads their moments: sw.fuse, unsharded --
                //  a row-sharded build all-reduces the whole of Mom)
                moments_array(nwv + nvb, nullptr, P.seed_h, P.D1, 2 * P.D1 - 1, Mom, (sw.fuse && shard_size <= 1) ? nwv : 0);
                momb = Mom + 2L * nwv * P.LDM;
            } else {
                moments_array(nwv, Dw, P.seed_h, P.D1, 2 * P.D1 - 1, Mom);
                if (P.Ne > 0) moments_array(nvb, BB, P.seed_tau, P.D1, 0, MomB);
            }
            if (lead_factor()) {
                // the 3 x 3 y-y block -- terms of the (sharded) frequency rows' rho / delta columns and of replicated rows, the
                // latter counted on their owner -- is summed over the ranks too: in the tail of the moment buffer when the
                // moments go in one piece (one collective for both), else in its own small all-reduce
                yy_sum = nullptr;
                if (momb == MomB) {
                    allreduce(Mom, 2L * nwv * P.LDM, 0);
                    if (P.Ne > 0) allreduce(MomB, 2L * nvb * P.LDM, 0);
                } else {
                    long cnt = 2L * (nwv + nvb) * P.LDM;
                    if (P.Ne > 0 && cnt + 16 <= 18L * P.LDM) {
                        yy_sum = Mom + cnt;
                        hipMemsetAsync(yy_sum, 0, sizeof(double) * 9, st);
                        if (P.nyrows > 0) hipLaunchKernelGGL(k_H_yy, lane_grid(dim3(1), nlanes), dim3(256), 0, st, P, dlw, w3, yy_sum, 3L, 0L, m3c);
                        cnt += 9;
                    }
                    allreduce(Mom, cnt, 0);
                }
            }
            hipLaunchKernelGGL(k_assemble_H_lat, lane_grid(dim3((P.np / 64) * (P.np / 64 + 1) / 2, 16), nlanes), dim3(256), 0, st, P, Mom, momb, H, 1.0);
            if (g1) hipEventRecord(g1, st);
        } else {
        // the dense Gram products, one lane after the other (a k_gram launch fills the chip by itself: 340 us at the
        // headline size); the lanes the host knows to be finished are skipped
        // (one design: the events bracket the k_gram launches ALONE -- what a kernel trace reports for the kernel north_star
        //  grades; round 3 bracketed the split-K fold and the gaps between the launches too, 0.368 against 0.334 ms in the profile.
        //  Lock-step lanes: around the lanes' products together)
        if (ar_overlap) {
            // chunk c: product + fold into the packed tiles on st; its all-reduce on st2 as soon as the fold is done, while st goes on
            // with chunk c + 1.  (The events bracket all of it: the product is no longer one stretch of k_gram launches.)
            if (g0) hipEventRecord(g0, st);
            if (!st2) MBFIR_HIP(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
            while (ovev.size() < 2 * gchunks.size()) { hipEvent_t e; MBFIR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); ovev.push_back(e); }
            for (size_t c = 0; c < gchunks.size(); ++c) {
                const GramChunk& ck = gchunks[c];
                gram_chunk_launch(gps[0], ck, A1, Dw, slab, tile_ij, chunk_tab, Tp, st);
                if (shard_size > 1) {
                    MBFIR_HIP(hipEventRecord(ovev[2 * c], st));
                    MBFIR_HIP(hipStreamWaitEvent(st2, ovev[2 * c], 0));
                    allreduce(Tp + (size_t)ck.plo * 16384, (long)(ck.phi - ck.plo) * 16384, 0, st2);
                    MBFIR_HIP(hipEventRecord(ovev[2 * c + 1], st2));
                }
            }
            if (g1) hipEventRecord(g1, st);
        } else if (nlanes == 1) gram_launch(gps[0], A1, Dw, slab, T, tile_ij, st, g0, g1, P.Mpad);
        else {
        if (g0) hipEventRecord(g0, st);
        for (int b = 0; b < nlanes; ++b) {
            if (nlanes > 1 && !lane_live[b]) continue;
            const size_t off = (size_t)b * lane_bytes;
            auto at = [&](double* p) { return reinterpret_cast<double*>(reinterpret_cast<char*>(p) + off); };
            // (a lane's own plan: the split of its frequency rows over the workgroups is that of its single solve)
            gram_launch(gps[b], at(A1), at(Dw), at(slab), at(T), reinterpret_cast<const int*>(reinterpret_cast<const char*>(tile_ij) + off), st, nullptr, nullptr, P.Mpad);
        }
        if (g1) hipEventRecord(g1, st);
        }
        if (P.Ne > 0) {
            int nvv = P.quad ? 2 * P.Ne : P.Ne;
            atmulti_array(nvv, BB);
            hipLaunchKernelGGL(k_fold_partials, lane_grid(dim3(cdiv(P.ld, FPC), nvv), nlanes), dim3(FPC, 16), 0, st, partial, nsplit_at, nvv, P.ld, P.LDV, TT, lane_bytes, P.mask, P.dims, -AT_ROWS);
        }
        if (ar_overlap) {
            // the small ingredients in one collective (border products, and behind them the 3 x 3 y-y block as in the lattice
            // mode), issued while the last chunks are still on their way; then wait for the chunks and spread the tiles into T
            if (P.Ne > 0) {
                yy_sum = TT + (size_t)P.Ne * P.LDV;
                hipMemsetAsync(yy_sum, 0, sizeof(double) * 9, st);
                if (P.nyrows > 0) hipLaunchKernelGGL(k_H_yy, lane_grid(dim3(1), nlanes), dim3(256), 0, st, P, dlw, w3, yy_sum, 3L, 0L, m3c);
            }
            if (shard_size > 1) {
                MBFIR_HIP(hipStreamWaitEvent(st, ovev[2 * gchunks.size() - 1], 0));      // (st2 runs the chunks in order: the last one's event covers them all)
                if (P.Ne > 0) allreduce(TT, (long)P.Ne * P.LDV + 9, 0);
            }
            gram_unpack_launch(gps[0], Tp, tile_ij, chunk_tab, T, st);
        }
        hipLaunchKernelGGL(k_assemble_H, lane_grid(dim3(cdiv(P.np, 256), P.np), nlanes), dim3(256), 0, st, P, T, TT, H, (ar_overlap || shard_rank == 0) ? 1.0 : 0.0);
        }
        const bool summed = shard_size > 1 && !lead_factor() && !ar_overlap;     // dense row-sharded path: H is summed over the ranks below
        if (ar_overlap && P.Ne > 0) hipLaunchKernelGGL(k_H_yy_add, lane_grid(dim3(1), nlanes), dim3(16), 0, st, P, yy_sum, H);
        if (lead_factor() && P.Ne > 0) {
            // (summed over the ranks -- with the moments above, or here -- then added by every rank to its own H)
            const double* yy = yy_sum;
            if (!yy) {
                hipMemsetAsync(RB, 0, sizeof(double) * 9, st);
                if (P.nyrows > 0) hipLaunchKernelGGL(k_H_yy, lane_grid(dim3(1), nlanes), dim3(256), 0, st, P, dlw, w3, RB, 3L, 0L, m3c);
                allreduce(RB, 9, 0);
                yy = RB;
            }
            hipLaunchKernelGGL(k_H_yy_add, lane_grid(dim3(1), nlanes), dim3(16), 0, st, P, yy, H);
        }
        {
            // identity rows (all of them replicated rows): every rank adds them to its own H; where H is summed over the ranks
            // afterwards (dense path) the owner alone does, and the y-y block (last block of the grid) weights the replicated rows
            const int yy_too = (!lead_factor() && !ar_overlap && P.Ne > 0 && P.nyrows > 0) ? 1 : 0;
            hipLaunchKernelGGL(k_H_identity, lane_grid(dim3(cdiv(P.Nt, 256) + yy_too), nlanes), dim3(256), 0, st, P, dlw, w3, H, m3c, yy_too, summed ? 1 : 0);
            if (P.big && (!summed || shard_rank == 0)) {
                memset_lanes(qv, sizeof(double) * 3 * P.LDV);
                if (ddk > 0) {
                    if (dd_unit) P.mask = mask_row(ROW_DD);
                    hipLaunchKernelGGL(k_big_q_dd, lane_grid(dim3(cdiv(P.big, 256)), nlanes), dim3(256), 0, st, P, D, qv, qv + P.LDV, qv + 2L * P.LDV);
                    hipLaunchKernelGGL(k_H_big_dd, lane_grid(dim3(cdiv(P.N, 256), P.N), nlanes), dim3(256), 0, st, P, D, qv, qv + P.LDV, qv + 2L * P.LDV, H);
                }
                if (ddk <= 0 || dd_unit) {
                    if (dd_unit && ddk > 0) P.mask = mask_row(ROW_PL);
                    hipLaunchKernelGGL(k_big_q, lane_grid(dim3(cdiv(P.big, 256)), nlanes), dim3(256), 0, st, P, wbb, qv, qv + P.LDV);
                    hipLaunchKernelGGL(k_H_big, lane_grid(dim3(cdiv(P.N, 256), P.N), nlanes), dim3(256), 0, st, P, qv, qv + P.LDV, Sc, H);
                }
                P.mask = live_mask;
            }
        }
        if (!lead_factor() && !ar_overlap && shard_size > 1) {
            // dense path: sum the shards' normal matrices -- the packed lower triangle (M, rewritten by the factorisation that
            // follows, is the staging buffer), in AR_CHUNKS collectives so that a ring's pipeline starts on the first tile rows
            // while the later ones are still queued behind it (MBFIR_AR_CHUNKS; 1 = one collective)
            const long nb = P.np / 64, ntile = nb * (nb + 1) / 2;
            hipLaunchKernelGGL(k_pack_tril, dim3((unsigned)ntile), dim3(256), 0, st, H, P.np, M, 0);
            const int chunks = int(std::min<long>(sw.ar_chunks > 0 ? sw.ar_chunks : 4, ntile));              // (read once at solve start: every rank must issue the same number of collectives)
            for (int c = 0; c < chunks; ++c) {
                const long lo = ntile * c / chunks, hi = ntile * (c + 1) / chunks;
                allreduce(M + lo * 4096, (hi - lo) * 4096, 0);
            }
            hipLaunchKernelGGL(k_pack_tril, dim3((unsigned)ntile), dim3(256), 0, st, H, P.np, M, 1);
        }
        // (test_unit_ops: every lane's H as the factorisation is about to find it)
        if (H_keep) MBFIR_HIP(hipMemcpy2DAsync(H_keep, sizeof(double) * P.np * P.np, H, nlanes > 1 ? lane_bytes : sizeof(double) * P.np * P.np,
                                               sizeof(double) * P.np * P.np, nlanes, hipMemcpyDeviceToDevice, st));
        hipEvent_t c0 = timing ? next_event() : nullptr, c1 = timing ? next_event() : nullptr;
        P.dd_lane = nullptr; P.dl_plain = nullptr;
        if (ddk > 0 && cap_form) {
            // capacitance form: the ordinary double-precision factorisation of H_w, then Yt = U M', Zt = Yt M, S = Yt Yt' + X^-1
            // on the matrix cores and the same factorisation routine on S (kp x kp).  A unit (dd_unit): the lanes' H (capped weights
            // on the lanes in the extended-precision mode, plain ones on the others) in one launch, then the capacitance matrices of
            // the former: launches sized to the unit's largest strong set, a lane's own count read from its arena, its U / Yt / Zt
            // rows and S rows beyond it zero resp. unit -- what a single solve padded to that size would hold
            const int kp = dd_unit ? dd_kp : std::max(int(round_up(ddk, 64)), sw.test_cap_kp);
            const size_t lb = dd_unit ? lane_bytes : 0;
            const int* mdd = mask_row(ROW_DD);                // (one design: no masks)
            chol_launch_count += chol_inv_launch(H, M, fused_hsolve ? nullptr : Mt, W1, P.np, flag, st, sw.chol_split, sw.poison, nullptr, c0, nullptr, nlanes, lb, P.mask);
            P.mask = mdd;
            hipLaunchKernelGGL(k_dd_rows, lane_grid(dim3(kp), nlanes), dim3(256), 0, st, P, D, P.np, dd_unit ? -1 : ddk);      // (one design: rows ddk .. kp-1 zero padding)
            P.mask = live_mask;
            hipEvent_t b0 = timing ? next_cap_event() : nullptr, b1 = timing ? next_cap_event() : nullptr;
            if (b0) hipEventRecord(b0, st);
            cap_build_launch(D.U, dd_unit ? kp : ddk, kp, P.np, M, D.sX, capYt, capZt, capS, capPart, st, nlanes, lb, mdd, dd_unit ? D.kcnt : nullptr);
            if (b1) hipEventRecord(b1, st);
            // (test_unit_ddkkt: every lane's S as its factorisation is about to find it -- the factorisation works in place)
            if (capS_keep) MBFIR_HIP(hipMemcpy2DAsync(capS_keep, sizeof(double) * kp * kp, capS, nlanes > 1 ? lane_bytes : sizeof(double) * kp * kp,
                                                      sizeof(double) * kp * kp, nlanes, hipMemcpyDeviceToDevice, st));
            // Yt and Zt: kp x np x np / 2 multiply-adds each (triangular M); S: kp x kp x np / 2 (lower tiles)
            cap_flop_sum += 2.0 * (double(kp) * P.np * P.np + 0.5 * double(kp) * kp * P.np);
            chol_inv_launch(capS, capMs, nullptr, capW1, kp, capflag, st, sw.chol_split, sw.poison, nullptr, nullptr, c1, nlanes, lb, mdd);
            cap_flag_add_launch(flag, capflag, st, nlanes, lb, mdd);      // pivots replaced in either factorisation count (oracle: chol_fixes += nfs)
        } else if (ddk > 0) {
            if (c0) hipEventRecord(c0, st);
            hipLaunchKernelGGL(k_dd_rows, lane_grid(dim3(ddk), nlanes), dim3(256), 0, st, P, D, P.np, ddk);
            dd_syrk_launch(D.U, P.np, D.sX, D.kcnt, P.np, H, M, st);
            dd_chol_launch(H, M, Mt, W1, ddri, ddri + P.np, ddd0, P.np, DD_PIVTOL, flag, st, ddinv);
            if (c1) hipEventRecord(c1, st);
        } else {
            // (with the one-pass M'(M b) nobody reads the transpose: it is not written)
            chol_launch_count += chol_inv_launch(H, M, fused_hsolve ? nullptr : Mt, W1, P.np, flag, st, sw.chol_split, sw.poison, nullptr, c0, c1, nlanes, lane_bytes, P.mask);
        }
    }
    // ---- the stages of Solver::solve_lanes ----------------------------------------------------------------------------------
    // Lane preparation: every lane's program (its row shard when sharded), the WHOLE program's norms, index structures, lattice.
    void prepare_lanes(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, std::vector<LaneHost>& LH) {
        // ---- row sharding: this process keeps the frequencies i % size == rank (program.h) ----------
        shard_rank = o.shard_size > 1 ? o.shard_rank : 0;
        shard_size = o.shard_size > 1 ? o.shard_size : 1;
        if (shard_size > 1 && !ar_fn && !comm) throw HipError("row-sharded solve without a communicator or an all-reduce hook");
        if (comm && shard_size > 1 && (comm_size != shard_size || comm_rank != shard_rank))
            throw HipError("row-sharded solve: shard_rank / shard_size differ from the RCCL communicator's");
        n_collectives = 0; collective_bytes = 0;
        n_gv = 0; n_gtv = 0; n_pair = 0;
        if (shard_size > 1 && nlanes > 1) throw ShapeError("row-sharded solves run one design at a time");
        for (int b = 0; b < nlanes; ++b) {
            LaneHost& L = LH[b];
            const TrigProgram& Qfull = *Qs[b];
            if (shard_size > 1) { L.local = shard_program(Qfull, shard_rank, shard_size); L.Q = &L.local; }
            else L.Q = &Qfull;
            // constants of the WHOLE program (identical on every shard)
            double nh = 0, nc = 0;
            for (double v : Qfull.h) nh += v * v;
            for (double v : Qfull.c) nc += v * v;
            L.nrm_h = std::max(1.0, std::sqrt(nh)); L.nrm_c = std::max(1.0, std::sqrt(nc));
            L.degree = double(Qfull.l + Qfull.nq3 + (Qfull.big ? 1 : 0));
            // (the extended-precision KKT solve forms its strong rows from the exact w_i: its programs keep every frequency
            // on its own so that the lattice operator and those rows see the same grid to the old 2 ulp)
            L.prep = lane_prep(*L.Q, o, sw);
            L.Lt = L.prep->Lt;
            L.nsweep = o.refine; L.nsweep_ctl = o.refine;
        }
        if (shard_size > 1 && !o.dense_trig) {
            // every rank must take the same path (it selects the sequence and the sizes of the collectives): the
            // lattice path only if EVERY shard has the structure -- a min all-reduce of the local verdicts
            ensure_arena(4096);
            double* dv = reinterpret_cast<double*>(ar.base);
            hostSc[0] = LH[0].Lt.ok ? -1.0 : 0.0;                // min(v) = -max(-v); the collective knows sum and max
            MBFIR_HIP(hipMemcpyAsync(dv, hostSc, sizeof(double), hipMemcpyHostToDevice, st));
            allreduce(dv, 1, 1);
            MBFIR_HIP(hipMemcpyAsync(hostSc, dv, sizeof(double), hipMemcpyDeviceToHost, st));
            MBFIR_HIP(hipStreamSynchronize(st));
            if (hostSc[0] > -0.5) LH[0].Lt = LatticeInfo();      // somebody lacks it: dense path everywhere
        }
    }
    // Unit planning: the lanes share one CLASS (designer, slack columns, cone kinds, lattice origin); their grids, row counts, chunk
    // lists and orders may differ: arrays and launches are sized to the unit's maxima, every lane carries its
    // own dimensions (DProg::dims).  Also the Gram plans and the unit's solve forms.
    UnitPlan plan_unit(const std::vector<LaneHost>& LH, const SolveOpts& o) {
        const TrigProgram& Q = *LH[0].Q;
        const LatticeInfo& Lt = LH[0].Lt;
        int Mf_max = Q.Mf, R_max = Q.R, l_max = Q.l, nyrows_max = int(LH[0].prep->yrows.size());
        int Nt_max = Q.Nt, nq3_max = Q.nq3, big_max = Q.big, D1_max = Lt.D1, n_max = Q.n;
        size_t nchunk_max = Lt.ch_start.size(), nfold_max = Lt.wf.size();
        bool hetero = false, orders = false;
        for (int b = 1; b < nlanes; ++b) {
            const TrigProgram& Qb = *LH[b].Q;
            const LatticeInfo& Lb = LH[b].Lt;
            if (Qb.which != Q.which || Qb.Ne != Q.Ne || (Qb.nq3 > 0) != (Q.nq3 > 0) || (Qb.big > 0) != (Q.big > 0) || Qb.quad != Q.quad ||
                Lb.ok != Lt.ok || (Lb.tmin == 0.0) != (Lt.tmin == 0.0))
                throw ShapeError("lock-step batch: lanes differ in class (designer, slack columns, cone kinds, lattice origin at zero or not)");
            if (Qb.n != Q.n || Qb.Nt != Q.Nt || Qb.nq3 != Q.nq3 || Qb.big != Q.big || Lb.D1 != Lt.D1 || Lb.tmin != Lt.tmin || LH[b].prep->c_rows.size() != LH[0].prep->c_rows.size())
                hetero = orders = true;
            if (Qb.Mf != Q.Mf || Qb.R != Q.R || Qb.l != Q.l || LH[b].prep->yrows.size() != LH[0].prep->yrows.size() || Lb.ch_start.size() != Lt.ch_start.size() ||
                Lb.wf.size() != Lt.wf.size())
                hetero = true;
            Mf_max = std::max(Mf_max, Qb.Mf); R_max = std::max(R_max, Qb.R); l_max = std::max(l_max, Qb.l);
            nyrows_max = std::max(nyrows_max, int(LH[b].prep->yrows.size()));
            nchunk_max = std::max(nchunk_max, Lb.ch_start.size()); nfold_max = std::max(nfold_max, Lb.wf.size());
            Nt_max = std::max(Nt_max, Qb.Nt); nq3_max = std::max(nq3_max, Qb.nq3); big_max = std::max(big_max, Qb.big);
            D1_max = std::max(D1_max, Lb.D1); n_max = std::max(n_max, Qb.n);
        }
        auto seg_of = [](int D1) { return std::min(SEGMAX, std::max(64, int(round_up(cdiv(std::max(D1, 1), 16), 8)))); };
        // what the per-lane dimensions do not cover: different ORDERS on the dense path (the row stride of A1 follows the order).
        // Different band edges are fine there too since round 5: every lane runs its own Gram plan and folds its own split partials.
        if (orders && (!Lt.ok || o.dense_trig)) throw ShapeError("lock-step batch: lanes differ in order (dense path)");
        // ---- sizes -----------------------------------------------------------------------------
        UnitPlan U;
        const int R = R_max, Nt = Nt_max, Ne = Q.Ne, N = Nt_max + Q.Ne, Mf = Mf_max;
        const int nw = Q.quad ? 3 : 1;
        // (dense row-sharded build with the chunked, overlapped all-reduce: see Impl::ar_overlap)
        ar_overlap = !Lt.ok && nw == 1 && nlanes == 1 && ((shard_size > 1 && sw.ar_overlap != 0) || sw.ar_overlap == 2);
        // (chunks: MBFIR_AR_CHUNKS, else one per 32 tiles, at most 8 -- below that a chunk's product is too short to hide a collective behind)
        const int gtiles = gram_plan(Mf, Nt, nw).ntiles;
        const int gfill = ar_overlap ? std::max(1, std::min(sw.ar_chunks > 0 ? sw.ar_chunks : std::min(8, gtiles / 32), gtiles)) : 1;
        gp = gram_plan(Mf, Nt, nw, gfill);
        gps.assign(nlanes, gp);
        for (int b = 0; b < nlanes; ++b) {
            gps[b] = gram_plan(LH[b].Q->Mf, Nt, nw, gfill);
            gp.Mpad = std::max(gp.Mpad, gps[b].Mpad); gp.slab_doubles = std::max(gp.slab_doubles, gps[b].slab_doubles);
        }
        P.trig = Lt.ok ? 1 : 0;
        P.D1 = D1_max; P.tmin = Lt.tmin; P.LDL = int(round_up(std::max(D1_max, 1), 64));
        P.seg = seg_of(D1_max);
        P.useg = 1;
        if (Lt.ok) for (int b = 0; b < nlanes; ++b) P.useg = std::max(P.useg, cdiv(LH[b].Lt.D1, seg_of(LH[b].Lt.D1)));      // (launches: the most segments any lane has)
        P.nchunk = int(nchunk_max); P.nfold = int(nfold_max);
        P.seeds_shared = 0;
        if (nlanes > 1 && Lt.ok) {         // sweeps over Peak / ripple keep the grid: one seed table serves the unit
            bool same = true;
            for (int b = 1; b < nlanes && same; ++b) {
                const LatticeInfo& Lb = LH[b].Lt;
                same = Lb.D1 == Lt.D1 && Lb.tmin == Lt.tmin && Lb.wf == Lt.wf && Lb.ch_w0 == Lt.ch_w0 && Lb.ch_dw == Lt.ch_dw && Lb.ch_start == Lt.ch_start && Lb.ch_count == Lt.ch_count;
            }
            P.seeds_shared = same ? 1 : 0;
        }
        P.cgrp = sw.cgrp;    // (4 unless set: two pairs of interleaved chunks per block, for one design and for lanes alike -- the same sums in
                             // both: half the partial-moment traffic of one pair per block -- with four units in flight the solver moves
                             // 3 TB/s through HBM, and that, not the recurrences, is what the moment kernels then wait for)
        P.LDM = int(round_up(3 * std::max(D1_max, 1), 256));
        P.Nt = Nt; P.Ne = Ne; P.N = N; P.Mf = Mf; P.R = R; P.l = l_max; P.nq3 = nq3_max; P.big = big_max; P.quad = Q.quad;
        P.ld = gp.ld; P.Mpad = gp.Mpad; P.np = int(round_up(N, 64));
        P.LDV = int(round_up(std::max(P.ld, P.np), 128)); P.Rp = int(round_up(R, 64));
        P.nyrows = nyrows_max;
        P.mask = nullptr; P.lane_bytes = 0; P.dims = nullptr; P.Mown = P.Mpad;
        P.own = shard_rank == 0 ? 1 : 0;                        // (1 when not sharded)
        if (hetero) {
            for (int b = 0; b < nlanes; ++b) {
                const TrigProgram& Qb = *LH[b].Q;
                const int d1 = LH[b].Lt.D1, sg = seg_of(d1);
                hostDims[b] = LaneDims{Qb.Mf, Qb.R, Qb.l, int(LH[b].prep->yrows.size()), int(LH[b].Lt.wf.size()), int(LH[b].Lt.ch_start.size()),
                                       Qb.Nt, Qb.Nt + Qb.Ne, Qb.nq3, Qb.big, d1, sg, LH[b].Lt.ok ? cdiv(d1, sg) : 1, gps[b].Mpad, LH[b].Lt.tmin};
            }
            MBFIR_HIP(hipMemcpyAsync(dimsT, hostDims, sizeof(LaneDims) * nlanes, hipMemcpyHostToDevice, st));
            P.dims = dimsT;
        }
        nsplit_at = cdiv(P.Mpad, AT_ROWS);
        nbR = cdiv(R, 256); nbN = cdiv(N, 256); nbC = cdiv(P.l + P.nq3, 256);
        if (nbR + 1 > NPART * 64) throw HipError("problem too large for the reduction buffers");
        U.n_max = n_max;
        U.lp = Q.which == DES_AP ? specfact_lp(n_max) : 0;
        for (int b = 0; b < nlanes; ++b) lane_n[b] = LH[b].Q->n;
        U.tiles.resize(nlanes);
        for (int b = 0; b < nlanes; ++b) { U.tiles[b].resize(gram_table_ints(gps[b])); gram_tiles_host(gps[b], U.tiles[b].data()); }
        gchunks.clear();
        if (ar_overlap) {              // the chunk tables ride behind the tile table
            std::vector<int> ctab;
            gram_chunk_tables(gps[0], gfill, ctab, gchunks);
            U.tiles[0].insert(U.tiles[0].end(), ctab.begin(), ctab.end());
        }
        cap_form = sw.ddform < 0 ? o.dd_form == 0 : sw.ddform != 0;      // its capacitance form in plain double (capkkt.hip) or the double-double one
        // extended-precision KKT solve (ddkkt.inc); lock-step units: in its capacitance form (round 5; the double-double kernels take one design)
        if (o.ddkkt_theta > 0 && nlanes > 1 && !cap_form) throw ShapeError("lock-step batch: the double-double form of the extended-precision solve runs one design at a time");
        U.use_dd = o.ddkkt_theta > 0 && shard_size <= 1;
        dd_unit = U.use_dd && nlanes > 1;
        dd_kp = 0;
        // refinement passes around the extended-precision solve: two for the double-double form, THREE for the capacitance form (with
        // two, a design of BASELINE config 3's batch lost its iterate near the end: DESIGN.md section 5)
        dd_passes = cap_form ? 3 : 2;
        fused_hsolve = hsolve_fused_ok(P.np, 2) && sw.hsolve;
        return U;
    }
    // Arena layout: the lanes' program arrays (one upload per lane) and the work buffers of ONE lane.  A measuring pass adds up the
    // sizes; the lanes then sit lane_bytes apart in one arena, and the work buffers start zeroed.
    void layout_arena(const std::vector<LaneHost>& LH, const UnitPlan& U) {
        const size_t ld = P.ld, np = P.np, LDV = P.LDV, Rp = P.Rp, Mpad = P.Mpad;
        const int nw = P.quad ? 3 : 1;
        char* zero_from = nullptr;
        size_t zero_bytes = 0;
        auto place = [&]() {
        // ---- upload the program (one copy per lane) ----------------------------------------------
#define UPQ(T, member) upload<T>([&](int b) -> const std::vector<T>& { return LH[b].Q->member; })
#define UPL(T, member) upload<T>([&](int b) -> const std::vector<T>& { return LH[b].member; })
        P.w = UPQ(double, w); P.col_kind = UPQ(int, col_kind); P.col_tau = UPQ(double, col_tau);
        P.col_scale = UPQ(double, col_scale); P.pcol = UPQ(int, pcol); P.psign = UPQ(double, psign);
        P.c = UPQ(double, c); P.freq = UPQ(int, freq); P.col = UPQ(int, col); P.alpha = UPQ(double, alpha);
        P.beta = UPQ(double, beta); P.ey = UPQ(double, ey); P.h = UPQ(double, h);
        P.f_ptr = UPL(int, prep->f_ptr); P.f_rows = UPL(int, prep->f_rows); P.c_ptr = UPL(int, prep->c_ptr); P.c_rows = UPL(int, prep->c_rows);
        P.yrows = UPL(int, prep->yrows); P.rep = UPL(int, prep->rep);
        tile_ij = upload<int>([&](int b) -> const std::vector<int>& { return U.tiles[b]; });
        P.lat = UPL(int, Lt.lat); P.lat_col = UPL(int, Lt.lat_col); P.lat_qcol = UPL(int, Lt.lat_qcol);
        P.lat_scale = UPL(double, Lt.lat_scale); P.lat_qscale = UPL(double, Lt.lat_qscale);
        P.ch_start = UPL(int, Lt.ch_start); P.ch_count = UPL(int, Lt.ch_count); P.ch_w0 = UPL(double, Lt.ch_w0); P.ch_dw = UPL(double, Lt.ch_dw);
        P.fold_pos = UPL(int, Lt.fold_pos); P.fold_neg = UPL(int, Lt.fold_neg); P.wf = UPL(double, Lt.wf);
#undef UPQ
#undef UPL
        if (!ar.measuring) flush_uploads();
        // ---- work buffers ----------------------------------------------------------------------
        zero_from = ar.base + ar.off;
        A1 = ar.get<double>(P.trig ? 0 : Mpad * ld);
        T = ar.get<double>(P.trig ? 0 : nw * ld * ld);
        Tp = ar.get<double>(ar_overlap ? (size_t)gps[0].ntiles * 16384 : 0);
        chunk_tab = ar_overlap ? tile_ij + gram_table_ints(gps[0]) : nullptr;
        {
            const size_t nch = std::max(P.nchunk, 1), d1 = std::max(P.D1, 1);
            P.seed_tau = ar.get<double4>(P.trig ? nch * d1 : 1);
            P.seed_h = ar.get<double4>(P.trig ? nch * (3 * d1 - 1) : 1);
            P.seed_eval = ar.get<double4>(P.trig ? (size_t)P.useg * Mpad : 1);
        }
        Mom = ar.get<double>(18 * (size_t)P.LDM); MomB = ar.get<double>(12 * (size_t)P.LDM);
        H = ar.get<double>(np * np); M = ar.get<double>(np * np); Mt = ar.get<double>(np * np); W1 = ar.get<double>(np * np + 65 * np);
        Sc = ar.get<double>(S_COUNT); flag = ar.get<int>(4); gt_cnt = ar.get<int>(4); RB = ar.get<double>(16);
        x = ar.get<double>(LDV); tmpN = ar.get<double>(2 * LDV); tmpN2 = ar.get<double>(2 * LDV);
        rhsN = ar.get<double>(2 * LDV); yN = ar.get<double>(2 * LDV); pN = ar.get<double>(2 * LDV); bx2 = ar.get<double>(2 * LDV);
        dx2 = ar.get<double>(2 * LDV); rx = ar.get<double>(LDV); GTz = ar.get<double>(LDV + 16);        /* + the mailbox of the residual sums, packed behind G'z */
        bxc = ar.get<double>(LDV); dxc = ar.get<double>(LDV); qv = ar.get<double>(3 * LDV);
        XX = ar.get<double>(4 * LDV); TT = ar.get<double>(6 * LDV); TT2 = ar.get<double>(4 * LDV); xout = ar.get<double>(LDV);
        s = ar.get<double>(Rp); z = ar.get<double>(Rp); lam = ar.get<double>(Rp); dl = ar.get<double>(Rp);
        wl = ar.get<double>(Rp); w3 = ar.get<double>(4 * (size_t)std::max(P.nq3, 1)); wbb = ar.get<double>(std::max(P.big, 1));
        tmpR = ar.get<double>(2 * Rp); wbz = ar.get<double>(2 * Rp); wpR = ar.get<double>(2 * Rp); bz2 = ar.get<double>(2 * Rp); dz2 = ar.get<double>(2 * Rp);
        gdx2 = ar.get<double>(2 * Rp); gdxc = ar.get<double>(Rp); xbest = ar.get<double>(LDV);
        rz = ar.get<double>(Rp); Gx = ar.get<double>(Rp); dssa = ar.get<double>(Rp); wdza = ar.get<double>(Rp);
        lds = ar.get<double>(Rp); bzc = ar.get<double>(Rp); dzc = ar.get<double>(Rp); ds = ar.get<double>(Rp);
        dz = ar.get<double>(Rp); scratch = ar.get<double>(4 * (size_t)std::max(P.big, 1) + 8);
        kbx = ar.get<double>(LDV); kbz = ar.get<double>(Rp); kx = ar.get<double>(LDV); kz = ar.get<double>(Rp); kg = ar.get<double>(Rp);
        kds = ar.get<double>(Rp); kdz = ar.get<double>(Rp);
        UU = ar.get<double>(4 * Mpad * (size_t)P.useg); PP = ar.get<double>(4 * Mpad); PPf = ar.get<double2>(6 * Mpad); Dw = ar.get<double>(9 * Mpad); BB = Dw + (size_t)nw * Mpad;       // border vectors right behind the nw weight vectors
        partial = ar.get<double>(std::max(P.trig ? (size_t)cdiv(P.nchunk, P.cgrp) * 12 * P.LDM : (size_t)nsplit_at * 6 * ld,
                                          std::max(hsolve_part_doubles(int(np)), hsolve_part_doubles(CAP_KMAX))));   // (also the partial vectors of the one-pass M'(M b), of H and of the capacitance matrix)
        partR = ar.get<double>(4 * (size_t)(nbR + 2)); partR2 = ar.get<double>(4 * (size_t)(nbR + 2)); partN = ar.get<double>(4 * (size_t)(nbN + 2));
        ddinv = nullptr;
        if (U.use_dd) {
            D.e3 = ar.get<double>(8 * (size_t)std::max(P.nq3, 1)); D.eb = ar.get<double>(8); D.whb = ar.get<double>(std::max(P.big, 1));
            D.dlc = ar.get<double>(Rp); D.m3c = ar.get<double>(6 * (size_t)std::max(P.nq3, 1));
            D.slotl = ar.get<int>(std::max(P.l, 1)); D.slot3 = ar.get<int>(3 * (size_t)std::max(P.nq3, 1)); D.slotb = ar.get<int>(2);
            D.kcnt = ar.get<int>(1); D.skind = ar.get<int>(DD_KMAX); D.sidx = ar.get<int>(DD_KMAX); D.sdir = ar.get<int>(DD_KMAX);
            ddtheta = ar.get<double>(MAX_LANES);
            D.sX = ar.get<double>(DD_KMAX); D.U = ar.get<double>((size_t)DD_KMAX * np);
            ddB = ar.get<double>(4 * LDV); ddtS = ar.get<double>(2 * (size_t)DD_KMAX); ddzeta = ar.get<double>(2 * (size_t)DD_KMAX);
            ddri = ar.get<double>(2 * np); ddd0 = ar.get<double>(np);
            ddflags = ar.get<int>(2 * np / 32 + 8);          // block flags of the multi-workgroup dd solve (zeroed with the arena)
            ddinv = ar.get<double>(2 * np * 64);
            if (!sw.dd_blockinv) ddinv = nullptr;
            if (cap_form) {
                capYt = ar.get<double>((size_t)CAP_KMAX * np); capZt = ar.get<double>((size_t)CAP_KMAX * np);
                capS = ar.get<double>((size_t)CAP_KMAX * CAP_KMAX); capMs = ar.get<double>((size_t)CAP_KMAX * CAP_KMAX);
                capW1 = ar.get<double>((size_t)CAP_KMAX * CAP_KMAX + 65 * (size_t)CAP_KMAX); capw = ar.get<double>(2 * (size_t)DD_KMAX);
                capflag = ar.get<int>(4);
                capPart = ar.get<double>(cap_part_doubles(CAP_KMAX, int(np)));
            }
        }
        hout = ar.get<double>(2 * (size_t)U.n_max + 8);
        sfwork = ar.get<double>(6 * (size_t)std::max(U.lp, 1));
        zero_bytes = size_t(ar.base + ar.off - zero_from);
        slab = ar.get<double>(P.trig ? 0 : gp.slab_doubles);
        };
        // first pass: only add up the sizes of ONE lane; the lanes then sit lane_bytes apart in one arena
        ar.measuring = true; ar.reset(); meas_lo = meas_hi = 0;
        { char* keep = ar.base; ar.base = nullptr; place(); ar.base = keep; }
        lane_bytes = (ar.off + 4095) & ~size_t(4095); ar.measuring = false;
        ensure_arena(lane_bytes * nlanes + 4096);
        pend.clear(); stage_lo = stage_hi = 0;
        place();
        P.lane_bytes = lane_bytes;
        memset_lanes(zero_from, zero_bytes);
    }
    // ---- lane masks: row 0 = live lanes, rows q = 1..MAX_SWEEPS: lanes that run CG sweep q, ROW_DD / ROW_PL: the live lanes whose
    // iteration runs the extended-precision / the plain solve.  mask_dev is what the device holds, mask_new what it is to hold.
    std::vector<int> mask_dev, mask_new;
    void push_masks(const std::vector<LaneHost>& LH) {
        if (nlanes == 1) return;
        for (int b = 0; b < nlanes; ++b) {
            mask_new[b] = LH[b].live ? 1 : 0;
            lane_live[b] = LH[b].live;
            // (a lane whose iteration runs the extended-precision solve takes no part in the plain solve's sweeps)
            for (int q = 1; q <= MAX_SWEEPS; ++q) mask_new[q * MAX_LANES + b] = (LH[b].live && LH[b].dd_k == 0 && LH[b].nsweep >= q) ? 1 : 0;
            mask_new[ROW_DD * MAX_LANES + b] = (LH[b].live && LH[b].dd_k > 0) ? 1 : 0;
            mask_new[ROW_PL * MAX_LANES + b] = (LH[b].live && LH[b].dd_k == 0) ? 1 : 0;
        }
        // rows [off, off + ints) to the device where they changed (most iterations change nothing: the copy is a launch of its own)
        auto send = [&](size_t off, size_t ints) {
            if (std::memcmp(mask_new.data() + off, mask_dev.data() + off, sizeof(int) * ints) == 0) return;
            std::memcpy(hostMask + off, mask_new.data() + off, sizeof(int) * ints);
            MBFIR_HIP(hipMemcpyAsync(maskT + off, hostMask + off, sizeof(int) * ints, hipMemcpyHostToDevice, st));
            std::memcpy(mask_dev.data() + off, mask_new.data() + off, sizeof(int) * ints);
        };
        send(0, size_t(MAX_SWEEPS + 1) * MAX_LANES);
        if (dd_unit) send(size_t(ROW_DD) * MAX_LANES, 2 * size_t(MAX_LANES));
    }
    // A1 (dense path) or the lattice seed tables, and every lane's initial scalars (norms, degree, tau = kappa = 1, cap on sigma)
    void start_lanes(const std::vector<LaneHost>& LH) {
        if (!P.trig) hipLaunchKernelGGL(k_build_A1, lane_grid(dim3(cdiv(P.Nt, 256), P.Mf), nlanes), dim3(256), 0, st, P, A1);
        else {
            const int seed_lanes = P.seeds_shared ? 1 : nlanes;
            hipLaunchKernelGGL(k_build_seeds_m, lane_grid(dim3(cdiv(P.D1, 256), P.nchunk), seed_lanes), dim3(256), 0, st, P, 1.0, P.D1, 0.0, 0,
                               const_cast<double4*>(P.seed_tau));
            hipLaunchKernelGGL(k_build_seeds_m, lane_grid(dim3(cdiv(3 * P.D1 - 1, 256), P.nchunk), seed_lanes), dim3(256), 0, st, P, 0.0, P.D1, 2.0,
                               2 * P.D1 - 1, const_cast<double4*>(P.seed_h));
            hipLaunchKernelGGL(k_build_seeds_e, lane_grid(dim3(cdiv(P.nfold, 256), P.useg), seed_lanes), dim3(256), 0, st, P, const_cast<double4*>(P.seed_eval));
        }
        std::vector<double> sc0((size_t)S_COUNT * nlanes, 0.0);
        for (int b = 0; b < nlanes; ++b) {
            double* q = sc0.data() + (size_t)b * S_COUNT;
            q[S_NRMH] = LH[b].nrm_h; q[S_NRMC] = LH[b].nrm_c; q[S_DEG] = LH[b].degree; q[S_TAU] = 1.0; q[S_KAPPA] = 1.0;
            q[S_SIGMAX] = (sw.corrector && LH[b].Q->l > 0 && LH[b].Q->big == 0) ? SIGMA_MAX_CORR : SIGMA_MAX;      // (not with a big cone: oracle/conic_ipm.py)
            MBFIR_HIP(hipMemcpyAsync(reinterpret_cast<char*>(Sc) + (size_t)b * lane_bytes, q, sizeof(double) * S_COUNT, hipMemcpyHostToDevice, st));
        }
    }
    // A unit up to its first launch that depends on an iterate: switches, lanes, plan, arena, masks (LH[b].live: all lanes in a
    // solve), A1 / seed tables and the lanes' scalars.  LH: one entry per lane.
    UnitPlan setup_unit(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, std::vector<LaneHost>& LH) {
        nlanes = int(Qs.size());
        sw = read_switches();
        chol_set_lose_step(sw.test_lose_flag, st);
        prepare_lanes(Qs, o, LH);
        const UnitPlan U = plan_unit(LH, o);
        layout_arena(LH, U);
        mask_dev.assign(size_t(MASK_ROWS) * MAX_LANES, -1); mask_new.assign(size_t(MASK_ROWS) * MAX_LANES, 0);
        push_masks(LH);
        P.mask = mask_row(0);
        start_lanes(LH);
        return U;
    }
    void cone_shift(double* v) {
        const int nb = std::max(nbC, 1);
        hipLaunchKernelGGL(k_cone_resid, lane_grid(dim3(nb), nlanes), dim3(256), 0, st, P, v, partR);
        if (P.big) hipLaunchKernelGGL(k_big_cone_resid, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, v, partR);
        hipLaunchKernelGGL(k_cone_fold, lane_grid(dim3(1), nlanes), dim3(256), 0, st, partR, nb + (P.big ? 1 : 0), RB, lane_bytes, P.mask);
        allreduce(RB, 1, 1);                          // max of the cone distances
        allreduce(RB + 1, 1, 0);                      // sum of squares
        hipLaunchKernelGGL(k_cone_shift, lane_grid(dim3(64), nlanes), dim3(256), 0, st, P, v, RB);
    }
    // initial point (W = I): x, s, z from the KKT solve of the initial right-hand sides, s and z shifted into their cones
    void initial_point(int nsweep, const KktObserver* obs = nullptr) {
        hipLaunchKernelGGL(k_unit_scaling, lane_grid(dim3(cdiv(std::max(std::max(P.l, P.nq3), std::max(P.big, 1)), 256)), nlanes), dim3(256), 0, st,
                           P, dl, wl, w3, wbb, Sc);
        build_H();
        hipLaunchKernelGGL(k_init_rhs, lane_grid(dim3(cdiv(std::max(P.N, P.R), 256)), nlanes), dim3(256), 0, st, P, bx2, bz2);
        kkt_solve<2>(bx2, bz2, dx2, dz2, gdx2, nsweep, S_RNA, false, obs);
        copy_lanes(x, dx2, sizeof(double) * P.LDV);
        hipLaunchKernelGGL(k_neg_copy_r, lane_grid(dim3(cdiv(P.R, 256)), nlanes), dim3(256), 0, st, P, dz2, s, -1.0);
        cone_shift(s);
        hipLaunchKernelGGL(k_neg_copy_r, lane_grid(dim3(cdiv(P.R, 256)), nlanes), dim3(256), 0, st, P, dz2 + P.Rp, z, 1.0);
        cone_shift(z);
    }
    // the residual kernels of an iterate (everything up to the one copy + synchronisation per iteration)
    void launch_residuals(int two = -1) {
        // row-sharded: the four row sums (||rz||^2, s'z, h'z, ||Gx + s||^2) are folded into a mailbox directly behind G'z and
        // summed over the ranks by the same all-reduce (they do not depend on G'z)
        const bool sharded = two_phase(two);        // (`two`: as for dots() below; test_unit_kkt runs the two-phase form on one rank)
        double* rmail = sharded ? GTz + P.LDV : RB;
        if (P.trig) {                                     // G x rows are formed inside k_resid_rows
            ++n_gv;
            trig_eval<1>(x);
            hipLaunchKernelGGL(k_resid_rows, lane_grid(dim3(nbR), nlanes), dim3(256), 0, st, P, nullptr, s, z, Sc, rz, bz2, partR, UU, x);
        } else {
            apply_G<1>(x, Gx);
            hipLaunchKernelGGL(k_resid_rows, lane_grid(dim3(nbR), nlanes), dim3(256), 0, st, P, Gx, s, z, Sc, rz, bz2, partR, nullptr, nullptr);
        }
        if (sharded) hipLaunchKernelGGL(k_scal_resid, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, GTz, x, rx, bx2, partR, nbR, rmail, 0, (const int*)flag);
        apply_GT<1>(z, GTz, sharded ? 5 : 0);
        hipLaunchKernelGGL(k_scal_resid, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, GTz, x, rx, bx2, partR, nbR, rmail, sharded ? 1 : 2, (const int*)flag);
    }
    // The head of an iteration -- NT scaling, normal matrix, factorisation: everything that depends on the iterate (s, z) alone.
    // On the extended-precision path it first takes every live lane's strong set (a host synchronisation).
    // the NT scaling of the iterate (s, z)
    void launch_scaling() {
        hipLaunchKernelGGL(k_scaling, lane_grid(dim3(std::max(nbC, 1)), nlanes), dim3(256), 0, st, P, s, z, dl, wl, w3, lam, bz2, wbz);
        if (P.big) hipLaunchKernelGGL(k_big_scaling, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, s, z, wbb, lam, Sc);
    }
    void launch_head(std::vector<LaneHost>& LH, const SolveOpts& o) {
        launch_scaling();
        int ks[MAX_LANES];
        if (dd_unit) {
            // every live lane its own strong set; then the masks of the two modes (the sweep rows follow: push_masks)
            bool lv[MAX_LANES];
            for (int b = 0; b < nlanes; ++b) lv[b] = LH[b].live;
            dd_k = dd_prepare_lanes(o.ddkkt_theta, ks, lv);
            dd_kp = int(round_up(std::max(dd_k, 1), 64));
        } else {
            ks[0] = dd_k = (o.ddkkt_theta > 0 && shard_size <= 1) ? dd_prepare(o.ddkkt_theta) : 0;
        }
        for (int b = 0; b < (dd_unit ? nlanes : 1); ++b) {
            LH[b].dd_k = ks[b];
            if (ks[b] > 0) { LH[b].dd_iters += 1; LH[b].dd_kmax = std::max(LH[b].dd_kmax, ks[b]); }
        }
        if (dd_unit) push_masks(LH);
        build_H(dd_k);
    }
    // the KKT solve of one right-hand side block on every live lane: the extended-precision solve where the strong set is non-empty,
    // the plain one with `nsweep` refinement sweeps elsewhere, each under its mask (every lane the sequence of its single solve)
    template <int NV>
    void solve_modes(bool dd_any, bool pl_any, const double* bx, const double* bz, double* dx, double* dz, double* gdx, int slot, int nsweep,
                     const KktObserver* dd_obs = nullptr) {
        const int* live_row = P.mask;
        if (dd_any) {
            if (dd_unit) P.mask = mask_row(ROW_DD);
            kkt_solve_dd<NV>(bx, bz, dx, dz, gdx, slot, dd_obs);
        }
        if (pl_any) {
            if (dd_unit) P.mask = mask_row(ROW_PL);
            kkt_solve<NV>(bx, bz, dx, dz, gdx, nsweep, slot, true);  // W^-2 bz came with k_scaling / k_comb_rhs / k_corr_rhs
        }
        P.mask = live_row;
    }
    // the cone products of direction (xx2, zz2) with the predictor's z1 = dz2; two-phase form (row-sharded solves; test_unit_cone on
    // request): folded by k_scal_dtau and summed over the ranks.  Returns the number of partial rows (otherwise k_dir_post folds them itself)
    // (`two`: -1 = the form of this solve, two-phase where it is row-sharded; 0 / 1 as asked)
    bool two_phase(int two) const { return two < 0 ? shard_size > 1 : two != 0; }
    // (add_corr: the corrector's candidate is formed by the same launch, in place in kx / kz / kg -- k_dots_r<true> in place of k_corr_add)
    int dots(const double* xx2, const double* zz2, int mode, int two = -1, bool add_corr = false) {
        const double* none = nullptr;
        if (add_corr)
            hipLaunchKernelGGL(k_dots_r<true>, lane_grid(dim3(std::max(nbC, 1)), nlanes), dim3(256), 0, st, P, wl, w3, dz2, none, partR, dxc, dzc, gdxc, kx, kz, kg);
        else
            hipLaunchKernelGGL(k_dots_r<false>, lane_grid(dim3(std::max(nbC, 1)), nlanes), dim3(256), 0, st, P, wl, w3, dz2, zz2, partR, none, none, none,
                               (double*)nullptr, (double*)nullptr, (double*)nullptr);
        int nb = std::max(nbC, 1);
        if (P.big) {
            hipLaunchKernelGGL(k_big_dots, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, wbb, Sc, dz2, zz2, scratch, partR);
            nb += 1;
        }
        if (two_phase(two)) {
            hipLaunchKernelGGL(k_scal_dtau, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, dx2, xx2, partR, nb, mode, RB, 0);
            allreduce(RB, 3, 0);
            hipLaunchKernelGGL(k_scal_dtau, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, dx2, xx2, partR, nb, mode, RB, 1);
        }
        return nb;
    }
    // the direction's ds / dz and step maxima; the maxima go to partR2 (k_dir_post reads the k_dots_r partials in partR while it
    // writes them).  Returns the number of partial rows
    int dir_post(const double* xx2, const double* zz2, const double* gg2, double* outA, double* outB, int mode, int ndots, int two = -1) {
        int nb = std::max(nbC, 1);
        hipLaunchKernelGGL(k_dir_post, lane_grid(dim3(nb), nlanes), dim3(256), 0, st, P, wl, w3, lam, dz2, zz2, gdx2, gg2, rz, Sc, outA, outB,
                           partR2, mode, two_phase(two) ? nullptr : partR, ndots, xx2);
        if (P.big) {
            hipLaunchKernelGGL(k_big_dir_post, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, wbb, lam, dz2, zz2, gdx2, gg2, rz, Sc, outA, outB,
                               scratch, partR2, mode);
            nb += 1;
        }
        return nb;
    }
    // k_scal_step on the step maxima of dir_post: in the two-phase form around an all-reduce, otherwise (where `unsharded`) in one
    void scal_step(int mode, int nb, bool unsharded, int two = -1) {
        if (two_phase(two)) {
            hipLaunchKernelGGL(k_scal_step, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, partR2, nb, mode, rx, bxc, RB, 0);
            allreduce(RB, 2, 1);
            hipLaunchKernelGGL(k_scal_step, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, partR2, nb, mode, rx, bxc, RB, 1);
        } else if (unsharded) {
            hipLaunchKernelGGL(k_scal_step, lane_grid(dim3(1), nlanes), dim3(SCAL_T), 0, st, P, Sc, partR2, nb, mode, rx, bxc, RB, 2);
        }
    }
    // ---- the cone stages of an iteration, between its KKT solves (launch_iteration; test_unit_cone runs the same stages with the
    // solutions uploaded in place of the solves).  `two`: the two-phase form of the folding kernels.
    // predictor tail: dtau / dkappa of the affine direction, its scaled ds / dz and step maxima (two-phase: also alpha_a, sigma, bx).
    // Returns the number of rows of step maxima
    int stage_pred_tail(bool two) {
        double *x2a = dx2 + P.LDV, *z2a = dz2 + P.Rp, *g2a = gdx2 + P.Rp;
        const int nd0 = dots(x2a, z2a, 0, two);
        const int ns0 = dir_post(x2a, z2a, g2a, dssa, wdza, 0, nd0, two);
        scal_step(0, ns0, false, two);
        return ns0;
    }
    // combined right-hand side (one-phase: sigma and bx are formed inside k_comb_rhs; W^-2 bz comes with it)
    void stage_comb_rhs(int ns0, bool two) {
        hipLaunchKernelGGL(k_comb_rhs, lane_grid(dim3(std::max(nbC, 1)), nlanes), dim3(256), 0, st, P, wl, w3, lam, dssa, wdza, rz, Sc,
                           lds, bzc, two ? nullptr : partR2, ns0, rx, bxc, dl, wbz);
        if (P.big)
            hipLaunchKernelGGL(k_big_comb_rhs, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, wbb, lam, dssa, wdza, rz, Sc, lds, bzc, scratch);
    }
    // combined tail: dtau / dkappa, ds, dz and the step maxima of the combined direction.  Returns the number of rows of maxima
    int stage_comb_tail(bool two) {
        const int nd1 = dots(dxc, dzc, 1, two);
        return dir_post(dxc, dzc, gdxc, ds, dz, 1, nd1, two);
    }
    int unknown_blocks() const { return cdiv(std::max(P.N, P.R), 256); }
    // update along the combined direction (sw.fuse, one-phase: k_update forms the step length itself)
    void stage_update(int ns1, bool two) {
        scal_step(1, ns1, !sw.fuse, two);
        hipLaunchKernelGGL(k_update, lane_grid(dim3(unknown_blocks()), nlanes), dim3(256), 0, st, P, Sc, dx2, dxc, x, ds, dz, s, z,
                           (!two && sw.fuse) ? (const double*)partR2 : (const double*)nullptr, ns1);
    }
    // corrector right-hand side: the step of the predictor-corrector direction is measured but not taken (k_scal_step mode 2); the
    // orthant rows' products at the trial step alpha0 + CORR_DELTA, projected onto the box around sigma mu, give one more right-hand
    // side for the factorisation at hand
    void stage_corr_rhs(int ns1, int corr_cones, const int* corr_ddm, bool two) {
        const bool fused = sw.fuse && !two;          // (the trial step is formed inside k_corr_rhs)
        if (!fused) scal_step(2, ns1, true, two);
        hipLaunchKernelGGL(k_corr_rhs, lane_grid(dim3(std::max(nbC, 1)), nlanes), dim3(256), 0, st, P, wl, dl, lam, ds, dz, Sc, kbz, wbz,
                           fused ? (const double*)partR2 : (const double*)nullptr, ns1);
        if (P.big) hipLaunchKernelGGL(k_big_corr_rhs, lane_grid(dim3(1), nlanes), dim3(1024), 0, st, P, wbb, lam, ds, dz, Sc, kbz, scratch, corr_cones, corr_ddm);
    }
    // corrector tail: the candidate (predictor-corrector + corrector solution) gets its own direction and step (mode 3: own dtau /
    // dkappa slots), k_scal_step picks the longer step by CORR_ACCEPT and moves tau, kappa, k_update_pick moves x, s, z along the
    // direction picked.  Every lane decides for itself.
    void stage_corr_tail(bool two) {
        const bool fused = sw.fuse && !two;          // (k_corr_add inside k_dots_r -- without a big cone, whose rows have no thread there --, the pick inside k_update_pick)
        const bool add_in_dots = fused && !P.big;
        if (!add_in_dots) hipLaunchKernelGGL(k_corr_add, lane_grid(dim3(unknown_blocks()), nlanes), dim3(256), 0, st, P, dxc, dzc, gdxc, kx, kz, kg);
        const int ndC = dots(kx, kz, 3, two, add_in_dots);
        const int nsC = dir_post(kx, kz, kg, kds, kdz, 3, ndC, two);
        if (!fused) scal_step(3, nsC, true, two);
        hipLaunchKernelGGL(k_update_pick, lane_grid(dim3(unknown_blocks()), nlanes), dim3(256), 0, st, P, Sc, dx2, dxc, kx, x, ds, dz, kds, kdz, s, z,
                           fused ? (const double*)partR2 : (const double*)nullptr, nsC);
    }
    // The body of an iteration: the head (unless it went out ahead of the verdicts), then the cone stages with the KKT solves in between
    void launch_iteration(std::vector<LaneHost>& LH, const SolveOpts& o, bool head_out, int nsweep, bool use_corr) {
        if (!head_out) launch_head(LH, o);
        const bool two = two_phase(-1);
        bool dd_any = dd_k > 0, pl_any = dd_k == 0;
        if (dd_unit) {
            pl_any = false;
            for (int b = 0; b < nlanes; ++b) pl_any = pl_any || (LH[b].live && LH[b].dd_k == 0);
        }
        // constant + affine systems in one batch: [x1 z1], [x2 z2]
        solve_modes<2>(dd_any, pl_any, bx2, bz2, dx2, dz2, gdx2, S_RNA, nsweep);
        const int ns0 = stage_pred_tail(two);
        stage_comb_rhs(ns0, two);
        solve_modes<1>(dd_any, pl_any, bxc, bzc, dxc, dzc, gdxc, S_RNB, nsweep);
        const int ns1 = stage_comb_tail(two);
        if (!use_corr) { stage_update(ns1, two); return; }
        // ---- one centrality corrector (round 6; oracle/conic_ipm.py solve(): CORR_*) -------------------------------------------
        // (extended-precision iterations: the corrector works on the orthant rows alone, with the usual passes: oracle/conic_ipm.py)
        const int corr_cones = (!sw.corr_big || (!dd_unit && dd_any)) ? 0 : 1;                 // one design: this iteration's mode ...
        const int* corr_ddm = (dd_unit && dd_any) ? mask_row(ROW_DD) : nullptr;               // ... a unit: lane by lane
        stage_corr_rhs(ns1, corr_cones, corr_ddm, two);
        // the Cholesky solve and its residual norm (S_RNC), no sweeps (lanes on the extended-precision path: their usual passes)
        solve_modes<1>(dd_any, pl_any, kbx, kbz, kx, kz, kg, S_RNC, 0);
        stage_corr_tail(two);
    }
    // The host's verdicts on the iterate in hostSc; lanes with a new best iterate get xbest = x / tau.  Returns whether any lane goes on.
    bool judge_lanes(std::vector<LaneHost>& LH, const SolveOpts& o, int it) {
        bool any_live = false, any_best = false;
        for (int b = 0; b < nlanes; ++b) hostMask[ROW_BEST * MAX_LANES + b] = 0;      // 1: the lane has a new best iterate
        for (int b = 0; b < nlanes; ++b) {
            LaneHost& L = LH[b];
            if (!L.live) continue;
            const double* hs = hostSc + (size_t)b * S_COUNT;
            const int chol_fixes = int(hs[S_CHOLFIX]);
            // a hand-off between workgroups inside the factorisation (or the extended-precision triangular solve) was
            // lost: its bounded poll expired and the block went on with stale data -- the numbers are void
            if (chol_fixes >= CHOL_SYNC_LOST) throw HipError("internal error: an in-launch hand-off of the KKT factorisation timed out (device flag never raised)");
            if (o.verbose)
                fprintf(stderr, "%s%3d pcost % .10e dcost % .10e gap %.2e pres %.1e dres %.1e k/t %.1e mu %.1e a %.3f sig %.1e sweeps %d chol %d%s\n",
                        nlanes > 1 ? ("[" + std::to_string(b) + "] ").c_str() : "", it, hs[S_PCOST], hs[S_DCOST], hs[S_GAP], hs[S_PRES],
                        hs[S_DRES], hs[S_KAPPA] / hs[S_TAU], hs[S_MU], hs[S_ALPHA], hs[S_SIGMA], L.nsweep, chol_fixes,
                        L.dd_k > 0 ? [&] { char bf[200]; std::snprintf(bf, sizeof(bf), " | k %d refinement norms %.2e -> %.2e -> %.2e , %.2e -> %.2e -> %.2e", L.dd_k,
                                       hs[S_RNA], hs[S_RNA + 1], dd_passes > 2 ? hs[S_RNA + 2] : 0.0, hs[S_RNB], hs[S_RNB + 1], dd_passes > 2 ? hs[S_RNB + 2] : 0.0);
                                       return std::string(bf); }().c_str() : "");
            if (lane_verdict(L, hs, o, it)) {
                hostMask[ROW_BEST * MAX_LANES + b] = 1;
                any_best = true;
            }
            any_live = any_live || L.live;
        }
        if (any_best) {
            // xbest = x / tau on the lanes with a new best iterate -- including a lane that max_iter (or the numerical
            // wall) retires in this very iteration: its best_info is this iterate's, so xbest has to be as well (the
            // new-best bits were cleared for every lane above and are set by the merit test alone, not by `live`)
            if (nlanes > 1) {
                MBFIR_HIP(hipMemcpyAsync(maskT + ROW_BEST * MAX_LANES, hostMask + ROW_BEST * MAX_LANES, sizeof(int) * MAX_LANES,
                                         hipMemcpyHostToDevice, st));
                P.mask = mask_row(ROW_BEST);
            }
            hipLaunchKernelGGL(k_finish_x, lane_grid(dim3(nbN), nlanes), dim3(256), 0, st, P, x, Sc, xbest);
            P.mask = mask_row(0);
        }
        return any_live;
    }
    // Finish: every lane's answer (the best iterate that met the stopping rule, a reduced-accuracy candidate, or x / tau) and report
    void finish_lanes(std::vector<LaneHost>& LH, const SolveOpts& o, std::vector<std::vector<double>>& xouts, std::vector<SolveInfo>& infos,
                      double t_begin, double t_assembled) {
        P.mask = nullptr;                                         // the final x / tau of every lane, finished or not
        hipLaunchKernelGGL(k_finish_x, lane_grid(dim3(nbN), nlanes), dim3(256), 0, st, P, x, Sc, xout);
        xouts.assign(nlanes, std::vector<double>());
        infos.assign(nlanes, SolveInfo());
        for (int b = 0; b < nlanes; ++b) {
            LaneHost& L = LH[b];
            if (L.live) L.status = ST_MAXIT;
            char* xo = reinterpret_cast<char*>(xout) + (size_t)b * lane_bytes;
            if (L.first_opt >= 0) {
                // an iterate met the stopping rule: the best of them (xbest) is the answer, however the end game ended -- its target,
                // its iteration cap, max_iter, the numerical wall, a non-finite iterate
                const SolveInfo last = L.info;
                L.info = L.opt_info; L.info.iters = last.iters; L.info.correctors = last.correctors; L.info.correctors_taken = last.correctors_taken;
                L.status = ST_OPTIMAL;
                MBFIR_HIP(hipMemcpyAsync(xo, reinterpret_cast<char*>(xbest) + (size_t)b * lane_bytes, sizeof(double) * P.LDV, hipMemcpyDeviceToDevice, st));
            } else if ((L.status == ST_MAXIT || L.status == ST_NUMERICAL) && L.have_best && L.best_info.pres <= INACC_FEAS &&
                L.best_info.dres <= INACC_FEAS && (L.best_info.relgap <= INACC_GAP || L.best_info.gap <= o.abstol)) {
                // the reference accepts CVX's 'Inaccurate/Solved' (fir_ap_cvx.m:176): reduced tolerances
                const int keep_it = L.info.iters;
                L.info = L.best_info; L.info.iters = keep_it;
                L.status = ST_OPTIMAL_INACCURATE;
                MBFIR_HIP(hipMemcpyAsync(xo, reinterpret_cast<char*>(xbest) + (size_t)b * lane_bytes, sizeof(double) * P.LDV, hipMemcpyDeviceToDevice, st));
            }
            const int Nb = L.Q->N();                              // (the lane's own unknowns: N is the unit's largest)
            xouts[b].assign(Nb, 0.0);
            MBFIR_HIP(hipMemcpyAsync(xouts[b].data(), xo, sizeof(double) * Nb, hipMemcpyDeviceToHost, st));
        }
        MBFIR_HIP(hipStreamSynchronize(st));
        const double t_end = now_ms();
        // the event pool holds (gram begin, gram end, chol begin, chol end) per build_H
        double ms_gram = 0, ms_chol = 0;
        int builds = 0;
        for (size_t i = 0; i + 3 < evused; i += 4, ++builds) {
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, evpool[i], evpool[i + 1]) == hipSuccess) ms_gram += a;
            if (hipEventElapsedTime(&b, evpool[i + 2], evpool[i + 3]) == hipSuccess) ms_chol += b;
        }
        double ms_cap = 0;
        for (size_t i = 0; i + 1 < capev_used; i += 2) { float t = 0; hipEventElapsedTime(&t, capev[i], capev[i + 1]); ms_cap += t; }
        const int nw = P.quad ? 3 : 1;
        for (int b = 0; b < nlanes; ++b) {
            SolveInfo& info = infos[b];
            info = LH[b].info;
            info.status = LH[b].status;
            info.ms_assemble = t_assembled - t_begin;
            info.ms_solve = t_end - t_assembled;                  // of the whole lock-step batch
            info.ms_gram = ms_gram; info.ms_chol = ms_chol; info.h_builds = builds;
            info.n_freq = LH[b].Q->Mf; info.n_rows = LH[b].Q->R; info.n_unknowns = LH[b].Q->N();
            info.lattice = P.trig;
            info.lanes = nlanes;
            info.collectives = int(n_collectives);
            info.collective_bytes = collective_bytes;
            info.gv_passes = int(n_gv); info.gtv_passes = int(n_gtv); info.pair_passes = int(n_pair);
            info.dd_iters = LH[b].dd_iters; info.dd_kmax = LH[b].dd_kmax;
            info.dd_form = cap_form ? 0 : 1; info.cap_flop = cap_flop_sum; info.ms_cap = ms_cap;
            info.chol_launches = int(chol_launch_count);
            info.chol_flop = 2.0 / 3.0 * double(P.np) * double(P.np) * double(P.np);
            info.gram_flop = P.trig ? double(3 * P.D1 - 1) * double(LH[b].Q->Mf) * (4.0 + 4.0 * nw)      // rotation + 2 fma per weight, per point and frequency
                                    : double(nw) * double(P.Mf) * double(P.Nt) * double(P.Nt + 1);
        }
        nlanes_last = nlanes; taps_valid = false;
    }
};

Solver::Solver(int device) : impl(new Impl()) {
    impl->device = device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw HipError("no HIP device available");
    MBFIR_HIP(hipSetDevice(device));
    {   // kernel attributes are per device function: once per device id, by one thread at a time
        static std::mutex warm_mu;
        static std::vector<char> warmed;
        std::lock_guard<std::mutex> lk(warm_mu);
        if (device < 0 || device >= ndev) throw HipError("no such HIP device");
        if ((int)warmed.size() < ndev) warmed.resize(ndev, 0);
        if (!warmed[device]) { dd_warm_kernels(); chol_warm_kernels(); warmed[device] = 1; }
    }
    MBFIR_HIP(hipStreamCreate(&impl->st));
    MBFIR_HIP(hipEventCreate(&impl->ev0));
    MBFIR_HIP(hipEventCreate(&impl->ev1));
    MBFIR_HIP(hipHostMalloc(&impl->hostSc, sizeof(double) * S_COUNT * MAX_LANES));
    MBFIR_HIP(hipHostMalloc(&impl->hostFlag, sizeof(int) * 4 * MAX_LANES));
    MBFIR_HIP(hipHostMalloc(&impl->hostMask, sizeof(int) * MASK_ROWS * MAX_LANES));
    MBFIR_HIP(hipMalloc(&impl->maskT, sizeof(int) * MASK_ROWS * MAX_LANES));
    MBFIR_HIP(hipMalloc(&impl->dimsT, sizeof(LaneDims) * MAX_LANES));
    MBFIR_HIP(hipHostMalloc(&impl->hostDims, sizeof(LaneDims) * MAX_LANES));
    std::memset(impl->hostMask, 0, sizeof(int) * MASK_ROWS * MAX_LANES);
}
Solver::~Solver() {
    if (!impl) return;
    hipSetDevice(impl->device);
    comm_destroy();
    if (impl->ar.base) hipFree(impl->ar.base);
    if (impl->hostSc) hipHostFree(impl->hostSc);
    if (impl->stage) hipHostFree(impl->stage);
    if (impl->hostFlag) hipHostFree(impl->hostFlag);
    if (impl->hostMask) hipHostFree(impl->hostMask);
    if (impl->maskT) hipFree(impl->maskT);
    if (impl->dimsT) hipFree(impl->dimsT);
    if (impl->hostDims) hipHostFree(impl->hostDims);
    for (hipEvent_t e : impl->evpool) hipEventDestroy(e);
    for (hipEvent_t e : impl->capev) hipEventDestroy(e);
    if (impl->ev0) hipEventDestroy(impl->ev0);
    if (impl->ev1) hipEventDestroy(impl->ev1);
    for (hipEvent_t e : impl->ovev) hipEventDestroy(e);
    if (impl->st2) hipStreamDestroy(impl->st2);
    if (impl->st) hipStreamDestroy(impl->st);
    delete impl;
}
void* Solver::stream() const { return impl->st; }
void Solver::comm_unique_id(char* id128) {
    RcclApi& R = rccl();
    if (!R.ok) throw HipError("RCCL unavailable: " + R.err);
    ncclUniqueId id;
    ncclResult_t r = R.GetUniqueId(&id);
    if (r != ncclSuccess) throw HipError("ncclGetUniqueId failed");
    std::memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
}
void Solver::comm_init(int nranks, int rank, const char* id128) {
    RcclApi& R = rccl();
    if (!R.ok) throw HipError("RCCL unavailable: " + R.err);
    MBFIR_HIP(hipSetDevice(impl->device));
    comm_destroy();
    ncclUniqueId id;
    std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    ncclResult_t r = R.CommInitRank(&impl->comm, nranks, id, rank);
    if (r != ncclSuccess) { impl->comm = nullptr; throw HipError(std::string("ncclCommInitRank: ") + (R.GetErrorString ? R.GetErrorString(r) : "failed")); }
    impl->comm_size = nranks; impl->comm_rank = rank;
}
// test hook: all-reduce a host array through the context's communicator on the solver stream
void Solver::test_comm_allreduce(double* v, long n, int op) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    if (!S.comm) throw HipError("no communicator (mbfir_comm_init)");
    void* d = nullptr;
    MBFIR_HIP(hipMalloc(&d, size_t(std::max<long>(n, 1)) * 8));
    MBFIR_HIP(hipMemcpyAsync(d, v, size_t(n) * 8, hipMemcpyHostToDevice, S.st));
    ncclResult_t r = rccl().AllReduce(d, d, size_t(n), ncclDouble, op == 1 ? ncclMax : ncclSum, S.comm, S.st);
    MBFIR_HIP(hipMemcpyAsync(v, d, size_t(n) * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    hipFree(d);
    if (r != ncclSuccess) throw HipError("ncclAllReduce failed");
}
void Solver::comm_destroy() {
    if (impl->comm) { hipStreamSynchronize(impl->st); rccl().CommDestroy(impl->comm); impl->comm = nullptr; }
}
void Solver::set_allreduce(int (*fn)(void*, long, int, void*), void* user) { impl->ar_fn = fn; impl->ar_user = user; }

std::vector<long> Solver::shape_key(const TrigProgram& Q, const SolveOpts& o) {
    const SolveSwitches sw = read_switches();
    const std::shared_ptr<LanePrep> pr = lane_prep(Q, o, sw);
    const LatticeInfo& Lt = pr->Lt;
    // (the lattice origin itself is a per-lane dimension since round 6 -- the centred delays of fir_qprog_phs / fir_qp_cvx move it with
    //  the order --; what a unit shares is whether it is ZERO: then the border moments ride the difference progression, build_H's one_pass)
    const long tbits = Lt.tmin == 0.0 ? 0 : 1;
    // the CLASS of the program: what all lanes of a unit must share (solve_lanes)
    // (round 5: designs of different ORDERS share a unit too -- the probes of a min-order search -- when their padded sizes fall into
    //  the same power-of-two bucket: a unit runs every lane at the size of its largest)
    long bucket = 64;
    while (bucket < round_up(Q.N(), 64)) bucket *= 2;
    // (units on the extended-precision path: the split of the capacitance products over K follows np -- lanes of one np only)
    if (o.ddkkt_theta > 0) bucket = round_up(Q.N(), 64);
    std::vector<long> key{long(Q.which), bucket, long(Q.Ne), long(Q.nq3 > 0), long(Q.big > 0), long(Q.quad), long(Lt.ok), tbits};
    // ... and on the dense path, where the per-lane dimensions of a heterogeneous unit do not reach, the ORDER: A1's row stride
    // follows it (the band edges may differ there too)
    if (!Lt.ok || o.dense_trig) {
        const long ord[] = {long(Q.n), long(Q.Nt), long(Q.nq3), long(Q.big), long(pr->c_rows.size()), long(Lt.D1)};
        key.insert(key.end(), std::begin(ord), std::end(ord));
    }
    return key;
}
void Solver::test_fold(const double* w, int Mf, int fold, long* out) {
    TrigProgram Q;
    Q.Nt = 1; Q.Mf = Mf; Q.w.assign(w, w + Mf);
    Q.col_kind = {0}; Q.col_tau = {0.0}; Q.col_scale = {1.0}; Q.pcol = {0}; Q.psign = {0.0};
    const SolveSwitches sw = read_switches();
    const LatticeInfo L = analyse_lattice(Q, sw.fold < 0 ? fold != 0 : sw.fold != 0);
    long pairs = 0, longest = 0, bad = 0;
    std::vector<int> seen(Mf, 0);
    double wmax = 1.0;
    for (int i = 0; i < Mf; ++i) wmax = std::max(wmax, std::fabs(w[i]));
    const double ulp = 2.2204460492503131e-16 * wmax;
    for (size_t k = 0; k < L.wf.size(); ++k) {
        const int ip = L.fold_pos[k], in = L.fold_neg[k];
        if (ip >= 0 && in >= 0) ++pairs;
        if (ip < 0 && in < 0) ++bad;
        if (ip >= 0) { if (ip >= Mf || seen[ip]++) ++bad; else if (std::fabs(w[ip] - L.wf[k]) > ulp + 1e-300 && fold) ++bad; }
        if (in >= 0) { if (in >= Mf || seen[in]++) ++bad; else if (std::fabs(-w[in] - L.wf[k]) > ulp + 1e-300) ++bad; }
    }
    for (int i = 0; i < Mf; ++i) if (seen[i] != 1) ++bad;
    long covered = 0;
    for (size_t c = 0; c < L.ch_start.size(); ++c) { longest = std::max<long>(longest, L.ch_count[c]); covered += L.ch_count[c]; }
    if (L.ok && covered != long(L.wf.size())) ++bad;
    out[0] = L.ok ? 1 : 0; out[1] = long(L.wf.size()); out[2] = pairs; out[3] = long(L.ch_start.size()); out[4] = longest; out[5] = bad;
}
// how many lanes of this shape one context runs in lock step (memory and occupancy)
int Solver::max_lanes(const TrigProgram& Q, const SolveOpts& o) {
    // lock-step batches exist on the lattice path only; the extended-precision KKT solve (on by default for
    // fir_qp_cvx) and row-sharded solves run one design at a time
    if (o.shard_size > 1) return 1;
    // (the extended-precision solve takes lock-step units in its capacitance form -- every lane switches to it when ITS strong set
    //  is non-empty, as its single solve does)
    const SolveSwitches sw = read_switches();
    const bool dd_lanes = o.ddkkt_theta > 0 && o.dd_form == 0 && sw.ddform != 0;
    if (o.ddkkt_theta > 0 && !dd_lanes) return 1;
    long np = round_up(Q.N(), 64);
    const bool lattice = !o.dense_trig && lane_prep(Q, o, sw)->Lt.ok;
    if (lattice) {        // (lattice path: designs of one size bucket share units -- shape_key -- and a unit
        long bucket = 64;                                     //  is as large as its largest lane)
        while (bucket < np) bucket *= 2;
        np = bucket;
    }
    long cap = std::min<long>(32, 16384 / np);
    if (!lattice) {
        // dense path (opts.dense_trig, or a grid / column set without the lattice structure): every lane materialises
        // its trig matrix and owns a split-K slab -- at most ~2 GB of them per unit
        const GramPlan gp = gram_plan(Q.Mf, Q.Nt, Q.quad ? 3 : 1);
        const double per_lane = 8.0 * (double(gp.Mpad) * gp.ld + double(gp.slab_doubles) + 3.0 * gp.ld * gp.ld);
        cap = std::min<long>(cap, std::max<long>(1, long(2.0e9 / per_lane)));
    }
    if (o.ddkkt_theta > 0) cap = std::min<long>(cap, 16);                               // (~100 MB of strong rows and capacitance matrices per lane)
    return int(std::max<long>(1, std::min<long>(MAX_LANES, cap)));
}

int Solver::solve(const TrigProgram& Qfull, const SolveOpts& o, std::vector<double>& xout, SolveInfo& info) {
    std::vector<const TrigProgram*> Qs{&Qfull};
    std::vector<std::vector<double>> xs;
    std::vector<SolveInfo> infos;
    solve_lanes(Qs, o, xs, infos);
    xout = xs[0]; info = infos[0];
    return info.status;
}

// The interior-point method on a lock-step unit (a single design is a unit of one): the lanes and the unit planned, the arena laid
// out, the initial point; then per iteration one scalar copy and one wait, the host's verdicts, and the iteration's launches.
void Solver::solve_lanes(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, std::vector<std::vector<double>>& xouts,
                         std::vector<SolveInfo>& infos) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const double t_begin = now_ms();
    const int nlanes = int(Qs.size());
    if (nlanes < 1 || nlanes > MAX_LANES) throw ShapeError("lock-step batch: bad lane count");
    std::vector<LaneHost> LH(nlanes);
    const UnitPlan U = S.setup_unit(Qs, o, LH);
    MBFIR_HIP(hipStreamSynchronize(S.st));
    const double t_assembled = now_ms();
    S.evused = 0; S.capev_used = 0; S.cap_flop_sum = 0;
    S.timing = o.timing;
    S.chol_launch_count = 0; S.dd_epoch = 0;
    S.initial_point(o.refine);

    const bool sharded = S.shard_size > 1;
    // (every lane of a unit is the same designer: orthant rows in all of them or in none.  What is corrected: the orthant rows and,
    //  on the plain path, the big cone -- oracle/conic_ipm.py)
    const bool use_corr = S.sw.corrector && S.P.l > 0;
    // MBFIR_TRACE_HOST=1: where the host thread of this unit spends the solve -- issuing launches, or waiting in the one
    // synchronisation per iteration (a stream whose host thread issues most of the time is launch-bound, not GPU-bound)
    const bool trace_host = S.sw.trace_host;
    double host_issue_ms = 0, host_wait_ms = 0, t_issue0 = trace_host ? now_ms() : 0.0;
    S.launch_residuals();
    // The head of the NEXT iteration goes to the stream BEFORE the host has looked at this iterate's scalars (round 5, DESIGN.md
    // section 5): the host waits on an event behind the scalars' copy while the GPU works on the head.  A lane the host then retires
    // has had one scaling and factorisation too many, which touch nothing the result is read from.  Not with the extended-precision
    // solve (its strong-set count needs the host mid-head) and row-sharded solves.
    const bool speculate = !U.use_dd && !sharded && S.sw.speculate;
    int it = 0;
    for (it = 0; it <= o.max_iter; ++it) {
        MBFIR_HIP(hipMemcpy2DAsync(S.hostSc, sizeof(double) * S_COUNT, S.Sc, S.lane_bytes, sizeof(double) * S_COUNT, nlanes, hipMemcpyDeviceToHost, S.st));
        const bool head_out = speculate && it < o.max_iter;
        if (head_out) {
            MBFIR_HIP(hipEventRecord(S.ev0, S.st));
            S.launch_head(LH, o);
        }
        const double t_sync0 = trace_host ? now_ms() : 0.0;
        if (head_out) MBFIR_HIP(hipEventSynchronize(S.ev0));
        else MBFIR_HIP(hipStreamSynchronize(S.st));
        if (trace_host) { const double t1 = now_ms(); host_issue_ms += t_sync0 - t_issue0; host_wait_ms += t1 - t_sync0; t_issue0 = t1; }
        if (!S.judge_lanes(LH, o, it)) break;
        int nsweep_max = 0;
        for (int b = 0; b < nlanes; ++b)
            if (LH[b].live) nsweep_max = std::max(nsweep_max, LH[b].nsweep);
        S.push_masks(LH);                                     // (a unit with opts.ddkkt pushes them again once the head knows the lanes' modes)
        S.launch_iteration(LH, o, head_out, nsweep_max, use_corr);
        S.launch_residuals();
    }
    S.finish_lanes(LH, o, xouts, infos, t_begin, t_assembled);
    if (trace_host)
        fprintf(stderr, "[host] unit of %d lanes, %d iterations: issuing launches %.1f ms, waiting in the per-iteration sync %.1f ms (%.0f %% issuing)\n",
                nlanes, it, host_issue_ms, host_wait_ms, 100.0 * host_issue_ms / std::max(host_issue_ms + host_wait_ms, 1e-9));
}

}  // namespace mbfir

// ================================================================================================
// post-processing and test hooks
// ================================================================================================
namespace mbfir {

// the solution vector the tap extraction of lane 0 starts from (api.cpp: the best of several attempts)
void Solver::set_solution(const std::vector<double>& x) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    MBFIR_HIP(hipMemcpyAsync(S.xout, x.data(), sizeof(double) * x.size(), hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    S.taps_valid = false;
}
void Solver::specfact_last(int n, double* h_re, double* h_im, int lane) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    if (lane < 0 || lane >= S.nlanes_last) throw HipError("specfact: no such lane");
    const size_t off = (size_t)lane * S.lane_bytes / sizeof(double);
    if (!S.taps_valid) {                                  // one launch factorises every lane of the last unit (a lane
        bool one_n = true;                                // without a solution yields numbers nobody asks for); a unit of
        for (int b = 1; b < S.nlanes_last; ++b) one_n = one_n && S.lane_n[b] == S.lane_n[0];       // different orders: lane by lane
        if (one_n) specfact_launch(S.xout, n, S.sfwork, S.hout, S.st, S.nlanes_last, S.lane_bytes);
        else
            for (int b = 0; b < S.nlanes_last; ++b) {
                const size_t ob = (size_t)b * S.lane_bytes / sizeof(double);
                specfact_launch(S.xout + ob, S.lane_n[b], S.sfwork + ob, S.hout + ob, S.st, 1, 0);
            }
        S.taps_valid = true;
    }
    if (n != S.lane_n[lane]) throw HipError("specfact: the lane holds a design of another order");
    std::vector<double> h(2 * (size_t)n);
    MBFIR_HIP(hipMemcpyAsync(h.data(), S.hout + off, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    for (int i = 0; i < n; ++i) { h_re[i] = h[2 * i]; h_im[i] = h[2 * i + 1]; }
}

void Solver::test_gram(int m, int nt, int nw, const double* A, const double* d, double* out) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    GramPlan gp = gram_plan(m, nt, nw);
    const size_t ld = gp.ld, Mpad = gp.Mpad;
    DevBuf dA(Mpad * ld * 8), dd(nw * Mpad * 8), dslab(gp.slab_doubles * 8), dT(nw * ld * ld * 8), dt((size_t)gram_table_ints(gp) * 4);
    MBFIR_HIP(hipMemsetAsync(dA.p, 0, Mpad * ld * 8, S.st));
    MBFIR_HIP(hipMemsetAsync(dd.p, 0, nw * Mpad * 8, S.st));
    MBFIR_HIP(hipMemcpy2DAsync(dA.p, ld * 8, A, (size_t)nt * 8, (size_t)nt * 8, m, hipMemcpyHostToDevice, S.st));
    for (int w = 0; w < nw; ++w)
        MBFIR_HIP(hipMemcpyAsync(dd.as<double>() + w * Mpad, d + (size_t)w * m, (size_t)m * 8, hipMemcpyHostToDevice, S.st));
    std::vector<int> tiles(gram_table_ints(gp));
    gram_tiles_host(gp, tiles.data());
    MBFIR_HIP(hipMemcpyAsync(dt.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, S.st));
    gram_launch(gp, dA.as<double>(), dd.as<double>(), dslab.as<double>(), dT.as<double>(), dt.as<int>(), S.st);
    for (int w = 0; w < nw; ++w)
        MBFIR_HIP(hipMemcpy2DAsync(out + (size_t)w * nt * nt, (size_t)nt * 8, dT.as<double>() + w * ld * ld, ld * 8,
                                   (size_t)nt * 8, nt, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
}

// The operators of one unit at a caller's iterate (include/mbfir.h: mbfir_test_unit_ops).  The unit is set up by the stages of
// solve_lanes (setup_unit), scaled as launch_head scales it (launch_scaling), and every product goes through the solve's own launch
// code: apply_G, apply_GT, apply_G_winv2, build_H(0).  The operands sit in work buffers the scaling does not write.
void Solver::test_unit_ops(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, const UnitOps& io) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const int nlanes = int(Qs.size()), nv = io.nv;
    if (nlanes < 1 || nlanes > MAX_LANES) throw ShapeError("lock-step batch: bad lane count");
    if (nv < 1 || nv > 2) throw HipError("test_unit_ops: one or two vectors");
    std::vector<LaneHost> LH(nlanes);
    for (int b = 0; b < nlanes; ++b) LH[b].live = !io.mask || io.mask[b] != 0;
    S.setup_unit(Qs, o, LH);
    S.evused = 0; S.capev_used = 0; S.cap_flop_sum = 0;
    S.timing = false;
    S.chol_launch_count = 0; S.dd_epoch = 0;
    S.taps_valid = false;
    const DProg& P = S.P;
    const size_t np2 = (size_t)P.np * P.np;
    if (io.ldx < P.N || io.ldx > P.LDV || io.ldr < P.R || io.ldr > P.Rp || io.ldh != P.np)
        throw HipError("test_unit_ops: ldx / ldr / ldh do not fit the unit (N " + std::to_string(P.N) + ", R " + std::to_string(P.R) + ", np " + std::to_string(P.np) + ")");
    DevBuf keep(np2 * sizeof(double) * nlanes);
    double *dv = S.dx2, *du = S.dz2, *dsub = S.gdx2, *dgv = S.tmpR, *dgtu = S.tmpN, *dwgv = S.wpR, *dgout = S.bz2;
    const size_t xb = sizeof(double) * io.ldx, rb = sizeof(double) * io.ldr;
    // host block of lane b <-> the lane's device vectors (nv vectors LDV or Rp apart)
    auto lane = [&](double* p, int b) { return reinterpret_cast<double*>(reinterpret_cast<char*>(p) + (size_t)b * S.lane_bytes); };
    auto up = [&](double* dst, size_t dpitch, const double* src, size_t row, int rows, int b) {
        MBFIR_HIP(hipMemcpy2DAsync(lane(dst, b), dpitch * sizeof(double), src + (size_t)b * rows * (row / sizeof(double)), row, row, rows, hipMemcpyHostToDevice, S.st));
    };
    auto down = [&](double* dst, const double* src, size_t spitch, size_t row, int rows, int b) {
        MBFIR_HIP(hipMemcpy2DAsync(dst + (size_t)b * rows * (row / sizeof(double)), row, lane(const_cast<double*>(src), b), spitch * sizeof(double), row, rows, hipMemcpyDeviceToHost, S.st));
    };
    for (int b = 0; b < nlanes; ++b) {
        up(dv, P.LDV, io.v, xb, nv, b); up(du, P.Rp, io.u, rb, nv, b);
        if (io.sub) up(dsub, P.Rp, io.sub, rb, nv, b);
        up(S.s, P.Rp, io.s, rb, 1, b); up(S.z, P.Rp, io.z, rb, 1, b);
        up(dgv, P.Rp, io.gv, rb, nv, b); up(dgtu, P.LDV, io.gtu, xb, nv, b); up(dwgv, P.Rp, io.wgv, rb, nv, b);
        MBFIR_HIP(hipMemcpyAsync(lane(S.H, b), io.H + (size_t)b * np2, np2 * sizeof(double), hipMemcpyHostToDevice, S.st));
    }
    S.launch_scaling();
    if (nv == 1) {
        S.apply_G<1>(dv, dgv);
        S.apply_GT<1>(du, dgtu);
        S.apply_G_winv2<1>(dv, dgout, io.sub ? dsub : nullptr, dwgv);
    } else {
        S.apply_G<2>(dv, dgv);
        S.apply_GT<2>(du, dgtu);
        S.apply_G_winv2<2>(dv, dgout, io.sub ? dsub : nullptr, dwgv);
    }
    S.H_keep = keep.as<double>();
    try { S.build_H(0); } catch (...) { S.H_keep = nullptr; throw; }
    S.H_keep = nullptr;
    for (int b = 0; b < nlanes; ++b) {
        down(io.gv, dgv, P.Rp, rb, nv, b); down(io.gtu, dgtu, P.LDV, xb, nv, b); down(io.wgv, dwgv, P.Rp, rb, nv, b);
        MBFIR_HIP(hipMemcpyAsync(io.H + (size_t)b * np2, keep.as<double>() + (size_t)b * np2, np2 * sizeof(double), hipMemcpyDeviceToHost, S.st));
    }
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    const LatticeInfo& L0 = LH[0].Lt;
    long empty = 0;
    for (size_t k = 0; k < L0.wf.size(); ++k) empty += (L0.fold_pos[k] < 0 || L0.fold_neg[k] < 0) ? 1 : 0;
    long* r = io.report;
    for (int i = 0; i < UNIT_OPS_REPORT; ++i) r[i] = 0;
    r[UO_LATTICE] = P.trig; r[UO_PAIR_PASSES] = S.n_pair; r[UO_ONE_PASS] = S.h_one_pass ? 1 : 0;
    r[UO_D1] = P.D1; r[UO_USEG] = P.useg; r[UO_NFOLD] = P.nfold; r[UO_NCHUNK] = P.nchunk; r[UO_CGRP] = P.cgrp; r[UO_NP] = P.np;
    r[UO_EMPTY_SIDE] = empty; r[UO_SEG] = P.seg; r[UO_HETERO] = P.dims ? 1 : 0; r[UO_SEEDS_SHARED] = P.seeds_shared;
    r[UO_GV_PASSES] = S.n_gv; r[UO_GTV_PASSES] = S.n_gtv; r[UO_LANES] = nlanes;
    *io.tmin = P.tmin;
}

// The cone stages of one iteration at a caller's iterate (include/mbfir.h: mbfir_test_unit_cone).  The unit is set up by the stages
// of solve_lanes (setup_unit); what the three KKT solves of an iteration would have produced is uploaded into the buffers they
// write, and the stages of launch_iteration run between the uploads exactly as they run between the solves.  Every output buffer
// holds the caller's sentinel when its stage starts and is read back when the stage ends (a later stage may write it again), the
// scalars and the mailbox RB with it.
void Solver::test_unit_cone(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, const UnitCone& io) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const int nlanes = int(Qs.size());
    if (nlanes < 1 || nlanes > MAX_LANES) throw ShapeError("lock-step batch: bad lane count");
    std::vector<LaneHost> LH(nlanes);
    for (int b = 0; b < nlanes; ++b) LH[b].live = !io.mask || io.mask[b] != 0;
    S.setup_unit(Qs, o, LH);
    S.evused = 0; S.capev_used = 0; S.cap_flop_sum = 0;
    S.timing = false;
    S.chol_launch_count = 0; S.dd_epoch = 0;
    S.taps_valid = false;
    const DProg& P = S.P;
    if (io.ldx < P.N || io.ldx > P.LDV || io.ldr < P.R || io.ldr > P.Rp || io.ldw != 4 * std::max(P.nq3, 1))
        throw HipError("test_unit_cone: ldx / ldr / ldw do not fit the unit (N " + std::to_string(P.N) + ", R " + std::to_string(P.R) + ", n_q3 " + std::to_string(P.nq3) + ")");
    const int two = io.form ? 1 : 0;
    const size_t ldx = io.ldx, ldr = io.ldr, ldw = io.ldw;
    auto lane = [&](const double* p, int b) { return reinterpret_cast<double*>(reinterpret_cast<char*>(const_cast<double*>(p)) + (size_t)b * S.lane_bytes); };
    auto h2d = [&](double* dst, const double* src, size_t n, int b) { MBFIR_HIP(hipMemcpyAsync(lane(dst, b), src, n * sizeof(double), hipMemcpyHostToDevice, S.st)); };
    auto d2h = [&](double* dst, const double* src, size_t n, int b) { MBFIR_HIP(hipMemcpyAsync(dst, lane(src, b), n * sizeof(double), hipMemcpyDeviceToHost, S.st)); };
    auto in_r = [&](int b, int row) { return io.in_r + ((size_t)b * UC_IN_R + row) * ldr; };
    auto in_x = [&](int b, int row) { return io.in_x + ((size_t)b * UC_IN_X + row) * ldx; };
    auto out_r = [&](int b, int row) { return io.out_r + ((size_t)b * UC_OUT_R + row) * ldr; };
    auto out_x = [&](int b, int row) { return io.out_x + ((size_t)b * UC_OUT_X + row) * ldx; };
    // an output of a stage: device buffer, its block in out_r (space 0; `n` entries), out_x (1) or out_w3 (2); inplace: the live lanes'
    // buffer holds an input of the stage, only the masked lanes get the sentinel
    struct Out { double* dev; int space, row; bool inplace; size_t n; };
    auto host_of = [&](const Out& q, int b) { return q.space == 0 ? out_r(b, q.row) : q.space == 1 ? out_x(b, q.row) : io.out_w3 + (size_t)b * ldw; };
    auto R_ = [&](double* dev, int row, bool inplace = false) { return Out{dev, 0, row, inplace, ldr}; };
    auto X_ = [&](double* dev, int row, bool inplace = false) { return Out{dev, 1, row, inplace, ldx}; };
    auto before = [&](const std::vector<Out>& outs) {
        for (int b = 0; b < nlanes; ++b)
            for (const Out& q : outs)
                if (!(q.inplace && LH[b].live)) h2d(q.dev, host_of(q, b), q.n, b);
    };
    std::vector<double> snap((size_t)UC_SNAPS * nlanes * (S_COUNT + 3), std::nan(""));
    std::vector<char> snapped(UC_SNAPS, 0);
    auto after = [&](const std::vector<Out>& outs, int k) {
        for (int b = 0; b < nlanes; ++b) {
            for (const Out& q : outs) d2h(host_of(q, b), q.dev, q.n, b);
            double* h = snap.data() + ((size_t)k * nlanes + b) * (S_COUNT + 3);
            d2h(h, S.Sc, S_COUNT, b); d2h(h + S_COUNT, S.RB, 3, b);
        }
        snapped[k] = 1;
    };
    // ---- inputs: the iterate, the residuals, the three solves' solutions, the scalars ------------------------------------------
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        h2d(S.s, in_r(b, UCR_S), ldr, b); h2d(S.z, in_r(b, UCR_Z), ldr, b); h2d(S.rz, in_r(b, UCR_RZ), ldr, b);
        h2d(S.bz2, in_r(b, UCR_BZ2), ldr, b); h2d(S.bz2 + P.Rp, in_r(b, UCR_BZ2 + 1), ldr, b);
        h2d(S.dz2, in_r(b, UCR_Z1), ldr, b); h2d(S.dz2 + P.Rp, in_r(b, UCR_Z2), ldr, b);
        h2d(S.gdx2, in_r(b, UCR_G1), ldr, b); h2d(S.gdx2 + P.Rp, in_r(b, UCR_G2), ldr, b);
        h2d(S.dzc, in_r(b, UCR_ZC), ldr, b); h2d(S.gdxc, in_r(b, UCR_GC), ldr, b);
        h2d(S.kz, in_r(b, UCR_KZ), ldr, b); h2d(S.kg, in_r(b, UCR_KG), ldr, b);
        h2d(S.tmpR, in_r(b, UCR_SHIFT), ldr, b);
        h2d(S.x, in_x(b, UCX_X), ldx, b); h2d(S.rx, in_x(b, UCX_RX), ldx, b);
        h2d(S.dx2, in_x(b, UCX_X1), ldx, b); h2d(S.dx2 + P.LDV, in_x(b, UCX_X2), ldx, b);
        h2d(S.dxc, in_x(b, UCX_XC), ldx, b); h2d(S.kx, in_x(b, UCX_KX), ldx, b);
        const double* sc = io.in_sc + (size_t)b * UC_IN_SC;
        const int slot[UC_IN_SC] = {S_TAU, S_KAPPA, S_MU, S_RT, S_SIGMAX, S_DRES, S_NRMC, S_RNC};
        for (int q = 0; q < UC_IN_SC; ++q) h2d(S.Sc + slot[q], sc + q, 1, b);
    }
    // ---- the stages of launch_iteration, the uploads above in place of its solves ---------------------------------------------------
    std::vector<Out> outs = {R_(S.dl, UCO_DL), R_(S.wl, UCO_WL), R_(S.lam, UCO_LAM), R_(S.wbz, UCO_WBZ2), R_(S.wbz + P.Rp, UCO_WBZ2 + 1),
                             Out{S.w3, 2, 0, false, ldw}, Out{S.wbb, 0, UCO_WBB, false, (size_t)std::max(P.big, 1)}};
    before(outs); S.launch_scaling(); after(outs, UCS_SCALING);
    outs = {R_(S.dssa, UCO_DSSA), R_(S.wdza, UCO_WDZA)};
    if (two) outs.push_back(X_(S.bxc, UCOX_BXC));
    before(outs); const int ns0 = S.stage_pred_tail(two); after(outs, UCS_PRED);
    outs = {R_(S.lds, UCO_LDS), R_(S.bzc, UCO_BZC), R_(S.wbz, UCO_WBZC)};
    if (!two) outs.push_back(X_(S.bxc, UCOX_BXC));
    before(outs); S.stage_comb_rhs(ns0, two); after(outs, UCS_COMB_RHS);
    outs = {R_(S.ds, UCO_DS), R_(S.dz, UCO_DZ)};
    before(outs); const int ns1 = S.stage_comb_tail(two); after(outs, UCS_COMB);
    const std::vector<Out> moved = {X_(S.x, UCOX_X, true), R_(S.s, UCO_S, true), R_(S.z, UCO_Z, true)};
    if (!io.corr) {
        before(moved); S.stage_update(ns1, two); after(moved, UCS_UPDATE);
    } else {
        outs = {R_(S.kbz, UCO_KBZ), R_(S.wbz, UCO_WBZK)};
        before(outs); S.stage_corr_rhs(ns1, S.sw.corr_big ? 1 : 0, nullptr, two); after(outs, UCS_CORR_RHS);
        outs = {X_(S.kx, UCOX_KX, true), R_(S.kz, UCO_KZ, true), R_(S.kg, UCO_KG, true), R_(S.kds, UCO_KDS), R_(S.kdz, UCO_KDZ)};
        outs.insert(outs.end(), moved.begin(), moved.end());
        before(outs); S.stage_corr_tail(two); after(outs, UCS_UPDATE);
    }
    outs = {R_(S.tmpR, UCO_SHIFT, true)};
    before(outs); S.cone_shift(S.tmpR); after(outs, UCS_SHIFT);
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    // the scalars of every stage that ran, live lanes only (a masked lane's block stays the caller's)
    const int pick[UC_SC - 3] = {S_ETAB, S_TAU, S_KAPPA, S_SIGMA, S_ALPHA, S_ALPHA_A, S_DTAU, S_DKAP, S_DTAU_A, S_DKAP_A, S_TMAX, S_TAU0, S_KAP0,
                                 S_ALPHA0, S_DTAU_C, S_DKAP_C, S_PICK, S_NCORR, S_NPICK, S_WB0, S_MU};
    for (int k = 0; k < UC_SNAPS; ++k)
        for (int b = 0; b < nlanes; ++b) {
            if (!snapped[k] || !LH[b].live) continue;
            const double* h = snap.data() + ((size_t)k * nlanes + b) * (S_COUNT + 3);
            double* d = io.out_sc + ((size_t)b * UC_SNAPS + k) * UC_SC;
            for (int q = 0; q < UC_SC - 3; ++q) d[q] = h[pick[q]];
            for (int q = 0; q < 3; ++q) d[UC_SC - 3 + q] = h[S_COUNT + q];
        }
    long* r = io.report;
    for (int i = 0; i < UNIT_CONE_REPORT; ++i) r[i] = 0;
    r[0] = std::max(S.nbC, 1); r[1] = P.l; r[2] = P.nq3; r[3] = P.big; r[4] = P.N; r[5] = P.R; r[6] = P.dims ? 1 : 0; r[7] = nlanes;
    r[8] = S.sw.fuse ? 1 : 0; r[9] = S.sw.corr_big ? 1 : 0; r[10] = two; r[11] = ns0; r[12] = ns1; r[13] = S.unknown_blocks();
}

// The residual kernels and the plain KKT solve of one unit at a caller's iterate (include/mbfir.h: mbfir_test_unit_kkt).  The unit
// is set up by the stages of solve_lanes (setup_unit); launch_residuals, launch_scaling, build_H and kkt_solve (or initial_point) run
// as a solve runs them, kkt_solve with an observer that enqueues the copies of what each group of launches wrote and sends the
// caller's sentinels into the buffers the next group writes.  Nothing synchronises between the launches.
void Solver::test_unit_kkt(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, const UnitKkt& io) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const int nlanes = int(Qs.size()), nv = io.nv;
    if (nlanes < 1 || nlanes > MAX_LANES) throw ShapeError("lock-step batch: bad lane count");
    std::vector<LaneHost> LH(nlanes);
    for (int b = 0; b < nlanes; ++b) LH[b].live = !io.mask || io.mask[b] != 0;
    S.setup_unit(Qs, o, LH);
    S.evused = 0; S.capev_used = 0; S.cap_flop_sum = 0;
    S.timing = false;
    S.chol_launch_count = 0; S.dd_epoch = 0;
    S.taps_valid = false;
    const DProg& P = S.P;
    if (io.ldx < P.N || io.ldx > P.LDV || io.ldr < P.R || io.ldr > P.Rp || io.ldh != P.np || io.ldw != 4 * std::max(P.nq3, 1))
        throw HipError("test_unit_kkt: ldx / ldr / ldh / ldw do not fit the unit (N " + std::to_string(P.N) + ", R " + std::to_string(P.R) + ", np " +
                       std::to_string(P.np) + ", n_q3 " + std::to_string(P.nq3) + ")");
    const size_t ldx = io.ldx, ldr = io.ldr, np2 = (size_t)P.np * P.np;
    const bool initial = io.mode == 1;
    int ns_max = 0;
    std::vector<int> ns(nlanes, 0);
    for (int b = 0; b < nlanes; ++b) {
        ns[b] = LH[b].live ? io.nsweep[b] : 0;
        LH[b].nsweep = ns[b];
        ns_max = std::max(ns_max, ns[b]);
    }
    auto lane = [&](const double* p, int b) { return reinterpret_cast<double*>(reinterpret_cast<char*>(const_cast<double*>(p)) + (size_t)b * S.lane_bytes); };
    auto h2d = [&](double* dst, const double* src, size_t n, int b) { MBFIR_HIP(hipMemcpyAsync(lane(dst, b), src, n * sizeof(double), hipMemcpyHostToDevice, S.st)); };
    auto d2h = [&](double* dst, const double* src, size_t n, int b) { MBFIR_HIP(hipMemcpyAsync(dst, lane(src, b), n * sizeof(double), hipMemcpyDeviceToHost, S.st)); };
    // the solve's buffers: the batch solve's (two right-hand sides) or the combined solve's (one)
    double *bx = nv == 2 ? S.bx2 : S.bxc, *bz = nv == 2 ? S.bz2 : S.bzc, *dx = nv == 2 ? S.dx2 : S.dxc, *dz = nv == 2 ? S.dz2 : S.dzc,
           *gdx = nv == 2 ? S.gdx2 : S.gdxc;
    const int slot = nv == 2 ? S_RNA : S_RNB;
    // block `blk` of out_x (space 1) or out_r (space 0): nv vectors, LDV resp. Rp apart on the device
    auto host_of = [&](int space, int b, int blk, int v) {
        return space ? io.out_x + (((size_t)b * UK_OUT_X + blk) * 2 + v) * ldx : io.out_r + (((size_t)b * UK_OUT_R + blk) * 2 + v) * ldr;
    };
    struct Blk { double* dev; int space, blk; };
    auto X_ = [&](double* dev, int blk) { return Blk{dev, 1, blk}; };
    auto R_ = [&](double* dev, int blk) { return Blk{dev, 0, blk}; };
    auto plant = [&](const std::vector<Blk>& bs) {
        for (int b = 0; b < nlanes; ++b)
            for (const Blk& q : bs)
                for (int v = 0; v < nv; ++v) h2d(q.dev + (size_t)v * (q.space ? P.LDV : P.Rp), host_of(q.space, b, q.blk, v), q.space ? ldx : ldr, b);
    };
    // (in-place blocks: the lanes that run the sweep; fresh ones: every lane -- a lane the mask switches off returns the sentinel)
    auto grab = [&](const std::vector<Blk>& bs, int need = -1) {
        for (int b = 0; b < nlanes; ++b) {
            if (need >= 0 && !(LH[b].live && ns[b] >= need)) continue;
            for (const Blk& q : bs)
                for (int v = 0; v < nv; ++v) d2h(host_of(q.space, b, q.blk, v), q.dev + (size_t)v * (q.space ? P.LDV : P.Rp), q.space ? ldx : ldr, b);
        }
    };
    std::vector<double> snap((size_t)UK_SNAPS * nlanes * S_COUNT, 0.0);
    std::vector<int> snap_need(UK_SNAPS, -1);               // a lane returns snapshot k if it runs at least that many sweeps
    auto snapshot = [&](int k, int need) {
        for (int b = 0; b < nlanes; ++b) d2h(snap.data() + ((size_t)k * nlanes + b) * S_COUNT, S.Sc, S_COUNT, b);
        snap_need[k] = need;
    };
    // ---- the iterate, then the residual kernels ------------------------------------------------------------------------------------
    const int res_pick[14] = {S_RT, S_MU, S_PCOST, S_DCOST, S_GAP, S_RELGAP, S_PRES, S_DRES, S_PINF, S_DINF, S_CX, S_HZ, S_SZ, S_CHOLFIX};
    double* rmail = io.form ? S.GTz + P.LDV : S.RB;
    for (int b = 0; b < nlanes; ++b) {
        double* rr = io.res_r + (size_t)b * UK_RES_R * ldr;
        double* rxh = io.res_x + (size_t)b * UK_RES_X * ldx;
        const double* sc = io.res_sc + (size_t)b * UK_RES_SC;
        if (LH[b].live) {
            h2d(S.s, io.s + (size_t)b * ldr, ldr, b); h2d(S.z, io.z + (size_t)b * ldr, ldr, b); h2d(S.x, io.x + (size_t)b * ldx, ldx, b);
            h2d(S.Sc + S_TAU, io.tau_kappa + 2 * (size_t)b, 1, b); h2d(S.Sc + S_KAPPA, io.tau_kappa + 2 * (size_t)b + 1, 1, b);
        }
        h2d(S.rz, rr, ldr, b); h2d(S.bz2, rr + ldr, ldr, b); h2d(S.bz2 + P.Rp, rr + 2 * ldr, ldr, b);
        h2d(S.GTz, rxh, ldx, b); h2d(S.rx, rxh + ldx, ldx, b); h2d(S.bx2, rxh + 2 * ldx, ldx, b); h2d(S.bx2 + P.LDV, rxh + 3 * ldx, ldx, b);
        for (int q = 0; q < 14; ++q) h2d(S.Sc + res_pick[q], sc + q, 1, b);
        h2d(rmail, sc + 19, 5, b);
    }
    S.launch_residuals(io.form ? 1 : 0);
    std::vector<double> res_snap((size_t)nlanes * (S_COUNT + 5), 0.0);
    for (int b = 0; b < nlanes; ++b) {
        double* rr = io.res_r + (size_t)b * UK_RES_R * ldr;
        double* rxh = io.res_x + (size_t)b * UK_RES_X * ldx;
        d2h(rr, S.rz, ldr, b); d2h(rr + ldr, S.bz2, ldr, b); d2h(rr + 2 * ldr, S.bz2 + P.Rp, ldr, b);
        d2h(rxh, S.GTz, ldx, b); d2h(rxh + ldx, S.rx, ldx, b); d2h(rxh + 2 * ldx, S.bx2, ldx, b); d2h(rxh + 3 * ldx, S.bx2 + P.LDV, ldx, b);
        d2h(res_snap.data() + (size_t)b * (S_COUNT + 5), S.Sc, S_COUNT, b);
        d2h(res_snap.data() + (size_t)b * (S_COUNT + 5) + S_COUNT, rmail, 5, b);
    }
    // ---- the right-hand sides, the scaling and the factor; or the initial point's own ------------------------------------------------
    // the norm slots and the sweep's scalars hold the sentinel (out_sc as the caller filled it) until a kernel writes them
    for (int b = 0; b < nlanes; ++b) {
        const double* sc = io.out_sc + (size_t)b * UK_SNAPS * UK_SC;
        h2d(S.Sc + slot, sc, MAX_SWEEPS + 1, b); h2d(S.Sc + S_CG_RZ, sc + 9, 2, b); h2d(S.Sc + S_CG_ALPHA, sc + 11, 2, b);
    }
    KktObserver obs;
    obs.two_launch_cg = io.two != 0;
    const bool z_written = !(S.sw.fuse && S.fused_hsolve);
    obs.fn = [&](int stage, int q) {
        switch (stage) {
            case KKT_ST_WBZ: grab({R_(S.wbz, UKR_WBZ)}); plant({X_(S.tmpN, UKX_T1)}); break;
            case KKT_ST_GTWBZ: grab({X_(S.tmpN, UKX_T1)}); plant({X_(dx, UKX_DX0)}); break;
            case KKT_ST_HSOLVE: grab({X_(dx, UKX_DX0)}); plant({R_(gdx, UKR_GDX0), R_(dz, UKR_DZ0)}); break;
            case KKT_ST_GDX: grab({R_(gdx, UKR_GDX0), R_(dz, UKR_DZ0)}); plant({X_(S.tmpN, UKX_T4), X_(S.rhsN, UKX_R0)}); break;
            case KKT_ST_RESID:
                grab({X_(S.tmpN, UKX_T4), X_(S.rhsN, UKX_R0)}); snapshot(UKS_RESID, 0);
                if (ns_max > 0) plant({X_(S.pN, UKX_P), X_(S.tmpN2, UKX_P + 1)});
                break;
            case KKT_ST_START:
                grab({X_(S.pN, UKX_P)}); if (z_written) grab({X_(S.tmpN2, UKX_P + 1)});
                snapshot(UKS_START, 1);
                plant({R_(S.tmpR, UKR_GP), R_(S.wpR, UKR_GP + 1)});
                break;
            case KKT_ST_GP: grab({R_(S.tmpR, UKR_GP + 4 * q), R_(S.wpR, UKR_GP + 4 * q + 1)}); plant({X_(S.tmpN, UKX_HP + 3 * q)}); break;
            case KKT_ST_HP: grab({X_(S.tmpN, UKX_HP + 3 * q)}); break;
            case KKT_ST_STEP:
                grab({X_(dx, UKX_HP + 3 * q + 1), X_(S.rhsN, UKX_HP + 3 * q + 2), R_(gdx, UKR_GP + 4 * q + 2), R_(dz, UKR_GP + 4 * q + 3)}, q + 1);
                snapshot(UKS_STEP + q, q + 1);
                if (q + 1 < ns_max) {
                    plant({X_(S.tmpN2, UKX_P + 2 * (q + 1) + 1), R_(S.tmpR, UKR_GP + 4 * (q + 1)), R_(S.wpR, UKR_GP + 4 * (q + 1) + 1)});
                    // (p is updated in place: a lane that does not start sweep q + 1 keeps the caller's block on the host)
                }
                break;
            case KKT_ST_RESTART:
                grab({X_(S.pN, UKX_P + 2 * (q + 1))}, q + 2); if (z_written) grab({X_(S.tmpN2, UKX_P + 2 * (q + 1) + 1)});
                snapshot(UKS_START + q + 1, q + 2);
                break;
            default: break;
        }
    };
    if (!initial) {
        if (io.bx)
            for (int b = 0; b < nlanes; ++b) {
                if (!LH[b].live) continue;
                for (int v = 0; v < nv; ++v) {
                    h2d(bx + (size_t)v * P.LDV, io.bx + ((size_t)b * nv + v) * ldx, ldx, b);
                    h2d(bz + (size_t)v * P.Rp, io.bz + ((size_t)b * nv + v) * ldr, ldr, b);
                }
            }
        if (io.wbz_ready) plant({R_(S.wbz, UKR_WBZ)});
        S.launch_scaling();
        S.build_H(0);
        if (!io.wbz_ready) plant({R_(S.wbz, UKR_WBZ)});
        S.push_masks(LH);
        if (nv == 2) S.kkt_solve<2>(bx, bz, dx, dz, gdx, ns_max, slot, io.wbz_ready != 0, &obs);
        else S.kkt_solve<1>(bx, bz, dx, dz, gdx, ns_max, slot, false, &obs);
    } else {
        for (int b = 0; b < nlanes; ++b) {
            double* ir = io.init_r + (size_t)b * UK_INIT_R * ldr;
            h2d(S.dl, ir, ldr, b); h2d(S.wl, ir + ldr, ldr, b); h2d(S.wbb, ir + 2 * ldr, (size_t)std::max(P.big, 1), b);
            h2d(S.w3, io.init_w3 + (size_t)b * io.ldw, io.ldw, b);
            double* ix = io.init_x + (size_t)b * UK_INIT_X * ldx;
            h2d(S.bz2, ir + 5 * ldr, ldr, b); h2d(S.bz2 + P.Rp, ir + 6 * ldr, ldr, b);
            h2d(S.bx2, ix + ldx, ldx, b); h2d(S.bx2 + P.LDV, ix + 2 * ldx, ldx, b);
            if (!LH[b].live) { h2d(S.s, ir + 3 * ldr, ldr, b); h2d(S.z, ir + 4 * ldr, ldr, b); h2d(S.x, ix, ldx, b); }
        }
        plant({R_(S.wbz, UKR_WBZ)});
        S.push_masks(LH);
        S.initial_point(ns_max, &obs);
        for (int b = 0; b < nlanes; ++b) {
            double* ir = io.init_r + (size_t)b * UK_INIT_R * ldr;
            d2h(ir, S.dl, ldr, b); d2h(ir + ldr, S.wl, ldr, b); d2h(ir + 2 * ldr, S.wbb, (size_t)std::max(P.big, 1), b);
            d2h(io.init_w3 + (size_t)b * io.ldw, S.w3, io.ldw, b);
            double* ix = io.init_x + (size_t)b * UK_INIT_X * ldx;
            d2h(ir + 3 * ldr, S.s, ldr, b); d2h(ir + 4 * ldr, S.z, ldr, b); d2h(ix, S.x, ldx, b);
            d2h(ir + 5 * ldr, S.bz2, ldr, b); d2h(ir + 6 * ldr, S.bz2 + P.Rp, ldr, b);
            d2h(ix + ldx, S.bx2, ldx, b); d2h(ix + 2 * ldx, S.bx2 + P.LDV, ldx, b);
        }
    }
    // what the solve leaves: the inverse factor, the pivot counter, the solution and the residual
    std::vector<int> fl(nlanes, 0);
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        MBFIR_HIP(hipMemcpyAsync(io.M + (size_t)b * np2, lane(S.M, b), np2 * sizeof(double), hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipMemcpyAsync(&fl[b], reinterpret_cast<char*>(S.flag) + (size_t)b * S.lane_bytes, sizeof(int), hipMemcpyDeviceToHost, S.st));
    }
    grab({X_(dx, UKX_DX_END), X_(S.rhsN, UKX_R_END), R_(gdx, UKR_GDX_END), R_(dz, UKR_DZ_END)}, 0);
    snapshot(UKS_END, 0);
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        io.flag[b] = fl[b];
        const double* h = res_snap.data() + (size_t)b * (S_COUNT + 5);
        double* d = io.res_sc + (size_t)b * UK_RES_SC;
        const int more[5] = {S_TAU, S_KAPPA, S_NRMH, S_NRMC, S_DEG};
        for (int q = 0; q < 14; ++q) d[q] = h[res_pick[q]];
        for (int q = 0; q < 5; ++q) d[14 + q] = h[more[q]];
        for (int q = 0; q < 5; ++q) d[19 + q] = h[S_COUNT + q];
        for (int k = 0; k < UK_SNAPS; ++k) {
            if (snap_need[k] < 0 || ns[b] < snap_need[k]) continue;
            const double* hs = snap.data() + ((size_t)k * nlanes + b) * S_COUNT;
            double* ds = io.out_sc + ((size_t)b * UK_SNAPS + k) * UK_SC;
            for (int q = 0; q <= MAX_SWEEPS; ++q) ds[q] = hs[slot + q];
            ds[9] = hs[S_CG_RZ]; ds[10] = hs[S_CG_RZ + 1]; ds[11] = hs[S_CG_ALPHA]; ds[12] = hs[S_CG_ALPHA + 1];
        }
    }
    long* r = io.report;
    for (int i = 0; i < UNIT_KKT_REPORT; ++i) r[i] = 0;
    r[0] = S.fused_hsolve ? 1 : 0; r[1] = S.sw.fuse ? 1 : 0; r[2] = io.form ? 1 : 0; r[3] = P.N; r[4] = P.R; r[5] = P.np; r[6] = P.big;
    r[7] = nlanes; r[8] = P.dims ? 1 : 0; r[9] = P.trig; r[10] = cdiv(P.Nt, GTC) + 1; r[11] = nv; r[12] = io.two ? 1 : 0;
    r[13] = io.wbz_ready ? 1 : 0; r[14] = initial ? 1 : 0; r[15] = ns_max; r[16] = P.l; r[17] = P.nq3; r[18] = S.nbR; r[19] = z_written ? 1 : 0;
    r[20] = S.n_gv; r[21] = S.n_gtv;
}

// The extended-precision path of one unit at a caller's iterate (include/mbfir.h: mbfir_test_unit_ddkkt).  The unit is set up by the
// stages of solve_lanes (setup_unit); launch_scaling, dd_prepare / dd_prepare_lanes, push_masks, build_H(dd_k) and solve_modes run as
// launch_head and launch_iteration run them, kkt_solve_dd with an observer that enqueues the copies of what each group of launches
// wrote and sends the caller's sentinels into the buffers the next group writes -- on the lanes in the extended-precision mode alone:
// a lane in the plain mode keeps W^-2 bz from the scaling in the buffer the other lanes' passes write.  The one synchronisation is the
// selection's own.
void Solver::test_unit_ddkkt(const std::vector<const TrigProgram*>& Qs, const SolveOpts& o, const UnitDdKkt& io) {
    static_assert(DK_KMAX == DD_KMAX && DK_SC == MAX_SWEEPS + 1, "solver.h: the blocks of UnitDdKkt do not fit the solver's");
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const int nlanes = int(Qs.size()), nv = io.nv;
    if (nlanes < 1 || nlanes > MAX_LANES) throw ShapeError("lock-step batch: bad lane count");
    std::vector<LaneHost> LH(nlanes);
    for (int b = 0; b < nlanes; ++b) LH[b].live = !io.mask || io.mask[b] != 0;
    S.setup_unit(Qs, o, LH);
    S.evused = 0; S.capev_used = 0; S.cap_flop_sum = 0;
    S.timing = false;
    S.chol_launch_count = 0; S.dd_epoch = 0;
    S.taps_valid = false;
    const DProg& P = S.P;
    const int nq = std::max(P.nq3, 1), nbig = std::max(P.big, 1), nl1 = std::max(P.l, 1);
    if (io.ldx < P.N || io.ldx > P.LDV || io.ldr < P.R || io.ldr > P.Rp || io.ldh != P.np || io.ldw != 4 * nq || io.ldu < 64 || io.ldu > DD_KMAX || io.ldp < 1)
        throw HipError("test_unit_ddkkt: ldx / ldr / ldh / ldw / ldu do not fit the unit (N " + std::to_string(P.N) + ", R " + std::to_string(P.R) + ", np " +
                       std::to_string(P.np) + ", n_q3 " + std::to_string(P.nq3) + ", rows of U 64 .. " + std::to_string(DD_KMAX) + ")");
    const size_t ldx = io.ldx, ldr = io.ldr, ldu = io.ldu, np = P.np, np2 = np * np, ldi = ldr + 3 * (size_t)nq + 3;
    auto lane = [&](const void* p, int b) { return reinterpret_cast<char*>(const_cast<void*>(p)) + (size_t)b * S.lane_bytes; };
    auto h2d = [&](const void* dst, const void* src, size_t bytes, int b) { MBFIR_HIP(hipMemcpyAsync(lane(dst, b), src, bytes, hipMemcpyHostToDevice, S.st)); };
    auto d2h = [&](void* dst, const void* src, size_t bytes, int b) { MBFIR_HIP(hipMemcpyAsync(dst, lane(src, b), bytes, hipMemcpyDeviceToHost, S.st)); };
    const size_t D8 = sizeof(double), I4 = sizeof(int);
    double *bx = nv == 2 ? S.bx2 : S.bxc, *bz = nv == 2 ? S.bz2 : S.bzc, *dx = nv == 2 ? S.dx2 : S.dxc, *dz = nv == 2 ? S.dz2 : S.dzc,
           *gdx = nv == 2 ? S.gdx2 : S.gdxc;
    const int slot = nv == 2 ? S_RNA : S_RNB;
    // ---- the iterate and the right-hand sides; the norm slots hold the caller's sentinel until a kernel writes them --------------------
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        h2d(S.s, io.s + (size_t)b * ldr, ldr * D8, b); h2d(S.z, io.z + (size_t)b * ldr, ldr * D8, b);
        for (int v = 0; v < nv; ++v) {
            h2d(bx + (size_t)v * P.LDV, io.bx + ((size_t)b * nv + v) * ldx, ldx * D8, b);
            h2d(bz + (size_t)v * P.Rp, io.bz + ((size_t)b * nv + v) * ldr, ldr * D8, b);
        }
        h2d(S.Sc + slot, io.out_sc + (size_t)b * (DK_PASSES + 1) * DK_SC, (MAX_SWEEPS + 1) * D8, b);
    }
    // ---- the head of an iteration: scaling, strong sets (the one synchronisation), masks ------------------------------------------------
    S.launch_scaling();
    int ks[MAX_LANES] = {0};
    if (S.dd_unit) {
        bool lv[MAX_LANES];
        for (int b = 0; b < nlanes; ++b) lv[b] = LH[b].live;
        S.dd_k = S.dd_prepare_lanes(o.ddkkt_theta, ks, lv);
        S.dd_kp = int(round_up(std::max(S.dd_k, 1), 64));
    } else {
        ks[0] = S.dd_k = S.dd_prepare(o.ddkkt_theta);
    }
    for (int b = 0; b < nlanes; ++b) LH[b].dd_k = LH[b].live ? ks[b] : 0;
    S.push_masks(LH);
    const bool dd_any = S.dd_k > 0;
    bool pl_any = S.dd_k == 0;
    if (S.dd_unit) {
        pl_any = false;
        for (int b = 0; b < nlanes; ++b) pl_any = pl_any || (LH[b].live && LH[b].dd_k == 0);
    }
    const int kp = !dd_any ? 0 : !S.cap_form ? S.dd_k : S.dd_unit ? S.dd_kp : std::max(int(round_up(S.dd_k, 64)), S.sw.test_cap_kp);
    const size_t rows_u = std::min<size_t>(kp, ldu);
    const int nbp = std::max(S.nbC, 1) + (P.big ? 1 : 0);
    auto ddl = [&](int b) { return LH[b].live && LH[b].dd_k > 0; };
    // what the selection left, every live lane
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        double* r = io.sel_r + (size_t)b * DK_SEL_R * ldr;
        d2h(r, S.dl, nl1 * D8, b); d2h(r + ldr, S.D.dlc, nl1 * D8, b); d2h(r + 2 * ldr, S.wbb, nbig * D8, b); d2h(r + 3 * ldr, S.D.whb, nbig * D8, b);
        double* q = io.sel_q + (size_t)b * 18 * nq;
        d2h(q, S.w3, 4 * nq * D8, b); d2h(q + 4 * nq, S.D.e3, 8 * nq * D8, b); d2h(q + 12 * nq, S.D.m3c, 6 * nq * D8, b);
        double* sc = io.sel_sc + (size_t)b * DK_SEL_SC;
        d2h(sc, S.D.eb, 8 * D8, b); d2h(sc + 8, S.Sc + S_ETAB, D8, b);
        // the partial rows of (sum log, count) the selection folds: the big cone's first, then k_dd_prep's blocks
        d2h(io.sel_part + (size_t)b * 2 * io.ldp, S.partR, 2 * (size_t)std::min(nbp, io.ldp) * D8, b);
        int* si = io.sel_i + (size_t)b * ldi;
        d2h(si, S.D.slotl, nl1 * I4, b); d2h(si + ldr, S.D.slot3, 3 * nq * I4, b); d2h(si + ldr + 3 * nq, S.D.slotb, 2 * I4, b);
        d2h(si + ldr + 3 * nq + 2, S.D.kcnt, I4, b);
        const size_t kb = std::min(ks[b], DD_KMAX);
        int* st = io.strong_i + (size_t)b * 3 * DD_KMAX;
        d2h(st, S.D.skind, kb * I4, b); d2h(st + DD_KMAX, S.D.sidx, kb * I4, b); d2h(st + 2 * DD_KMAX, S.D.sdir, kb * I4, b);
        d2h(io.strong_x + (size_t)b * DD_KMAX, S.D.sX, kb * D8, b);
    }
    // ---- the capped normal matrix: H ahead of the factorisation, the rows of U over the caller's sentinel, the capacitance matrices --------
    DevBuf keep(np2 * D8 * nlanes), keepS(S.cap_form && dd_any ? (size_t)kp * kp * D8 * nlanes : 8);
    if (dd_any)
        for (int b = 0; b < nlanes; ++b)
            if (LH[b].live) h2d(S.D.U, io.U + (size_t)b * ldu * np, rows_u * np * D8, b);
    S.H_keep = keep.as<double>();
    if (S.cap_form && dd_any) S.capS_keep = keepS.as<double>();
    try { S.build_H(S.dd_k); } catch (...) { S.H_keep = nullptr; S.capS_keep = nullptr; throw; }
    S.H_keep = nullptr; S.capS_keep = nullptr;
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        MBFIR_HIP(hipMemcpyAsync(io.H + (size_t)b * np2, keep.as<double>() + (size_t)b * np2, np2 * D8, hipMemcpyDeviceToHost, S.st));
        if (dd_any) d2h(io.U + (size_t)b * ldu * np, S.D.U, rows_u * np * D8, b);
        if (!(S.cap_form && ddl(b) && io.Yt)) continue;
        d2h(io.Yt + (size_t)b * ldu * np, S.capYt, rows_u * np * D8, b); d2h(io.Zt + (size_t)b * ldu * np, S.capZt, rows_u * np * D8, b);
        MBFIR_HIP(hipMemcpy2DAsync(io.S + (size_t)b * ldu * ldu, ldu * D8, keepS.as<double>() + (size_t)b * kp * kp, (size_t)kp * D8, rows_u * D8, rows_u,
                                   hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipMemcpy2DAsync(io.Ms + (size_t)b * ldu * ldu, ldu * D8, lane(S.capMs, b), (size_t)kp * D8, rows_u * D8, rows_u, hipMemcpyDeviceToHost, S.st));
    }
    // ---- the solve: kkt_solve_dd under ROW_DD with the observer, the plain kkt_solve under ROW_PL ------------------------------------------
    struct Blk { double* dev; int space, blk; };            // space 0: rows (Rp apart), 1: unknowns (LDV apart), 2: strong slots (DD_KMAX apart)
    auto X_ = [&](double* dev, int blk) { return Blk{dev, 1, blk}; };
    auto R_ = [&](double* dev, int blk) { return Blk{dev, 0, blk}; };
    auto K_ = [&](double* dev, int blk) { return Blk{dev, 2, blk}; };
    auto host_of = [&](const Blk& q, int b, int pass, int v) {
        const size_t lp = (size_t)b * DK_PASSES + pass;
        return q.space == 1 ? io.out_x + (((lp * DK_OUT_X) + q.blk) * 2 + v) * ldx
             : q.space == 0 ? io.out_r + (((lp * DK_OUT_R) + q.blk) * 2 + v) * ldr
                            : io.out_k + (((lp * DK_OUT_K) + q.blk) * 2 + v) * (size_t)DD_KMAX;
    };
    auto dstride = [&](const Blk& q) { return q.space == 1 ? (size_t)P.LDV : q.space == 0 ? (size_t)P.Rp : (size_t)DD_KMAX; };
    auto hlen = [&](const Blk& q) { return q.space == 1 ? ldx : q.space == 0 ? ldr : (size_t)DD_KMAX; };
    auto plant = [&](int pass, const std::vector<Blk>& bs) {
        if (pass >= DK_PASSES) return;
        for (int b = 0; b < nlanes; ++b)
            for (const Blk& q : bs)
                for (int v = 0; ddl(b) && v < nv; ++v) h2d(q.dev + (size_t)v * dstride(q), host_of(q, b, pass, v), hlen(q) * D8, b);
    };
    auto grab = [&](int pass, const std::vector<Blk>& bs) {
        if (pass >= DK_PASSES) return;
        for (int b = 0; b < nlanes; ++b)
            for (const Blk& q : bs)
                for (int v = 0; ddl(b) && v < nv; ++v) d2h(host_of(q, b, pass, v), q.dev + (size_t)v * dstride(q), hlen(q) * D8, b);
    };
    double *Bh = S.ddB, *Bl = S.ddB + 2L * P.LDV;
    const bool cap = S.cap_form;
    KktObserver obs;
    obs.fn = [&](int stage, int q) {
        switch (stage) {
            case DD_ST_R1:
                grab(q, {X_(S.tmpN, DKX_GTDZ), X_(S.rhsN, DKX_R1)});
                for (int b = 0; q < DK_PASSES && b < nlanes; ++b)
                    if (ddl(b)) d2h(io.out_sc + ((size_t)b * (DK_PASSES + 1) + q) * DK_SC, S.Sc + slot, (MAX_SWEEPS + 1) * D8, b);
                plant(q, {R_(S.tmpR, DKR_R2), K_(S.ddtS, DKK_TS)});
                break;
            case DD_ST_R2: grab(q, {R_(S.tmpR, DKR_R2), K_(S.ddtS, DKK_TS)}); plant(q, {R_(S.wbz, DKR_WBZ)}); break;
            case DD_ST_WBZ: grab(q, {R_(S.wbz, DKR_WBZ)}); plant(q, {X_(S.tmpN2, DKX_GTW)}); break;
            case DD_ST_GTW:
                grab(q, {X_(S.tmpN2, DKX_GTW)});
                if (cap) plant(q, {X_(Bl, DKX_RHS_L)}); else plant(q, {X_(Bh, DKX_RHS_H), X_(Bl, DKX_RHS_L)});
                break;
            case DD_ST_RHS:
                if (cap) { grab(q, {X_(Bl, DKX_RHS_L)}); plant(q, {X_(S.tmpN2, DKX_Y)}); }
                else grab(q, {X_(Bh, DKX_RHS_H), X_(Bl, DKX_RHS_L)});
                break;
            case DD_ST_Y: grab(q, {X_(S.tmpN2, DKX_Y)}); plant(q, {K_(S.capw, DKK_CAPW)}); break;
            case DD_ST_CAPW: grab(q, {K_(S.capw, DKK_CAPW)}); plant(q, {K_(S.ddzeta, DKK_ZETA)}); break;
            case DD_ST_ZETAC: grab(q, {K_(S.ddzeta, DKK_ZETA)}); plant(q, {X_(Bh, DKX_BH)}); break;
            case DD_ST_SOLVE:
                grab(q, {X_(Bh, DKX_BH)}); if (!cap) grab(q, {X_(Bl, DKX_BL)});
                plant(q, {R_(S.wpR, DKR_GBH)});
                break;
            case DD_ST_GBH: grab(q, {R_(S.wpR, DKR_GBH)}); plant(q, {R_(S.wbz, DKR_WBZ2)}); break;
            case DD_ST_WBZ2: grab(q, {R_(S.wbz, DKR_WBZ2)}); if (!cap) plant(q, {K_(S.ddzeta, DKK_ZETA)}); break;
            case DD_ST_ZETA: grab(q, {K_(S.ddzeta, DKK_ZETA)}); break;
            case DD_ST_ACCUM:
                grab(q, {R_(dz, DKR_DZ), R_(gdx, DKR_GDX), X_(dx, DKX_DX)});
                if (q + 1 < S.dd_passes) plant(q + 1, {X_(S.tmpN, DKX_GTDZ), X_(S.rhsN, DKX_R1)});
                break;
            default: break;
        }
    };
    int ns_plain = 0;
    for (int b = 0; b < nlanes; ++b)
        if (LH[b].live) ns_plain = std::max(ns_plain, LH[b].nsweep);
    if (io.solve) {
        if (pl_any && nv == 1) {
            // (the combined solve's W^-2 bz comes with k_comb_rhs in an iteration: here for the lanes in the plain mode)
            const int* live_row = S.P.mask;
            if (S.dd_unit) S.P.mask = S.mask_row(ROW_PL);
            S.winv2<1>(bz, nullptr, S.wbz, 0);
            S.P.mask = live_row;
        }
        if (dd_any) plant(0, {X_(S.tmpN, DKX_GTDZ), X_(S.rhsN, DKX_R1)});
        if (nv == 2) S.solve_modes<2>(dd_any, pl_any, bx, bz, dx, dz, gdx, slot, ns_plain, &obs);
        else S.solve_modes<1>(dd_any, pl_any, bx, bz, dx, dz, gdx, slot, ns_plain, &obs);
    }
    // what the solve leaves, every live lane: the factor (double-double form: its high and low parts), the pivot counter, the solution
    std::vector<int> fl(nlanes, 0);
    for (int b = 0; b < nlanes; ++b) {
        if (!LH[b].live) continue;
        d2h(io.M + (size_t)b * np2, S.M, np2 * D8, b); d2h(io.Hf + (size_t)b * np2, S.H, np2 * D8, b);
        d2h(&fl[b], S.flag, I4, b);
        if (!io.solve) continue;
        for (int v = 0; v < nv; ++v) {
            d2h(io.end_x + ((size_t)b * 2 + v) * ldx, dx + (size_t)v * P.LDV, ldx * D8, b);
            d2h(io.end_r + (((size_t)b * 2 + 0) * 2 + v) * ldr, dz + (size_t)v * P.Rp, ldr * D8, b);
            d2h(io.end_r + (((size_t)b * 2 + 1) * 2 + v) * ldr, gdx + (size_t)v * P.Rp, ldr * D8, b);
        }
        d2h(io.out_sc + ((size_t)b * (DK_PASSES + 1) + DK_PASSES) * DK_SC, S.Sc + slot, (MAX_SWEEPS + 1) * D8, b);
    }
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    for (int b = 0; b < nlanes; ++b) {
        long* lr = io.lane_rep + 4 * (size_t)b;
        lr[0] = !LH[b].live ? 0 : LH[b].dd_k > 0 ? 1 : 2; lr[1] = LH[b].dd_k; lr[2] = LH[b].live ? S.dd_attempts : 0; lr[3] = LH[b].live ? nbp : 0;
        if (!LH[b].live) continue;
        io.flag[b] = fl[b];
        io.sel_sc[(size_t)b * DK_SEL_SC + 9] = S.hostTheta[b];
    }
    long* r = io.report;
    for (int i = 0; i < UNIT_DDKKT_REPORT; ++i) r[i] = 0;
    r[0] = kp; r[1] = cap ? 1 : 0; r[2] = S.dd_passes; r[3] = nlanes; r[4] = P.N; r[5] = P.R; r[6] = P.np; r[7] = P.l; r[8] = P.nq3; r[9] = P.big;
    r[10] = S.dd_k; r[11] = S.dd_attempts; r[12] = nv; r[13] = io.solve ? 1 : 0; r[14] = P.dims ? 1 : 0; r[15] = ns_plain;
}

void Solver::test_chol(int n, const double* Hh, double* out_l, double* out_m) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const SolveSwitches sw = read_switches();
    chol_set_lose_step(sw.test_lose_flag, S.st);
    const size_t np = round_up(n, 64);
    std::vector<double> Hp(np * np, 0.0);
    for (size_t i = 0; i < np; ++i) Hp[i * np + i] = 1.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Hp[i * np + j] = Hh[(size_t)i * n + j];
    DevBuf dH(np * np * 8), dM(np * np * 8), dMt(np * np * 8), dW((np * np + 65 * np) * 8), df(16), dL(np * np * 8);
    // The inverse factor is never initialised by the factorisation (the solver zeroes its arena once per solve, later
    // builds find the previous build's numbers in the lower tiles): mimic that -- zero once, factorise a DIFFERENT
    // matrix first, then the one asked for -- and check the transpose the inverse-row blocks write beside it.
    MBFIR_HIP(hipMemsetAsync(dM.p, 0, np * np * 8, S.st));
    MBFIR_HIP(hipMemsetAsync(dMt.p, 0, np * np * 8, S.st));
    {
        std::vector<double> H2(Hp);
        for (size_t i = 0; i < np; ++i) H2[i * np + i] = 2.0 * H2[i * np + i] + 1.0;
        MBFIR_HIP(hipMemcpyAsync(dH.p, H2.data(), np * np * 8, hipMemcpyHostToDevice, S.st));
        chol_inv_launch(dH.as<double>(), dM.as<double>(), dMt.as<double>(), dW.as<double>(), int(np), df.as<int>(), S.st, sw.chol_split, sw.poison);
        MBFIR_HIP(hipStreamSynchronize(S.st));
    }
    MBFIR_HIP(hipMemcpyAsync(dH.p, Hp.data(), np * np * 8, hipMemcpyHostToDevice, S.st));
    chol_inv_launch(dH.as<double>(), dM.as<double>(), dMt.as<double>(), dW.as<double>(), int(np), df.as<int>(), S.st, sw.chol_split, sw.poison,
                    dL.as<double>());
    MBFIR_HIP(hipMemcpy2DAsync(out_l, (size_t)n * 8, dL.p, np * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpy2DAsync(out_m, (size_t)n * 8, dM.p, np * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, S.st));
    std::vector<double> Mh(np * np), Mth(np * np);
    MBFIR_HIP(hipMemcpyAsync(Mh.data(), dM.p, np * np * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(Mth.data(), dMt.p, np * np * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    for (size_t i = 0; i < np; ++i)
        for (size_t j = 0; j < np; ++j)
            if (Mh[i * np + j] != Mth[j * np + i]) throw HipError("test_chol: the stored transpose differs from the inverse factor");
}

// nlanes matrices factorised together, lanes lane_bytes apart in ONE arena like a lock-step batch's (H | M | Mt | W1 | flag);
// form >= 0 forces the factorisation's form (otherwise MBFIR_CHOL_SPLIT, or its own choice)
void Solver::test_chol_lanes(int n, int nlanes, int form, const int* mask, const double* Hh, double* out_l, double* out_m) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const SolveSwitches sw = read_switches();
    chol_set_lose_step(sw.test_lose_flag, S.st);
    if (nlanes < 1 || nlanes > MAX_LANES) throw HipError("test_chol_lanes: bad lane count");
    const size_t np = round_up(n, 64);
    const size_t lane_doubles = 4 * np * np + 80 * np + 64, lane_bytes = lane_doubles * 8;
    DevBuf arena(lane_bytes * nlanes), dL(np * np * 8), dmask(sizeof(int) * MAX_LANES);
    MBFIR_HIP(hipMemsetAsync(arena.p, 0, lane_bytes * nlanes, S.st));
    double* base = arena.as<double>();
    double *dH = base, *dM = base + np * np, *dMt = dM + np * np, *dW = dMt + np * np;
    int* df = reinterpret_cast<int*>(dW + np * np + 70 * np);
    if (mask) MBFIR_HIP(hipMemcpyAsync(dmask.p, mask, sizeof(int) * nlanes, hipMemcpyHostToDevice, S.st));
    std::vector<double> Hp(np * np);
    // a different matrix first (later builds find the previous build's numbers in the buffers), then the ones asked for
    for (int pass = 0; pass < 2; ++pass) {
        for (int b = 0; b < nlanes; ++b) {
            std::fill(Hp.begin(), Hp.end(), 0.0);
            for (size_t i = 0; i < np; ++i) Hp[i * np + i] = 1.0;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) Hp[i * np + j] = Hh[((size_t)b * n + i) * n + j];
            if (pass == 0) for (size_t i = 0; i < np; ++i) Hp[i * np + i] = 2.0 * Hp[i * np + i] + 1.0;
            MBFIR_HIP(hipMemcpyAsync(reinterpret_cast<char*>(dH) + b * lane_bytes, Hp.data(), np * np * 8, hipMemcpyHostToDevice, S.st));
            MBFIR_HIP(hipStreamSynchronize(S.st));
        }
        chol_inv_launch(dH, dM, dMt, dW, int(np), df, S.st, form >= 0 ? form : sw.chol_split, sw.poison, nullptr, nullptr, nullptr, nlanes, lane_bytes,
                        mask ? dmask.as<int>() : nullptr);
        MBFIR_HIP(hipStreamSynchronize(S.st));
    }
    MBFIR_HIP(hipGetLastError());
    std::vector<int> fl(1);
    for (int b = 0; b < nlanes; ++b) {
        if (mask && !mask[b]) continue;
        const size_t off = (size_t)b * lane_bytes;
        auto at = [&](double* p) { return reinterpret_cast<double*>(reinterpret_cast<char*>(p) + off); };
        MBFIR_HIP(hipMemcpyAsync(fl.data(), reinterpret_cast<char*>(df) + off, sizeof(int), hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipStreamSynchronize(S.st));
        if (fl[0] != 0) throw HipError("test_chol_lanes: pivots replaced or a hand-off lost (counter " + std::to_string(fl[0]) + ")");
        hipLaunchKernelGGL(k_extract_L_pub, dim3(cdiv((long)np * np, 256)), dim3(256), 0, S.st, at(dH), int(np), at(dW) + np, at(dW) + 65 * np, dL.as<double>());
        MBFIR_HIP(hipMemcpy2DAsync(out_l + (size_t)b * n * n, (size_t)n * 8, dL.p, np * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipMemcpy2DAsync(out_m + (size_t)b * n * n, (size_t)n * 8, at(dM), np * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, S.st));
        // the stored transpose (what the second triangular GEMV reads) against the inverse factor
        std::vector<double> Mh(np * np), Mth(np * np);
        MBFIR_HIP(hipMemcpyAsync(Mh.data(), at(dM), np * np * 8, hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipMemcpyAsync(Mth.data(), at(dMt), np * np * 8, hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipStreamSynchronize(S.st));
        for (size_t i = 0; i < np; ++i)
            for (size_t j = 0; j <= i; ++j)
                if (Mh[i * np + j] != Mth[j * np + i]) throw HipError("test_chol_lanes: the stored transpose differs from the inverse factor");
    }
}

// x = (H + U' diag(X) U)^-1 b through the double-double kernels (ddlin.hip); b and x are dd (hi, lo), nrhs <= 2
void Solver::test_ddsolve(int n, int k, const double* Hh, const double* U, const double* X, int nrhs, const double* bh,
                          const double* bl, double* xh, double* xl, int* nfix, double* Lh_out, double* Ll_out) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const size_t np = round_up(n, 64), ldv = np;
    std::vector<double> Hp(np * np, 0.0), Up((size_t)std::max(k, 1) * np, 0.0), B(2 * ldv, 0.0), Bl(2 * ldv, 0.0);
    for (size_t i = 0; i < np; ++i) Hp[i * np + i] = 1.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Hp[i * np + j] = Hh[(size_t)i * n + j];
    for (int r = 0; r < k; ++r)
        for (int j = 0; j < n; ++j) Up[r * np + j] = U[(size_t)r * n + j];
    for (int v = 0; v < nrhs; ++v)
        for (int j = 0; j < n; ++j) { B[v * ldv + j] = bh[(size_t)v * n + j]; Bl[v * ldv + j] = bl[(size_t)v * n + j]; }
    DevBuf dH(np * np * 8), dHl(np * np * 8), dLt(np * np * 8), dLtl(np * np * 8), dU(Up.size() * 8), dX((size_t)std::max(k, 1) * 8),
        dri(2 * np * 8), dd0(np * 8), dB(2 * ldv * 8), dBl(2 * ldv * 8), df(16);
    MBFIR_HIP(hipMemcpyAsync(dH.p, Hp.data(), np * np * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dU.p, Up.data(), Up.size() * 8, hipMemcpyHostToDevice, S.st));
    if (k > 0) MBFIR_HIP(hipMemcpyAsync(dX.p, X, (size_t)k * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dB.p, B.data(), 2 * ldv * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dBl.p, Bl.data(), 2 * ldv * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(df.as<int>() + 1, &k, sizeof(int), hipMemcpyHostToDevice, S.st));
    dd_syrk_launch(dU.as<double>(), int(np), dX.as<double>(), df.as<int>() + 1, int(np), dH.as<double>(), dHl.as<double>(), S.st);
    DevBuf dinv(2 * np * 64 * 8);
    double* dinvp = dinv.as<double>();
    if (!read_switches().dd_blockinv) dinvp = nullptr;
    dd_chol_launch(dH.as<double>(), dHl.as<double>(), dLt.as<double>(), dLtl.as<double>(), dri.as<double>(), dri.as<double>() + np,
                   dd0.as<double>(), int(np), 1e-28, df.as<int>(), S.st, dinvp);
    DevBuf dflags(sizeof(int) * (2 * np / 32 + 8));
    MBFIR_HIP(hipMemsetAsync(dflags.p, 0, sizeof(int) * (2 * np / 32 + 8), S.st));
    dd_trsv_launch(dH.as<double>(), dHl.as<double>(), dLt.as<double>(), dLtl.as<double>(), dri.as<double>(), dri.as<double>() + np,
                   int(np), dB.as<double>(), dBl.as<double>(), nrhs, int(ldv), S.st, dflags.as<int>(), 1, df.as<int>(), dinvp);
    MBFIR_HIP(hipMemcpyAsync(B.data(), dB.p, 2 * ldv * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(Bl.data(), dBl.p, 2 * ldv * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(nfix, df.p, sizeof(int), hipMemcpyDeviceToHost, S.st));
    if (Lh_out && Ll_out) {
        MBFIR_HIP(hipMemcpy2DAsync(Lh_out, (size_t)n * 8, dH.p, np * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipMemcpy2DAsync(Ll_out, (size_t)n * 8, dHl.p, np * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, S.st));
    }
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    for (int v = 0; v < nrhs; ++v)
        for (int j = 0; j < n; ++j) { xh[(size_t)v * n + j] = B[v * ldv + j]; xl[(size_t)v * n + j] = Bl[v * ldv + j]; }
}

// The double-double kernels of ddlin.hip stage by stage (mbfir_test_ddstages checks the arguments): the padding of test_ddsolve
// (identity past n, zero coupling), then the production launches in order -- dd_syrk_launch, dd_chol_launch (the block inverses for
// form 2 only), nsolve calls of dd_trsv_launch on ONE flag array with the epochs 1 .. nsolve, each from a fresh copy of the right-hand
// sides -- and a read-back after every group, full padded size.  Hl, d0, Lth / Ltl, ri, dinv and the rows nrhs .. 1 of every solution
// go to the device as the caller filled them: what no launch writes comes back as it went in.
void Solver::test_ddstages(const DdStagesIO& io) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const int n = io.n, k = io.k, nrhs = io.nrhs;
    const size_t np = round_up(n, 64), ldv = np, nn = np * np * 8;
    std::vector<double> Hp(np * np, 0.0), Up((size_t)std::max(k, 1) * np, 0.0);
    for (size_t i = 0; i < np; ++i) Hp[i * np + i] = 1.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Hp[i * np + j] = io.H[(size_t)i * n + j];
    for (int r = 0; r < k; ++r)
        for (int j = 0; j < n; ++j) Up[r * np + j] = io.U[(size_t)r * n + j];
    DevBuf dH(nn), dHl(nn), dLt(nn), dLtl(nn), dU(Up.size() * 8), dX((size_t)std::max(k, 1) * 8), dri(2 * np * 8), dd0(np * 8),
        dB(2 * ldv * 8), dBl(2 * ldv * 8), df(16), dinv(2 * np * 64 * 8), dflags(sizeof(int) * (2 * np / 32 + 8));
    MBFIR_HIP(hipMemcpyAsync(dH.p, Hp.data(), nn, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dHl.p, io.Hl, nn, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dLt.p, io.Lth, nn, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dLtl.p, io.Ltl, nn, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dri.p, io.ri, 2 * np * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dd0.p, io.d0, np * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dinv.p, io.dinv, 2 * np * 64 * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemcpyAsync(dU.p, Up.data(), Up.size() * 8, hipMemcpyHostToDevice, S.st));
    if (k > 0) MBFIR_HIP(hipMemcpyAsync(dX.p, io.X, (size_t)k * 8, hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemsetAsync(df.p, 0, 16, S.st));
    MBFIR_HIP(hipMemcpyAsync(df.as<int>() + 1, &k, sizeof(int), hipMemcpyHostToDevice, S.st));
    MBFIR_HIP(hipMemsetAsync(dflags.p, 0, sizeof(int) * (2 * np / 32 + 8), S.st));
    // 1: the rank-k update
    dd_syrk_launch(dU.as<double>(), int(np), dX.as<double>(), df.as<int>() + 1, int(np), dH.as<double>(), dHl.as<double>(), S.st);
    MBFIR_HIP(hipMemcpyAsync(io.Hh, dH.p, nn, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.Hl, dHl.p, nn, hipMemcpyDeviceToHost, S.st));
    // 2: the factorisation
    double* dinvp = io.form == 2 ? dinv.as<double>() : nullptr;
    dd_chol_launch(dH.as<double>(), dHl.as<double>(), dLt.as<double>(), dLtl.as<double>(), dri.as<double>(), dri.as<double>() + np,
                   dd0.as<double>(), int(np), io.pivtol, df.as<int>(), S.st, dinvp);
    MBFIR_HIP(hipMemcpyAsync(io.Lh, dH.p, nn, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.Ll, dHl.p, nn, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.Lth, dLt.p, nn, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.Ltl, dLtl.p, nn, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.ri, dri.p, 2 * np * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.d0, dd0.p, np * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.dinv, dinv.p, 2 * np * 64 * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipMemcpyAsync(io.counter, df.p, sizeof(int), hipMemcpyDeviceToHost, S.st));
    // 3: the solves, every one from the caller's right-hand sides, on the same flags
    for (int s = 0; s < io.nsolve; ++s) {
        double* xh = io.xh + (size_t)s * 2 * ldv;
        double* xl = io.xl + (size_t)s * 2 * ldv;
        for (int v = 0; v < nrhs; ++v)
            for (size_t j = 0; j < np; ++j) {
                xh[v * ldv + j] = j < size_t(n) ? io.bh[(size_t)v * n + j] : 0.0;
                xl[v * ldv + j] = j < size_t(n) ? io.bl[(size_t)v * n + j] : 0.0;
            }
        MBFIR_HIP(hipMemcpyAsync(dB.p, xh, 2 * ldv * 8, hipMemcpyHostToDevice, S.st));
        MBFIR_HIP(hipMemcpyAsync(dBl.p, xl, 2 * ldv * 8, hipMemcpyHostToDevice, S.st));
        dd_trsv_launch(dH.as<double>(), dHl.as<double>(), dLt.as<double>(), dLtl.as<double>(), dri.as<double>(), dri.as<double>() + np,
                       int(np), dB.as<double>(), dBl.as<double>(), nrhs, int(ldv), S.st, io.form == 0 ? nullptr : dflags.as<int>(), s + 1,
                       df.as<int>(), dinvp);
        MBFIR_HIP(hipMemcpyAsync(xh, dB.p, 2 * ldv * 8, hipMemcpyDeviceToHost, S.st));
        MBFIR_HIP(hipMemcpyAsync(xl, dBl.p, 2 * ldv * 8, hipMemcpyDeviceToHost, S.st));
    }
    MBFIR_HIP(hipMemcpyAsync(io.counter + 1, df.p, sizeof(int), hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
}

// The capacitance form of the extended-precision solve as build_H and one pass of kkt_solve_dd launch it (mbfir_test_capsolve checks
// the arguments).  One arena per lane, lanes lane_bytes apart, kcnt and the pivot counters in the lane's arena, the mask in lane 0's.
// A single problem runs as a single design does (no lane stride, no kcnt, the launches carry its own k); several run as a unit (the
// launches carry kp, every lane reads its own count).  Before the launches NaN goes where the kernels claim not to read: the 64 x 64
// tiles of M, S and Ms strictly above the diagonal and their mirror images in Mt, X[k .. kp), t[.][k .. kp), a / b[.][n .. np), the
// split-K slab, the partial vectors of the one-pass M'(M b) and the GEMV pair's intermediate.  The output arrays go to the device
// as the caller filled them and come back after the launches: what a masked lane's hold on return, it held on entry.
void Solver::test_capsolve(const CapSolveIO& io) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const SolveSwitches sw = read_switches();
    chol_set_lose_step(sw.test_lose_flag, S.st);
    const int nl = io.nlanes, nv = io.nrhs, n = io.n, kp = io.kp;
    const size_t np = round_up(n, 64), kq = size_t(kp), ldv = np, ldk = kq;
    const bool fused = io.hsolve_form < 0 ? (hsolve_fused_ok(int(np), 2) && sw.hsolve) : io.hsolve_form == 1;      // (< 0: prepare_lanes' choice)
    if (fused && !hsolve_fused_ok(int(np), nv)) throw HipError("test_capsolve: the one-pass M'(M b) does not take this size");
    size_t top = 0;
    auto take = [&](size_t c) { const size_t o = top; top += (c + 7) & ~size_t(7); return o; };
    const size_t oH = take(np * np), oM = take(np * np), oMt = take(np * np), oW1 = take(np * np + 65 * np);
    const size_t oU = take(kq * np), oX = take(kq), oYt = take(kq * np), oZt = take(kq * np), oS = take(kq * kq), oMs = take(kq * kq);
    const size_t oW1s = take(kq * kq + 65 * kq), nPart = cap_part_doubles(kp, int(np)), oPart = take(nPart);
    const size_t nHs = hsolve_part_doubles(int(std::max(fused ? np : size_t(0), kq))), oHs = take(nHs);
    const size_t oA = take(2 * ldv), oB = take(2 * ldv), oRw = take(2 * ldv), oYn = take(2 * ldv), oY = take(2 * ldv), oDx = take(2 * ldv);
    const size_t oT = take(2 * ldk), oW = take(2 * ldk), oZeta = take(2 * ldk), oInt = take(16 + MAX_LANES);
    const size_t oSk = take(kq * kq);                       // S as the build left it (the factorisation works in place: its S is scratch on exit)
    const size_t lane_bytes = top * 8;
    enum { I_FLAG = 0, I_CAPFLAG = 4, I_KCNT = 8, I_MASK = 16 };
    DevBuf arena(lane_bytes * nl);
    double* base = arena.as<double>();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> img(top);
    // (tile (I, J) of a q x q matrix, I < J: above the diagonal; below = its mirror image, what Mt keeps of it)
    auto poison_tiles = [&](double* A, size_t q, bool above, bool below) {
        for (size_t i = 0; i < q; ++i)
            for (size_t j = 0; j < q; ++j)
                if ((above && j / 64 > i / 64) || (below && j / 64 < i / 64)) A[i * q + j] = nan;
    };
    auto rows_in = [&](size_t o, size_t ld, const double* src, size_t rows, size_t cols, size_t keep) {       // rows x cols -> stride ld; NaN from `keep` to ld
        for (size_t r = 0; r < rows; ++r)
            for (size_t j = 0; j < ld; ++j) img[o + r * ld + j] = j < std::min(cols, keep) ? src[r * cols + j] : nan;
    };
    for (int b = 0; b < nl; ++b) {
        const size_t kb = size_t(io.k[b]);
        std::fill(img.begin(), img.end(), 0.0);
        for (size_t i = 0; i < np; ++i) img[oH + i * np + i] = 1.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) img[oH + i * np + j] = io.H[((size_t)b * n + i) * n + j];
        std::copy(io.M + b * np * np, io.M + (b + 1) * np * np, img.begin() + oM);
        poison_tiles(&img[oM], np, true, false);
        poison_tiles(&img[oMt], np, true, true);            // (the factorisation writes the tiles above its diagonal, nobody the ones below)
        for (size_t r = 0; r < kb; ++r)
            for (int j = 0; j < n; ++j) img[oU + r * np + j] = io.U[((size_t)b * kq + r) * n + j];
        rows_in(oX, kq, io.X + b * kq, 1, kq, kb);
        std::copy(io.Yt + b * kq * np, io.Yt + (b + 1) * kq * np, img.begin() + oYt);
        std::copy(io.Zt + b * kq * np, io.Zt + (b + 1) * kq * np, img.begin() + oZt);
        std::copy(io.S + b * kq * kq, io.S + (b + 1) * kq * kq, img.begin() + oS);
        std::copy(io.Ms + b * kq * kq, io.Ms + (b + 1) * kq * kq, img.begin() + oMs);
        poison_tiles(&img[oS], kq, true, false);
        poison_tiles(&img[oMs], kq, true, false);
        std::fill(img.begin() + oPart, img.begin() + oPart + nPart, nan);
        std::fill(img.begin() + oHs, img.begin() + oHs + nHs, nan);
        std::fill(img.begin() + oYn, img.begin() + oYn + 2 * ldv, nan);
        rows_in(oA, ldv, io.a + (size_t)b * nv * n, nv, n, n);
        rows_in(oB, ldv, io.b + (size_t)b * nv * n, nv, n, n);
        rows_in(oT, ldk, io.t + (size_t)b * nv * kq, nv, kq, kb);
        const struct { size_t o, ld; double* p; } vecs[] = {{oRw, ldv, io.rhs_w}, {oY, ldv, io.y}, {oDx, ldv, io.dx}, {oW, ldk, io.w}, {oZeta, ldk, io.zeta}};
        for (const auto& v : vecs) std::copy(v.p + (size_t)b * nv * v.ld, v.p + (size_t)(b + 1) * nv * v.ld, img.begin() + v.o);
        int* ints = reinterpret_cast<int*>(&img[oInt]);
        ints[I_FLAG] = io.flag[b]; ints[I_KCNT] = int(kb);
        if (b == 0 && io.mask) for (int q = 0; q < nl; ++q) ints[I_MASK + q] = io.mask[q];
        MBFIR_HIP(hipMemcpy(reinterpret_cast<char*>(base) + b * lane_bytes, img.data(), lane_bytes, hipMemcpyHostToDevice));
    }
    double *dH = base + oH, *dM = base + oM, *dMt = base + oMt, *dW1 = base + oW1, *dU = base + oU, *dX = base + oX, *dYt = base + oYt, *dZt = base + oZt;
    double *dS = base + oS, *dMs = base + oMs, *dW1s = base + oW1s, *dPart = base + oPart, *dHs = base + oHs, *dA = base + oA, *dB = base + oB;
    double *dRw = base + oRw, *dYn = base + oYn, *dY = base + oY, *dDx = base + oDx, *dT = base + oT, *dW = base + oW, *dZeta = base + oZeta;
    int* dint = reinterpret_cast<int*>(base + oInt);
    const int* mask = io.mask ? dint + I_MASK : nullptr;
    const bool unit = nl > 1;
    const size_t lb = unit ? lane_bytes : 0;
    const int* kcnt = unit ? dint + I_KCNT : nullptr;
    const int k = unit ? kp : io.k[0];
    // build_H's capacitance branch
    chol_inv_launch(dH, dM, fused ? nullptr : dMt, dW1, int(np), dint + I_FLAG, S.st, sw.chol_split, sw.poison, nullptr, nullptr, nullptr, nl, lb, mask);
    cap_build_launch(dU, k, kp, int(np), dM, dX, dYt, dZt, dS, dPart, S.st, nl, lb, mask, kcnt);
    MBFIR_HIP(hipMemcpy2DAsync(base + oSk, lane_bytes, dS, lane_bytes, kq * kq * 8, nl, hipMemcpyDeviceToDevice, S.st));
    chol_inv_launch(dS, dMs, nullptr, dW1s, kp, dint + I_CAPFLAG, S.st, sw.chol_split, sw.poison, nullptr, nullptr, nullptr, nl, lb, mask);
    cap_flag_add_launch(dint + I_FLAG, dint + I_CAPFLAG, S.st, nl, lb, mask);
    // one pass of kkt_solve_dd's capacitance branch
    cap_add_launch(dA, dB, dRw, n, int(np), int(ldv), nv, S.st, nl, lane_bytes, mask);
    if (fused) {
        hsolve_launch(dM, int(np), dRw, nullptr, dY, dHs, nv, int(ldv), S.st, nl, lane_bytes, mask);
    } else {
        trigemv_launch(dM, int(np), 0, dRw, dYn, nv, int(ldv), S.st, nullptr, nl, lane_bytes, mask);
        trigemv_launch(dMt, int(np), 1, dYn, dY, nv, int(ldv), S.st, nullptr, nl, lane_bytes, mask);
    }
    cap_uy_launch(dU, k, kp, n, int(np), dY, int(ldv), dT, dW, int(ldk), nv, S.st, nl, lane_bytes, mask, kcnt);
    hsolve_launch(dMs, kp, dW, nullptr, dZeta, dHs, nv, int(ldk), S.st, nl, lane_bytes, mask);
    cap_dx_launch(dZt, k, n, int(np), dZeta, int(ldk), dY, dDx, int(ldv), nv, S.st, nl, lane_bytes, mask, kcnt);
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    for (int b = 0; b < nl; ++b) {
        MBFIR_HIP(hipMemcpy(img.data(), reinterpret_cast<char*>(base) + b * lane_bytes, lane_bytes, hipMemcpyDeviceToHost));
        std::copy(img.begin() + oM, img.begin() + oM + np * np, io.M + b * np * np);
        std::copy(img.begin() + oYt, img.begin() + oYt + kq * np, io.Yt + b * kq * np);
        std::copy(img.begin() + oZt, img.begin() + oZt + kq * np, io.Zt + b * kq * np);
        std::copy(img.begin() + oSk, img.begin() + oSk + kq * kq, io.S + b * kq * kq);
        std::copy(img.begin() + oMs, img.begin() + oMs + kq * kq, io.Ms + b * kq * kq);
        const struct { size_t o, ld; double* p; } vecs[] = {{oRw, ldv, io.rhs_w}, {oY, ldv, io.y}, {oDx, ldv, io.dx}, {oW, ldk, io.w}, {oZeta, ldk, io.zeta}};
        for (const auto& v : vecs) std::copy(img.begin() + v.o, img.begin() + v.o + nv * v.ld, v.p + (size_t)b * nv * v.ld);
        io.flag[b] = reinterpret_cast<const int*>(&img[oInt])[I_FLAG];
        if (fused || (io.mask && !io.mask[b])) continue;
        // the stored transpose (what the second triangular GEMV read) against the inverse factor
        for (size_t i = 0; i < np; ++i)
            for (size_t j = 0; j <= i; ++j)
                if (img[oM + i * np + j] != img[oMt + j * np + i]) throw HipError("test_capsolve: the stored transpose differs from the inverse factor");
    }
}

void Solver::test_specfact(int n, const double* x, double* h_re, double* h_im) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const int lp = specfact_lp(n);
    DevBuf dx((2 * (size_t)n) * 8), dw(6 * (size_t)lp * 8), dh(2 * (size_t)n * 8);
    MBFIR_HIP(hipMemcpyAsync(dx.p, x, (2 * (size_t)n - 1) * 8, hipMemcpyHostToDevice, S.st));
    specfact_launch(dx.as<double>(), n, dw.as<double>(), dh.as<double>(), S.st);
    std::vector<double> h(2 * (size_t)n);
    MBFIR_HIP(hipMemcpyAsync(h.data(), dh.p, 2 * (size_t)n * 8, hipMemcpyDeviceToHost, S.st));
    MBFIR_HIP(hipStreamSynchronize(S.st));
    MBFIR_HIP(hipGetLastError());
    for (int i = 0; i < n; ++i) { h_re[i] = h[2 * i]; h_im[i] = h[2 * i + 1]; }
}

// fp64 peak microbenchmarks (roofline denominators; the local hardware guide lists no fp64
// matrix peak).  One wave per SIMD, 8 independent accumulators, operands in registers.
__global__ __launch_bounds__(256) void k_peak_mfma(double* out, int iters) {
    double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    v4d c[8];
    for (int i = 0; i < 8; ++i) c[i] = (v4d){0, 0, 0, 0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c[i], 0, 0, 0);
    }
    double s = 0;
    for (int i = 0; i < 8; ++i) s += c[i][0] + c[i][1] + c[i][2] + c[i][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_peak_valu(double* out, int iters) {
    double a = 1.0 + threadIdx.x * 1e-9, b = 1e-9;
    double c[16];
    for (int i = 0; i < 16; ++i) c[i] = i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = fma(c[i], a, b);
    }
    double s = 0;
    for (int i = 0; i < 16; ++i) s += c[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
void Solver::test_mfma_peak(double* tf_mfma, double* tf_valu) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    hipDeviceProp_t prop;
    MBFIR_HIP(hipGetDeviceProperties(&prop, S.device));
    const int blocks = prop.multiProcessorCount * 4, iters = 20000;      // 4 waves per SIMD
    DevBuf dout((size_t)blocks * 256 * 8);
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {
        hipEventRecord(S.ev0, S.st);
        hipLaunchKernelGGL(k_peak_mfma, dim3(blocks), dim3(256), 0, S.st, dout.as<double>(), iters);
        hipEventRecord(S.ev1, S.st);
        MBFIR_HIP(hipEventSynchronize(S.ev1));
        hipEventElapsedTime(&ms, S.ev0, S.ev1);
    }
    *tf_mfma = double(blocks) * 4 * iters * 8 * 2048.0 / (ms * 1e-3) / 1e12;
    for (int rep = 0; rep < 2; ++rep) {
        hipEventRecord(S.ev0, S.st);
        hipLaunchKernelGGL(k_peak_valu, dim3(blocks), dim3(256), 0, S.st, dout.as<double>(), iters);
        hipEventRecord(S.ev1, S.st);
        MBFIR_HIP(hipEventSynchronize(S.ev1));
        hipEventElapsedTime(&ms, S.ev0, S.ev1);
    }
    *tf_valu = double(blocks) * 256 * iters * 16 * 2.0 / (ms * 1e-3) / 1e12;
    MBFIR_HIP(hipGetLastError());
}

__global__ void k_fill_spd(double* H, int np, int n) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)np * np) return;
    long i = e / np, j = e - i * np;
    double v = 0;
    if (i < n && j < n) v = 1.0 / (1.0 + double(i > j ? i - j : j - i)) + (i == j ? 2.0 : 0.0);   // SPD (diagonally dominant-ish)
    else if (i == j) v = 1.0;
    H[e] = v;
}
void Solver::test_time_kernels(int n, int m, int nt, int reps, double* ms_chol, double* ms_gram) {
    Impl& S = *impl;
    MBFIR_HIP(hipSetDevice(S.device));
    const SolveSwitches sw = read_switches();
    chol_set_lose_step(sw.test_lose_flag, S.st);
    const size_t np = round_up(n, 64);
    DevBuf dH(np * np * 8), dH0(np * np * 8), dM(np * np * 8), dMt(np * np * 8), dW((np * np + 65 * np) * 8), df(16);
    hipLaunchKernelGGL(k_fill_spd, dim3(cdiv((long)np * np, 256)), dim3(256), 0, S.st, dH0.as<double>(), int(np), n);
    float ms = 0, tot = 0;
    for (int r = 0; r < reps + 1; ++r) {
        MBFIR_HIP(hipMemcpyAsync(dH.p, dH0.p, np * np * 8, hipMemcpyDeviceToDevice, S.st));
        hipEventRecord(S.ev0, S.st);
        chol_inv_launch(dH.as<double>(), dM.as<double>(), dMt.as<double>(), dW.as<double>(), int(np), df.as<int>(), S.st, sw.chol_split, sw.poison);
        hipEventRecord(S.ev1, S.st);
        MBFIR_HIP(hipEventSynchronize(S.ev1));
        hipEventElapsedTime(&ms, S.ev0, S.ev1);
        if (r > 0) tot += ms;
    }
    *ms_chol = tot / reps;
    GramPlan gp = gram_plan(m, nt, 1);
    DevBuf dA((size_t)gp.Mpad * gp.ld * 8), dd((size_t)gp.Mpad * 8), dslab(gp.slab_doubles * 8), dT((size_t)gp.ld * gp.ld * 8), dt((size_t)gram_table_ints(gp) * 4);
    MBFIR_HIP(hipMemsetAsync(dA.p, 0x3c, (size_t)gp.Mpad * gp.ld * 8, S.st));      // arbitrary finite doubles
    MBFIR_HIP(hipMemsetAsync(dd.p, 0x3c, (size_t)gp.Mpad * 8, S.st));
    std::vector<int> tiles(gram_table_ints(gp));
    gram_tiles_host(gp, tiles.data());
    MBFIR_HIP(hipMemcpyAsync(dt.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, S.st));
    tot = 0;
    for (int r = 0; r < reps + 1; ++r) {
        gram_launch(gp, dA.as<double>(), dd.as<double>(), dslab.as<double>(), dT.as<double>(), dt.as<int>(), S.st, S.ev0, S.ev1);
        MBFIR_HIP(hipStreamSynchronize(S.st));
        hipEventElapsedTime(&ms, S.ev0, S.ev1);
        if (r > 0) tot += ms;
    }
    *ms_gram = tot / reps;
    MBFIR_HIP(hipGetLastError());
}

}  // namespace mbfir
