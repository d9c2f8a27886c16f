// Host-visible interface of the device IPM (solver.hip).
#pragma once
#include "program.h"
#include <stdexcept>
#include <string>
#include <vector>

namespace mbfir {

// solve_lanes was handed programs the lock-step path does not take as ONE unit (too many lanes, different designers or
// orders): the caller may run the designs one by one.  Every other exception of the solver is an internal / device error
// and is reported as such, never retried.
struct ShapeError : std::runtime_error {
    explicit ShapeError(const std::string& s) : std::runtime_error(s) {}
};
// a lock-step unit did not get its device memory (every lane is sized to the unit's maxima): recoverable -- the caller takes
// the unit's designs through the single-design path -- unlike an internal or device error, which is reported
struct ResourceError : std::runtime_error {
    explicit ResourceError(const std::string& s) : std::runtime_error(s) {}
};

enum { ST_OPTIMAL = 0, ST_PRIMAL_INFEASIBLE = 1, ST_DUAL_INFEASIBLE = 2, ST_MAXIT = 3, ST_NUMERICAL = 4,
       ST_OPTIMAL_INACCURATE = 5 };

struct SolveOpts {
    int max_iter = 200;
    double feastol = 1e-8, abstol = 1e-10, reltol = 1e-8;
    int refine = 2;
    int verbose = 0;
    int shard_rank = 0, shard_size = 1;     // frequency-row sharding (one process per GPU)
    bool dense_trig = false; // keep the materialised trig matrix and the dense MFMA Gram even when the lattice structure is there
    double ddkkt_theta = 0; // > 0: extended-precision (double-double) KKT solve for every NT weight above theta x the typical weight
    int dd_form = 0;        // the extended-precision solve: 0 its capacitance (saddle-point) form in plain double on the matrix cores
                            // (capkkt.hip), 1 the double-double factorisation of the whole normal matrix (ddlin.hip)
    bool timing = true;     // HIP-event timing of the k_gram launches and the Cholesky phase (events read at the end)
};

struct SolveInfo {
    int status = 0, iters = 0, n_unknowns = 0, n_rows = 0, n_freq = 0;
    double pcost = 0, dcost = 0, gap = 0, relgap = 0, pres = 0, dres = 0;
    double ms_assemble = 0, ms_solve = 0, ms_gram = 0, ms_chol = 0, gram_flop = 0;
    int h_builds = 0;       // number of (Gram, Cholesky) builds = iterations + 1 (initial point)
    int chol_launches = 0;  // k_chol_step launches timed in ms_chol
    double chol_flop = 0;   // factorisation + triangular inverse, per build
    int dd_iters = 0, dd_kmax = 0;   // iterations that ran the extended-precision solve; largest strong set
    double ms_cap = 0, cap_flop = 0; // capacitance form: device time and flop of the three matrix-core products (Yt, Zt, S), summed over the builds
    int dd_form = 0;                 // which form of that solve ran (0 capacitance / double, 1 double-double)
    int collectives = 0;    // all-reduces the (row-sharded) solve issued
    double collective_bytes = 0;   // ... and the bytes they carried (per rank)
    int lanes = 1;          // designs that shared the lock-step batch (ms_* are those of the whole batch)
    int lattice = 0;        // 1: lattice (matrix-free) mode; gram_flop then counts the moment recurrences
    int correctors = 0, correctors_taken = 0;   // centrality-corrector solves of this design, and how many of the corrected directions were taken
    int pair_passes = 0;                        // lattice passes (G v, G'v, H-build moments) that ran in the paired form (one thread per two lanes; 0 for a single design)
    int gv_passes = 0, gtv_passes = 0;          // row-response passes G v and transposed passes G'v the solve launched (all iterations; a lock-step unit's count)
};

// Arguments of Solver::test_unit_ops (mbfir_test_unit_ops of include/mbfir.h, which says what each array holds): host arrays of
// nlanes blocks each; report: UNIT_OPS_REPORT longs, see the UO_* indices.
struct UnitOps {
    int nv = 1, ldx = 0, ldr = 0, ldh = 0;
    const double *v = nullptr, *u = nullptr, *sub = nullptr, *s = nullptr, *z = nullptr;
    const int* mask = nullptr;
    double *gv = nullptr, *gtu = nullptr, *wgv = nullptr, *H = nullptr;
    long* report = nullptr;
    double* tmin = nullptr;
};
enum { UO_LATTICE = 0, UO_PAIR_PASSES, UO_ONE_PASS, UO_D1, UO_USEG, UO_NFOLD, UO_NCHUNK, UO_CGRP, UO_NP, UO_EMPTY_SIDE, UO_SEG,
       UO_HETERO, UO_SEEDS_SHARED, UO_GV_PASSES, UO_GTV_PASSES, UO_LANES, UNIT_OPS_REPORT = 16 };

// Arguments of Solver::test_unit_cone (mbfir_test_unit_cone of include/mbfir.h, which says what each block holds): host arrays of
// nlanes blocks each.  in_r / out_r: UC_IN_R / UC_OUT_R rows of ldr, in_x / out_x: UC_IN_X / UC_OUT_X rows of ldx, out_w3: ldw,
// in_sc: UC_IN_SC scalars, out_sc: UC_SNAPS snapshots of UC_SC scalars
enum { UCR_S = 0, UCR_Z, UCR_RZ, UCR_BZ2 /* two rows */, UCR_Z1 = UCR_BZ2 + 2, UCR_Z2, UCR_G1, UCR_G2, UCR_ZC, UCR_GC, UCR_KZ, UCR_KG, UCR_SHIFT, UC_IN_R };
enum { UCX_X = 0, UCX_RX, UCX_X1, UCX_X2, UCX_XC, UCX_KX, UC_IN_X };
enum { UCO_DL = 0, UCO_WL, UCO_LAM, UCO_WBZ2 /* two rows */, UCO_WBB = UCO_WBZ2 + 2, UCO_DSSA, UCO_WDZA, UCO_LDS, UCO_BZC, UCO_WBZC, UCO_DS, UCO_DZ,
       UCO_KBZ, UCO_WBZK, UCO_KZ, UCO_KG, UCO_KDS, UCO_KDZ, UCO_S, UCO_Z, UCO_SHIFT, UC_OUT_R };
enum { UCOX_BXC = 0, UCOX_KX, UCOX_X, UC_OUT_X };
enum { UCS_SCALING = 0, UCS_PRED, UCS_COMB_RHS, UCS_COMB, UCS_CORR_RHS, UCS_UPDATE, UCS_SHIFT, UC_SNAPS };
enum { UC_IN_SC = 8, UC_SC = 24, UNIT_CONE_REPORT = 16 };
struct UnitCone {
    int form = 0, corr = 0, ldx = 0, ldr = 0, ldw = 0;
    const int* mask = nullptr;
    const double *in_r = nullptr, *in_x = nullptr, *in_sc = nullptr;
    double *out_r = nullptr, *out_x = nullptr, *out_w3 = nullptr, *out_sc = nullptr;
    long* report = nullptr;
};

// Arguments of Solver::test_unit_kkt (mbfir_test_unit_kkt of include/mbfir.h, which says what each block holds): host arrays of
// nlanes blocks each.  Blocks of out_x / out_r hold two vectors of ldx / ldr (the second stays the caller's where nv = 1).
enum { UKX_T1 = 0, UKX_DX0, UKX_T4, UKX_R0, UKX_P /* + 2 s: p, z of start s = 0 .. 7 */, UKX_HP = UKX_P + 16 /* + 3 q: Hp, dx, r of sweep q */,
       UKX_DX_END = UKX_HP + 24, UKX_R_END, UK_OUT_X };
enum { UKR_WBZ = 0, UKR_GDX0, UKR_DZ0, UKR_GP /* + 4 q: Gp, W^-2 Gp, gdx, dz of sweep q */, UKR_GDX_END = UKR_GP + 32, UKR_DZ_END, UK_OUT_R };
enum { UKS_RESID = 0, UKS_START /* + s */, UKS_STEP = UKS_START + 8 /* + q */, UKS_END = UKS_STEP + 8, UK_SNAPS };
enum { UK_SC = 13 /* n_0 .. n_8, rz[2], alpha[2] */, UK_RES_SC = 24, UK_RES_X = 4, UK_RES_R = 3, UK_INIT_R = 7, UK_INIT_X = 3, UNIT_KKT_REPORT = 24 };
struct UnitKkt {
    int mode = 0 /* 1: initial_point */, form = 0, two = 0, wbz_ready = 0, nv = 2, ldx = 0, ldr = 0, ldh = 0, ldw = 0;
    const int *mask = nullptr, *nsweep = nullptr;
    const double *s = nullptr, *z = nullptr, *x = nullptr, *tau_kappa = nullptr, *bx = nullptr, *bz = nullptr;
    double *res_r = nullptr, *res_x = nullptr, *res_sc = nullptr, *M = nullptr, *out_x = nullptr, *out_r = nullptr, *out_sc = nullptr,
           *init_r = nullptr, *init_x = nullptr, *init_w3 = nullptr;
    long *flag = nullptr, *report = nullptr;
};

// Arguments of Solver::test_unit_ddkkt (mbfir_test_unit_ddkkt of include/mbfir.h, which says what each block holds): host arrays of
// nlanes blocks each.  out_x / out_r / out_k: DK_PASSES passes of DK_OUT_X / DK_OUT_R / DK_OUT_K blocks of two vectors of ldx / ldr /
// DK_KMAX (the second stays the caller's where nv = 1)
enum { DKX_GTDZ = 0, DKX_R1, DKX_GTW, DKX_RHS_H, DKX_RHS_L, DKX_Y, DKX_BH, DKX_BL, DKX_DX, DK_OUT_X };
enum { DKR_R2 = 0, DKR_WBZ, DKR_GBH, DKR_WBZ2, DKR_DZ, DKR_GDX, DK_OUT_R };
enum { DKK_TS = 0, DKK_CAPW, DKK_ZETA, DK_OUT_K };
enum { DK_PASSES = 3, DK_SC = 9 /* n_0 .. n_8 */, DK_SEL_R = 4, DK_SEL_SC = 16, DK_KMAX = 3072, UNIT_DDKKT_REPORT = 16 };
struct UnitDdKkt {
    int nv = 2, solve = 1, ldx = 0, ldr = 0, ldh = 0, ldw = 0, ldu = 0, ldp = 0;
    const int* mask = nullptr;
    const double *s = nullptr, *z = nullptr, *bx = nullptr, *bz = nullptr;
    double *sel_r = nullptr, *sel_q = nullptr, *sel_sc = nullptr, *sel_part = nullptr, *strong_x = nullptr;
    int *sel_i = nullptr, *strong_i = nullptr;
    double *H = nullptr, *U = nullptr, *M = nullptr, *Hf = nullptr, *Yt = nullptr, *Zt = nullptr, *S = nullptr, *Ms = nullptr;
    double *out_x = nullptr, *out_r = nullptr, *out_k = nullptr, *out_sc = nullptr, *end_x = nullptr, *end_r = nullptr;
    long *flag = nullptr, *lane_rep = nullptr, *report = nullptr;
};

// Arguments of Solver::test_capsolve (mbfir_test_capsolve of include/mbfir.h, which says what each array holds and checks them)
struct CapSolveIO {
    int n = 0, nlanes = 1, kp = 0, nrhs = 1, hsolve_form = -1;
    const int *k = nullptr, *mask = nullptr;
    const double *H = nullptr, *U = nullptr, *X = nullptr, *a = nullptr, *b = nullptr, *t = nullptr;
    double *M = nullptr, *Yt = nullptr, *Zt = nullptr, *S = nullptr, *Ms = nullptr, *rhs_w = nullptr, *y = nullptr, *w = nullptr,
           *zeta = nullptr, *dx = nullptr;
    int* flag = nullptr;
};

// mbfir_test_ddstages (include/mbfir.h): the launches of ddlin.hip with every stage read back, np = n rounded up to 64
struct DdStagesIO {
    int n = 0, k = 0, nrhs = 1, form = 1, nsolve = 1;          // form: 0 k_dd_trsv, 1 k_dd_trsv_mw, 2 k_dd_trsv_bi
    double pivtol = 0.0;
    const double *H = nullptr, *U = nullptr, *X = nullptr, *bh = nullptr, *bl = nullptr;
    double *Hh = nullptr, *Hl = nullptr, *d0 = nullptr, *Lh = nullptr, *Ll = nullptr, *Lth = nullptr, *Ltl = nullptr, *ri = nullptr,
           *dinv = nullptr, *xh = nullptr, *xl = nullptr;
    int* counter = nullptr;
};

class Solver {
public:
    explicit Solver(int device);
    ~Solver();
    Solver(const Solver&) = delete;
    Solver& operator=(const Solver&) = delete;
    // Solve the conic program; xout = x / tau (N entries).  Returns ST_*; throws HipError.
    int solve(const TrigProgram& P, const SolveOpts& o, std::vector<double>& xout, SolveInfo& info);
    // Lock-step batch: the programs (all of one shape, see shape_key) advance together through one stream, one
    // launch per phase with the design index as a grid dimension; designs that finish are masked out.
    void solve_lanes(const std::vector<const TrigProgram*>& Ps, const SolveOpts& o, std::vector<std::vector<double>>& xouts,
                     std::vector<SolveInfo>& infos);
    // equal keys = may share a lock-step unit: the program's CLASS (designer, order, unknowns, cones, lattice extent); grids,
    // row counts and chunk lists may differ within a unit on the lattice path without a big cone (heterogeneous units), elsewhere
    // the key also holds the exact shape
    static std::vector<long> shape_key(const TrigProgram& P, const SolveOpts& o);
    static int max_lanes(const TrigProgram& P, const SolveOpts& o);
    // host analysis of a frequency grid (no GPU needed): out[0] lattice ok, [1] folded entries, [2] pairs, [3] runs,
    // [4] longest run, [5] entries that fail the self-check (every frequency exactly once, |w| within 1 ulp of the entry's)
    static void test_fold(const double* w, int Mf, int fold, long* out);
    // fir_ap_cvx tap extraction on the device from the solution left by the last solve() / lane of solve_lanes().
    void specfact_last(int n, double* h_re, double* h_im, int lane = 0);
    void set_solution(const std::vector<double>& x);
    // kernel test hooks
    void test_gram(int m, int nt, int nw, const double* A, const double* d, double* out);
    void test_chol(int n, const double* H, double* out_l, double* out_m);
    void test_chol_lanes(int n, int nlanes, int form, const int* mask, const double* H, double* out_l, double* out_m);
    void test_specfact(int n, const double* x, double* h_re, double* h_im);
    // the operators of one lock-step unit (a unit of one included) at a caller's (s, z), through the stages and launch code of
    // solve_lanes: G v, G'u, W^-2 G v - sub and the normal matrix as build_H leaves it ahead of its factorisation
    void test_unit_ops(const std::vector<const TrigProgram*>& Ps, const SolveOpts& o, const UnitOps& io);
    // the cone stages of one iteration of a lock-step unit (a unit of one included) at a caller's iterate, through the stages of
    // launch_iteration, with the caller's "solutions" in place of the KKT solves
    void test_unit_cone(const std::vector<const TrigProgram*>& Ps, const SolveOpts& o, const UnitCone& io);
    // the residual kernels of an iterate and the plain KKT solve (or the initial point) of a lock-step unit at a caller's iterate and
    // right-hand sides, every group of launches of kkt_solve read back through its observer
    void test_unit_kkt(const std::vector<const TrigProgram*>& Ps, const SolveOpts& o, const UnitKkt& io);
    // the extended-precision path of a lock-step unit at a caller's iterate and right-hand sides: the selection of the strong sets, the
    // capped normal matrix with its strong rows, and every group of launches of kkt_solve_dd read back through its observer
    void test_unit_ddkkt(const std::vector<const TrigProgram*>& Ps, const SolveOpts& o, const UnitDdKkt& io);
    void test_ddsolve(int n, int k, const double* H, const double* U, const double* X, int nrhs, const double* bh,
                      const double* bl, double* xh, double* xl, int* nfix, double* Lh_out = nullptr, double* Ll_out = nullptr);
    // the same kernels stage by stage: the update, the factorisation (with the block inverses), nsolve solves in a chosen form on one
    // flag array, everything read back at the padded size
    void test_ddstages(const DdStagesIO& io);
    // the capacitance form of the extended-precision solve: the launches of its build and of one pass of its solve, for nlanes
    // problems laid out as a lock-step unit lays them out, every intermediate returned
    void test_capsolve(const CapSolveIO& io);
    void test_mfma_peak(double* tf_mfma, double* tf_valu);
    void test_time_kernels(int n, int m, int nt, int reps, double* ms_chol, double* ms_gram);
    void* stream() const;
    // RCCL communicator for row-sharded solves (one process per GPU): rank 0 makes the id, everybody joins
    void comm_unique_id(char* id128);
    void comm_init(int nranks, int rank, const char* id128);
    void comm_destroy();
    void test_comm_allreduce(double* v, long n, int op);
    void set_allreduce(int (*fn)(void*, long, int, void*), void* user);

private:
    struct Impl;
    Impl* impl;
};

}  // namespace mbfir
