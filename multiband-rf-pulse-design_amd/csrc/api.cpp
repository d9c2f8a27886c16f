// C ABI of include/mbfir.h: context management and the four designer entry points.
// Each entry point = host assembly (assemble.cpp) -> device IPM (solver.hip) -> tap extraction.
#include "../../include/mbfir.h"
#include "program.h"
#include "pulse.h"
#include "solver.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <memory>
#include <stdexcept>
#include <system_error>
#include <thread>

using namespace mbfir;

struct mbfir_ctx {
    std::unique_ptr<Solver> solver;
    int device = 0;                 // the solver's device, on which the pulse tools run too
    std::vector<double> last_x;
    std::string err;
    mbfir_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    bool has_comm = false;
};

namespace {

thread_local std::string g_create_error;

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

constexpr double DDKKT_THETA = 1e6;       // oracle/designers.py uses the same value

// which: the designer (DES_*): the extended-precision KKT solve is on by default for fir_qp_cvx only
SolveOpts to_opts(const mbfir_opts* o, int which) {
    SolveOpts s;
    s.ddkkt_theta = which == DES_QP ? DDKKT_THETA : 0.0;
    if (!o) return s;
    if (o->ddkkt > 0) s.ddkkt_theta = DDKKT_THETA;
    if (o->ddkkt < 0) s.ddkkt_theta = 0.0;
    if (o->max_iter > 0) s.max_iter = o->max_iter;
    if (o->feastol > 0) s.feastol = o->feastol;
    if (o->abstol > 0) s.abstol = o->abstol;
    if (o->reltol > 0) s.reltol = o->reltol;
    if (o->refine >= 0) s.refine = o->refine > 8 ? 8 : o->refine;   // MAX_SWEEPS of solver.hip: the norm slots hold 9 values
    s.verbose = o->verbose;
    s.shard_rank = o->shard_rank;
    s.shard_size = o->shard_size;
    s.dense_trig = o->dense_trig != 0;
    return s;
}

int status_to_rc(int st) {
    switch (st) {
        case ST_OPTIMAL:
        case ST_OPTIMAL_INACCURATE: return MBFIR_SOLVED;      // reference accepts 'Inaccurate/Solved' (fir_ap_cvx.m:176)
        case ST_PRIMAL_INFEASIBLE:
        case ST_DUAL_INFEASIBLE: return MBFIR_INFEASIBLE;
        default: return MBFIR_NUMERICAL;
    }
}

void fill_info(mbfir_info* info, const TrigProgram& P, const SolveInfo& si, int rc, double t0, double t_asm,
               double t_solved, double t_end) {
    if (!info) return;
    std::memset(info, 0, sizeof(*info));
    info->status = rc; info->iters = si.iters; info->n_unknowns = P.N();
    info->n_rows = si.n_rows; info->n_freq = si.n_freq;      // of this process's row shard
    info->n_lp = P.l; info->n_q3 = P.nq3; info->n_big = P.big;
    info->pcost = si.pcost; info->dcost = si.dcost; info->gap = si.gap; info->relgap = si.relgap;
    info->pres = si.pres; info->dres = si.dres;
    info->ms_assemble = (t_asm - t0) + si.ms_assemble; info->ms_solve = si.ms_solve;
    info->ms_post = t_end - t_solved; info->ms_total = t_end - t0;
    info->ms_gram = si.ms_gram; info->ms_chol = si.ms_chol; info->gram_flop = si.gram_flop;
    info->gram_launches = si.lattice ? 0 : si.h_builds * (P.quad ? 3 : 1);
    info->lattice = si.lattice;
    info->chol_launches = si.chol_launches; info->chol_flop = si.chol_flop; info->builds = si.h_builds;
    info->dd_iters = si.dd_iters; info->dd_kmax = si.dd_kmax; info->lanes = si.lanes; info->collectives = si.collectives;
    info->collective_bytes = si.collective_bytes;
    info->ms_cap = si.ms_cap; info->cap_flop = si.cap_flop; info->dd_form = si.dd_iters > 0 ? si.dd_form : -1;
    info->correctors = si.correctors; info->correctors_taken = si.correctors_taken; info->gv_passes = si.gv_passes; info->gtv_passes = si.gtv_passes; info->pair_passes = si.pair_passes;
}

// Solution vector -> taps, per designer.  lane: which design of the solver's last lock-step batch (fir_ap_cvx runs
// the spectral factorisation on the device from the solution left there).
void taps_from_solution(Solver& solver, const TrigProgram& P, const std::vector<double>& x, int lane, double* h_re, double* h_im) {
    const int n = P.n;
    switch (P.which) {
        case DES_AP:
            solver.specfact_last(n, h_re, h_im, lane);           // fir_ap_cvx.m:185-186,202
            break;
        case DES_LINPROG: {
            // fill_h, ss/fir_linprog.m:274-296: Hermitian extension of the half filter
            const int nh = P.nhalf;
            for (int i = 0; i < n; ++i) { h_re[i] = 0; h_im[i] = 0; }
            if (P.real_filter) {
                if (P.odd_filter) for (int k = 0; k < nh; ++k) { h_re[nh - 1 + k] = x[k]; h_re[nh - 1 - k] = x[k]; }
                else for (int k = 0; k < nh; ++k) { h_re[nh + k] = x[k]; h_re[nh - 1 - k] = x[k]; }
            } else if (P.odd_filter) {
                for (int k = 0; k < nh; ++k) {
                    double re = x[k], im = k == 0 ? 0.0 : x[nh + k - 1];
                    h_re[nh - 1 + k] = re; h_im[nh - 1 + k] = im;
                    h_re[nh - 1 - k] = re; h_im[nh - 1 - k] = -im;
                }
            } else {
                for (int k = 0; k < nh; ++k) {
                    double re = x[k], im = x[nh + k];
                    h_re[nh + k] = re; h_im[nh + k] = im;
                    h_re[nh - 1 - k] = re; h_im[nh - 1 - k] = -im;
                }
            }
            break;
        }
        default:                                                 // fir_qp_cvx.m:209, ss/fir_qprog_phs.m:389
            for (int i = 0; i < n; ++i) { h_re[i] = x[i]; h_im[i] = x[n + i]; }
    }
}

// Common driver of one design: `asm_rc` / `asm_err` are the result of assembling `P`; on success the taps go to h_re / h_im.
int run(mbfir_ctx* ctx, int asm_rc, const std::string& asm_err, const TrigProgram& P, const mbfir_opts* opts,
        mbfir_info* info, double t0, double* h_re, double* h_im) {
    if (!ctx) return MBFIR_E_ARG;
    if (info) std::memset(info, 0, sizeof(*info));
    if (asm_rc != 0) {
        ctx->err = asm_err;
        if (info) info->status = asm_rc;
        return asm_rc;
    }
    if (opts && opts->shard_size > 1 && !ctx->allreduce && !ctx->has_comm) {
        ctx->err = "row-sharded solve requested without a communicator (mbfir_comm_init) or an all-reduce hook";
        return MBFIR_E_ARG;
    }
    try {
        double t_asm = now_ms();
        SolveInfo si;
        std::vector<double> x;
        SolveOpts so = to_opts(opts, P.which);
        int st = ctx->solver->solve(P, so, x, si);
        // A numerical failure (never an infeasibility certificate) -- or a solve that only met the reduced tolerances
        // ('Inaccurate/Solved') -- is a precision limit of the double-precision normal equations: near cond(H) ~ 1e14 the
        // Cholesky factor starts replacing pivots, a few iterations earlier on the lattice path, whose moments carry
        // 1e-14 of recurrence noise, than on the dense one.  The remedy is precision, not the
        // path: retry once with the extended-precision KKT solve (same path), and only if that does not give a full-
        // accuracy solve either once more on the dense path.  The best of the attempts is returned.
        bool ran_retry = false;
        auto rank_of = [](int status) { return status == ST_OPTIMAL ? 2 : status == ST_OPTIMAL_INACCURATE ? 1 : 0; };
        auto retry = [&](bool dense) {
            const SolveInfo first = si;
            const std::vector<double> x_first = x;
            const int st_first = st;
            so.ddkkt_theta = DDKKT_THETA;
            so.dense_trig = so.dense_trig || dense;
            st = ctx->solver->solve(P, so, x, si);
            const bool keep_first = rank_of(st_first) > rank_of(st);
            const SolveInfo second = si;
            if (keep_first) { si = first; x = x_first; st = st_first; }
            const SolveInfo& other = keep_first ? second : first;
            si.ms_assemble += other.ms_assemble; si.ms_solve += other.ms_solve; si.ms_chol += other.ms_chol;
            si.ms_gram += other.ms_gram; si.h_builds += other.h_builds; si.chol_launches += other.chol_launches;
            si.iters += other.iters; si.dd_iters += other.dd_iters; si.ms_cap += other.ms_cap; si.cap_flop += other.cap_flop;
            ran_retry = true;
            return !keep_first;
        };
        auto wants_retry = [&]() { return status_to_rc(st) == MBFIR_NUMERICAL || st == ST_OPTIMAL_INACCURATE; };
        if (wants_retry() && so.shard_size <= 1 && !(so.ddkkt_theta > 0) && !(opts && opts->ddkkt < 0)) retry(false);
        // the extended-precision retry does not exist row-sharded (its double-double factorisation works on the whole normal
        // matrix of ONE context): the verdict stands, with the reason on record for the caller
        if (wants_retry() && so.shard_size > 1)
            ctx->err = st == ST_OPTIMAL_INACCURATE
                           ? "row-sharded solve met the reduced tolerances only ('Inaccurate/Solved'); the extended-precision retry runs unsharded only"
                           : "row-sharded solve ended 'numerical'; the extended-precision retry (opts.ddkkt) runs unsharded only -- solve this design on one GPU";
        // the capacitance form of the extended-precision solve works in plain double on a k x k matrix that loses rank when the
        // strong directions become dependent; the double-double factorisation of the whole matrix does not care: one more try
        if (wants_retry() && so.shard_size <= 1 && so.ddkkt_theta > 0 && so.dd_form == 0 && !std::getenv("MBFIR_DDFORM")) { so.dd_form = 1; retry(false); }
        if (wants_retry() && si.lattice && !so.dense_trig && so.shard_size <= 1 && (double)P.Mf * P.N() <= 6e8) retry(true);
        // fir_ap_cvx extracts its taps on the device from the solution the LAST solve left there; after a retry the
        // winner may be an earlier attempt: put the returned solution there
        if (ran_retry && status_to_rc(st) == MBFIR_SOLVED) ctx->solver->set_solution(x);
        ctx->last_x = x;
        double t_solved = now_ms();
        int rc = status_to_rc(st);
        if (rc == MBFIR_SOLVED) taps_from_solution(*ctx->solver, P, x, 0, h_re, h_im);
        fill_info(info, P, si, rc, t0, t_asm, t_solved, now_ms());
        return rc;
    } catch (const std::exception& e) {
        ctx->err = e.what();
        if (info) info->status = MBFIR_E_HIP;
        return MBFIR_E_HIP;
    }
}

// ---- batch of independent designs --------------------------------------------------------------
// The jobs are assembled on the host, grouped by shape (Solver::shape_key: same dimensions, same lattice
// structure) and cut into units of up to `lanes` designs.  A unit of one design runs as a single solve; a unit of
// several runs in LOCK STEP on one context: one stream, one launch per phase with the design index as a grid
// dimension, finished designs masked out (Solver::solve_lanes).  One host thread per context pulls units from a
// shared counter, so units also overlap across the contexts' streams.  The dependency-chain phases of one design
// (Cholesky panels, reductions) leave most of the chip idle; the other lanes' blocks fill it.
int assemble_job(const mbfir_job& J, int grid_m, TrigProgram& P, std::string& e) {
    switch (J.which) {
        case DES_AP: return assemble_ap(J.n, J.nband, J.f, J.a, J.d, J.params[0], J.params[1], grid_m, P, e);
        case DES_QP: return assemble_qp(J.n, J.nband, J.f, J.a, J.d, J.params[0], J.params + 1, int(J.params[3]), grid_m, P, e);
        case DES_LINPROG: return assemble_linprog(J.n, J.nband, J.f, J.a, J.d, grid_m, P, e);
        case DES_QPROG_PHS: {
            std::vector<double> are(2 * J.nband), aim(2 * J.nband), dre(J.nband), dim(J.nband);
            for (int i = 0; i < 2 * J.nband; ++i) { are[i] = J.a[2 * i]; aim[i] = J.a[2 * i + 1]; }
            for (int i = 0; i < J.nband; ++i) { dre[i] = J.d[2 * i]; dim[i] = J.d[2 * i + 1]; }
            return assemble_qprog_phs(J.n, J.nband, J.f, are.data(), aim.data(), dre.data(), dim.data(), grid_m, P, e);
        }
        default: e = "unknown designer"; return MBFIR_E_ARG;
    }
}

// Assembled programs are a few MB of vectors each; giving them back to the allocator is 0.1-0.2 ms a piece (munmap).  The
// workers do that for their unit while other units still run; the programs of the LAST unit to finish -- the one every
// caller waits for -- are parked here and freed by the next batch's coordinator while its units run (or at unload).
std::mutex g_parked_mu;
std::vector<TrigProgram> g_parked;

// One call of mbfir_solve_batch.  Round 2 assembled all jobs, then grouped, then started the units: 8 ms of a 265 ms headline
// batch with the GPU idle, and the unit that decides the makespan (the tight-ripple designs at the head of a sweep) started
// last of all.  Now the assembly threads take the jobs in order, and a coordinator (the calling thread) hands a unit to the
// waiting contexts the moment its designs are there.  The units are formed SPECULATIVELY from neighbours in the job list on
// the assumption that the batch has one shape (a sweep): the first design that differs from job 0, or fails to assemble,
// ends the speculation, and what has not been handed out yet is grouped by shape.
struct Batch {
    mbfir_ctx* const* ctxs; int nctx;
    mbfir_job* jobs; int njobs;
    const mbfir_opts* opts;
    double t0 = now_ms();
    int lanes_cap = opts ? opts->lanes : 0;                    // 0 = automatic, 1 = never lock-step
    // the assembly threads assemble every job; row-sharded and with lanes == 1 every unit is one design, assembled by its
    // worker just before the solve (one program alive per context)
    bool early = !(opts && opts->shard_size > 1) && lanes_cap != 1;
    bool trace = std::getenv("MBFIR_TRACE_BATCH") != nullptr;
    std::vector<TrigProgram> progs = std::vector<TrigProgram>(njobs);
    std::vector<int> arc = std::vector<int>(njobs, 0);         // assembly result per job (its message is in jobs[q].err)
    std::vector<std::vector<long>> keys = std::vector<std::vector<long>>(njobs);   // shape key, the shape's lane cap last
    std::vector<char> assembled = std::vector<char>(njobs, 0);
    std::vector<std::vector<int>> units;
    std::atomic<int> next_asm{0};
    size_t units_taken = 0, units_done = 0;
    bool units_closed = false;
    std::mutex mu;
    std::condition_variable cv_asm, cv_units;
    std::string thread_err;                                   // the first exception a thread let out

    // job q into progs[q]; with early assembly its shape key too (CSR maps, lattice analysis: a sort of the grid) -- here,
    // not in the serial grouping: 64 headline designs cost 40 ms there with the GPU idle; the structures stay with the program
    void assemble(int q) {
        std::string e;
        jobs[q].err[0] = 0;
        try {
            arc[q] = assemble_job(jobs[q], opts ? opts->grid_m : 0, progs[q], e);
            if (arc[q] == 0 && early) {
                const SolveOpts so = to_opts(opts, progs[q].which);
                keys[q] = Solver::shape_key(progs[q], so);
                keys[q].push_back(Solver::max_lanes(progs[q], so));
            }
        } catch (const std::exception& ex) {                  // (host memory: the job is reported, the coordinator is not left waiting)
            arc[q] = MBFIR_E_HIP; e = ex.what();
        }
        if (arc[q] != 0) std::snprintf(jobs[q].err, sizeof(jobs[q].err), "%s", e.c_str());
    }
    void assemble_loop() {
        for (int q; (q = next_asm.fetch_add(1)) < njobs;) {
            assemble(q);
            { std::lock_guard<std::mutex> lk(mu); assembled[q] = 1; }
            cv_asm.notify_all();
        }
    }
    void wait_assembled(int lo, int hi) {
        std::unique_lock<std::mutex> lk(mu);
        cv_asm.wait(lk, [&] { for (int q = lo; q < hi; ++q) if (!assembled[q]) return false; return true; });
    }
    void push_unit(std::vector<int> u) {
        { std::lock_guard<std::mutex> lk(mu); units.push_back(std::move(u)); }
        cv_units.notify_one();
    }

    // ---- units: designs of one shape, up to `lanes` of them ------------------------------------------
    // enough units to occupy every context, no more lanes per unit than the shape allows; an explicit request never
    // exceeds what the shape allows
    int lanes_per_unit(int cap, int G) const {
        int per = std::min(cap, std::max(1, (G + nctx - 1) / nctx));
        if (lanes_cap > 1) per = std::min(std::min(lanes_cap, cap), G);
        return std::max(1, per);
    }
    // units of job 0's shape, each handed out as soon as its designs are assembled; returns how many jobs went out
    int hand_out_first_shape() {
        if (njobs == 0) return 0;
        wait_assembled(0, 1);
        if (arc[0] != 0) return 0;
        const int per = lanes_per_unit(int(keys[0].back()), njobs);
        int handed = 0;
        while (handed < njobs) {
            const int hi = std::min(njobs, handed + per);
            wait_assembled(handed, hi);
            for (int q = handed; q < hi; ++q)
                if (arc[q] != 0 || keys[q] != keys[0]) return handed;
            std::vector<int> u;
            for (int q = handed; q < hi; ++q) u.push_back(q);
            push_unit(std::move(u));
            if (trace && handed == 0) std::fprintf(stderr, "[batch] first unit handed out at %.2f ms\n", now_ms() - t0);
            handed = hi;
        }
        return handed;
    }
    // jobs [handed, njobs) by shape; which designs share a unit: neighbours in the job list (a sweep's neighbours tend to
    // need similar iteration counts, so the lanes of a unit finish together)
    void group_rest(int handed) {
        std::map<std::vector<long>, std::vector<int>> groups;
        for (int q = handed; q < njobs; ++q) {
            if (arc[q] != 0) { push_unit({q}); continue; }                  // the single-design path reports the assembly error
            groups[keys[q]].push_back(q);
        }
        for (auto& g : groups) {
            const int G = int(g.second.size()), per = lanes_per_unit(int(g.first.back()), G);
            for (int i = 0; i < G; i += per) push_unit(std::vector<int>(g.second.begin() + i, g.second.begin() + std::min(G, i + per)));
        }
    }
    void coordinate() {
        if (!early) {
            for (int q = 0; q < njobs; ++q) push_unit({q});
            return;
        }
        const int handed = hand_out_first_shape();
        wait_assembled(handed, njobs);
        if (trace) std::fprintf(stderr, "[batch] %d jobs assembled at %.2f ms\n", njobs, now_ms() - t0);
        group_rest(handed);
    }
    // a context's worker: pulls units until the coordinator has closed the list
    void work(int c) {
        mbfir_ctx* ctx = ctxs[c];
        for (;;) {
            std::vector<int> U;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_units.wait(lk, [&] { return units_taken < units.size() || units_closed; });
                if (units_taken >= units.size()) break;
                U = units[units_taken++];
            }
            if (U.size() == 1) solve_singles(ctx, U, {0});
            else solve_lock_step(ctx, U);
            release(U);
        }
    }
    void solve_lock_step(mbfir_ctx* ctx, const std::vector<int>& U) {
        std::vector<char> done(U.size(), 0);         // designs whose result is already out (a later error must not overwrite it)
        try {
            const double t_asm = now_ms();
            std::vector<const TrigProgram*> Ps;
            for (int q : U) Ps.push_back(&progs[q]);
            std::vector<std::vector<double>> xs;
            std::vector<SolveInfo> sis;
            ctx->solver->solve_lanes(Ps, to_opts(opts, progs[U[0]].which), xs, sis);
            const double t_solved = now_ms();
            for (size_t b = 0; b < U.size(); ++b) {
                mbfir_job& J = jobs[U[b]];
                const int rc = status_to_rc(sis[b].status);
                if (rc == MBFIR_NUMERICAL || sis[b].status == ST_OPTIMAL_INACCURATE) continue;   // single path: retries in extended precision
                if (rc == MBFIR_SOLVED) taps_from_solution(*ctx->solver, progs[U[b]], xs[b], int(b), J.h_re, J.h_im);
                fill_info(&J.info, progs[U[b]], sis[b], rc, t0, t_asm, t_solved, now_ms());
                J.rc = rc;
                ctx->last_x = xs[b];
                report(ctx, U[b]);
                done[b] = 1;
            }
        } catch (const std::exception& e) {
            ctx->err = e.what();
            // A ShapeError (the lock-step path does not take these programs as one unit) or a ResourceError (the unit did not
            // get its device memory, lanes sized to the unit's maxima: ADVICE r4) is recoverable: one design at a time needs a
            // lane's worth, and the single-design path reports its own verdict or error.  Any other error (a lost in-launch
            // hand-off of the factorisation, a HIP error) is reported for every design of the unit that has no result yet,
            // NOT retried -- the single-design path takes other kernels and would hide a defect of the lock-step ones behind
            // a slow success.
            if (!dynamic_cast<const ShapeError*>(&e) && !dynamic_cast<const ResourceError*>(&e)) {
                for (size_t b = 0; b < U.size(); ++b) {
                    if (done[b]) continue;
                    mbfir_job& J = jobs[U[b]];
                    std::memset(&J.info, 0, sizeof(J.info));
                    J.info.status = MBFIR_E_HIP; J.info.lanes = int(U.size());
                    J.rc = MBFIR_E_HIP;
                    std::snprintf(J.err, sizeof(J.err), "lock-step unit of %d: %s", int(U.size()), e.what());
                }
                return;
            }
        }
        solve_singles(ctx, U, done);
    }
    // the designs of unit U without a result (done[b] == 0) one at a time, each on its assembled program: run re-derives what
    // a solve with other options needs (TrigProgram::prep is keyed by fold and dense path)
    void solve_singles(mbfir_ctx* ctx, const std::vector<int>& U, const std::vector<char>& done) {
        for (size_t b = 0; b < U.size(); ++b) {
            if (done[b]) continue;
            const int q = U[b];
            mbfir_job& J = jobs[q];
            const double t = now_ms();
            if (!early) assemble(q);
            J.rc = run(ctx, arc[q], J.err, progs[q], opts, &J.info, t, J.h_re, J.h_im);
            report(ctx, q);
        }
    }
    void report(mbfir_ctx* ctx, int q) {
        mbfir_job& J = jobs[q];
        if (J.rc < 0 && !J.err[0]) std::snprintf(J.err, sizeof(J.err), "%s", ctx->err.c_str());
        if (J.z && J.z_cap > 0 && J.rc >= 0) {
            const std::vector<double>& x = ctx->last_x;
            std::memcpy(J.z, x.data(), sizeof(double) * std::min<size_t>(x.size(), size_t(J.z_cap)));
        }
    }
    void release(const std::vector<int>& U) {
        bool last;
        { std::lock_guard<std::mutex> lk(mu); ++units_done; last = units_closed && units_done == units.size(); }
        if (!last) { for (int q : U) progs[q] = TrigProgram(); return; }
        std::lock_guard<std::mutex> lk(g_parked_mu);
        for (int q : U) g_parked.push_back(std::move(progs[q]));
    }
    // a worker / assembler that throws (bad_alloc while parking programs, ...) must not take the process down
    // (std::terminate from a thread's entry function): the first message is kept and the call returns MBFIR_E_HIP
    template <class F>
    void guarded(F&& body) {
        try { body(); }
        catch (const std::exception& e) { std::lock_guard<std::mutex> lk(mu); if (thread_err.empty()) thread_err = e.what(); }
        catch (...) { std::lock_guard<std::mutex> lk(mu); if (thread_err.empty()) thread_err = "unknown exception in a batch thread"; }
    }
    // Starts the assembly threads and one worker per context, coordinates, joins; returns the first error, or "".  Thread
    // creation can fail (EAGAIN: up to 16 + nctx threads per call): what was started is joined and the rest of the work is
    // done by fewer threads -- in the limit by the calling thread alone (assembly inline, then the units one context after
    // the other) -- instead of destroying joinable threads, which ends the process.
    std::string run_threads() {
        std::vector<std::thread> th;
        const int nasm = early ? std::max(1, std::min(njobs, std::min(16, int(std::thread::hardware_concurrency())))) : 0;
        const int nwork = std::max(1, std::min(nctx, njobs));
        int started_asm = 0, started_work = 0;
        try {
            for (int i = 0; i < nasm; ++i) { th.emplace_back([this] { guarded([this] { assemble_loop(); }); }); ++started_asm; }
            for (int c = 0; c < nwork; ++c) { th.emplace_back([this, c] { guarded([this, c] { work(c); }); }); ++started_work; }
        } catch (const std::system_error&) {}
        if (nasm > 0 && started_asm == 0) guarded([this] { assemble_loop(); });
        std::string err;
        try { coordinate(); } catch (const std::exception& e) { err = e.what(); }
        { std::lock_guard<std::mutex> lk(mu); units_closed = true; }
        cv_units.notify_all();
        {
            std::vector<TrigProgram> old;
            { std::lock_guard<std::mutex> lk(g_parked_mu); old.swap(g_parked); }
        }                                                                // (the previous batch's last programs, freed while the units run)
        if (started_work == 0) guarded([this] { work(0); });
        for (auto& t : th) t.join();
        if (trace) std::fprintf(stderr, "[batch] %zu units, all done at %.2f ms\n", units.size(), now_ms() - t0);
        return err.empty() ? thread_err : err;
    }
};

}  // namespace

// ---- fault diagnostics (MBFIR_FAULT_MAPS=<file>) ---------------------------------------------------
// Round 3 recorded a SIGSEGV below hipLaunchKernel under `rocprofv3 --kernel-trace` whose log held bare PCs and no module map,
// so the frames between this library and the faulting copy could not be attributed.  With MBFIR_FAULT_MAPS set, the first
// mbfir_create installs a SIGSEGV / SIGBUS handler that writes the fault address and /proc/self/maps -- taken AT THE FAULT,
// so that queue rings, kernarg pools and thread arenas mapped since start-up are in it -- to that file (async-signal-safe
// calls only) and then hands the signal to whoever was installed before (the profiler's stack printer, the default action).
#include <csignal>
#include <fcntl.h>
#include <unistd.h>
namespace {
char g_maps_path[512];
struct sigaction g_old_segv, g_old_bus;
void put_hex(int fd, unsigned long v) {
    char b[19] = "0x0000000000000000";
    for (int i = 0; i < 16; ++i) b[17 - i] = "0123456789abcdef"[(v >> (4 * i)) & 15];
    (void)!write(fd, b, 18);
}
void fault_handler(int sig, siginfo_t* si, void* uc) {
    const int out = open(g_maps_path, O_WRONLY | O_CREAT | O_APPEND, 0644);
    if (out >= 0) {
        const char h1[] = "\n==== mbfir fault: signal ";
        (void)!write(out, h1, sizeof(h1) - 1);
        put_hex(out, (unsigned long)sig);
        const char h2[] = " at address ";
        (void)!write(out, h2, sizeof(h2) - 1);
        put_hex(out, (unsigned long)si->si_addr);
        const char h3[] = " ; /proc/self/maps at the fault:\n";
        (void)!write(out, h3, sizeof(h3) - 1);
        const int in = open("/proc/self/maps", O_RDONLY);
        if (in >= 0) {
            char buf[4096];
            for (;;) { const ssize_t n = read(in, buf, sizeof(buf)); if (n <= 0) break; (void)!write(out, buf, size_t(n)); }
            close(in);
        }
        close(out);
    }
    struct sigaction* old = sig == SIGBUS ? &g_old_bus : &g_old_segv;
    sigaction(sig, old, nullptr);                          // back to the previous handler: returning re-executes the faulting access
    (void)uc;
}
void install_fault_maps() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char* pth = std::getenv("MBFIR_FAULT_MAPS");
        if (!pth || !*pth) return;
        std::snprintf(g_maps_path, sizeof(g_maps_path), "%s", pth);
        struct sigaction sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.sa_sigaction = fault_handler;
        sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
        sigemptyset(&sa.sa_mask);
        sigaction(SIGSEGV, &sa, &g_old_segv);
        sigaction(SIGBUS, &sa, &g_old_bus);
    });
}
}  // namespace

extern "C" {

const char* mbfir_version(void) { return "mbfir 0.1 (gfx950)"; }

void mbfir_default_opts(mbfir_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->refine = -1;
}

mbfir_ctx* mbfir_create(int device_id) {
    try {
        install_fault_maps();                                  // (a profiler's handlers are installed at load: this one chains to them)
        mbfir_ctx* c = new mbfir_ctx();
        c->solver.reset(new Solver(device_id));
        c->device = device_id;
        return c;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return nullptr;
    }
}

void mbfir_destroy(mbfir_ctx* ctx) { delete ctx; }

const char* mbfir_last_error(mbfir_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void mbfir_set_allreduce(mbfir_ctx* ctx, mbfir_allreduce_fn fn, void* user) {
    if (!ctx) return;
    ctx->allreduce = fn;
    ctx->allreduce_user = user;
    ctx->solver->set_allreduce(fn, user);
}

int mbfir_comm_unique_id(mbfir_ctx* ctx, char* id128) {
    if (!ctx || !id128) return MBFIR_E_ARG;
    try { ctx->solver->comm_unique_id(id128); return 0; }
    catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_comm_init(mbfir_ctx* ctx, int nranks, int rank, const char* id128) {
    if (!ctx || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return MBFIR_E_ARG;
    try { ctx->solver->comm_init(nranks, rank, id128); ctx->has_comm = true; return 0; }
    catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_comm_allreduce(mbfir_ctx* ctx, double* v, long n, int op) {
    if (!ctx || !v || n < 0) return MBFIR_E_ARG;
    try { ctx->solver->test_comm_allreduce(v, n, op); return 0; }
    catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
void mbfir_comm_destroy(mbfir_ctx* ctx) {
    if (!ctx) return;
    ctx->solver->comm_destroy();
    ctx->has_comm = false;
}

int mbfir_last_solution(mbfir_ctx* ctx, double* z, int capacity) {
    if (!ctx || !z) return MBFIR_E_ARG;
    int n = int(ctx->last_x.size());
    if (capacity < n) n = capacity;
    std::memcpy(z, ctx->last_x.data(), sizeof(double) * n);
    return n;
}

int mbfir_ap_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* a, const double* d,
                   double obj, double peak, const mbfir_opts* opts, double* h_re, double* h_im,
                   mbfir_info* info) {
    double t0 = now_ms();
    TrigProgram P;
    std::string e;
    int rc = assemble_ap(n, nband, f, a, d, obj, peak, opts ? opts->grid_m : 0, P, e);
    return run(ctx, rc, e, P, opts, info, t0, h_re, h_im);
}

int mbfir_qp_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* a, const double* d,
                   double kquad, const double* obj, int nobj, const mbfir_opts* opts, double* h_re,
                   double* h_im, mbfir_info* info) {
    double t0 = now_ms();
    TrigProgram P;
    std::string e;
    int rc = assemble_qp(n, nband, f, a, d, kquad, obj, nobj, opts ? opts->grid_m : 0, P, e);
    return run(ctx, rc, e, P, opts, info, t0, h_re, h_im);
}

int mbfir_linprog_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* a, const double* d,
                        const mbfir_opts* opts, double* h_re, double* h_im, mbfir_info* info) {
    double t0 = now_ms();
    TrigProgram P;
    std::string e;
    int rc = assemble_linprog(n, nband, f, a, d, opts ? opts->grid_m : 0, P, e);
    return run(ctx, rc, e, P, opts, info, t0, h_re, h_im);
}

int mbfir_qprog_phs_solve(mbfir_ctx* ctx, int n, int nband, const double* f, const double* ac_re,
                          const double* ac_im, const double* dc_re, const double* dc_im,
                          const mbfir_opts* opts, double* h_re, double* h_im, mbfir_info* info) {
    double t0 = now_ms();
    TrigProgram P;
    std::string e;
    int rc = assemble_qprog_phs(n, nband, f, ac_re, ac_im, dc_re, dc_im, opts ? opts->grid_m : 0, P, e);
    return run(ctx, rc, e, P, opts, info, t0, h_re, h_im);
}

// the batch of independent designs: see Batch above
int mbfir_solve_batch(mbfir_ctx* const* ctxs, int nctx, mbfir_job* jobs, int njobs, const mbfir_opts* opts) {
    if (!ctxs || nctx < 1 || (!jobs && njobs > 0) || njobs < 0) return MBFIR_E_ARG;
    for (int c = 0; c < nctx; ++c)
        if (!ctxs[c]) return MBFIR_E_ARG;
    const std::string err = Batch{ctxs, nctx, jobs, njobs, opts}.run_threads();
    if (!err.empty()) {
        for (int q = 0; q < njobs; ++q) {                  // (host memory exhausted while forming units: nothing of the batch is reported)
            jobs[q].rc = MBFIR_E_HIP;
            std::snprintf(jobs[q].err, sizeof(jobs[q].err), "%s", err.c_str());
        }
        return MBFIR_E_HIP;
    }
    int worst = 0;
    for (int q = 0; q < njobs; ++q)
        if (jobs[q].rc < worst) worst = jobs[q].rc;
    return worst;                                         // 0, or the most negative error code of the batch
}

// ---- device kernel test hooks ------------------------------------------------------------------
#define MBFIR_TRY(ctx, stmt)                   \
    if (!ctx) return MBFIR_E_ARG;              \
    try { stmt; return 0; }                    \
    catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }

int mbfir_test_gram(mbfir_ctx* ctx, int m, int nt, int nw, const double* A, const double* d, double* out) {
    MBFIR_TRY(ctx, ctx->solver->test_gram(m, nt, nw, A, d, out));
}
int mbfir_test_chol(mbfir_ctx* ctx, int n, const double* H, double* out_l, double* out_m) {
    MBFIR_TRY(ctx, ctx->solver->test_chol(n, H, out_l, out_m));
}
int mbfir_test_chol_lanes(mbfir_ctx* ctx, int n, int nlanes, int form, const int* mask, const double* H, double* out_l, double* out_m) {
    MBFIR_TRY(ctx, ctx->solver->test_chol_lanes(n, nlanes, form, mask, H, out_l, out_m));
}
int mbfir_test_unit_ops(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int nv, int ldx, int ldr, int ldh,
                        const double* v, const double* u, const double* sub, const double* s, const double* z, const int* mask,
                        double* gv, double* gtu, double* wgv, double* H, long* report, double* tmin) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_unit_ops: " + why; return MBFIR_E_ARG; };
    if (!jobs || njobs < 1 || nv < 1 || nv > 2 || !v || !u || !s || !z || !gv || !gtu || !wgv || !H || !report || !tmin) return bad("bad argument");
    try {
        std::vector<TrigProgram> progs(njobs);
        std::vector<const TrigProgram*> Ps;
        for (int q = 0; q < njobs; ++q) {
            std::string e;
            if (assemble_job(jobs[q], opts ? opts->grid_m : 0, progs[q], e) != 0) return bad("job " + std::to_string(q) + ": " + e);
            Ps.push_back(&progs[q]);
        }
        const SolveOpts so = to_opts(opts, progs[0].which);
        if (so.shard_size > 1) return bad("row-sharded units are not taken");
        if (so.ddkkt_theta > 0) return bad("units on the extended-precision path are not taken (opts.ddkkt = -1 for fir_qp_cvx)");
        UnitOps io;
        io.nv = nv; io.ldx = ldx; io.ldr = ldr; io.ldh = ldh; io.v = v; io.u = u; io.sub = sub; io.s = s; io.z = z; io.mask = mask;
        io.gv = gv; io.gtu = gtu; io.wgv = wgv; io.H = H; io.report = report; io.tmin = tmin;
        ctx->solver->test_unit_ops(Ps, so, io);
        return 0;
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_unit_cone(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int form, int corrector, int ldx, int ldr,
                         int ldw, const int* mask, const double* in_r, const double* in_x, const double* in_sc, double* out_r, double* out_x,
                         double* out_w3, double* out_sc, long* report) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_unit_cone: " + why; return MBFIR_E_ARG; };
    if (!jobs || njobs < 1 || !in_r || !in_x || !in_sc || !out_r || !out_x || !out_w3 || !out_sc || !report) return bad("bad argument");
    if (form < 0 || form > 1) return bad("form must be 0 (the form a solve on one rank runs) or 1 (two-phase)");
    try {
        std::vector<TrigProgram> progs(njobs);
        std::vector<const TrigProgram*> Ps;
        for (int q = 0; q < njobs; ++q) {
            std::string e;
            if (assemble_job(jobs[q], opts ? opts->grid_m : 0, progs[q], e) != 0) return bad("job " + std::to_string(q) + ": " + e);
            Ps.push_back(&progs[q]);
        }
        const SolveOpts so = to_opts(opts, progs[0].which);
        if (so.shard_size > 1) return bad("row-sharded units are not taken");
        if (so.ddkkt_theta > 0) return bad("units on the extended-precision path are not taken (opts.ddkkt = -1 for fir_qp_cvx)");
        UnitCone io;
        io.form = form; io.corr = corrector != 0; io.ldx = ldx; io.ldr = ldr; io.ldw = ldw; io.mask = mask;
        io.in_r = in_r; io.in_x = in_x; io.in_sc = in_sc; io.out_r = out_r; io.out_x = out_x; io.out_w3 = out_w3; io.out_sc = out_sc;
        io.report = report;
        ctx->solver->test_unit_cone(Ps, so, io);
        return 0;
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_unit_kkt(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int mode, int form, int two, int wbz_ready,
                        int nv, int ldx, int ldr, int ldh, int ldw, const int* mask, const int* nsweep, const double* s, const double* z,
                        const double* x, const double* tau_kappa, const double* bx, const double* bz, double* res_r, double* res_x,
                        double* res_sc, double* M, long* flag, double* out_x, double* out_r, double* out_sc, double* init_r, double* init_x,
                        double* init_w3, long* report) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_unit_kkt: " + why; return MBFIR_E_ARG; };
    if (!jobs || njobs < 1 || !nsweep || !s || !z || !x || !tau_kappa || !res_r || !res_x || !res_sc || !M || !flag || !out_x || !out_r ||
        !out_sc || !report)
        return bad("bad argument");
    if (mode < 0 || mode > 1) return bad("mode must be 0 (a solve of the caller's right-hand sides) or 1 (the initial point)");
    if (form < 0 || form > 1) return bad("form must be 0 (the residual kernels of a solve on one rank) or 1 (two-phase)");
    if (nv < 1 || nv > 2) return bad("one or two right-hand sides");
    if (mode == 1 && (nv != 2 || wbz_ready || !init_r || !init_x || !init_w3)) return bad("the initial point solves two right-hand sides from the winv2 entry and needs the init blocks");
    if (wbz_ready && nv != 2) return bad("wbz_ready goes with two right-hand sides");
    if ((bx == nullptr) != (bz == nullptr)) return bad("bx and bz go together");
    if (mode == 0 && !bx && nv != 2) return bad("the residual kernels leave two right-hand sides");
    for (int b = 0; b < njobs; ++b)
        if (nsweep[b] < 0 || nsweep[b] > 8) return bad("a sweep count outside 0 .. 8");
    try {
        std::vector<TrigProgram> progs(njobs);
        std::vector<const TrigProgram*> Ps;
        for (int q = 0; q < njobs; ++q) {
            std::string e;
            if (assemble_job(jobs[q], opts ? opts->grid_m : 0, progs[q], e) != 0) return bad("job " + std::to_string(q) + ": " + e);
            Ps.push_back(&progs[q]);
        }
        const SolveOpts so = to_opts(opts, progs[0].which);
        if (so.shard_size > 1) return bad("row-sharded units are not taken");
        if (so.ddkkt_theta > 0) return bad("units on the extended-precision path are not taken (opts.ddkkt = -1 for fir_qp_cvx)");
        UnitKkt io;
        io.mode = mode; io.form = form; io.two = two; io.wbz_ready = wbz_ready; io.nv = nv; io.ldx = ldx; io.ldr = ldr; io.ldh = ldh; io.ldw = ldw;
        io.mask = mask; io.nsweep = nsweep; io.s = s; io.z = z; io.x = x; io.tau_kappa = tau_kappa; io.bx = bx; io.bz = bz;
        io.res_r = res_r; io.res_x = res_x; io.res_sc = res_sc; io.M = M; io.flag = flag; io.out_x = out_x; io.out_r = out_r; io.out_sc = out_sc;
        io.init_r = init_r; io.init_x = init_x; io.init_w3 = init_w3; io.report = report;
        ctx->solver->test_unit_kkt(Ps, so, io);
        return 0;
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_unit_ddkkt(mbfir_ctx* ctx, const mbfir_job* jobs, int njobs, const mbfir_opts* opts, int nv, int solve, int ldx, int ldr, int ldh,
                          int ldw, int ldu, int ldp, const int* mask, const double* s, const double* z, const double* bx, const double* bz, double* sel_r,
                          double* sel_q, double* sel_sc, double* sel_part, int* sel_i, int* strong_i, double* strong_x, double* H, double* U, double* M, double* Hf,
                          double* Yt, double* Zt, double* S, double* Ms, long* flag, double* out_x, double* out_r, double* out_k, double* out_sc,
                          double* end_x, double* end_r, long* lane_rep, long* report) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_unit_ddkkt: " + why; return MBFIR_E_ARG; };
    // (nothing is allocated, copied or launched before every argument has passed)
    if (!jobs || !s || !z || !bx || !bz || !sel_r || !sel_q || !sel_sc || !sel_part || !sel_i || !strong_i || !strong_x || !H || !U || !M || !Hf || !flag ||
        !out_x || !out_r || !out_k || !out_sc || !end_x || !end_r || !lane_rep || !report)
        return bad("bad argument");
    if ((Yt == nullptr) != (Zt == nullptr) || (Yt == nullptr) != (S == nullptr) || (Yt == nullptr) != (Ms == nullptr)) return bad("Yt, Zt, S and Ms go together");
    if (njobs < 1 || njobs > 64) return bad("the lane count must be 1 .. 64");
    if (nv < 1 || nv > 2) return bad("one or two right-hand sides");
    if (ldx < 1 || ldr < 1 || ldh < 64 || ldh % 64 != 0 || ldx > ldh || ldw < 4 || ldw % 4 != 0 || ldu < 64 || ldu > DK_KMAX || ldp < 1)
        return bad("leading dimensions: 1 <= ldx <= ldh = np, a multiple of 64; ldr >= 1; ldw = 4 max(n_q3, 1); 64 <= ldu <= 3072; ldp >= 1");
    try {
        std::vector<TrigProgram> progs(njobs);
        std::vector<const TrigProgram*> Ps;
        for (int q = 0; q < njobs; ++q) {
            std::string e;
            if (assemble_job(jobs[q], opts ? opts->grid_m : 0, progs[q], e) != 0) return bad("job " + std::to_string(q) + ": " + e);
            Ps.push_back(&progs[q]);
        }
        const SolveOpts so = to_opts(opts, progs[0].which);
        if (so.shard_size > 1) return bad("row-sharded units are not taken");
        if (!(so.ddkkt_theta > 0)) return bad("the unit is not on the extended-precision path (opts.ddkkt = 1)");
        const char* env = std::getenv("MBFIR_DDFORM");
        const bool dd_form = env ? std::string(env) == "dd" : so.dd_form != 0;                 // (the solve's own choice: read_switches, plan_unit)
        if (dd_form && njobs > 1) return bad("the double-double form of the extended-precision solve runs one design at a time");
        for (int q = 0; q < njobs; ++q) {
            const TrigProgram& T = *Ps[q];
            const int N = T.Nt + T.Ne, R = T.l + 3 * T.nq3 + T.big;
            if (ldx < N || ldr < R || ldh != int((N + 63) / 64 * 64) || ldw < 4 * T.nq3)
                return bad("job " + std::to_string(q) + ": ldx / ldr / ldh / ldw do not fit the design (N " + std::to_string(N) + ", R " + std::to_string(R) + ")");
        }
        UnitDdKkt io;
        io.nv = nv; io.solve = solve; io.ldx = ldx; io.ldr = ldr; io.ldh = ldh; io.ldw = ldw; io.ldu = ldu; io.ldp = ldp; io.mask = mask; io.s = s; io.z = z;
        io.bx = bx; io.bz = bz; io.sel_r = sel_r; io.sel_q = sel_q; io.sel_sc = sel_sc; io.sel_part = sel_part; io.sel_i = sel_i; io.strong_i = strong_i;
        io.strong_x = strong_x; io.H = H; io.U = U; io.M = M; io.Hf = Hf; io.Yt = Yt; io.Zt = Zt; io.S = S; io.Ms = Ms; io.flag = flag;
        io.out_x = out_x; io.out_r = out_r; io.out_k = out_k; io.out_sc = out_sc; io.end_x = end_x; io.end_r = end_r; io.lane_rep = lane_rep;
        io.report = report;
        ctx->solver->test_unit_ddkkt(Ps, so, io);
        return 0;
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_ddsolve(mbfir_ctx* ctx, int n, int k, const double* H, const double* U, const double* X, int nrhs,
                       const double* bh, const double* bl, double* xh, double* xl, int* nfix, double* Lh, double* Ll) {
    if (!ctx || n < 1 || k < 0 || nrhs < 1 || nrhs > 2 || !H || !bh || !bl || !xh || !xl || !nfix) return MBFIR_E_ARG;
    MBFIR_TRY(ctx, ctx->solver->test_ddsolve(n, k, H, U, X, nrhs, bh, bl, xh, xl, nfix, Lh, Ll));
}
int mbfir_test_ddstages(mbfir_ctx* ctx, int n, int k, const double* H, const double* U, const double* X, int nrhs, const double* bh,
                        const double* bl, double pivtol, int form, int nsolve, double* Hh, double* Hl, double* d0, double* Lh, double* Ll,
                        double* Lth, double* Ltl, double* ri, double* dinv, double* xh, double* xl, int* counter) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_ddstages: " + why; return MBFIR_E_ARG; };
    if (n < 1 || n > 4096) return bad("n must be 1 .. 4096");
    if (k < 0) return bad("k < 0");
    if (nrhs < 1 || nrhs > 2) return bad("nrhs must be 1 or 2");
    if (form < 0 || form > 2) return bad("form must be 0 (single), 1 (mw) or 2 (bi)");
    if (nsolve < 1 || nsolve > 64) return bad("nsolve must be 1 .. 64");
    if (!H || (k > 0 && (!U || !X)) || !bh || !bl || !Hh || !Hl || !d0 || !Lh || !Ll || !Lth || !Ltl || !ri || !dinv || !xh || !xl || !counter)
        return bad("null array");
    try {
        DdStagesIO io;
        io.n = n; io.k = k; io.nrhs = nrhs; io.form = form; io.nsolve = nsolve; io.pivtol = pivtol; io.H = H; io.U = U; io.X = X; io.bh = bh; io.bl = bl;
        io.Hh = Hh; io.Hl = Hl; io.d0 = d0; io.Lh = Lh; io.Ll = Ll; io.Lth = Lth; io.Ltl = Ltl; io.ri = ri; io.dinv = dinv; io.xh = xh; io.xl = xl;
        io.counter = counter;
        ctx->solver->test_ddstages(io);
        return 0;
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_capsolve(mbfir_ctx* ctx, int n, int nlanes, const int* k, int kp, int nrhs, int hsolve_form, const int* mask,
                        const double* H, const double* U, const double* X, const double* a, const double* b, const double* t,
                        double* M, double* Yt, double* Zt, double* S, double* Ms, double* rhs_w, double* y, double* w,
                        double* zeta, double* dx, int* flag) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_capsolve: " + why; return MBFIR_E_ARG; };
    // (nothing is allocated, copied or launched before every argument has passed)
    if (n < 1) return bad("n < 1");
    if (nlanes < 1 || nlanes > 16) return bad("nlanes must be 1 .. 16");
    if (nrhs < 1 || nrhs > 2) return bad("nrhs must be 1 or 2");
    if (kp < 64 || kp > 1024 || kp % 64 != 0) return bad("kp must be a multiple of 64, at most 1024");
    if (!k || !H || !U || !X || !a || !b || !t || !M || !Yt || !Zt || !S || !Ms || !rhs_w || !y || !w || !zeta || !dx || !flag) return bad("null array");
    for (int q = 0; q < nlanes; ++q)
        if (k[q] < 1 || k[q] > kp) return bad("lane " + std::to_string(q) + ": k = " + std::to_string(k[q]) + " is not in 1 .. kp = " + std::to_string(kp));
    if (hsolve_form < -1 || hsolve_form > 1) return bad("hsolve_form must be -1, 0 or 1");
    if (hsolve_form == 1 && (n + 63) / 64 * 64 > 1024) return bad("the one-pass M'(M b) takes np <= 1024");
    try {
        CapSolveIO io;
        io.n = n; io.nlanes = nlanes; io.kp = kp; io.nrhs = nrhs; io.hsolve_form = hsolve_form; io.k = k; io.mask = mask;
        io.H = H; io.U = U; io.X = X; io.a = a; io.b = b; io.t = t;
        io.M = M; io.Yt = Yt; io.Zt = Zt; io.S = S; io.Ms = Ms; io.rhs_w = rhs_w; io.y = y; io.w = w; io.zeta = zeta; io.dx = dx; io.flag = flag;
        ctx->solver->test_capsolve(io);
        return 0;
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
}
int mbfir_test_fold(const double* w, int m, int fold, long* out) {
    if (!w || m < 1 || !out) return MBFIR_E_ARG;
    try { Solver::test_fold(w, m, fold, out); } catch (const std::exception&) { return MBFIR_E_HIP; }
    return 0;
}
int mbfir_test_specfact(mbfir_ctx* ctx, int n, const double* x, double* h_re, double* h_im) {
    MBFIR_TRY(ctx, ctx->solver->test_specfact(n, x, h_re, h_im));
}
int mbfir_b2a(mbfir_ctx* ctx, int n, const double* b_re, const double* b_im, double* a_re, double* a_im) {
    if (!ctx || n < 1 || !b_re || !b_im || !a_re || !a_im) return MBFIR_E_ARG;
    MBFIR_TRY(ctx, slr_run(ctx->device, ctx->solver->stream(), n, b_re, b_im, nullptr, nullptr, a_re, a_im, nullptr, nullptr));
}
int mbfir_ab2rf(mbfir_ctx* ctx, int n, const double* a_re, const double* a_im, const double* b_re, const double* b_im,
                double* rf_re, double* rf_im) {
    if (!ctx || n < 1 || n > 2048 || !a_re || !a_im || !b_re || !b_im || !rf_re || !rf_im) return MBFIR_E_ARG;
    MBFIR_TRY(ctx, slr_run(ctx->device, ctx->solver->stream(), n, b_re, b_im, a_re, a_im, nullptr, nullptr, rf_re, rf_im));
}
int mbfir_b2rf(mbfir_ctx* ctx, int n, const double* b_re, const double* b_im, double* rf_re, double* rf_im) {
    if (!ctx || n < 1 || n > 2048 || !b_re || !b_im || !rf_re || !rf_im) return MBFIR_E_ARG;
    MBFIR_TRY(ctx, slr_run(ctx->device, ctx->solver->stream(), n, b_re, b_im, nullptr, nullptr, nullptr, nullptr, rf_re, rf_im));
}
int mbfir_b2rf_batch(mbfir_ctx* ctx, int n, int count, const double* b_re, const double* b_im, double* rf_re, double* rf_im) {
    if (!ctx) return MBFIR_E_ARG;
    if (n < 2 || n > 2048 || count < 1 || !b_re || !rf_re || !rf_im) {
        ctx->err = "b2rf_batch: need 2 <= n <= 2048, count >= 1 and the b_re / rf arrays";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, slr_b2rf_batch_run(ctx->device, ctx->solver->stream(), n, count, b_re, b_im, rf_re, rf_im));
}
int mbfir_slr2d_batch(mbfir_ctx* ctx, int m, int n, int count, const double* r_re, const double* r_im, double* out_re,
                      double* out_im, int literal) {
    if (!ctx) return MBFIR_E_ARG;
    if (n < 2 || n > 2048 || m < 2 || m > 2048 || m % 2 || count < 1 || (long)count * (m > n ? m : n) > 2147483647L || !r_re ||
        !out_re || !out_im || (literal != 0 && literal != 1)) {
        ctx->err = "slr2d_batch: need 2 <= n <= 2048, 2 <= m <= 2048 with m even, count >= 1 (count max(m, n) < 2^31), the "
                   "r_re / out arrays and literal 0 or 1";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, slr_slr2d_batch_run(ctx->device, ctx->solver->stream(), m, n, count, r_re, r_im, out_re, out_im, literal));
}
// the argument rules of mbfir_flip_search, shared with its test hook
static bool flip_args_ok(mbfir_ctx* ctx, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re, const double* z_im,
                         const double* zf_re, const double* zf_im, long ncand, const unsigned* masks, const int* enum_bits,
                         int scale_rule, double s_re, int criterion, const double* beta_re, const double* beta_im, const long* winner) {
    if (!ctx || n < 2 || n > 1024 || nz < 0 || nz > n - 1 || nz > 1023 || ncand < 1 || !c0_re || !c0_im || !winner ||
        (nz > 0 && (!z_re || !z_im || !zf_re || !zf_im)) || (!beta_re) != (!beta_im) || (criterion != 0 && criterion != 1) ||
        (scale_rule != 0 && scale_rule != 1) || (scale_rule == 1 && !(s_re >= 0.0 && s_re <= 1.0)))
        return false;
    if (!masks) {
        if (ncand > (1L << 24)) return false;
        if (!enum_bits && (nz > 24 || ncand != (1L << nz))) return false;
        for (int j = 0; enum_bits && j < nz; ++j)
            if (enum_bits[j] < 0 || (enum_bits[j] >> 1) >= 24) return false;
    }
    return true;
}
int mbfir_flip_search(mbfir_ctx* ctx, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re, const double* z_im,
                      const double* zf_re, const double* zf_im, long ncand, const unsigned* masks, const int* enum_bits,
                      int scale_rule, double s_re, double s_im, int criterion, int tie_high, double* peaks, double* beta_re,
                      double* beta_im, long* winner, double* winner_peak) {
    if (!flip_args_ok(ctx, n, nz, c0_re, c0_im, z_re, z_im, zf_re, zf_im, ncand, masks, enum_bits, scale_rule, s_re, criterion, beta_re,
                      beta_im, winner))
        return MBFIR_E_ARG;
    try {
        *winner = flip_search_run(ctx->device, ctx->solver->stream(), n, nz, c0_re, c0_im, z_re, z_im, zf_re, zf_im, ncand, masks,
                                  enum_bits, scale_rule, s_re, s_im, criterion, tie_high ? 1 : 0, peaks, beta_re, beta_im, winner_peak);
    } catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
    if (*winner < 0) { ctx->err = "flip search: no candidate has a finite peak"; return MBFIR_NUMERICAL; }
    return 0;
}
int mbfir_test_flip_stages(mbfir_ctx* ctx, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re,
                           const double* z_im, const double* zf_re, const double* zf_im, long ncand, const unsigned* masks,
                           const int* enum_bits, int scale_rule, double s_re, double s_im, int criterion, int tie_high, int force_mode,
                           int max_blocks, int nsel, const long* sel, double* peaks, double* blk_p, long* blk_i, double* beta_re,
                           double* beta_im, long* winner, double* winner_peak, double* st_beta, double* st_bf, double* st_xl,
                           double* st_xlfp, double* st_afa, double* st_a, double* st_theta, double* st_peak, long* report) {
    if (!flip_args_ok(ctx, n, nz, c0_re, c0_im, z_re, z_im, zf_re, zf_im, ncand, masks, enum_bits, scale_rule, s_re, criterion, beta_re,
                      beta_im, winner))
        return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_flip_stages: " + why; return MBFIR_E_ARG; };
    if (force_mode < -1 || force_mode > 2) return bad("force_mode must be -1, 0, 1 or 2");
    if (max_blocks < 0) return bad("max_blocks must be 0 (as a search chooses) or a positive cap");
    if (nsel < 0 || nsel > 1024) return bad("nsel must lie in [0, 1024]");
    if (!peaks || !blk_p || !blk_i || !report || !beta_re) return bad("peaks, blk_p, blk_i, beta and report are required");
    if (nsel > 0 && (!sel || !st_beta || !st_bf || !st_xl || !st_xlfp || !st_afa || !st_a || !st_theta || !st_peak))
        return bad("sel and every stage block are required when nsel > 0");
    for (int q = 0; q < nsel; ++q)
        if (sel[q] < 0 || sel[q] >= ncand) return bad("sel[" + std::to_string(q) + "] is not a candidate index");
    const FlipStages hook{force_mode, max_blocks, nsel, sel, blk_p, blk_i, st_beta, st_bf, st_xl, st_xlfp, st_afa, st_a, st_theta, st_peak,
                          report};
    try {
        *winner = flip_search_run(ctx->device, ctx->solver->stream(), n, nz, c0_re, c0_im, z_re, z_im, zf_re, zf_im, ncand, masks,
                                  enum_bits, scale_rule, s_re, s_im, criterion, tie_high ? 1 : 0, peaks, beta_re, beta_im, winner_peak,
                                  &hook);
    } catch (const std::invalid_argument& e) { return bad(e.what()); }
    catch (const std::exception& e) { ctx->err = e.what(); return MBFIR_E_HIP; }
    if (*winner < 0) { ctx->err = "flip search: no candidate has a finite peak"; return MBFIR_NUMERICAL; }
    return 0;
}
int mbfir_remez_batch(mbfir_ctx* ctx, mbfir_remez_job* jobs, int njobs, const mbfir_remez_opts* opts) {
    if (!ctx) return MBFIR_E_ARG;
    const int density = opts && opts->grid_density > 0 ? opts->grid_density : 16;
    const int maxiter = opts && opts->maxiter > 0 ? opts->maxiter : 25;
    if (!jobs || njobs < 1 || density > 1024 || maxiter > 10000) { ctx->err = "remez: bad batch or options"; return MBFIR_E_ARG; }
    std::vector<RemezJobHost> hj(njobs);
    for (int q = 0; q < njobs; ++q) {
        mbfir_remez_job& j = jobs[q];
        auto bad = [&](const char* why) { ctx->err = "remez job " + std::to_string(q) + ": " + why; return MBFIR_E_ARG; };
        if (j.type != MBFIR_REMEZ_BANDPASS) return bad("only symmetric (bandpass) filters; no Hilbert or differentiator");
        if (j.numtaps < 3 || j.numtaps > 2047) return bad("numtaps must be in [3, 2047]");
        if (j.nband < 1 || j.nband > 64) return bad("nband must be in [1, 64]");
        if (!j.edges || !j.desired || !j.weight || !j.h) return bad("null array");
        for (int b = 0; b < 2 * j.nband; ++b) {
            const double e = j.edges[b];
            if (!(e >= 0.0 && e <= 1.0)) return bad("band edges must lie in [0, 1]");
            if (b > 0 && !(e >= j.edges[b - 1])) return bad("band edges must ascend");
            if ((b & 1) == 0 && b > 0 && !(e > j.edges[b - 1])) return bad("bands must not touch or overlap");
            if (!std::isfinite(j.desired[b])) return bad("desired amplitude not finite");
        }
        for (int b = 0; b < j.nband; ++b)
            if (!(j.weight[b] > 0.0) || !std::isfinite(j.weight[b])) return bad("weights must be positive and finite");
        const int L = (j.numtaps & 1) ? (j.numtaps + 1) / 2 : j.numtaps / 2;
        std::vector<int> cnt(j.nband);
        if (remez_grid_counts(j.numtaps, j.nband, j.edges, density, cnt.data()) < L + 1) return bad("dense grid smaller than L + 1");
        hj[q] = RemezJobHost{j.numtaps, j.nband, j.edges, j.desired, j.weight, j.h, j.ext, &j.status, &j.iterations, &j.delta};
    }
    MBFIR_TRY(ctx, remez_run(ctx->device, ctx->solver->stream(), njobs, hj.data(), density, maxiter));
}
int mbfir_fmp(mbfir_ctx* ctx, int l, const double* h_re, const double* h_im, double* out_re, double* out_im) {
    if (!ctx) return MBFIR_E_ARG;
    if (l < 1 || l > 2047 || (l & 1) == 0 || !h_re || !out_re || !out_im) {
        ctx->err = "fmp: filter length must be odd and at most 2047";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, fmp_run(ctx->device, ctx->solver->stream(), l, h_re, h_im, out_re, out_im));
}
int mbfir_test_specfact_stages(mbfir_ctx* ctx, int kind, int n, int nlanes, const double* in_re, const double* in_im, int guard,
                               double fill, long extra, long* layout, double* raw) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "mbfir_test_specfact_stages: " + why; return MBFIR_E_ARG; };
    if (kind != 0 && kind != 1) return bad("kind must be 0 (k_specfact) or 1 (k_fmp)");
    if (kind == 0 && (n < 1 || n > 4096)) return bad("n must lie in [1, 4096] (lp <= 65536)");
    if (kind == 1 && (n < 1 || n > 2047 || (n & 1) == 0)) return bad("filter length must be odd and at most 2047");
    if (nlanes < 1 || nlanes > 64 || (kind == 1 && nlanes != 1)) return bad("nlanes must lie in [1, 64], and be 1 for k_fmp");
    if (guard < 0 || guard > 65536 || extra < 0 || extra > 1048576) return bad("guard must lie in [0, 65536], extra in [0, 1048576]");
    if (!layout || (raw && !in_re)) return bad("layout is required, and the input when raw is given");
    MBFIR_TRY(ctx, specfact_stages_run(ctx->device, ctx->solver->stream(), kind, n, nlanes, in_re, in_im, guard, fill, extra, layout, raw));
}
int mbfir_test_mfma_peak(mbfir_ctx* ctx, double* tf_mfma, double* tf_valu) {
    MBFIR_TRY(ctx, ctx->solver->test_mfma_peak(tf_mfma, tf_valu));
}

// ---- forward simulators: every offset and size checked before any device work ----------------------------------------------
// An offset table of count + 1 entries (count items of at least one and at most 2^31 - 1 entries each): null, or the reason.
static const char* sim_offsets_bad(const long* off, int count) {
    if (off[0] != 0) return "does not start at 0";
    for (int i = 0; i < count; ++i) {
        if (off[i + 1] == off[i]) return "has an empty item";
        if (off[i + 1] < off[i]) return "descends";
        if (off[i + 1] - off[i] > 2147483647L) return "has an item of more than 2^31 - 1 entries";
    }
    return nullptr;
}
// Output entries and workgroups of a batch (pulse p: npoint[p] points of ntout[p] entries at each of nscale scales): false when
// a sum overflows, the output exceeds 2^56 entries or the launch 2^31 - 1 workgroups.
static bool sim_sizes(int npulse, int nscale, const long* npoint, const long* ntout) {
    long total = 0, nblk = 0;
    for (int p = 0; p < npulse; ++p) {
        long e, b;
        if (__builtin_mul_overflow(npoint[p], (long)nscale, &e) || __builtin_mul_overflow(e, ntout[p], &e) ||
            __builtin_add_overflow(total, e, &total) || __builtin_mul_overflow((npoint[p] + 255) / 256, (long)nscale, &b) ||
            __builtin_add_overflow(nblk, b, &nblk))
            return false;
    }
    return total <= (1L << 56) && nblk <= 2147483647L;
}
// The offset table of the pulses themselves (named `name`): 0, or what bad returns for the first fault, an empty pulse by its index.
static int sim_pulse_offsets_bad(const long* off, int npulse, const char* name, const std::function<int(const std::string&)>& bad) {
    const char* why = sim_offsets_bad(off, npulse);
    if (!why) return 0;
    for (int p = 0; p < npulse && off[0] == 0 && off[p + 1] >= off[p]; ++p)
        if (off[p + 1] == off[p]) return bad("pulse " + std::to_string(p) + " has no samples");
    return bad(std::string("inconsistent offsets: ") + name + " " + why);
}

// The single-pulse calls, after their own checks, are the batch of one pulse (offset tables {0, n}) at one scale, 1.0.
static const double SIM_ONE = 1.0;
int mbfir_bloch(mbfir_ctx* ctx, int ntime, const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                const double* gz, const double* tsteps, double t1, double t2, int nfreq, const double* df, int npos,
                const double* dx, const double* dy, const double* dz, int mode, double gamma, double* mx, double* my, double* mz) {
    if (!ctx || ntime < 1 || nfreq < 1 || npos < 1 || !b1_re || !b1_im || !tsteps || !df || !mx || !my || !mz || mode < 0 || mode > 3 ||
        !(t1 > 0) || !(t2 > 0))
        return MBFIR_E_ARG;
    const long toff[2] = {0, ntime}, foff[2] = {0, nfreq}, poff[2] = {0, npos}, npoint = (long)nfreq * npos, ntout = (mode & 2) ? ntime : 1;
    if (!sim_sizes(1, 1, &npoint, &ntout)) return MBFIR_E_ARG;
    MBFIR_TRY(ctx, bloch_batch_run(ctx->device, ctx->solver->stream(), 1, toff, b1_re, b1_im, gx, gy, gz, toff, tsteps, &t1, &t2, &gamma,
                                   1, foff, df, 1, poff, dx, dy, dz, 1, &SIM_ONE, mode, mx, my, mz));
}
int mbfir_abr(mbfir_ctx* ctx, int n, const double* rf_re, const double* rf_im, const double* g, int nx, const double* x,
              int mode, double* a_re, double* a_im, double* b_re, double* b_im) {
    if (!ctx || n < 1 || nx < 1 || !rf_re || !rf_im || !x || !a_re || !a_im || !b_re || !b_im || (mode != 0 && mode != 1))
        return MBFIR_E_ARG;
    const long roff[2] = {0, n}, xoff[2] = {0, nx};
    MBFIR_TRY(ctx, abr_batch_run(ctx->device, ctx->solver->stream(), 1, roff, rf_re, rf_im, g, 1, xoff, x, 1, &SIM_ONE, mode, a_re, a_im,
                                 b_re, b_im));
}
int mbfir_abr2(mbfir_ctx* ctx, int n, const double* rf_re, const double* rf_im, const double* gx, const double* gy, int nx,
               const double* x, int ny, const double* y, double* a_re, double* a_im, double* b_re, double* b_im) {
    if (!ctx) return MBFIR_E_ARG;
    if (n < 1 || nx < 1 || ny < 1 || (long)nx * ny > (1L << 30) || !rf_re || !rf_im || !x || !y || !a_re || !a_im || !b_re || !b_im) {
        ctx->err = "abr2: need n, nx, ny >= 1 (nx ny <= 2^30) and the rf, x, y, a, b arrays";
        return MBFIR_E_ARG;
    }
    const long roff[2] = {0, n}, xoff[2] = {0, nx}, yoff[2] = {0, ny};
    MBFIR_TRY(ctx, abr2_batch_run(ctx->device, ctx->solver->stream(), 1, roff, rf_re, rf_im, gx, gy, 1, xoff, x, 1, yoff, y, 1, &SIM_ONE,
                                  0, a_re, a_im, b_re, b_im));
}

// The argument checks of mbfir_bloch_batch, shared with its adjoint (who: the call's name in the message; arrays: the caller's own
// required arrays are all there).  0, or MBFIR_E_ARG with ctx->err set.  npoint (npulse entries) receives the points per pulse.
static int bloch_batch_check(mbfir_ctx* ctx, const char* who, int npulse, const long* toff, const long* tsoff, const double* t1,
                             const double* t2, int nfgrid, const long* foff, int npgrid, const long* poff, int nscale, int mode,
                             bool arrays, std::vector<long>& npoint) {
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (npulse < 1) return bad("no pulses");
    if (nscale < 1) return bad("the scale list is empty");
    if (mode < 0 || mode > 3) return bad("mode must be 0, 1, 2 or 3");
    if ((nfgrid != 1 && nfgrid != npulse) || (npgrid != 1 && npgrid != npulse)) return bad("nfgrid and npgrid must be 1 or npulse");
    if (!arrays) return bad("a required array is null");
    if (const int e = sim_pulse_offsets_bad(toff, npulse, "toff", bad)) return e;
    if (tsoff[0] != 0) return bad("inconsistent offsets: tsoff does not start at 0");
    for (int p = 0; p < npulse; ++p) {
        const long nt = toff[p + 1] - toff[p], nts = tsoff[p + 1] - tsoff[p];
        if (nts != 1 && nts != nt)
            return bad("tp of pulse " + std::to_string(p) + " has " + std::to_string(nts) + " entries, neither 1 nor its " +
                       std::to_string(nt) + " samples");
        if (!(t1[p] > 0) || !(t2[p] > 0)) return bad("t1 and t2 of pulse " + std::to_string(p) + " must be positive");
    }
    if (const char* why = sim_offsets_bad(foff, nfgrid)) return bad(std::string("inconsistent offsets: foff ") + why);
    if (const char* why = sim_offsets_bad(poff, npgrid)) return bad(std::string("inconsistent offsets: poff ") + why);
    npoint.assign(npulse, 0);
    std::vector<long> ntout(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int fg = nfgrid == 1 ? 0 : p, pg = npgrid == 1 ? 0 : p;
        npoint[p] = (foff[fg + 1] - foff[fg]) * (poff[pg + 1] - poff[pg]);
        ntout[p] = (mode & 2) ? toff[p + 1] - toff[p] : 1;
    }
    if (toff[npulse] > (1L << 56) || !sim_sizes(npulse, nscale, npoint.data(), ntout.data()))
        return bad("the output size or the workgroup count overflows");
    return 0;
}

int mbfir_bloch_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                      const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                      const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                      const double* dx, const double* dy, const double* dz, int nscale, const double* scales, int mode, double* mx,
                      double* my, double* mz) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && mx && my && mz;
    if (const int e = bloch_batch_check(ctx, "bloch_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, mode,
                                        arrays, npoint))
        return e;
    MBFIR_TRY(ctx, bloch_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                   gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, mode, mx, my, mz));
}

// The argument checks of mbfir_abr_batch / mbfir_abr2_batch, shared with their adjoints (who: the call's name in the message; two: the
// 2D calls, which alone have y grids; arrays: the caller's own required arrays are all there).  0, or MBFIR_E_ARG with ctx->err set.
// npoint (npulse entries) receives the points per pulse.
static int abr_batch_check(mbfir_ctx* ctx, const char* who, bool two, int npulse, const long* roff, int nxgrid, const long* xoff,
                           int nygrid, const long* yoff, int nscale, int mode, bool arrays, std::vector<long>& npoint) {
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (npulse < 1) return bad("no pulses");
    if (nscale < 1) return bad("the scale list is empty");
    if (mode != 0 && mode != 1) return bad("mode must be 0 or 1");
    if ((nxgrid != 1 && nxgrid != npulse) || (two && nygrid != 1 && nygrid != npulse))
        return bad(two ? "nxgrid and nygrid must be 1 or npulse" : "nxgrid must be 1 or npulse");
    if (!arrays) return bad("a required array is null");
    if (const int e = sim_pulse_offsets_bad(roff, npulse, "roff", bad)) return e;
    if (const char* why = sim_offsets_bad(xoff, nxgrid)) return bad(std::string("inconsistent offsets: xoff ") + why);
    if (two)
        if (const char* why = sim_offsets_bad(yoff, nygrid)) return bad(std::string("inconsistent offsets: yoff ") + why);
    npoint.assign(npulse, 0);
    std::vector<long> ntout(npulse, 1);
    for (int p = 0; p < npulse; ++p) {
        const int xg = nxgrid == 1 ? 0 : p, yg = nygrid == 1 ? 0 : p;
        npoint[p] = (xoff[xg + 1] - xoff[xg]) * (two ? yoff[yg + 1] - yoff[yg] : 1L);      // each factor < 2^31
    }
    if (roff[npulse] > (1L << 56) || !sim_sizes(npulse, nscale, npoint.data(), ntout.data()))
        return bad("the output size or the workgroup count overflows");
    return 0;
}
// The adjoints keep one partial per (workgroup, sample): false when their count overflows or exceeds 2^56.
static bool vjp_partials_fit(int npulse, int nscale, const long* roff, const long* npoint) {
    long total = 0;
    for (int p = 0; p < npulse; ++p) {
        long e;
        if (__builtin_mul_overflow((npoint[p] + 255) / 256 * nscale, roff[p + 1] - roff[p], &e) ||
            __builtin_add_overflow(total, e, &total))
            return false;
    }
    return total <= (1L << 56);
}

int mbfir_abr_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                    int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, double* a_re,
                    double* a_im, double* b_re, double* b_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales && a_re && a_im && b_re && b_im;
    if (const int e = abr_batch_check(ctx, "abr_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays, npoint)) return e;
    MBFIR_TRY(ctx, abr_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales,
                                 mode, a_re, a_im, b_re, b_im));
}

int mbfir_abr2_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                     const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff, const double* y,
                     int nscale, const double* scales, int mode, double* a_re, double* a_im, double* b_re, double* b_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales && a_re && a_im && b_re && b_im;
    if (const int e = abr_batch_check(ctx, "abr2_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays, npoint))
        return e;
    MBFIR_TRY(ctx, abr2_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff,
                                  y, nscale, scales, mode, a_re, a_im, b_re, b_im));
}

int mbfir_abr_vjp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                        int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                        const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im, double* g_re,
                        double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales && ca_re && ca_im && cb_re && cb_im && g_re && g_im;
    if (const int e = abr_batch_check(ctx, "abr_vjp_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays, npoint))
        return e;
    if (!vjp_partials_fit(npulse, nscale, roff, npoint.data())) {
        ctx->err = "abr_vjp_batch: the output size or the workgroup count overflows";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, abr_vjp_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales,
                                     mode, ca_re, ca_im, cb_re, cb_im, g_re, g_im));
}

int mbfir_abr2_vjp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                         const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                         const double* y, int nscale, const double* scales, int mode, const double* ca_re, const double* ca_im,
                         const double* cb_re, const double* cb_im, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales && ca_re && ca_im && cb_re && cb_im && g_re && g_im;
    if (const int e = abr_batch_check(ctx, "abr2_vjp_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays,
                                      npoint))
        return e;
    if (!vjp_partials_fit(npulse, nscale, roff, npoint.data())) {
        ctx->err = "abr2_vjp_batch: the output size or the workgroup count overflows";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, abr2_vjp_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid,
                                      yoff, y, nscale, scales, mode, ca_re, ca_im, cb_re, cb_im, g_re, g_im));
}

// The Bloch adjoint keeps 3 x 256 checkpoint doubles per (workgroup, group of 8 samples): false when their count overflows or
// exceeds 2^56.
static bool bloch_checkpoints_fit(int npulse, int nscale, const long* toff, const long* npoint) {
    long total = 0;
    for (int p = 0; p < npulse; ++p) {
        long e;
        if (__builtin_mul_overflow((npoint[p] + 255) / 256 * nscale, (toff[p + 1] - toff[p] + 7) / 8 * 768, &e) ||
            __builtin_add_overflow(total, e, &total))
            return false;
    }
    return total <= (1L << 56);
}

int mbfir_bloch_vjp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                          const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                          const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                          const double* m0x, const double* m0y, const double* m0z, const double* cmx, const double* cmy,
                          const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y, double* gm0z) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string("bloch_vjp_batch: ") + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, "bloch_vjp_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    if (!cmx || !cmy || !cmz || !g_re || !g_im) return bad("a cotangent or gradient plane is null");
    if ((m0x || m0y || m0z) && !(m0x && m0y && m0z)) return bad("m0x, m0y and m0z are given together or not at all");
    if ((gm0x || gm0y || gm0z) && !(gm0x && gm0y && gm0z)) return bad("gm0x, gm0y and gm0z are given together or not at all");
    if (!vjp_partials_fit(npulse, nscale, toff, npoint.data()) || !bloch_checkpoints_fit(npulse, nscale, toff, npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_vjp_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                       gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, cmx, cmy,
                                       cmz, g_re, g_im, gm0x, gm0y, gm0z));
}

// The Bloch b1 and gr adjoint keeps five doubles per (workgroup, sample): the rf pair and the three g components.
static bool bloch_gr_partials_fit(int npulse, int nscale, const long* toff, const long* npoint) {
    long total = 0;
    for (int p = 0; p < npulse; ++p) {
        long e;
        if (__builtin_mul_overflow((npoint[p] + 255) / 256 * nscale, toff[p + 1] - toff[p], &e) ||
            __builtin_add_overflow(total, e, &total))
            return false;
    }
    return total <= (1L << 54);
}

int mbfir_bloch_vjp_gr_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* m0x, const double* m0y, const double* m0z, const double* cmx,
                             const double* cmy, const double* cmz, double* g_re, double* g_im, double* gm0x, double* gm0y,
                             double* gm0z, double* ggx, double* ggy, double* ggz, double* gdf) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string("bloch_vjp_gr_batch: ") + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, "bloch_vjp_gr_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    if (!cmx || !cmy || !cmz || !g_re || !g_im) return bad("a cotangent or gradient plane is null");
    if (!ggx || !ggy || !ggz) return bad("a plane of the gradient waveform's gradient (ggx, ggy, ggz) is null");
    if ((m0x || m0y || m0z) && !(m0x && m0y && m0z)) return bad("m0x, m0y and m0z are given together or not at all");
    if ((gm0x || gm0y || gm0z) && !(gm0x && gm0y && gm0z)) return bad("gm0x, gm0y and gm0z are given together or not at all");
    if (!bloch_gr_partials_fit(npulse, nscale, toff, npoint.data()) || !bloch_checkpoints_fit(npulse, nscale, toff, npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_vjp_gr_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                          t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, cmx,
                                          cmy, cmz, g_re, g_im, gm0x, gm0y, gm0z, ggx, ggy, ggz, gdf));
}

// The rf and g adjoints keep up to two double2 per (workgroup, sample): the rf pair and the g component(s).
static bool vjp_rfg_partials_fit(int npulse, int nscale, const long* roff, const long* npoint) {
    long total = 0;
    for (int p = 0; p < npulse; ++p) {
        long e;
        if (__builtin_mul_overflow((npoint[p] + 255) / 256 * nscale, roff[p + 1] - roff[p], &e) ||
            __builtin_add_overflow(total, e, &total))
            return false;
    }
    return total <= (1L << 55);
}

int mbfir_abr_vjp_rfg_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                            int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode,
                            const double* ca_re, const double* ca_im, const double* cb_re, const double* cb_im, double* g_re,
                            double* g_im, double* gg) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales && ca_re && ca_im && cb_re && cb_im && g_re && g_im && gg;
    if (const int e = abr_batch_check(ctx, "abr_vjp_rfg_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays,
                                      npoint))
        return e;
    if (!vjp_rfg_partials_fit(npulse, nscale, roff, npoint.data())) {
        ctx->err = "abr_vjp_rfg_batch: the output size or the workgroup count overflows";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, abr_vjp_rfg_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale,
                                         scales, mode, ca_re, ca_im, cb_re, cb_im, g_re, g_im, gg));
}

int mbfir_abr2_vjp_rfg_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im,
                             const double* gx, const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid,
                             const long* yoff, const double* y, int nscale, const double* scales, int mode, const double* ca_re,
                             const double* ca_im, const double* cb_re, const double* cb_im, double* g_re, double* g_im,
                             double* ggx, double* ggy) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales && ca_re && ca_im && cb_re && cb_im && g_re &&
                        g_im && ggx && ggy;
    if (const int e = abr_batch_check(ctx, "abr2_vjp_rfg_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays,
                                      npoint))
        return e;
    if (!vjp_rfg_partials_fit(npulse, nscale, roff, npoint.data())) {
        ctx->err = "abr2_vjp_rfg_batch: the output size or the workgroup count overflows";
        return MBFIR_E_ARG;
    }
    MBFIR_TRY(ctx, abr2_vjp_rfg_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x,
                                          nygrid, yoff, y, nscale, scales, mode, ca_re, ca_im, cb_re, cb_im, g_re, g_im, ggx, ggy));
}

// What the tangent calls check after abr_batch_check (bloch_batch_check): ndir, and that ndir times the R rf samples, ndir times the
// forward output (at most 2^56 entries each) and the forward workgroups times the direction groups (group: the directions one
// workgroup carries; at most 2^31 - 1) fit.  0, or MBFIR_E_ARG with ctx->err set.
static int jvp_check(mbfir_ctx* ctx, const char* who, int npulse, int nscale, int ndir, long R, const long* npoint,
                     int group = jvp_group()) {
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (ndir < 1) return bad("ndir must be at least 1");
    long total = 0, nblk = 0;                                  // abr_batch_check has bounded both for one direction
    for (int p = 0; p < npulse; ++p) {
        total += npoint[p] * nscale;
        nblk += (npoint[p] + 255) / 256 * nscale;
    }
    const long ngrp = (ndir + (long)group - 1) / group;
    if (R > (1L << 56) / ndir || total > (1L << 56) / ndir || nblk > 2147483647L / ngrp) return bad("the output size or the workgroup count overflows");
    return 0;
}

int mbfir_abr_jvp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                        int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int ndir,
                        const double* v_re, const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im,
                        double* da_re, double* da_im, double* db_re, double* db_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool primal = (a_re && a_im && b_re && b_im) || (!a_re && !a_im && !b_re && !b_im);      // all four or none
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales && v_re && v_im && primal && da_re && da_im && db_re && db_im;
    if (const int e = abr_batch_check(ctx, "abr_jvp_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays, npoint))
        return e;
    if (const int e = jvp_check(ctx, "abr_jvp_batch", npulse, nscale, ndir, roff[npulse], npoint.data())) return e;
    MBFIR_TRY(ctx, abr_jvp_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales,
                                     mode, ndir, v_re, v_im, a_re, a_im, b_re, b_im, da_re, da_im, db_re, db_im));
}

int mbfir_abr2_jvp_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                         const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                         const double* y, int nscale, const double* scales, int mode, int ndir, const double* v_re,
                         const double* v_im, double* a_re, double* a_im, double* b_re, double* b_im, double* da_re, double* da_im,
                         double* db_re, double* db_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool primal = (a_re && a_im && b_re && b_im) || (!a_re && !a_im && !b_re && !b_im);
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales && v_re && v_im && primal && da_re && da_im &&
                        db_re && db_im;
    if (const int e = abr_batch_check(ctx, "abr2_jvp_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays,
                                      npoint))
        return e;
    if (const int e = jvp_check(ctx, "abr2_jvp_batch", npulse, nscale, ndir, roff[npulse], npoint.data())) return e;
    MBFIR_TRY(ctx, abr2_jvp_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid,
                                      yoff, y, nscale, scales, mode, ndir, v_re, v_im, a_re, a_im, b_re, b_im, da_re, da_im, db_re,
                                      db_im));
}

int mbfir_bloch_jvp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                          const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                          const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                          const double* m0x, const double* m0y, const double* m0z, int ndir, const double* v_re, const double* v_im,
                          const double* dm0x, const double* dm0y, const double* dm0z, double* mx, double* my, double* mz,
                          double* dmx, double* dmy, double* dmz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string("bloch_jvp_batch: ") + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, "bloch_jvp_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    if (!v_re || !v_im || !dmx || !dmy || !dmz) return bad("a direction or tangent plane is null");
    if ((m0x || m0y || m0z) && !(m0x && m0y && m0z)) return bad("m0x, m0y and m0z are given together or not at all");
    if ((dm0x || dm0y || dm0z) && !(dm0x && dm0y && dm0z)) return bad("dm0x, dm0y and dm0z are given together or not at all");
    if ((mx || my || mz) && !(mx && my && mz)) return bad("mx, my and mz are given together or not at all");
    if (const int e = jvp_check(ctx, "bloch_jvp_batch", npulse, nscale, ndir, toff[npulse], npoint.data(), bloch_jvp_group())) return e;
    MBFIR_TRY(ctx, bloch_jvp_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                       gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, ndir, v_re,
                                       v_im, dm0x, dm0y, dm0z, mx, my, mz, dmx, dmy, dmz));
}

// The steady state's derivatives (blochss.hip): mbfir_bloch_batch's checks at mode 1, then the call's own planes, then
// the counts of the adjoint (partials, checkpoints) or of the tangent (jvp_check, and one plane of (I - A)^-1 per workgroup).
int mbfir_bloch_ss_vjp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, const double* cmx, const double* cmy, const double* cmz, double* g_re, double* g_im,
                             double* mx, double* my, double* mz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string("bloch_ss_vjp_batch: ") + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, "bloch_ss_vjp_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 1,
                                        arrays, npoint))
        return e;
    if (!cmx || !cmy || !cmz || !g_re || !g_im) return bad("a cotangent or gradient plane is null");
    if ((mx || my || mz) && !(mx && my && mz)) return bad("mx, my and mz are given together or not at all");
    if (!vjp_partials_fit(npulse, nscale, toff, npoint.data()) || !bloch_checkpoints_fit(npulse, nscale, toff, npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_ss_vjp_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                          t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, cmx, cmy, cmz, g_re,
                                          g_im, mx, my, mz));
}

// The steady state's adjoint in b1, gr and df (blochssg.hip): mbfir_bloch_ss_vjp_batch's checks, the planes of dL / dgr
// and the counts of mbfir_bloch_vjp_gr_batch.
int mbfir_bloch_ss_vjp_gr_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const double* cmx, const double* cmy, const double* cmz,
                                double* g_re, double* g_im, double* mx, double* my, double* mz, double* ggx, double* ggy,
                                double* ggz, double* gdf) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string("bloch_ss_vjp_gr_batch: ") + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, "bloch_ss_vjp_gr_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        1, arrays, npoint))
        return e;
    if (!cmx || !cmy || !cmz || !g_re || !g_im) return bad("a cotangent or gradient plane is null");
    if (!ggx || !ggy || !ggz) return bad("a plane of the gradient waveform's gradient (ggx, ggy, ggz) is null");
    if ((mx || my || mz) && !(mx && my && mz)) return bad("mx, my and mz are given together or not at all");
    if (!bloch_gr_partials_fit(npulse, nscale, toff, npoint.data()) || !bloch_checkpoints_fit(npulse, nscale, toff, npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_ss_vjp_gr_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                             t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, cmx, cmy, cmz,
                                             g_re, g_im, mx, my, mz, ggx, ggy, ggz, gdf));
}

int mbfir_bloch_ss_jvp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                             int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                             const double* scales, int ndir, const double* v_re, const double* v_im, double* mx, double* my,
                             double* mz, double* dmx, double* dmy, double* dmz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string("bloch_ss_jvp_batch: ") + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, "bloch_ss_jvp_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 1,
                                        arrays, npoint))
        return e;
    if (!v_re || !v_im || !dmx || !dmy || !dmz) return bad("a direction or tangent plane is null");
    if ((mx || my || mz) && !(mx && my && mz)) return bad("mx, my and mz are given together or not at all");
    if (const int e = jvp_check(ctx, "bloch_ss_jvp_batch", npulse, nscale, ndir, toff[npulse], npoint.data(), bloch_ss_jvp_group()))
        return e;
    long nblk = 0;                                              // jvp_check has bounded it times the direction groups by 2^31 - 1
    for (int p = 0; p < npulse; ++p) nblk += (npoint[p] + 255) / 256 * nscale;
    if (nblk * ((ndir + (long)bloch_ss_jvp_group() - 1) / bloch_ss_jvp_group()) > (1L << 56) / 2304)
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_ss_jvp_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                          t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ndir, v_re, v_im, mx,
                                          my, mz, dmx, dmy, dmz));
}

int mbfir_test_bloch_ss_jvp_group(void) { return bloch_ss_jvp_group(); }

// The pulse train (blochtrain.hip).  What both calls check after bloch_batch_check: echo (per pulse) within [0, ntime],
// and that the propagators' planes (24 doubles per point and combination, ncomb[p] = nscale ngain_p combinations) and their
// workgroups fit.
static int bloch_prop_check(mbfir_ctx* ctx, const char* who, int npulse, const long* toff, const int* echo, const long* ncomb,
                            const long* npoint) {
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    for (int p = 0; p < npulse; ++p)
        if (echo[p] < 0 || echo[p] > toff[p + 1] - toff[p])
            return bad("echo of pulse " + std::to_string(p) + " must lie in [0, ntime]");
    long total = 0, nblk = 0;
    for (int p = 0; p < npulse; ++p) {
        long e, b;
        if (__builtin_mul_overflow(npoint[p], ncomb[p] * 24, &e) || __builtin_add_overflow(total, e, &total) ||
            __builtin_mul_overflow((npoint[p] + 255) / 256, ncomb[p], &b) || __builtin_add_overflow(nblk, b, &nblk))
            return bad("the output size or the workgroup count overflows");
    }
    if (total > (1L << 56) || nblk > 2147483647L) return bad("the output size or the workgroup count overflows");
    return 0;
}

// What the train and its adjoint check, in this order: bloch_batch_check, ntr, the offsets, the distinct gains, bloch_prop_check, the
// echo planes' size and the workgroups, the tables' values, meq and m0.  npoint and ncomb (npulse entries each) receive the points
// and the (scale, distinct gain) combinations per pulse.
static int bloch_train_check(mbfir_ctx* ctx, const char* who, int npulse, const long* toff, const long* tsoff, const double* t1,
                             const double* t2, int nfgrid, const long* foff, int npgrid, const long* poff, int nscale, bool arrays,
                             const int* ntr, const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                             const long* goff, const double* gains, const int* echo, const double* meq, const double* m0x,
                             const double* m0y, const double* m0z, std::vector<long>& npoint, std::vector<long>& ncomb) {
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0, arrays, npoint))
        return e;
    for (int p = 0; p < npulse; ++p)
        if (ntr[p] < 1) return bad("ntr of pulse " + std::to_string(p) + " must be at least 1");
    if (roff[0] != 0 || goff[0] != 0) return bad("inconsistent offsets: roff or goff does not start at 0");
    std::vector<long> ntout(npulse);
    ncomb.assign(npulse, 0);
    for (int p = 0; p < npulse; ++p) {
        if (roff[p + 1] - roff[p] != ntr[p])
            return bad("inconsistent offsets: roff of pulse " + std::to_string(p) + " does not span its ntr repetitions");
        const long G = goff[p + 1] - goff[p];
        if (G < 1 || G > ntr[p]) return bad("pulse " + std::to_string(p) + " needs between 1 and ntr distinct gains");
        ncomb[p] = G * nscale;
        ntout[p] = ntr[p];
    }
    if (const int e = bloch_prop_check(ctx, who, npulse, toff, echo, ncomb.data(), npoint.data())) return e;
    // the sizes before the tables are read: a table is as long as ntr says
    if (roff[npulse] > (1L << 56) || !sim_sizes(npulse, nscale, npoint.data(), ntout.data()))
        return bad("the output size or the workgroup count overflows");
    for (int p = 0; p < npulse; ++p)
        for (long k = roff[p]; k < roff[p + 1]; ++k)
            if (gidx[k] < 0 || gidx[k] >= goff[p + 1] - goff[p])
                return bad("a gain index of pulse " + std::to_string(p) + " lies outside [0, ngain)");
    for (long g = 0; g < goff[npulse]; ++g)
        if (!std::isfinite(gains[g])) return bad("a gain is not finite");
    for (long k = 0; k < roff[npulse]; ++k)
        if (!std::isfinite(cosphi[k]) || !std::isfinite(sinphi[k])) return bad("a cosine or sine of the phase table is not finite");
    for (int p = 0; p < npulse; ++p)
        if (!std::isfinite(meq[p])) return bad("meq of pulse " + std::to_string(p) + " is not finite");
    if ((m0x || m0y || m0z) && !(m0x && m0y && m0z)) return bad("m0x, m0y and m0z are given together or not at all");
    return 0;
}

int mbfir_bloch_train_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                            const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                            const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                            const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                            const int* ntr, const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                            const long* goff, const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                            const double* m0y, const double* m0z, double* ex, double* ey, double* ez, double* fx, double* fy,
                            double* fz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "bloch_train_batch: " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, "bloch_train_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint, ncomb))
        return e;
    if ((ex || ey || ez) && !(ex && ey && ez)) return bad("the echo planes are given together or not at all");
    if ((fx || fy || fz) && !(fx && fy && fz)) return bad("the final planes are given together or not at all");
    if (!ex && !fx) return bad("neither the echo planes nor the final planes are wanted");
    MBFIR_TRY(ctx, bloch_train_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                         t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff, cosphi,
                                         sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ex, ey, ez, fx, fy, fz));
}

// The train's adjoint (blochtrainvjp.hip) keeps one double2 partial per (combination, chunk of 64 points, sample), 3 x 256
// checkpoint doubles per (scale, chunk of 256 points, group of 8 repetitions) and per (combination, chunk of 64 points, group of 8
// samples), and launches one workgroup per (combination, chunk of 64 points): false when a count overflows, exceeds 2^56 or, for
// the workgroups, 2^31 - 1.
static bool bloch_train_vjp_fits(int npulse, int nscale, const long* toff, const int* ntr, const long* ncomb, const long* npoint) {
    long part = 0, ckr = 0, ckp = 0, nwg = 0;
    for (int p = 0; p < npulse; ++p) {
        const long n = toff[p + 1] - toff[p], nch = (npoint[p] + 255) / 256, nch64 = (npoint[p] + 63) / 64;
        long w, a, b, c;
        if (__builtin_mul_overflow(ncomb[p], nch64, &w) || __builtin_add_overflow(nwg, w, &nwg) ||
            __builtin_mul_overflow(w, n, &a) || __builtin_add_overflow(part, a, &part) ||
            __builtin_mul_overflow(w, (n + 7) / 8 * 768, &b) || __builtin_add_overflow(ckp, b, &ckp) ||
            __builtin_mul_overflow(nch * nscale, ((long)ntr[p] + 7) / 8 * 768, &c) || __builtin_add_overflow(ckr, c, &ckr))
            return false;
    }
    return part <= (1L << 56) && ckr <= (1L << 56) && ckp <= (1L << 56) && nwg <= 2147483647L;
}

int mbfir_bloch_train_vjp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                const double* cex, const double* cey, const double* cez, const double* cfx, const double* cfy,
                                const double* cfz, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "bloch_train_vjp_batch: " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, "bloch_train_vjp_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint, ncomb))
        return e;
    if ((cex || cey || cez) && !(cex && cey && cez)) return bad("the echo cotangents are given together or not at all");
    if ((cfx || cfy || cfz) && !(cfx && cfy && cfz)) return bad("the final cotangents are given together or not at all");
    if (!cex && !cfx) return bad("neither echo cotangents nor final cotangents are given");
    if (!g_re || !g_im) return bad("a gradient plane is null");
    if ((gmx || gmy || gmz) && !(gmx && gmy && gmz)) return bad("gmx, gmy and gmz are given together or not at all");
    if (!bloch_train_vjp_fits(npulse, nscale, toff, ntr, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_train_vjp_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                             t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff,
                                             cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, cex, cey, cez, cfx,
                                             cfy, cfz, g_re, g_im, gmx, gmy, gmz));
}

// The train's adjoint in b1, gr and df (blochtrainvjpg.hip) keeps five doubles per (combination, chunk of 64 points,
// sample), the rf pair and the three g components, and one double per (combination, point) for dL / d df: false when a count
// overflows or exceeds 2^54 (the partials) or 2^56 (the workspace).
static bool bloch_train_gr_fits(int npulse, const long* toff, const long* ncomb, const long* npoint) {
    long part = 0, dfw = 0;
    for (int p = 0; p < npulse; ++p) {
        long w, a, d;
        if (__builtin_mul_overflow(ncomb[p], (npoint[p] + 63) / 64, &w) || __builtin_mul_overflow(w, toff[p + 1] - toff[p], &a) ||
            __builtin_add_overflow(part, a, &part) || __builtin_mul_overflow(ncomb[p], npoint[p], &d) ||
            __builtin_add_overflow(dfw, d, &dfw))
            return false;
    }
    return part <= (1L << 54) && dfw <= (1L << 56);
}

int mbfir_bloch_train_vjp_gr_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                   const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                   const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                   const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                   int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                   const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                   const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                   const double* cex, const double* cey, const double* cez, const double* cfx, const double* cfy,
                                   const double* cfz, double* g_re, double* g_im, double* gmx, double* gmy, double* gmz, double* ggx,
                                   double* ggy, double* ggz, double* gdf) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "bloch_train_vjp_gr_batch: " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, "bloch_train_vjp_gr_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff,
                                        nscale, arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint,
                                        ncomb))
        return e;
    if ((cex || cey || cez) && !(cex && cey && cez)) return bad("the echo cotangents are given together or not at all");
    if ((cfx || cfy || cfz) && !(cfx && cfy && cfz)) return bad("the final cotangents are given together or not at all");
    if (!cex && !cfx) return bad("neither echo cotangents nor final cotangents are given");
    if (!g_re || !g_im) return bad("a gradient plane is null");
    if ((gmx || gmy || gmz) && !(gmx && gmy && gmz)) return bad("gmx, gmy and gmz are given together or not at all");
    if (!ggx || !ggy || !ggz) return bad("a plane of the gradient waveform's gradient (ggx, ggy, ggz) is null");
    if (!bloch_train_vjp_fits(npulse, nscale, toff, ntr, ncomb.data(), npoint.data()) ||
        !bloch_train_gr_fits(npulse, toff, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_train_vjp_gr_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr,
                                                roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, cex, cey, cez,
                                                cfx, cfy, cfz, g_re, g_im, gmx, gmy, gmz, ggx, ggy, ggz, gdf));
}

// The train's adjoint in its schedule (blochtrainsched.hip) keeps one double2 partial per (scale, chunk of 256 points,
// repetition), 3 x 256 checkpoint doubles per (scale, chunk of 256 points, group of 8 repetitions) and the propagators' planes
// twice (bloch_prop_check has bounded them once), and launches one workgroup per (combination, chunk of 64 points): false when a
// count overflows, exceeds 2^56 or, for the workgroups, 2^31 - 1.
static bool bloch_train_sched_fits(int npulse, int nscale, const int* ntr, const long* ncomb, const long* npoint) {
    long part = 0, ckr = 0, nwg = 0, ws = 0;
    for (int p = 0; p < npulse; ++p) {
        const long nch = (npoint[p] + 255) / 256, nch64 = (npoint[p] + 63) / 64;
        long w, a, c, e;
        if (__builtin_mul_overflow(ncomb[p], nch64, &w) || __builtin_add_overflow(nwg, w, &nwg) ||
            __builtin_mul_overflow(nch * nscale, (long)ntr[p], &a) || __builtin_add_overflow(part, a, &part) ||
            __builtin_mul_overflow(nch * nscale, ((long)ntr[p] + 7) / 8 * 768, &c) || __builtin_add_overflow(ckr, c, &ckr) ||
            __builtin_mul_overflow(npoint[p], ncomb[p] * 48, &e) || __builtin_add_overflow(ws, e, &ws))
            return false;
    }
    return part <= (1L << 56) && ckr <= (1L << 56) && ws <= (1L << 56) && nwg <= 2147483647L;
}

int mbfir_bloch_train_vjp_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                      const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                      const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                      const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                      const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                      const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                      const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                      const double* m0y, const double* m0z, const double* cex, const double* cey, const double* cez,
                                      const double* cfx, const double* cfy, const double* cfz, double* ggain, double* gphi,
                                      double* gmx, double* gmy, double* gmz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "bloch_train_vjp_sched_batch: " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, "bloch_train_vjp_sched_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff,
                                        nscale, arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint,
                                        ncomb))
        return e;
    if ((cex || cey || cez) && !(cex && cey && cez)) return bad("the echo cotangents are given together or not at all");
    if ((cfx || cfy || cfz) && !(cfx && cfy && cfz)) return bad("the final cotangents are given together or not at all");
    if (!cex && !cfx) return bad("neither echo cotangents nor final cotangents are given");
    if (!ggain && !gphi) return bad("neither the gradient in the gains nor the gradient in the phases is wanted");
    if ((gmx || gmy || gmz) && !(gmx && gmy && gmz)) return bad("gmx, gmy and gmz are given together or not at all");
    if (!bloch_train_sched_fits(npulse, nscale, ntr, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_train_vjp_sched_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                   tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales,
                                                   ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, cex,
                                                   cey, cez, cfx, cfy, cfz, ggain, gphi, gmx, gmy, gmz));
}

// The train's tangent (blochtrainjvp.hip) reads ndir directions of the samples, writes ndir tangents of the echoes and of
// the final state, keeps ndir x 24 doubles per (combination, point) and launches one workgroup per (combination, chunk of 64 points,
// group of bloch_train_jvp_group(0) directions) and per (scale, chunk of 256 points, group of bloch_train_jvp_group(1)): false when
// a count overflows, exceeds 2^56 or, for the workgroups, 2^31 - 1.
static bool bloch_train_jvp_fits(int npulse, int nscale, int ndir, const long* toff, const int* ntr, const long* ncomb,
                                 const long* npoint) {
    const long ngp = (ndir + (long)bloch_train_jvp_group(0) - 1) / bloch_train_jvp_group(0);
    const long ngr = (ndir + (long)bloch_train_jvp_group(1) - 1) / bloch_train_jvp_group(1);
    long ech = 0, fin = 0, wsp = 0, wgp = 0, wgr = 0;
    for (int p = 0; p < npulse; ++p) {
        long e, f, w, a, b;
        if (__builtin_mul_overflow(npoint[p] * nscale, (long)ntr[p], &e) || __builtin_mul_overflow(e, (long)ndir, &e) ||
            __builtin_add_overflow(ech, e, &ech) || __builtin_mul_overflow(npoint[p] * nscale, (long)ndir, &f) ||
            __builtin_add_overflow(fin, f, &fin) || __builtin_mul_overflow(npoint[p], ncomb[p] * 24, &w) ||
            __builtin_mul_overflow(w, (long)ndir, &w) || __builtin_add_overflow(wsp, w, &wsp) ||
            __builtin_mul_overflow((npoint[p] + 63) / 64, ncomb[p], &a) || __builtin_mul_overflow(a, ngp, &a) ||
            __builtin_add_overflow(wgp, a, &wgp) || __builtin_mul_overflow((npoint[p] + 255) / 256 * nscale, ngr, &b) ||
            __builtin_add_overflow(wgr, b, &wgr))
            return false;
    }
    return toff[npulse] <= (1L << 56) / ndir && ech <= (1L << 56) && fin <= (1L << 56) && wsp <= (1L << 56) &&
           wgp <= 2147483647L && wgr <= 2147483647L;
}

int mbfir_bloch_train_jvp_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                                const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z, int ndir,
                                const double* v_re, const double* v_im, const double* dm0x, const double* dm0y, const double* dm0z,
                                double* ex, double* ey, double* ez, double* fx, double* fy, double* fz, double* dex, double* dey,
                                double* dez, double* dfx, double* dfy, double* dfz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "bloch_train_jvp_batch: " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, "bloch_train_jvp_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint, ncomb))
        return e;
    if (!v_re || !v_im) return bad("a direction plane is null");
    if ((dm0x || dm0y || dm0z) && !(dm0x && dm0y && dm0z)) return bad("dm0x, dm0y and dm0z are given together or not at all");
    if ((ex || ey || ez) && !(ex && ey && ez)) return bad("the echo planes are given together or not at all");
    if ((fx || fy || fz) && !(fx && fy && fz)) return bad("the final planes are given together or not at all");
    if ((dex || dey || dez) && !(dex && dey && dez)) return bad("the tangent echo planes are given together or not at all");
    if ((dfx || dfy || dfz) && !(dfx && dfy && dfz)) return bad("the tangent final planes are given together or not at all");
    if (!dex && !dfx) return bad("neither the tangent echo planes nor the tangent final planes are wanted");
    if (ndir < 1) return bad("ndir must be at least 1");
    if (!bloch_train_jvp_fits(npulse, nscale, ndir, toff, ntr, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_train_jvp_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                             t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff,
                                             cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ndir, v_re, v_im,
                                             dm0x, dm0y, dm0z, ex, ey, ez, fx, fy, fz, dex, dey, dez, dfx, dfy, dfz));
}

int mbfir_test_bloch_train_jvp_group(int which) { return bloch_train_jvp_group(which); }

// The train's tangent in its schedule (blochtrainschedjvp.hip) reads ndir directions of the repetitions, writes ndir
// tangents of the echoes and of the final state, keeps the propagators' planes twice whatever ndir is (bloch_prop_check has bounded
// them once) and launches one workgroup per (combination, chunk of 64 points) and per (scale, chunk of 256 points, group of
// bloch_train_sched_jvp_group() directions): false when a count overflows, exceeds 2^56 or, for the workgroups, 2^31 - 1.
static bool bloch_train_sched_jvp_fits(int npulse, int nscale, int ndir, const int* ntr, const long* roff, const long* ncomb,
                                       const long* npoint) {
    const long ngr = (ndir + (long)bloch_train_sched_jvp_group() - 1) / bloch_train_sched_jvp_group();
    long ech = 0, fin = 0, wsp = 0, wgp = 0, wgr = 0;
    for (int p = 0; p < npulse; ++p) {
        long e, f, w, a, b;
        if (__builtin_mul_overflow(npoint[p] * nscale, (long)ntr[p], &e) || __builtin_mul_overflow(e, (long)ndir, &e) ||
            __builtin_add_overflow(ech, e, &ech) || __builtin_mul_overflow(npoint[p] * nscale, (long)ndir, &f) ||
            __builtin_add_overflow(fin, f, &fin) || __builtin_mul_overflow(npoint[p], ncomb[p] * 48, &w) ||
            __builtin_add_overflow(wsp, w, &wsp) || __builtin_mul_overflow((npoint[p] + 63) / 64, ncomb[p], &a) ||
            __builtin_add_overflow(wgp, a, &wgp) || __builtin_mul_overflow((npoint[p] + 255) / 256 * nscale, ngr, &b) ||
            __builtin_add_overflow(wgr, b, &wgr))
            return false;
    }
    return roff[npulse] <= (1L << 56) / ndir && ech <= (1L << 56) && fin <= (1L << 56) && wsp <= (1L << 56) &&
           wgp <= 2147483647L && wgr <= 2147483647L;
}

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
                                      double* dfy, double* dfz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = "bloch_train_jvp_sched_batch: " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, "bloch_train_jvp_sched_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff,
                                        nscale, arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint,
                                        ncomb))
        return e;
    if ((dm0x || dm0y || dm0z) && !(dm0x && dm0y && dm0z)) return bad("dm0x, dm0y and dm0z are given together or not at all");
    if ((ex || ey || ez) && !(ex && ey && ez)) return bad("the echo planes are given together or not at all");
    if ((fx || fy || fz) && !(fx && fy && fz)) return bad("the final planes are given together or not at all");
    if ((dex || dey || dez) && !(dex && dey && dez)) return bad("the tangent echo planes are given together or not at all");
    if ((dfx || dfy || dfz) && !(dfx && dfy && dfz)) return bad("the tangent final planes are given together or not at all");
    if (!dgain && !dphi && !dm0x) return bad("no direction is given: dgain, dphi and the m0 directions are all null");
    if (!dex && !dfx) return bad("neither the tangent echo planes nor the tangent final planes are wanted");
    if (ndir < 1) return bad("ndir must be at least 1");
    if (!bloch_train_sched_jvp_fits(npulse, nscale, ndir, ntr, roff, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_train_jvp_sched_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                   tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales,
                                                   ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ndir,
                                                   dgain, dphi, dm0x, dm0y, dm0z, ex, ey, ez, fx, fy, fz, dex, dey, dez, dfx, dfy,
                                                   dfz));
}

int mbfir_test_bloch_train_sched_jvp_group() { return bloch_train_sched_jvp_group(); }

// The six train calls below (lsq, gn and the device step, in b1 and in the schedule) have magnitude twins (mbfir_bloch_train_*_mag_batch,
// DESIGN 8ai) that take pairs (xy, z) where they take triples: each pair of twins is one body, `mag` telling which; with it a pair lies
// in the first two entries of its triple, the third is null and is not asked for, and every check, its place and its message are
// the same.
// The train's fused products (blochtraingn.hip).  What both calls check after bloch_train_check, in this order: ebcast,
// the echo and final planes given whole or not at all and not both absent, the outputs, then (bloch_train_gn_check) the sizes, before
// any plane is read: the adjoint's partials, checkpoints and workgroups (bloch_train_vjp_fits) and, per direction, the planes' tangents and
// cotangents, the partials, the run's checkpoints (two states) and the workgroups: MBFIR_E_ARG when a count overflows, exceeds 2^56
// or, for the workgroups, 2^31 - 1; last the weights and rw, non-negative and finite.
static int bloch_train_gn_check(mbfir_ctx* ctx, const char* who, int npulse, int nscale, int ndir, const long* toff, const int* ntr,
                                const long* roff, const long* ncomb, const long* npoint, int ebcast, const double* const w[3],
                                const double* rw, const double* const wf[3]) {
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    long E = 0, O = 0;
    for (int p = 0; p < npulse; ++p) {
        E += npoint[p] * nscale * ntr[p];                                 // bloch_train_check has bounded both
        O += npoint[p] * nscale;
    }
    auto neg = [](const double* v, long n) {
        for (long i = 0; i < n; ++i)
            if (!(v[i] >= 0) || !std::isfinite(v[i])) return true;
        return false;
    };
    if (!bloch_train_vjp_fits(npulse, nscale, toff, ntr, ncomb, npoint)) return bad("the output size or the workgroup count overflows");
    long wsp = 0, part = 0, ckr = 0, wgr = 0, wgf = 0;
    for (int p = 0; p < npulse; ++p) {
        const long n = toff[p + 1] - toff[p], nch = (npoint[p] + 255) / 256, nch64 = (npoint[p] + 63) / 64;
        long a, b, c, d, f;
        if (__builtin_mul_overflow(npoint[p], ncomb[p] * 24, &a) || __builtin_mul_overflow(a, (long)ndir, &a) ||
            __builtin_add_overflow(wsp, a, &wsp) || __builtin_mul_overflow(ncomb[p] * nch64, n, &b) ||
            __builtin_mul_overflow(b, (long)ndir, &b) || __builtin_add_overflow(part, b, &part) ||
            __builtin_mul_overflow(nch * nscale, ((long)ntr[p] + 7) / 8 * 1536, &c) || __builtin_mul_overflow(c, (long)ndir, &c) ||
            __builtin_add_overflow(ckr, c, &ckr) || __builtin_mul_overflow(nch * nscale, (long)ndir, &d) ||
            __builtin_add_overflow(wgr, d, &wgr) || __builtin_mul_overflow((n + 255) / 256, (long)ndir, &f) ||
            __builtin_add_overflow(wgf, f, &wgf))
            return bad("the output size or the workgroup count overflows");
    }
    if (toff[npulse] > (1L << 56) / ndir || wsp > (1L << 56) || part > (1L << 56) || ckr > (1L << 56) || wgr > 2147483647L ||
        wgf > 2147483647L)
        return bad("the output size or the workgroup count overflows");
    for (int c = 0; c < 3; ++c)                                           // the magnitude calls have two planes: their third is null
        if ((w[0] && w[c] && neg(w[c], ebcast ? O : E)) || (wf[0] && wf[c] && neg(wf[c], O)))
            return bad("a weight is negative or not finite");
    if (rw && neg(rw, roff[npulse])) return bad("a repetition weight is negative or not finite");
    return 0;
}

static int bloch_train_lsq_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff,
                                      const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                                      const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                                      const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                                      int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                      int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                      const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                      const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                      const double* m0z, int ebcast, const double* wx, const double* wy, const double* wz,
                                      const double* tx, const double* ty, const double* tz, const double* rw, const double* wfx,
                                      const double* wfy, const double* wfz, const double* tfx, const double* tfy,
                                      const double* tfz, double* loss, double* g_re, double* g_im, double* gmx, double* gmy,
                                      double* gmz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint, ncomb))
        return e;
    if (ebcast != 0 && ebcast != 1) return bad("ebcast must be 0 or 1");
    const bool any_e = wx || wy || wz || tx || ty || tz, all_e = wx && wy && (mag || wz) && tx && ty && (mag || tz);
    const bool any_f = wfx || wfy || wfz || tfx || tfy || tfz, all_f = wfx && wfy && (mag || wfz) && tfx && tfy && (mag || tfz);
    if (any_e && !all_e) return bad("the echo weights and targets are given together or not at all");
    if (any_f && !all_f) return bad("the final weights and targets are given together or not at all");
    if (!any_e && !any_f) return bad("neither an echo term nor a final term is given");
    if (!loss || !g_re || !g_im) return bad("a loss or gradient plane is null");
    if ((gmx || gmy || gmz) && !(gmx && gmy && gmz)) return bad("gmx, gmy and gmz are given together or not at all");
    const double* const w[3] = {wx, wy, wz};
    const double* const t[3] = {tx, ty, tz};
    const double* const wf[3] = {wfx, wfy, wfz};
    const double* const tf[3] = {tfx, tfy, tfz};
    if (const int e = bloch_train_gn_check(ctx, who, npulse, nscale, 1, toff, ntr, roff, ncomb.data(),
                                           npoint.data(), ebcast, w, rw, wf))
        return e;
    MBFIR_TRY(ctx, bloch_train_lsq_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                             t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff,
                                             cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, w, t, rw, wf,
                                             tf, loss, g_re, g_im, gmx, gmy, gmz, mag));
}
int mbfir_bloch_train_lsq_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                                const double* wz, const double* tx, const double* ty, const double* tz, const double* rw,
                                const double* wfx, const double* wfy, const double* wfz, const double* tfx, const double* tfy,
                                const double* tfz, double* loss, double* g_re, double* g_im, double* gmx, double* gmy,
                                double* gmz) {
    return bloch_train_lsq_batch_call(ctx, "bloch_train_lsq_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                      t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff,
                                      cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, wx, wy, wz, tx,
                                      ty, tz, rw, wfx, wfy, wfz, tfx, tfy, tfz, loss, g_re, g_im, gmx, gmy, gmz);
}
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
                                    double* g_im, double* gmx, double* gmy, double* gmz) {
    return bloch_train_lsq_batch_call(ctx, "bloch_train_lsq_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                      tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr,
                                      roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, wxy, wz,
                                      nullptr, txy, tz, nullptr, rw, wfxy, wfz, nullptr, tfxy, tfz, nullptr, loss, g_re, g_im,
                                      gmx, gmy, gmz);
}

static int bloch_train_gn_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff,
                                     const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                                     const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                                     const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                                     int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                     int nscale, const double* scales, const int* ntr, const long* roff, const double* cosphi,
                                     const double* sinphi, const int* gidx, const long* goff, const double* gains,
                                     const int* echo, const double* meq, int demod, const double* m0x, const double* m0y,
                                     const double* m0z, int ebcast, const double* wx, const double* wy, const double* wz,
                                     const double* rw, const double* wfx, const double* wfy, const double* wfz, int ndir,
                                     const double* v_re, const double* v_im, double* h_re, double* h_im) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint, ncomb))
        return e;
    if (ebcast != 0 && ebcast != 1) return bad("ebcast must be 0 or 1");
    const bool any_e = wx || wy || wz, any_f = wfx || wfy || wfz;
    if (any_e && !(wx && wy && (mag || wz))) return bad("the echo weights are given together or not at all");
    if (any_f && !(wfx && wfy && (mag || wfz))) return bad("the final weights are given together or not at all");
    if (!any_e && !any_f) return bad("neither an echo term nor a final term is given");
    if (!v_re || !v_im || !h_re || !h_im) return bad("a direction or product plane is null");
    if (ndir < 1) return bad("ndir must be at least 1");
    const double* const w[3] = {wx, wy, wz};
    const double* const wf[3] = {wfx, wfy, wfz};
    if (const int e = bloch_train_gn_check(ctx, who, npulse, nscale, ndir, toff, ntr, roff, ncomb.data(),
                                           npoint.data(), ebcast, w, rw, wf))
        return e;
    if (!bloch_train_jvp_fits(npulse, nscale, ndir, toff, ntr, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_train_gn_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                            t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff,
                                            cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, w, rw, wf, ndir,
                                            v_re, v_im, h_re, h_im, mag));
}
int mbfir_bloch_train_gn_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                               const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                               const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                               const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                               const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                               const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                               const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                               const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                               const double* wz, const double* rw, const double* wfx, const double* wfy, const double* wfz,
                               int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im) {
    return bloch_train_gn_batch_call(ctx, "bloch_train_gn_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                     t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr, roff,
                                     cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, wx, wy, wz, rw,
                                     wfx, wfy, wfz, ndir, v_re, v_im, h_re, h_im);
}
int mbfir_bloch_train_gn_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                   const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                   const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                   const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                   const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                   const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                   const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                   const double* m0y, const double* m0z, int ebcast, const double* wxy, const double* wz,
                                   const double* rw, const double* wfxy, const double* wfz, int ndir, const double* v_re,
                                   const double* v_im, double* h_re, double* h_im) {
    return bloch_train_gn_batch_call(ctx, "bloch_train_gn_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                     tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr,
                                     roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, wxy, wz,
                                     nullptr, rw, wfxy, wfz, nullptr, ndir, v_re, v_im, h_re, h_im);
}

// The fused products of the train's schedule (blochtrainschedgn.hip).  What both calls check after bloch_train_check, in
// this order: ebcast, the echo and final planes given whole or not at all and not both absent, the outputs, the directions and ndir,
// then (bloch_train_sched_gn_check) the sizes, before any plane is read: the propagators' planes twice (bloch_prop_check has bounded
// them once) and, times the directions, one double2 partial per (scale, chunk of 256 points, repetition), 3 x 256 checkpoint doubles
// per state (one for lsq, two for gn) and (scale, chunk of 256 points, group of 8 repetitions), the workgroups of the run and of
// the fold, and the directions' entries: MBFIR_E_ARG when a count overflows, exceeds 2^56 or, for the workgroups, 2^31 - 1; last
// the weights and rw, non-negative and finite.
static int bloch_train_sched_gn_check(mbfir_ctx* ctx, const char* who, int npulse, int nscale, int ndir, int states, const int* ntr,
                                      const long* roff, const long* ncomb, const long* npoint, int ebcast, const double* const w[3],
                                      const double* rw, const double* const wf[3]) {
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    long E = 0, O = 0;
    for (int p = 0; p < npulse; ++p) {
        E += npoint[p] * nscale * ntr[p];                                 // bloch_train_check has bounded both
        O += npoint[p] * nscale;
    }
    auto neg = [](const double* v, long n) {
        for (long i = 0; i < n; ++i)
            if (!(v[i] >= 0) || !std::isfinite(v[i])) return true;
        return false;
    };
    long wsp = 0, part = 0, ckr = 0, wgp = 0, wgr = 0, wgf = 0;
    for (int p = 0; p < npulse; ++p) {
        const long nch = (npoint[p] + 255) / 256, nch64 = (npoint[p] + 63) / 64;
        long a, b, c, d, e, f;
        if (__builtin_mul_overflow(npoint[p], ncomb[p] * 48, &a) || __builtin_add_overflow(wsp, a, &wsp) ||
            __builtin_mul_overflow(nch * nscale, (long)ntr[p], &b) || __builtin_mul_overflow(b, (long)ndir, &b) ||
            __builtin_add_overflow(part, b, &part) ||
            __builtin_mul_overflow(nch * nscale, ((long)ntr[p] + 7) / 8 * 768 * states, &c) ||
            __builtin_mul_overflow(c, (long)ndir, &c) || __builtin_add_overflow(ckr, c, &ckr) ||
            __builtin_mul_overflow(ncomb[p], nch64, &d) || __builtin_add_overflow(wgp, d, &wgp) ||
            __builtin_mul_overflow(nch * nscale, (long)ndir, &e) || __builtin_add_overflow(wgr, e, &wgr) ||
            __builtin_mul_overflow(((long)ntr[p] + 255) / 256, (long)ndir, &f) || __builtin_add_overflow(wgf, f, &wgf))
            return bad("the output size or the workgroup count overflows");
    }
    if (roff[npulse] > (1L << 56) / ndir || wsp > (1L << 56) || part > (1L << 56) || ckr > (1L << 56) || wgp > 2147483647L ||
        wgr > 2147483647L || wgf > 2147483647L)
        return bad("the output size or the workgroup count overflows");
    for (int c = 0; c < 3; ++c)                                           // the magnitude calls have two planes: their third is null
        if ((w[0] && w[c] && neg(w[c], ebcast ? O : E)) || (wf[0] && wf[c] && neg(wf[c], O)))
            return bad("a weight is negative or not finite");
    if (rw && neg(rw, roff[npulse])) return bad("a repetition weight is negative or not finite");
    return 0;
}

static int bloch_train_lsq_sched_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff,
                                            const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                                            const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                                            const double* t2, const double* gamma, int nfgrid, const long* foff,
                                            const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                            const double* dz, int nscale, const double* scales, const int* ntr, const long* roff,
                                            const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                            const double* gains, const int* echo, const double* meq, int demod,
                                            const double* m0x, const double* m0y, const double* m0z, int ebcast,
                                            const double* wx, const double* wy, const double* wz, const double* tx,
                                            const double* ty, const double* tz, const double* rw, const double* wfx,
                                            const double* wfy, const double* wfz, const double* tfx, const double* tfy,
                                            const double* tfz, double* loss, double* ggain, double* gphi, double* gmx,
                                            double* gmy, double* gmz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff,
                                        nscale, arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint,
                                        ncomb))
        return e;
    if (ebcast != 0 && ebcast != 1) return bad("ebcast must be 0 or 1");
    const bool any_e = wx || wy || wz || tx || ty || tz, all_e = wx && wy && (mag || wz) && tx && ty && (mag || tz);
    const bool any_f = wfx || wfy || wfz || tfx || tfy || tfz, all_f = wfx && wfy && (mag || wfz) && tfx && tfy && (mag || tfz);
    if (any_e && !all_e) return bad("the echo weights and targets are given together or not at all");
    if (any_f && !all_f) return bad("the final weights and targets are given together or not at all");
    if (!any_e && !any_f) return bad("neither an echo term nor a final term is given");
    if (!loss) return bad("the loss plane is null");
    if (!ggain && !gphi) return bad("neither the gradient in the gains nor the gradient in the phases is wanted");
    if ((gmx || gmy || gmz) && !(gmx && gmy && gmz)) return bad("gmx, gmy and gmz are given together or not at all");
    const double* const w[3] = {wx, wy, wz};
    const double* const t[3] = {tx, ty, tz};
    const double* const wf[3] = {wfx, wfy, wfz};
    const double* const tf[3] = {tfx, tfy, tfz};
    if (const int e = bloch_train_sched_gn_check(ctx, who, npulse, nscale, 1, 1, ntr, roff, ncomb.data(),
                                                 npoint.data(), ebcast, w, rw, wf))
        return e;
    MBFIR_TRY(ctx, bloch_train_lsq_sched_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                   tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales,
                                                   ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z,
                                                   ebcast, w, t, rw, wf, tf, loss, ggain, gphi, gmx, gmy, gmz, mag));
}
int mbfir_bloch_train_lsq_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                      const double* gx, const double* gy, const double* gz, const long* tsoff,
                                      const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                      const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                      const double* dy, const double* dz, int nscale, const double* scales, const int* ntr,
                                      const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                                      const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                                      const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wx,
                                      const double* wy, const double* wz, const double* tx, const double* ty, const double* tz,
                                      const double* rw, const double* wfx, const double* wfy, const double* wfz,
                                      const double* tfx, const double* tfy, const double* tfz, double* loss, double* ggain,
                                      double* gphi, double* gmx, double* gmy, double* gmz) {
    return bloch_train_lsq_sched_batch_call(ctx, "bloch_train_lsq_sched_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz,
                                            tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale,
                                            scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y,
                                            m0z, ebcast, wx, wy, wz, tx, ty, tz, rw, wfx, wfy, wfz, tfx, tfy, tfz, loss, ggain,
                                            gphi, gmx, gmy, gmz);
}
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
                                          double* gmz) {
    return bloch_train_lsq_sched_batch_call(ctx, "bloch_train_lsq_sched_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz,
                                            tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale,
                                            scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y,
                                            m0z, ebcast, wxy, wz, nullptr, txy, tz, nullptr, rw, wfxy, wfz, nullptr, tfxy, tfz,
                                            nullptr, loss, ggain, gphi, gmx, gmy, gmz);
}

static int bloch_train_gn_sched_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff,
                                           const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                                           const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                                           const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                                           int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                           int nscale, const double* scales, const int* ntr, const long* roff,
                                           const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                           const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                           const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                                           const double* wz, const double* rw, const double* wfx, const double* wfy,
                                           const double* wfz, int ndir, const double* dgain, const double* dphi, double* hgain,
                                           double* hphi) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff,
                                        nscale, arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint,
                                        ncomb))
        return e;
    if (ebcast != 0 && ebcast != 1) return bad("ebcast must be 0 or 1");
    const bool any_e = wx || wy || wz, any_f = wfx || wfy || wfz;
    if (any_e && !(wx && wy && (mag || wz))) return bad("the echo weights are given together or not at all");
    if (any_f && !(wfx && wfy && (mag || wfz))) return bad("the final weights are given together or not at all");
    if (!any_e && !any_f) return bad("neither an echo term nor a final term is given");
    if (!hgain && !hphi) return bad("neither the product's gains half nor its phases half is wanted");
    if (!dgain && !dphi) return bad("no direction is given: dgain and dphi are both null");
    if (ndir < 1) return bad("ndir must be at least 1");
    const double* const w[3] = {wx, wy, wz};
    const double* const wf[3] = {wfx, wfy, wfz};
    if (const int e = bloch_train_sched_gn_check(ctx, who, npulse, nscale, ndir, 2, ntr, roff, ncomb.data(),
                                                 npoint.data(), ebcast, w, rw, wf))
        return e;
    MBFIR_TRY(ctx, bloch_train_gn_sched_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                  tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales,
                                                  ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast,
                                                  w, rw, wf, ndir, dgain, dphi, hgain, hphi, mag));
}
int mbfir_bloch_train_gn_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff,
                                     const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                     const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                     const double* dy, const double* dz, int nscale, const double* scales, const int* ntr,
                                     const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                                     const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                                     const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wx,
                                     const double* wy, const double* wz, const double* rw, const double* wfx, const double* wfy,
                                     const double* wfz, int ndir, const double* dgain, const double* dphi, double* hgain,
                                     double* hphi) {
    return bloch_train_gn_sched_batch_call(ctx, "bloch_train_gn_sched_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz,
                                           tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale,
                                           scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z,
                                           ebcast, wx, wy, wz, rw, wfx, wfy, wfz, ndir, dgain, dphi, hgain, hphi);
}
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
                                         double* hphi) {
    return bloch_train_gn_sched_batch_call(ctx, "bloch_train_gn_sched_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz,
                                           tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale,
                                           scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z,
                                           ebcast, wxy, wz, nullptr, rw, wfxy, wfz, nullptr, ndir, dgain, dphi, hgain, hphi);
}

int mbfir_bloch_prop_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                           const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                           const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                           const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                           const int* echo, double* a, double* b, double* ae, double* be) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && echo && a &&
                        b && ae && be;
    if (const int e = bloch_batch_check(ctx, "bloch_prop_batch", npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    std::vector<long> ncomb(npulse, nscale);
    if (const int e = bloch_prop_check(ctx, "bloch_prop_batch", npulse, toff, echo, ncomb.data(), npoint.data())) return e;
    MBFIR_TRY(ctx, bloch_prop_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                        t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, echo, a, b, ae, be));
}

// What the Bloch least-squares calls check after bloch_batch_check, in this order: their own planes (what: the message of a null
// one), m0, the 3 O weights (O: the forward call's output entries), ndir, and that ndir times the T b1 samples, the partials (one per
// workgroup and sample, per direction) and the checkpoints (at most 2^56 entries each) and the workgroups of the sweep and of the
// fold (at most 2^31 - 1 each) fit.  0, or MBFIR_E_ARG with ctx->err set.
// The six calls below have magnitude twins (mbfir_bloch_*_mag_batch) that take pairs (xy, z) where they take triples:
// each pair of twins is one body, `mag` telling which; with it the pair lies in (wx, wy) and (tx, ty), wz and tz are null and are
// not asked for, and every check, its place and its message are the same.
static int bloch_gn_check(mbfir_ctx* ctx, const char* who, bool planes, const char* what, const double* m0x, const double* m0y,
                          const double* m0z, int npulse, int nscale, const double* wx, const double* wy, const double* wz, int ndir,
                          const long* toff, const long* npoint) {
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (!planes) return bad(what);
    if ((m0x || m0y || m0z) && !(m0x && m0y && m0z)) return bad("m0x, m0y and m0z are given together or not at all");
    long O = 0, nblk = 0, nfold = 0;                           // bloch_batch_check has bounded O and nblk
    for (int p = 0; p < npulse; ++p) {
        O += npoint[p] * nscale;
        nblk += (npoint[p] + 255) / 256 * nscale;
        nfold += (toff[p + 1] - toff[p] + 255) / 256;
    }
    for (const double* w : {wx, wy, wz})                       // the magnitude calls have two planes: their wz is null
        for (long i = 0; w && i < O; ++i)
            if (!(w[i] >= 0) || !std::isfinite(w[i])) return bad("a weight is negative or not finite");
    if (ndir < 1) return bad("ndir must be at least 1");
    if (!vjp_partials_fit(npulse, nscale, toff, npoint) || !bloch_checkpoints_fit(npulse, nscale, toff, npoint))
        return bad("the output size or the workgroup count overflows");
    long part = 0, cks = 0;                                    // one direction's partials and checkpoints: bounded just above
    for (int p = 0; p < npulse; ++p) {
        part += (npoint[p] + 255) / 256 * nscale * (toff[p + 1] - toff[p]);
        cks += (npoint[p] + 255) / 256 * nscale * ((toff[p + 1] - toff[p] + 7) / 8 * 768);
    }
    if (toff[npulse] > (1L << 56) / ndir || part > (1L << 56) / ndir || cks > (1L << 56) / ndir || nblk > 2147483647L / ndir ||
        nfold > 2147483647L / ndir)
        return bad("the output size or the workgroup count overflows");
    return 0;
}

static int bloch_lsq_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff, const double* b1_re,
                                const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                                const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                const double* dy, const double* dz, int nscale, const double* scales, const double* m0x,
                                const double* m0y, const double* m0z, const double* wx, const double* wy, const double* wz,
                                const double* tx, const double* ty, const double* tz, double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    if (const int e = bloch_gn_check(ctx, who, wx && wy && (mag || wz) && tx && ty && (mag || tz) && loss && g_re && g_im,
                                     "a weight, target, loss or gradient plane is null", m0x, m0y, m0z, npulse, nscale, wx, wy, wz, 1,
                                     toff, npoint.data()))
        return e;
    MBFIR_TRY(ctx, bloch_lsq_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                       gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wx, wy, wz, tx,
                                       ty, tz, loss, g_re, g_im, mag));
}
int mbfir_bloch_lsq_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                          const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                          const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                          const double* m0x, const double* m0y, const double* m0z, const double* wx, const double* wy,
                          const double* wz, const double* tx, const double* ty, const double* tz, double* loss, double* g_re,
                          double* g_im) {
    return bloch_lsq_batch_call(ctx, "bloch_lsq_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma,
                                nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wx, wy, wz, tx, ty, tz,
                                loss, g_re, g_im);
}
int mbfir_bloch_lsq_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                              const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                              const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                              const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                              int nscale, const double* scales, const double* m0x, const double* m0y, const double* m0z,
                              const double* wxy, const double* wz, const double* txy, const double* tz, double* loss, double* g_re,
                              double* g_im) {
    return bloch_lsq_batch_call(ctx, "bloch_lsq_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wxy, wz, nullptr,
                                txy, tz, nullptr, loss, g_re, g_im);
}

static int bloch_gn_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff, const double* b1_re,
                               const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                               const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                               const long* foff, const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                               const double* dz, int nscale, const double* scales, const double* m0x, const double* m0y,
                               const double* m0z, const double* wx, const double* wy, const double* wz, int ndir,
                               const double* v_re, const double* v_im, double* h_re, double* h_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    if (const int e = bloch_gn_check(ctx, who, wx && wy && (mag || wz) && v_re && v_im && h_re && h_im,
                                     "a weight, direction or product plane is null", m0x, m0y, m0z, npulse, nscale, wx, wy, wz, ndir,
                                     toff, npoint.data()))
        return e;
    MBFIR_TRY(ctx, bloch_gn_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                      gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wx, wy, wz,
                                      ndir, v_re, v_im, h_re, h_im, mag));
}
int mbfir_bloch_gn_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                         const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                         const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid,
                         const long* poff, const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                         const double* m0x, const double* m0y, const double* m0z, const double* wx, const double* wy,
                         const double* wz, int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im) {
    return bloch_gn_batch_call(ctx, "bloch_gn_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma,
                               nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wx, wy, wz, ndir, v_re,
                               v_im, h_re, h_im);
}
int mbfir_bloch_gn_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                             const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                             int nscale, const double* scales, const double* m0x, const double* m0y, const double* m0z,
                             const double* wxy, const double* wz, int ndir, const double* v_re, const double* v_im, double* h_re,
                             double* h_im) {
    return bloch_gn_batch_call(ctx, "bloch_gn_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                               gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wxy, wz, nullptr,
                               ndir, v_re, v_im, h_re, h_im);
}

// The steady state's least-squares products (blochssgn.hip): mbfir_bloch_batch's checks at mode 1, then the call's own
// planes, M given whole or not at all, then bloch_gn_check's (no m0): the weights, ndir, the partials, the checkpoints and the
// workgroup counts; gn also one plane of (I - A)^-1 per workgroup, as mbfir_bloch_ss_jvp_batch bounds it.
static int bloch_ss_lsq_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff, const double* b1_re,
                                   const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                                   const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                   const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                   const double* dy, const double* dz, int nscale, const double* scales, const double* wx,
                                   const double* wy, const double* wz, const double* tx, const double* ty, const double* tz,
                                   double* loss, double* g_re, double* g_im, double* mx, double* my, double* mz) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 1,
                                        arrays, npoint))
        return e;
    if (!(wx && wy && (mag || wz) && tx && ty && (mag || tz) && loss && g_re && g_im))
        return bad("a weight, target, loss or gradient plane is null");
    if ((mx || my || mz) && !(mx && my && mz)) return bad("mx, my and mz are given together or not at all");
    if (const int e = bloch_gn_check(ctx, who, true, "", nullptr, nullptr, nullptr, npulse, nscale, wx, wy, wz, 1, toff,
                                     npoint.data()))
        return e;
    MBFIR_TRY(ctx, bloch_ss_lsq_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                          t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wx, wy, wz, tx, ty, tz,
                                          loss, g_re, g_im, mx, my, mz, mag));
}
int mbfir_bloch_ss_lsq_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                             const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                             const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                             const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                             int nscale, const double* scales, const double* wx, const double* wy, const double* wz,
                             const double* tx, const double* ty, const double* tz, double* loss, double* g_re, double* g_im,
                             double* mx, double* my, double* mz) {
    return bloch_ss_lsq_batch_call(ctx, "bloch_ss_lsq_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                   gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wx, wy, wz, tx, ty, tz, loss,
                                   g_re, g_im, mx, my, mz);
}
int mbfir_bloch_ss_lsq_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                 const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                 const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                 const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                 const double* dz, int nscale, const double* scales, const double* wxy, const double* wz,
                                 const double* txy, const double* tz, double* loss, double* g_re, double* g_im, double* mx,
                                 double* my, double* mz) {
    return bloch_ss_lsq_batch_call(ctx, "bloch_ss_lsq_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                   t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wxy, wz, nullptr, txy, tz,
                                   nullptr, loss, g_re, g_im, mx, my, mz);
}

static int bloch_ss_gn_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff, const double* b1_re,
                                  const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                                  const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                  const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                  const double* dy, const double* dz, int nscale, const double* scales, const double* wx,
                                  const double* wy, const double* wz, int ndir, const double* v_re, const double* v_im,
                                  double* h_re, double* h_im) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 1,
                                        arrays, npoint))
        return e;
    if (!(wx && wy && (mag || wz) && v_re && v_im && h_re && h_im)) return bad("a weight, direction or product plane is null");
    if (const int e = bloch_gn_check(ctx, who, true, "", nullptr, nullptr, nullptr, npulse, nscale, wx, wy, wz, ndir, toff,
                                     npoint.data()))
        return e;
    long nblk = 0;                                              // bloch_gn_check has bounded it times ndir by 2^31 - 1
    for (int p = 0; p < npulse; ++p) nblk += (npoint[p] + 255) / 256 * nscale;
    if (nblk * ndir > (1L << 56) / 2304) return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_ss_gn_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                         t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wx, wy, wz, ndir, v_re,
                                         v_im, h_re, h_im, mag));
}
int mbfir_bloch_ss_gn_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                            const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                            const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                            int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                            const double* scales, const double* wx, const double* wy, const double* wz, int ndir,
                            const double* v_re, const double* v_im, double* h_re, double* h_im) {
    return bloch_ss_gn_batch_call(ctx, "bloch_ss_gn_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                  gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wx, wy, wz, ndir, v_re, v_im,
                                  h_re, h_im);
}
int mbfir_bloch_ss_gn_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                const double* dz, int nscale, const double* scales, const double* wxy, const double* wz, int ndir,
                                const double* v_re, const double* v_im, double* h_re, double* h_im) {
    return bloch_ss_gn_batch_call(ctx, "bloch_ss_gn_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2,
                                  gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wxy, wz, nullptr, ndir, v_re,
                                  v_im, h_re, h_im);
}

// What the least-squares calls check after abr_batch_check, in this order: their own arrays, the profile, the O weights (O: the
// forward call's output entries), ndir, and that ndir times the R rf samples, the partials (one per workgroup and sample, per
// direction; at most 2^56 entries each) and the workgroups of the sweep and of the fold (at most 2^31 - 1 each) fit.  0, or
// MBFIR_E_ARG with ctx->err set.
static int gn_check(mbfir_ctx* ctx, const char* who, bool arrays, int profile, int npulse, int nscale, const double* w, int ndir,
                    const long* roff, const long* npoint) {
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (!arrays) return bad("a required array is null");
    if (profile < 0 || profile > 3) return bad("profile must be 0, 1, 2 or 3");
    long O = 0, nblk = 0, nfold = 0;                           // abr_batch_check has bounded O and nblk
    for (int p = 0; p < npulse; ++p) {
        O += npoint[p] * nscale;
        nblk += (npoint[p] + 255) / 256 * nscale;
        nfold += (roff[p + 1] - roff[p] + 255) / 256;
    }
    for (long i = 0; i < O; ++i)
        if (!(w[i] >= 0) || !std::isfinite(w[i])) return bad("a weight is negative or not finite");
    if (ndir < 1) return bad("ndir must be at least 1");
    if (!vjp_partials_fit(npulse, nscale, roff, npoint)) return bad("the output size or the workgroup count overflows");
    long part = 0;                                             // one direction's partials: vjp_partials_fit has bounded them
    for (int p = 0; p < npulse; ++p) part += (npoint[p] + 255) / 256 * nscale * (roff[p + 1] - roff[p]);
    if (roff[npulse] > (1L << 56) / ndir || part > (1L << 56) / ndir || nblk > 2147483647L / ndir || nfold > 2147483647L / ndir)
        return bad("the output size or the workgroup count overflows");
    return 0;
}

int mbfir_abr_lsq_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                        int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int profile,
                        const double* w, const double* t_re, const double* t_im, double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales;
    if (const int e = abr_batch_check(ctx, "abr_lsq_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays, npoint))
        return e;
    if (const int e = gn_check(ctx, "abr_lsq_batch", w && t_re && loss && g_re && g_im, profile, npulse, nscale, w, 1, roff,
                               npoint.data()))
        return e;
    MBFIR_TRY(ctx, abr_lsq_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales,
                                     mode, profile, w, t_re, profile == 2 ? nullptr : t_im, loss, g_re, g_im));
}

int mbfir_abr2_lsq_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                         const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                         const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                         const double* t_re, const double* t_im, double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales;
    if (const int e = abr_batch_check(ctx, "abr2_lsq_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays,
                                      npoint))
        return e;
    if (const int e = gn_check(ctx, "abr2_lsq_batch", w && t_re && loss && g_re && g_im, profile, npulse, nscale, w, 1, roff,
                               npoint.data()))
        return e;
    MBFIR_TRY(ctx, abr2_lsq_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid,
                                      yoff, y, nscale, scales, mode, profile, w, t_re, profile == 2 ? nullptr : t_im, loss, g_re,
                                      g_im));
}

int mbfir_abr_gn_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                       int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int profile,
                       const double* w, int ndir, const double* v_re, const double* v_im, double* h_re, double* h_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales;
    if (const int e = abr_batch_check(ctx, "abr_gn_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays, npoint))
        return e;
    if (const int e = gn_check(ctx, "abr_gn_batch", w && v_re && v_im && h_re && h_im, profile, npulse, nscale, w, ndir, roff,
                               npoint.data()))
        return e;
    MBFIR_TRY(ctx, abr_gn_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales,
                                    mode, profile, w, ndir, v_re, v_im, h_re, h_im));
}

int mbfir_abr2_gn_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                        const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                        const double* y, int nscale, const double* scales, int mode, int profile, const double* w, int ndir,
                        const double* v_re, const double* v_im, double* h_re, double* h_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales;
    if (const int e = abr_batch_check(ctx, "abr2_gn_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays,
                                      npoint))
        return e;
    if (const int e = gn_check(ctx, "abr2_gn_batch", w && v_re && v_im && h_re && h_im, profile, npulse, nscale, w, ndir, roff,
                               npoint.data()))
        return e;
    MBFIR_TRY(ctx, abr2_gn_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid,
                                     yoff, y, nscale, scales, mode, profile, w, ndir, v_re, v_im, h_re, h_im));
}

// What the Levenberg-Marquardt step checks after abr_batch_check and gn_check (at ndir = 1), in this order: its own arrays, mu, cg,
// rtol, and that its per-sample sections (eight times the R rf samples, at most 2^56 entries) and the workgroups of the trial (at
// most 2^31 - 1) fit.  0, or MBFIR_E_ARG with ctx->err set.
static int lm_check(mbfir_ctx* ctx, const char* who, bool arrays, int npulse, const long* roff, const double* mu, int cg,
                    double rtol) {
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (!arrays) return bad("a required array is null");
    for (int p = 0; p < npulse; ++p)
        if (!(mu[p] >= 0) || !std::isfinite(mu[p])) return bad("a damping mu is negative or not finite");
    if (cg < 0) return bad("cg must be at least 0");
    if (!(rtol >= 0)) return bad("rtol is negative or not a number");
    if (roff[npulse] > (1L << 56) / 8 || (roff[npulse] + 255) / 256 > 2147483647L)
        return bad("the output size or the workgroup count overflows");
    return 0;
}

int mbfir_abr_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                            int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, int profile,
                            const double* w, const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                            const double* t_re, const double* t_im, double* d_re, double* d_im, int* ncg, double* rr, double* gg,
                            int* status, double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && scales;
    if (const int e = abr_batch_check(ctx, "abr_lm_step_batch", false, npulse, roff, nxgrid, xoff, 1, nullptr, nscale, mode, arrays,
                                      npoint))
        return e;
    if (const int e = gn_check(ctx, "abr_lm_step_batch", w != nullptr, profile, npulse, nscale, w, 1, roff, npoint.data())) return e;
    const bool own = b_re && b_im && mu && d_re && d_im && ncg && rr && gg && status &&
                     (t_re ? loss && g_re && g_im : t_im == nullptr);
    if (const int e = lm_check(ctx, "abr_lm_step_batch", own, npulse, roff, mu, cg, rtol)) return e;
    MBFIR_TRY(ctx, abr_lm_step_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale,
                                         scales, mode, profile, w, b_re, b_im, mu, cg, rtol, t_re, profile == 2 ? nullptr : t_im,
                                         d_re, d_im, ncg, rr, gg, status, loss, g_re, g_im));
}

int mbfir_abr2_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                             const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff,
                             const double* y, int nscale, const double* scales, int mode, int profile, const double* w,
                             const double* b_re, const double* b_im, const double* mu, int cg, double rtol, const double* t_re,
                             const double* t_im, double* d_re, double* d_im, int* ncg, double* rr, double* gg, int* status,
                             double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = roff && rf_re && rf_im && xoff && x && yoff && y && scales;
    if (const int e = abr_batch_check(ctx, "abr2_lm_step_batch", true, npulse, roff, nxgrid, xoff, nygrid, yoff, nscale, mode, arrays,
                                      npoint))
        return e;
    if (const int e = gn_check(ctx, "abr2_lm_step_batch", w != nullptr, profile, npulse, nscale, w, 1, roff, npoint.data())) return e;
    const bool own = b_re && b_im && mu && d_re && d_im && ncg && rr && gg && status &&
                     (t_re ? loss && g_re && g_im : t_im == nullptr);
    if (const int e = lm_check(ctx, "abr2_lm_step_batch", own, npulse, roff, mu, cg, rtol)) return e;
    MBFIR_TRY(ctx, abr2_lm_step_batch_run(ctx->device, ctx->solver->stream(), npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x,
                                          nygrid, yoff, y, nscale, scales, mode, profile, w, b_re, b_im, mu, cg, rtol, t_re,
                                          profile == 2 ? nullptr : t_im, d_re, d_im, ncg, rr, gg, status, loss, g_re, g_im));
}

// What the Bloch Levenberg-Marquardt step checks after bloch_batch_check and bloch_gn_check (at ndir = 1), in this order: its own
// arrays, the targets, mu, cg, rtol, and that its per-sample sections (the five vectors and the trial rows: fewer than sixteen
// double2 per b1 sample, at most 2^56 entries) and the workgroups of the trial (at most 2^31 - 1) fit.  bloch_gn_check's bounds
// on the checkpoints (96 doubles per sample) and on the fold's workgroups are the tighter ones today: the last check states what
// this call's own sections need and does not rely on them.
static int bloch_lm_check(mbfir_ctx* ctx, const char* who, bool arrays, bool targets_ok, int npulse, const long* toff,
                          const double* mu, int cg, double rtol, bool mag = false) {
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    if (!arrays) return bad("a required array is null");
    if (!targets_ok)
        return bad(mag ? "txy and tz are given together or not at all" : "tx, ty and tz are given together or not at all");
    for (int p = 0; p < npulse; ++p)
        if (!(mu[p] >= 0) || !std::isfinite(mu[p])) return bad("a damping mu is negative or not finite");
    if (cg < 0) return bad("cg must be at least 0");
    if (!(rtol >= 0)) return bad("rtol is negative or not a number");
    if (toff[npulse] > (1L << 56) / 16 || (toff[npulse] + 255) / 256 > 2147483647L)
        return bad("the output size or the workgroup count overflows");
    return 0;
}

static int bloch_lm_step_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff, const double* b1_re,
                                    const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                                    const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                    const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                    const double* dy, const double* dz, int nscale, const double* scales, const double* m0x,
                                    const double* m0y, const double* m0z, const double* wx, const double* wy, const double* wz,
                                    const double* b_re, const double* b_im, const double* mu, int cg, double rtol, const double* tx,
                                    const double* ty, const double* tz, double* d_re, double* d_im, int* ncg, double* rr,
                                    double* gg, int* status, double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, 0,
                                        arrays, npoint))
        return e;
    if (const int e = bloch_gn_check(ctx, who, wx && wy && (mag || wz), "a weight, direction or product plane is null", m0x,
                                     m0y, m0z, npulse, nscale, wx, wy, wz, 1, toff, npoint.data()))
        return e;
    const bool targets = tx || ty || tz;
    const bool own = b_re && b_im && mu && d_re && d_im && ncg && rr && gg && status && (!targets || (loss && g_re && g_im));
    if (const int e = bloch_lm_check(ctx, who, own, !targets || (tx && ty && (mag || tz)), npulse, toff, mu, cg, rtol, mag))
        return e;
    MBFIR_TRY(ctx, bloch_lm_step_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                           t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wx,
                                           wy, wz, b_re, b_im, mu, cg, rtol, tx, ty, tz, d_re, d_im, ncg, rr, gg, status, loss, g_re,
                                           g_im, mag));
}
int mbfir_bloch_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                              const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                              const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                              const double* df, int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                              int nscale, const double* scales, const double* m0x, const double* m0y, const double* m0z,
                              const double* wx, const double* wy, const double* wz, const double* b_re, const double* b_im,
                              const double* mu, int cg, double rtol, const double* tx, const double* ty, const double* tz,
                              double* d_re, double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss, double* g_re,
                              double* g_im) {
    return bloch_lm_step_batch_call(ctx, "bloch_lm_step_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                    t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wx, wy,
                                    wz, b_re, b_im, mu, cg, rtol, tx, ty, tz, d_re, d_im, ncg, rr, gg, status, loss, g_re, g_im);
}
int mbfir_bloch_lm_step_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                  const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                  const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                  const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                  const double* dz, int nscale, const double* scales, const double* m0x, const double* m0y,
                                  const double* m0z, const double* wxy, const double* wz, const double* b_re, const double* b_im,
                                  const double* mu, int cg, double rtol, const double* txy, const double* tz, double* d_re,
                                  double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss, double* g_re,
                                  double* g_im) {
    return bloch_lm_step_batch_call(ctx, "bloch_lm_step_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1,
                                    t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, m0x, m0y, m0z, wxy, wz,
                                    nullptr, b_re, b_im, mu, cg, rtol, txy, tz, nullptr, d_re, d_im, ncg, rr, gg, status, loss,
                                    g_re, g_im);
}

// The steady state's step (blochssgn.hip): mbfir_bloch_batch's checks at mode 1, bloch_gn_check's at ndir = 1 (no m0),
// bloch_lm_check's, and one plane of (I - A)^-1 and M (12 x 256 doubles) per forward workgroup.
static int bloch_ss_lm_step_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff, const double* b1_re,
                                       const double* b1_im, const double* gx, const double* gy, const double* gz, const long* tsoff,
                                       const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                       const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                       const double* dy, const double* dz, int nscale, const double* scales, const double* wx,
                                       const double* wy, const double* wz, const double* b_re, const double* b_im, const double* mu,
                                       int cg, double rtol, const double* tx, const double* ty, const double* tz, double* d_re,
                                       double* d_im, int* ncg, double* rr, double* gg, int* status, double* loss, double* g_re,
                                       double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const char* why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales;
    if (const int e = bloch_batch_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale,
                                        1, arrays, npoint))
        return e;
    if (const int e = bloch_gn_check(ctx, who, wx && wy && (mag || wz), "a weight, direction or product plane is null",
                                     nullptr, nullptr, nullptr, npulse, nscale, wx, wy, wz, 1, toff, npoint.data()))
        return e;
    const bool targets = tx || ty || tz;
    const bool own = b_re && b_im && mu && d_re && d_im && ncg && rr && gg && status && (!targets || (loss && g_re && g_im));
    if (const int e = bloch_lm_check(ctx, who, own, !targets || (tx && ty && (mag || tz)), npulse, toff, mu, cg, rtol, mag))
        return e;
    long nblk = 0;                                              // bloch_gn_check has bounded it by 2^31 - 1
    for (int p = 0; p < npulse; ++p) nblk += (npoint[p] + 255) / 256 * nscale;
    if (nblk > (1L << 56) / 3072) return bad("the output size or the workgroup count overflows");
    MBFIR_TRY(ctx, bloch_ss_lm_step_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                              t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wx, wy, wz,
                                              b_re, b_im, mu, cg, rtol, tx, ty, tz, d_re, d_im, ncg, rr, gg, status, loss, g_re,
                                              g_im, mag));
}
int mbfir_bloch_ss_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                 const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                 const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                 const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                 const double* dz, int nscale, const double* scales, const double* wx, const double* wy,
                                 const double* wz, const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                                 const double* tx, const double* ty, const double* tz, double* d_re, double* d_im, int* ncg,
                                 double* rr, double* gg, int* status, double* loss, double* g_re, double* g_im) {
    return bloch_ss_lm_step_batch_call(ctx, "bloch_ss_lm_step_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps,
                                       t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wx, wy, wz, b_re,
                                       b_im, mu, cg, rtol, tx, ty, tz, d_re, d_im, ncg, rr, gg, status, loss, g_re, g_im);
}
int mbfir_bloch_ss_lm_step_mag_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                     const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                                     const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff,
                                     const double* df, int npgrid, const long* poff, const double* dx, const double* dy,
                                     const double* dz, int nscale, const double* scales, const double* wxy, const double* wz,
                                     const double* b_re, const double* b_im, const double* mu, int cg, double rtol,
                                     const double* txy, const double* tz, double* d_re, double* d_im, int* ncg, double* rr,
                                     double* gg, int* status, double* loss, double* g_re, double* g_im) {
    return bloch_ss_lm_step_batch_call(ctx, "bloch_ss_lm_step_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                       tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, wxy, wz,
                                       nullptr, b_re, b_im, mu, cg, rtol, txy, tz, nullptr, d_re, d_im, ncg, rr, gg, status, loss,
                                       g_re, g_im);
}

// The train's step (blochtrainlm.hip): bloch_train_check, the checks of mbfir_bloch_train_gn_batch at ndir = 1 with their
// messages and order (ebcast, the weights, the sizes), bloch_lm_check's for its own arrays, mu, cg and rtol, then the targets:
// each triple whole or absent, and, when any is given, one for every term that has weights and none for a term that has not.
static int bloch_train_lm_step_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff,
                                          const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                                          const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                                          const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                                          int npgrid, const long* poff, const double* dx, const double* dy, const double* dz,
                                          int nscale, const double* scales, const int* ntr, const long* roff,
                                          const double* cosphi, const double* sinphi, const int* gidx, const long* goff,
                                          const double* gains, const int* echo, const double* meq, int demod, const double* m0x,
                                          const double* m0y, const double* m0z, int ebcast, const double* wx, const double* wy,
                                          const double* wz, const double* rw, const double* wfx, const double* wfy,
                                          const double* wfz, const double* b_re, const double* b_im, const double* mu, int cg,
                                          double rtol, const double* tx, const double* ty, const double* tz, const double* tfx,
                                          const double* tfy, const double* tfz, double* d_re, double* d_im, int* ncg, double* rr,
                                          double* gg, int* status, double* loss, double* g_re, double* g_im) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff,
                                        nscale, arrays, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint,
                                        ncomb))
        return e;
    if (ebcast != 0 && ebcast != 1) return bad("ebcast must be 0 or 1");
    const bool any_e = wx || wy || wz, any_f = wfx || wfy || wfz;
    if (any_e && !(wx && wy && (mag || wz))) return bad("the echo weights are given together or not at all");
    if (any_f && !(wfx && wfy && (mag || wfz))) return bad("the final weights are given together or not at all");
    if (!any_e && !any_f) return bad("neither an echo term nor a final term is given");
    const double* const w[3] = {wx, wy, wz};
    const double* const wf[3] = {wfx, wfy, wfz};
    if (const int e = bloch_train_gn_check(ctx, who, npulse, nscale, 1, toff, ntr, roff, ncomb.data(),
                                           npoint.data(), ebcast, w, rw, wf))
        return e;
    if (!bloch_train_jvp_fits(npulse, nscale, 1, toff, ntr, ncomb.data(), npoint.data()))
        return bad("the output size or the workgroup count overflows");
    const bool tg_e = tx || ty || tz, tg_f = tfx || tfy || tfz, targets = tg_e || tg_f;
    const bool own = b_re && b_im && mu && d_re && d_im && ncg && rr && gg && status && (!targets || (loss && g_re && g_im));
    if (const int e = bloch_lm_check(ctx, who, own, true, npulse, toff, mu, cg, rtol)) return e;
    if (tg_e && !(tx && ty && (mag || tz)))
        return bad(mag ? "txy and tz are given together or not at all" : "tx, ty and tz are given together or not at all");
    if (tg_f && !(tfx && tfy && (mag || tfz)))
        return bad(mag ? "tfxy and tfz are given together or not at all" : "tfx, tfy and tfz are given together or not at all");
    if ((tg_e && !any_e) || (tg_f && !any_f)) return bad("a target is given for a term that has no weights");
    if (targets && ((any_e && !tg_e) || (any_f && !tg_f))) return bad("a term that has weights has no target while the other has one");
    const double* const t[3] = {tx, ty, tz};
    const double* const tf[3] = {tfx, tfy, tfz};
    MBFIR_TRY(ctx, bloch_train_lm_step_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                 tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr,
                                                 roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, w, rw,
                                                 wf, b_re, b_im, mu, cg, rtol, t, tf, d_re, d_im, ncg, rr, gg, status, loss, g_re,
                                                 g_im, mag));
}
int mbfir_bloch_train_lm_step_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                    const double* gx, const double* gy, const double* gz, const long* tsoff,
                                    const double* tsteps, const double* t1, const double* t2, const double* gamma, int nfgrid,
                                    const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                                    const double* dy, const double* dz, int nscale, const double* scales, const int* ntr,
                                    const long* roff, const double* cosphi, const double* sinphi, const int* gidx,
                                    const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                                    const double* m0x, const double* m0y, const double* m0z, int ebcast, const double* wx,
                                    const double* wy, const double* wz, const double* rw, const double* wfx, const double* wfy,
                                    const double* wfz, const double* b_re, const double* b_im, const double* mu, int cg,
                                    double rtol, const double* tx, const double* ty, const double* tz, const double* tfx,
                                    const double* tfy, const double* tfz, double* d_re, double* d_im, int* ncg, double* rr,
                                    double* gg, int* status, double* loss, double* g_re, double* g_im) {
    return bloch_train_lm_step_batch_call(ctx, "bloch_train_lm_step_batch", false, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                          tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale, scales, ntr,
                                          roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z, ebcast, wx,
                                          wy, wz, rw, wfx, wfy, wfz, b_re, b_im, mu, cg, rtol, tx, ty, tz, tfx, tfy, tfz, d_re,
                                          d_im, ncg, rr, gg, status, loss, g_re, g_im);
}
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
                                        double* g_re, double* g_im) {
    return bloch_train_lm_step_batch_call(ctx, "bloch_train_lm_step_mag_batch", true, npulse, toff, b1_re, b1_im, gx, gy, gz,
                                          tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale,
                                          scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y, m0z,
                                          ebcast, wxy, wz, nullptr, rw, wfxy, wfz, nullptr, b_re, b_im, mu, cg, rtol, txy, tz,
                                          nullptr, tfxy, tfz, nullptr, d_re, d_im, ncg, rr, gg, status, loss, g_re, g_im);
}

// The schedule's step (blochtrainschedlm.hip): bloch_train_check, then the checks mbfir_bloch_train_lsq_sched_batch and
// mbfir_bloch_train_gn_sched_batch at ndir = 1 share, in their order and with their messages (ebcast, the weights, both terms absent,
// both halves absent, the sizes at two checkpointed states), bloch_lm_check's for its own arrays, mu, cg and rtol, then the halves
// (nothing given for a half that does not vary), the targets as mbfir_bloch_train_lm_step_batch checks them, and the right-hand side.
static int bloch_train_lm_step_sched_batch_call(mbfir_ctx* ctx, const char* who, bool mag, int npulse, const long* toff,
                                                const double* b1_re, const double* b1_im, const double* gx, const double* gy,
                                                const double* gz, const long* tsoff, const double* tsteps, const double* t1,
                                                const double* t2, const double* gamma, int nfgrid, const long* foff,
                                                const double* df, int npgrid, const long* poff, const double* dx,
                                                const double* dy, const double* dz, int nscale, const double* scales,
                                                const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                                                const int* gidx, const long* goff, const double* gains, const int* echo,
                                                const double* meq, int demod, const double* m0x, const double* m0y,
                                                const double* m0z, int ebcast, const double* wx, const double* wy,
                                                const double* wz, const double* tx, const double* ty, const double* tz,
                                                const double* rw, const double* wfx, const double* wfy, const double* wfz,
                                                const double* tfx, const double* tfy, const double* tfz, const double* bgain,
                                                const double* bphi, const double* mu, int cg, double rtol, double* dgain,
                                                double* dphi, int* ncg, double* rr, double* gg, int* status, double* loss,
                                                double* ggain, double* gphi) {
    if (!ctx) return MBFIR_E_ARG;
    auto bad = [&](const std::string& why) { ctx->err = std::string(who) + ": " + why; return MBFIR_E_ARG; };
    std::vector<long> npoint, ncomb;
    const bool arrays = toff && b1_re && b1_im && tsoff && tsteps && t1 && t2 && gamma && foff && df && poff && scales && ntr &&
                        roff && cosphi && sinphi && gidx && goff && gains && echo && meq;
    if (const int e = bloch_train_check(ctx, who, npulse, toff, tsoff, t1, t2, nfgrid, foff, npgrid, poff, nscale, arrays, ntr, roff,
                                        cosphi, sinphi, gidx, goff, gains, echo, meq, m0x, m0y, m0z, npoint, ncomb))
        return e;
    if (ebcast != 0 && ebcast != 1) return bad("ebcast must be 0 or 1");
    const bool any_e = wx || wy || wz, any_f = wfx || wfy || wfz;
    if (any_e && !(wx && wy && (mag || wz))) return bad("the echo weights are given together or not at all");
    if (any_f && !(wfx && wfy && (mag || wfz))) return bad("the final weights are given together or not at all");
    if (!any_e && !any_f) return bad("neither an echo term nor a final term is given");
    if (!dgain && !dphi) return bad("neither the gains nor the phases vary: dgain and dphi are both null");
    const double* const w[3] = {wx, wy, wz};
    const double* const wf[3] = {wfx, wfy, wfz};
    if (const int e = bloch_train_sched_gn_check(ctx, who, npulse, nscale, 1, 2, ntr, roff, ncomb.data(), npoint.data(), ebcast, w, rw,
                                                 wf))
        return e;
    const bool tg_e = tx || ty || tz, tg_f = tfx || tfy || tfz, targets = tg_e || tg_f;
    const bool own = mu && ncg && rr && gg && status && (!targets || (loss && (!dgain || ggain) && (!dphi || gphi)));
    if (const int e = bloch_lm_check(ctx, who, own, true, npulse, roff, mu, cg, rtol)) return e;
    if ((!dgain && (bgain || ggain)) || (!dphi && (bphi || gphi)))
        return bad("a right-hand side or a gradient is given for a half that does not vary");
    if (tg_e && !(tx && ty && (mag || tz)))
        return bad(mag ? "txy and tz are given together or not at all" : "tx, ty and tz are given together or not at all");
    if (tg_f && !(tfx && tfy && (mag || tfz)))
        return bad(mag ? "tfxy and tfz are given together or not at all" : "tfx, tfy and tfz are given together or not at all");
    if ((tg_e && !any_e) || (tg_f && !any_f)) return bad("a target is given for a term that has no weights");
    if (targets && ((any_e && !tg_e) || (any_f && !tg_f))) return bad("a term that has weights has no target while the other has one");
    if ((bgain || bphi) && ((dgain && !bgain) || (dphi && !bphi)))
        return bad("the right-hand side is given for every half that varies or not at all");
    if (!targets && !bgain && !bphi) return bad("neither targets nor a right-hand side is given");
    const double* const t[3] = {tx, ty, tz};
    const double* const tf[3] = {tfx, tfy, tfz};
    MBFIR_TRY(ctx, bloch_train_lm_step_sched_batch_run(ctx->device, ctx->solver->stream(), npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff,
                                                       tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz, nscale,
                                                       scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod, m0x, m0y,
                                                       m0z, ebcast, w, t, rw, wf, tf, bgain, bphi, mu, cg, rtol, dgain, dphi, ncg, rr,
                                                       gg, status, loss, ggain, gphi, mag));
}
int mbfir_bloch_train_lm_step_sched_batch(mbfir_ctx* ctx, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                                          const double* gx, const double* gy, const double* gz, const long* tsoff,
                                          const double* tsteps, const double* t1, const double* t2, const double* gamma,
                                          int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                                          const double* dx, const double* dy, const double* dz, int nscale, const double* scales,
                                          const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                                          const int* gidx, const long* goff, const double* gains, const int* echo,
                                          const double* meq, int demod, const double* m0x, const double* m0y, const double* m0z,
                                          int ebcast, const double* wx, const double* wy, const double* wz, const double* tx,
                                          const double* ty, const double* tz, const double* rw, const double* wfx,
                                          const double* wfy, const double* wfz, const double* tfx, const double* tfy,
                                          const double* tfz, const double* bgain, const double* bphi, const double* mu, int cg,
                                          double rtol, double* dgain, double* dphi, int* ncg, double* rr, double* gg,
                                          int* status, double* loss, double* ggain, double* gphi) {
    return bloch_train_lm_step_sched_batch_call(ctx, "bloch_train_lm_step_sched_batch", false, npulse, toff, b1_re, b1_im, gx,
                                                gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                                                nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod,
                                                m0x, m0y, m0z, ebcast, wx, wy, wz, tx, ty, tz, rw, wfx, wfy, wfz, tfx, tfy, tfz,
                                                bgain, bphi, mu, cg, rtol, dgain, dphi, ncg, rr, gg, status, loss, ggain, gphi);
}
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
                                              double* loss, double* ggain, double* gphi) {
    return bloch_train_lm_step_sched_batch_call(ctx, "bloch_train_lm_step_sched_mag_batch", true, npulse, toff, b1_re, b1_im, gx,
                                                gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                                                nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq, demod,
                                                m0x, m0y, m0z, ebcast, wxy, wz, nullptr, txy, tz, nullptr, rw, wfxy, wfz,
                                                nullptr, tfxy, tfz, nullptr, bgain, bphi, mu, cg, rtol, dgain, dphi, ncg, rr, gg,
                                                status, loss, ggain, gphi);
}

int mbfir_test_jvp_group(void) { return jvp_group(); }
int mbfir_test_bloch_jvp_group(void) { return bloch_jvp_group(); }

long mbfir_test_sim_blocks(int npulse, const int* ntime, const long* npoint, int nscale, int* out) {
    if (npulse < 1 || nscale < 1 || !ntime || !npoint) return -1;
    std::vector<long> ntout(npulse, 1);
    for (int p = 0; p < npulse; ++p)
        if (ntime[p] < 1 || npoint[p] < 1) return -1;
    if (!sim_sizes(npulse, nscale, npoint, ntout.data())) return -1;
    try {
        return sim_block_table(npulse, ntime, npoint, nscale, reinterpret_cast<SimBlock*>(out));
    } catch (const std::exception&) { return -1; }
}

int mbfir_test_time_kernels(mbfir_ctx* ctx, int n, int m, int nt, int reps, double* ms_chol, double* ms_gram) {
    MBFIR_TRY(ctx, ctx->solver->test_time_kernels(n, m, nt, reps, ms_chol, ms_gram));
}

}  // extern "C"
