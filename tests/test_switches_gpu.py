"""Implementation switches of the device solver must not change results: every optimisation of this round has an
environment switch (read at solve time), and the switched-off form is the reference for the switched-on one.

  MBFIR_FOLD=0         every frequency on its own instead of the +w / -w pairs of the folded lattice kernels
  MBFIR_CHOL_SPLIT     4 (default for lock-step batches): the factorisation in one launch; 1: one launch per panel step with
                       the device flag; 2: the split step as two launches; 0: the fused single-design step
  MBFIR_POISON=1       NaN in the diagonal-block images before every build (a stale read shows deterministically)
  MBFIR_HSOLVE=0       the preconditioner M'(M b) as two triangular GEMVs on M and the stored M' instead of one pass over M
  MBFIR_CGRP=1         one chunk per block in the moment kernel (no interleaved pair)
  MBFIR_FUSE=0         round 4's separate launches: k_freq_fold in front of the moment kernel, k_resid_norm behind k_gt_finish,
                       k_hsolve_fold + k_cg_start behind the one-pass M'(M b), k_scal_step in front of k_update (round 5 fused them
                       into their neighbours; the sums and their order are unchanged)
  MBFIR_CORRECTOR=0    round 5's iteration, without the centrality corrector (round 6; the oracle: corrector=False)
"""
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu

F6 = [-0.6, -0.35, -0.1, 0.15, 0.45, 0.8]
A6 = [0, 0, 0.7, 0.7, 0, 0]
D3 = [0.01, 0.02, 0.01]


class env:
    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def relinf(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# Two forms of one solve whose sums run in another ORDER (folded / unfolded lattice kernels, one-pass / two-pass preconditioner, chunk
# grouping) differ by rounding, and since round 6 the iteration no longer damps such differences: the centrality corrector's
# take-or-leave decisions amplify them (~2-3 x per iteration), so the two forms may need a different number of iterations.  What
# makes them comparable all the same is the end game (oracle/conic_ipm.py POLISH): both end well inside the stopping tolerances -- the
# conic solution agrees to 1e-6 whatever the path (1e-9 ... 1e-7 measured on these cases).  The TAPS of fir_ap_cvx are that solution seen through the spectral
# factorisation (log of a spectrum that touches 1e-20: fir_ap_cvx.m:281,296), which amplifies by 1e1 ... 1e9 depending on the
# instance (the n = 40 case below: 7e8, measured in the oracle), so the taps are held at 1e-6 where the instance allows it.
ITER_SLACK = 4


def same_optimum(h0, i0, h1, i1, z0=None, z1=None, tap_tol=1e-6):
    assert abs(i0["iters"] - i1["iters"]) <= ITER_SLACK, (i0["iters"], i1["iters"])
    assert abs(i0["pcost"] - i1["pcost"]) <= 1e-9 * max(1.0, abs(i0["pcost"]))
    if z0 is not None:
        assert relinf(z1, z0) <= 1e-6
    if tap_tol is not None:
        assert relinf(h1, h0) <= tap_tol


def solution_of(info):
    return mbfir.get_context().last_solution(info["n_unknowns"])


CASES = [
    ("fir_ap_cvx", (33, F6, A6, D3, 0.1, 1e-2), {}),                                   # symmetric grid: every point has a partner
    ("fir_ap_cvx", (40, F6, A6, D3, 0.1, 1e-2), dict(grid_m=1201)),                    # odd grid: w = 0 pairs with itself
    ("fir_linprog", (31, [0, 0.2, 0.35, 1], [1, 1, 0, 0], [0.02, 0.02]), {}),         # one-sided grid: no partners at all
    ("fir_qprog_phs", (23, [-1, -0.6, -0.2, 0.2], [1, 1, 0, 0], [0.05 * np.exp(0.3j), 0.02]), {}),
]


@pytest.mark.parametrize("which,args,okw", CASES)
def test_folded_lattice_kernels_equal_the_unfolded_ones(which, args, okw):
    fn = getattr(mbfir, which)
    opts = mbfir.make_opts(**okw) if okw else None
    with env(MBFIR_FOLD=0):
        h0, s0, i0 = fn(*args, info=True, opts=opts)
        z0 = solution_of(i0)
    with env(MBFIR_FOLD=1):
        h1, s1, i1 = fn(*args, info=True, opts=opts)
        z1 = solution_of(i1)
    assert s0 == s1 == "Solved" and i0["lattice"] == i1["lattice"] == 1
    same_optimum(h0, i0, h1, i1, z0, z1, tap_tol=None if okw.get("grid_m") == 1201 else 1e-6)      # (n = 40 on 1201 points: taps ill-conditioned, see above)


def _batch(**envkw):
    jobs = [("fir_ap_cvx", (64, F6, A6, D3, 0.1, 1e-2 * (1 + 0.5 * k))) for k in range(6)]
    ctx = mbfir.Context(0)
    try:
        with env(**envkw):
            res = mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=6))
    finally:
        ctx.close()
    assert all(r[1] == "Solved" for r in res) and res[0][2]["lanes"] == 6
    return res


def test_lock_step_switches_are_bit_identical():
    """The default lock-step batch runs the factorisation in ONE launch (MBFIR_CHOL_SPLIT=4: ticket-ordered tasks,
    dependency counters); the per-step forms (1: split step with the device flag, 2: two launches per step, 0: fused
    step) do the same arithmetic per tile in the same order.  MBFIR_POISON=1 fills the images of the diagonal blocks
    and 1 / diag(L) with NaN before every build: a block that read them before this build's diagonal block had
    published them would carry NaN into the factor (instead of the previous build's plausible numbers), so
    bit-identical taps under the poison show every in-launch hand-off of the image in order, deterministically."""
    base = _batch()
    for kw in (dict(MBFIR_CHOL_SPLIT=1), dict(MBFIR_CHOL_SPLIT=2), dict(MBFIR_CHOL_SPLIT=0), dict(MBFIR_POISON=1),
               dict(MBFIR_POISON=1, MBFIR_CHOL_SPLIT=1)):
        other = _batch(**kw)
        for (h0, _, i0), (h1, _, i1) in zip(base, other):
            assert np.array_equal(h0, h1) and i0["pcost"] == i1["pcost"] and i0["iters"] == i1["iters"], kw


def test_single_chunk_blocks_agree_to_rounding():
    base = _batch()
    other = _batch(MBFIR_CGRP=1)
    for (h0, _, i0), (h1, _, i1) in zip(base, other):
        same_optimum(h0, i0, h1, i1)


def test_one_pass_preconditioner_application_agrees_with_the_two_triangular_products():
    """x = M'(M b) in one pass over the inverse factor (x = sum_i m_i (m_i . b), the default up to np = 1024: M is read once
    and its transpose is never stored) against the two triangular GEMVs on M and the stored M' (MBFIR_HSOLVE=0): the same
    sums in another order -- same iteration counts, taps equal to rounding; single solves and lock-step lanes."""
    base = _batch()
    other = _batch(MBFIR_HSOLVE=0)
    for (h0, _, i0), (h1, _, i1) in zip(base, other):
        same_optimum(h0, i0, h1, i1)
    for which, args, okw in CASES[:2]:
        fn = getattr(mbfir, which)
        opts = mbfir.make_opts(**okw) if okw else None
        with env(MBFIR_HSOLVE=0):
            h0, s0, i0 = fn(*args, info=True, opts=opts)
            z0 = solution_of(i0)
        h1, s1, i1 = fn(*args, info=True, opts=opts)
        assert s0 == s1 == "Solved"
        same_optimum(h0, i0, h1, i1, z0, solution_of(i1), tap_tol=None if okw.get("grid_m") == 1201 else 1e-6)


def test_dense_path_runs_lock_step_batches_too():
    """opts.dense_trig = 1 (the trig matrix materialised, A' D A on the fp64 matrix cores -- north_star's own route, and
    the path of a program without the lattice structure) batches like the lattice path: every lane owns its trig matrix
    and split-K slab, the Gram products run lane after lane, everything else with the lane as a grid dimension.  The
    lanes' results equal the single dense solves bit for bit."""
    jobs = [("fir_ap_cvx", (48, F6, A6, D3, 0.1, 1e-2 * (1 + 0.5 * k))) for k in range(5)]
    ctx = mbfir.Context(0)
    try:
        res = mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=5, dense_trig=1))
        assert all(r[1] == "Solved" for r in res) and res[0][2]["lanes"] == 5 and res[0][2]["lattice"] == 0
        for (name, args), (h, st, info) in zip(jobs, res):
            h1, s1, i1 = mbfir.fir_ap_cvx(*args, opts=mbfir.make_opts(dense_trig=1), ctx=ctx, info=True)
            assert s1 == "Solved" and i1["lattice"] == 0 and i1["iters"] == info["iters"]
            assert np.array_equal(h, h1) and info["pcost"] == i1["pcost"]
    finally:
        ctx.close()


def test_a_lost_in_launch_hand_off_fails_loudly(monkeypatch):
    """when a hand-off between workgroups inside the factorisation never arrives (here: the diagonal
    block of panel step 3 is told not to raise its flag -- a test hook), the waiting blocks' bounded polls expire, the
    lane's pivot counter carries CHOL_SYNC_LOST, and the solve returns an internal ERROR -- it neither hangs nor goes on
    with the previous build's image as if it were this build's.  Both forms that hand over inside a launch, and the
    DEFAULT form with nothing forced (the unit's failure used to be answered by re-solving every design through
    the single-design path, whose fused per-step factorisation has no in-launch hand-offs -- rc 0 after a stall; an
    internal error of a unit is now reported for its designs, not retried)."""
    jobs = [("fir_ap_cvx", (64, F6, A6, D3, 0.1, 1e-2 * (1 + 0.5 * k))) for k in range(4)]
    for split in (None, "4", "1"):
        ctx = mbfir.Context(0)
        forced = {} if split is None else {"MBFIR_CHOL_SPLIT": split}
        try:
            with env(MBFIR_TEST_LOSE_FLAG=0, **forced):
                with pytest.raises(mbfir.MbfirError, match="hand-off"):
                    mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=4, ddkkt=-1))
            with env(MBFIR_TEST_LOSE_FLAG=-1, **forced):       # and the same context works again afterwards
                res = mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=4))
                assert all(r[1] == "Solved" for r in res)
        finally:
            ctx.close()


def test_eight_contexts_enter_the_extended_precision_path_at_once():
    """Round 3's open defect was a SIGSEGV under `rocprofv3 --kernel-trace` with EIGHT host threads entering the extended-
    precision (double-double) path on their contexts' FIRST builds at the same moment (profiles/README.md).
    This is the unprofiled regression of exactly that condition: eight fresh contexts, eight fir_qp_cvx designs whose first
    solve of the process takes the dd path on every context at once; every result must equal the same design solved alone on
    one context afterwards.  (Kernel attributes are set per device in the Solver's constructor; every dd launch above 64 KB of
    LDS is checked.)"""
    # fir_qp_cvx the way dzrf_mb calls it (k = 120, obj = 1e6: dzrf_mb.m:210-213) on narrow bands around DC: the regime in which
    # nearly active cones carry NT weights far above the rest and the extended-precision solve takes over
    # (seed 1 of tests/test_fuzz_gpu.py's large-weight generator: the oracle solves it and its loosened variants in 23-28 iterations)
    f, a = [-0.13531530807246703, -0.055981529031701, 0.003511847329634643, 0.06198453304672341], [0.0, 0.0, 0.8, 0.8]
    d0 = [0.03450611451870719, 0.015199726365129066]
    jobs = [("fir_qp_cvx", (116, f, a, [x * (1.0 + 0.03 * q) for x in d0], 124.04990661153212, 639631.6986321354)) for q in range(8)]
    opts = mbfir.make_opts(ddkkt=1)
    ctxs = [mbfir.Context(0) for _ in range(8)]
    try:
        res = mbfir.solve_batch(jobs, ctxs=ctxs, info=True, opts=opts)
    finally:
        for c in ctxs:
            c.close()
    assert all(r[1] == "Solved" for r in res) and sum(1 for r in res if r[2]["dd_iters"] > 0) >= 4, [(r[1], r[2]["iters"], r[2]["dd_iters"]) for r in res]
    one = mbfir.Context(0)
    try:
        for (name, args), (h, st, info) in zip(jobs, res):
            h1, s1, i1 = mbfir.fir_qp_cvx(*args, opts=opts, ctx=one, info=True)
            assert s1 == st and i1["iters"] == info["iters"] and i1["dd_iters"] == info["dd_iters"]
            assert np.array_equal(h, h1)
    finally:
        one.close()


@pytest.mark.parametrize("which,args,okw", CASES)
def test_speculative_head_changes_nothing_but_the_build_count(which, args, okw):
    """Round 5: the head of the next iteration (NT scaling, normal matrix, factorisation) is on the stream before the host has read
    this iterate's scalars (MBFIR_SPECULATE=0: the old order).  Same kernels on the same data: verdict, iterations, objective and
    taps are bit-identical; a solve that ends has run one scaling + factorisation more."""
    fn = getattr(mbfir, which)
    opts = mbfir.make_opts(**okw) if okw else None
    with env(MBFIR_SPECULATE=0):
        h0, s0, i0 = fn(*args, info=True, opts=opts)
    with env(MBFIR_SPECULATE=1):
        h1, s1, i1 = fn(*args, info=True, opts=opts)
    assert s0 == s1 and i0["iters"] == i1["iters"] and i0["pcost"] == i1["pcost"] and np.array_equal(h0, h1)
    assert i1["builds"] in (i0["builds"], i0["builds"] + 1)


def test_speculative_head_in_a_lock_step_batch():
    """... and for lock-step units: every lane bit-identical to the batch solved in the old order (lanes that finish early have had
    one factorisation too many under the previous iteration's masks)."""
    jobs = [("fir_ap_cvx", CASES[0][1][:4] + (0.1, 1e-3 * (1 + 0.3 * q))) for q in range(6)] if CASES[0][0] == "fir_ap_cvx" else None
    if jobs is None:
        pytest.skip("first case is not fir_ap_cvx")
    out = {}
    for mode in ("0", "1"):
        with env(MBFIR_SPECULATE=mode):
            out[mode] = mbfir.solve_batch(jobs, info=True, opts=mbfir.make_opts(lanes=6))
    for (h1, s1, i1), (h0, s0, i0) in zip(out["1"], out["0"]):
        assert s1 == s0 and i1["iters"] == i0["iters"] and i1["pcost"] == i0["pcost"] and np.array_equal(h1, h0)


# ---- round 5: launch fusions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,args,okw", CASES)
def test_fused_launches_change_no_bit(which, args, okw):
    """fewer launches per iteration -- the folded operands formed inside the moment kernel, the partial vectors of
    M'(M b) added by the last workgroup to finish, the CG start riding there too.  Same sums in the same order: not one bit moves."""
    fn = getattr(mbfir, which)
    opts = mbfir.make_opts(**okw) if okw else None
    with env(MBFIR_FUSE=0):
        h0, s0, i0 = fn(*args, info=True, opts=opts)
    with env(MBFIR_FUSE=1):
        h1, s1, i1 = fn(*args, info=True, opts=opts)
    assert s0 == s1 == "Solved" and i0["iters"] == i1["iters"] and i0["pcost"] == i1["pcost"] and np.array_equal(h0, h1)


def test_fused_launches_change_no_bit_in_a_lock_step_batch():
    jobs = [("fir_ap_cvx", CASES[0][1][:4] + (0.1, 1e-3 * (1 + 0.3 * q))) for q in range(6)]
    jobs += [("fir_ap_cvx", (36 + 2 * q, F6, A6, D3, 0.1, 1e-2)) for q in range(4)]              # other orders: per-lane N in the CG start
    out = {}
    for mode in ("0", "1"):
        with env(MBFIR_FUSE=mode):
            out[mode] = mbfir.solve_batch(jobs, info=True, opts=mbfir.make_opts(lanes=5))
    assert any(i["lanes"] == 5 for _, _, i in out["1"])
    for (h1, s1, i1), (h0, s0, i0) in zip(out["1"], out["0"]):
        assert s1 == s0 and i1["iters"] == i0["iters"] and i1["pcost"] == i0["pcost"] and np.array_equal(h1, h0)


@pytest.mark.parametrize("which,args,okw", CASES)        # (the last one, fir_qprog_phs: orthant rows AND the big cone are corrected)
def test_centrality_corrector_is_the_oracles_twin_on_and_off(which, args, okw):
    """MBFIR_CORRECTOR=0 is round 5's iteration (no corrector solve); either way the device follows the oracle run with the same
    setting -- iteration count, number of corrected directions taken, taps -- and both settings end at the same optimum (the end
    game makes the answer independent of the path: oracle/conic_ipm.py POLISH)."""
    from oracle import designers
    out = {}
    for corr in (1, 0):
        with env(MBFIR_CORRECTOR=corr):
            h, st, i = getattr(mbfir, which)(*args, info=True, opts=mbfir.make_opts(**okw))
        ho, so, io = getattr(designers, which)(*args, info=True, corrector=bool(corr), **okw)
        assert st == so == "Solved"
        # (short runs: the device's path IS the oracle's -- same iterations, same take-or-leave decisions)
        # (fir_qprog_phs: one of the 21 decisions is a tie the two arithmetics break differently -- a step longer by 1.01 or not)
        assert i["iters"] == io["iters"] and i["correctors"] == io["correctors"], (corr, i["iters"], io["iters"])
        assert abs(i["correctors_taken"] - io["correctors_taken"]) <= (1 if which == "fir_qprog_phs" else 0), (corr, i["correctors_taken"], io["correctors_taken"])
        z = solution_of(i)
        assert relinf(z, io["x"]) <= (1e-7 if which == "fir_qprog_phs" else 1e-9)      # (a quadratic objective: the solution moves with the square root of the gap)
        if okw.get("grid_m") != 1201:
            assert relinf(h, ho) <= 1e-6
        out[corr] = (h, i, z)
    assert out[1][1]["correctors"] == out[1][1]["iters"] and out[0][1]["correctors"] == 0
    assert out[1][1]["iters"] < out[0][1]["iters"]                       # (what it is for)
    same_optimum(out[0][0], dict(out[0][1], iters=0), out[1][0], dict(out[1][1], iters=0), out[0][2], out[1][2], tap_tol=None if okw.get("grid_m") == 1201 else 1e-6)
    assert out[1][1]["gv_passes"] > 0 and out[1][1]["gtv_passes"] > out[1][1]["gv_passes"]


def test_centrality_corrector_in_a_lock_step_batch_every_lane_picks_for_itself():
    """Lanes take or leave the corrected direction independently (S_PICK per lane): a unit equals the single solves bit for bit."""
    jobs = [("fir_ap_cvx", (33, F6, A6, [0.01 * (1 + 0.2 * q), 0.02, 0.01], 0.1, 1e-2 * (1 + q))) for q in range(6)]
    res = mbfir.solve_batch(jobs, streams=1, info=True, opts=mbfir.make_opts(lanes=6))
    assert res[0][2]["lanes"] == 6
    taken = set()
    for job, (h, st, i) in zip(jobs, res):
        h1, s1, i1 = mbfir.fir_ap_cvx(*job[1], info=True)
        assert s1 == st == "Solved" and i1["iters"] == i["iters"] and i1["correctors_taken"] == i["correctors_taken"] and i1["pcost"] == i["pcost"]
        assert np.array_equal(h, h1)
        taken.add(i["correctors_taken"])
    assert len(taken) >= 2                                               # (the lanes did decide differently)


def test_centrality_corrector_on_the_big_cone_of_fir_qprog_phs():
    """fir_qprog_phs keeps its quadratic objective as one big second-order cone beside the orthant rows; the corrector projects the
    two eigenvalues of that cone's scaled product like the rows' products (k_big_corr_rhs; oracle _soc_target).  MBFIR_CORR_BIG=0
    is round 6's first form (orthant rows alone): more iterations, the same optimum.  And a lock-step unit of such designs equals
    the single solves bit for bit."""
    which, args, okw = CASES[3]
    h1, s1, i1 = mbfir.fir_qprog_phs(*args, info=True)
    z1 = solution_of(i1)
    with env(MBFIR_CORR_BIG=0):
        h0, s0, i0 = mbfir.fir_qprog_phs(*args, info=True)
        z0 = solution_of(i0)
    assert s0 == s1 == "Solved" and i1["iters"] < i0["iters"] and i1["correctors_taken"] > i0["correctors_taken"]
    same_optimum(h0, dict(i0, iters=0), h1, dict(i1, iters=0), z0, z1)
    n, f, a, d = args
    jobs = [("fir_qprog_phs", (n, f, a, [d[0] * (1 + 0.15 * q), d[1] * (1 + 0.1 * q)])) for q in range(5)]
    res = mbfir.solve_batch(jobs, streams=1, info=True, opts=mbfir.make_opts(lanes=5))
    assert res[0][2]["lanes"] == 5
    for job, (h, st, i) in zip(jobs, res):
        hs, ss, is_ = mbfir.fir_qprog_phs(*job[1], info=True)
        assert ss == st == "Solved" and is_["iters"] == i["iters"] and is_["correctors_taken"] == i["correctors_taken"] and is_["pcost"] == i["pcost"]
        assert np.array_equal(h, hs)


@pytest.mark.parametrize("which,args,okw", [CASES[0], CASES[2], ("fir_ap_cvx", (100, F6, A6, D3, 0.1, 1e-2), {})])      # (the last: 3 tiles)
def test_chunked_gram_product_of_the_row_sharded_build_equals_the_one_launch_product(which, args, okw):
    """MBFIR_AR_OVERLAP=2 runs the dense row-sharded build's form of the Gram product WITHOUT shards: the tiles in MBFIR_AR_CHUNKS
    launches, folded into the packed buffer the ranks would all-reduce chunk by chunk on the second stream, spread into T
    afterwards, border products and y-y block added as on the lattice path.  Same sums per tile up to the split of the frequency
    rows (more slices per tile: each chunk fills the chip by itself) -- the same optimum as the one-launch product."""
    fn = getattr(mbfir, which)
    h0, s0, i0 = fn(*args, info=True, opts=mbfir.make_opts(dense_trig=1))
    z0 = solution_of(i0)
    for chunks in (1, 3, 4):
        with env(MBFIR_AR_OVERLAP=2, MBFIR_AR_CHUNKS=chunks):
            h1, s1, i1 = fn(*args, info=True, opts=mbfir.make_opts(dense_trig=1))
            z1 = solution_of(i1)
        assert s0 == s1 == "Solved" and i1["lattice"] == 0
        same_optimum(h0, i0, h1, i1, z0, z1)
