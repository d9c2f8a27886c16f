"""The plain KKT solve of an iteration and the residual kernels in front of it (mbfir_test_unit_kkt: launch_residuals, the NT
scaling, build_H, then Impl::kkt_solve -- or initial_point -- with an observer that reads every group of launches back) against the
high-precision reference of tests/kkt_ref.py, group by group, within the bounds derived there and validated on the CPU by
tests/test_kkt_cpu.py.  Every group is handed the device's own earlier outputs, so a wrong kernel fails alone; every entry of every
output of every live lane is checked; what no launch of a lane writes must come back holding the sentinel it went in with.

Runs (kkt_ref.RUNS): eight designs -- c8_dup12 (Nt <= 32: k_gt_finish's shortest hand-over, two workgroups; 3-row cones, duplicate
frequencies), c2_ap150 (several column workgroups; N > SCAL_T: a second pass of every strided loop; three evaluation segments),
c3_lin64 (orthant only), c4_qphs21 (quad program, big cone: k_big_winv2 on the wbz_ready entry), c6_qp25 with ddkkt = -1 (3-row cones
and a big cone, no orthant rows), c1_ap24 with dense_trig (the Gx form of k_resid_rows, the dense operators), fir_ap_cvx at n = 512
(np = 1024: the largest the one-pass M'(M b) and the 1024-thread k_fold_cg_start take, the benchmark unit's size) and fir_qprog_phs at
n = 512 (np = 1088: the two triangular products by size, k_cg_start), each on the smallest grid its designer takes -- at centred, wide and
late iterates, with the iteration's own right-hand sides (-c, -rx), (h, s - rz) taken from the residual kernels' output, random ones
(nv = 1 and 2) and an all-zero second column, each at 0, 1, 3 and 8 sweeps.  pytest -s prints the worst error / bound per stage.

Bit-identities asserted: the two forms of the residual kernels (phase 2 against phases 0 + 1: both fold with SCAL_T threads in one
order, so every vector and every scalar agrees to the bit); MBFIR_FUSE=0 against the default, stage for stage (the code says so:
k_resid_norm forms gt_resid_tail's sums in its order, k_cg_start those of k_fold_cg_start); every lane of a unit against the same
lane alone with its own sweep count.  MBFIR_HSOLVE=0 (two triangular products instead of the one-pass M'(M b)) sums in another
order: held to the reference, not to the default's bits.

That the tests can fail -- seven arithmetic-only changes, each built apart and this file run once on it (101 tests; fractions are
error / bound; every other test passed, none faulted):
  1 S_CG_ALPHA + q -> S_CG_ALPHA, k_cg_update_r       1 fails: test_sharded_cg_form_on_one_rank on n512_qphs, group 8: dz (100), gdx (3).
                                                      On every other run alpha is 1 within 4e-14 for both vectors and a sweep's
                                                      correction is 1e-12 of gdx: the other vector's alpha moves no bit there
  2 r - alpha Hp -> r + alpha Hp, k_cg_step_update    75 fail: every run with a sweep in test_stages (48), the two-phase form, both
                                                      switches, the units, the initial point: group 8, r (2e16); the two-launch form
                                                      runs k_cg_step and passes
  3 slot + it + 1 -> slot + it, kkt_solve             the same 75: group 8, n_1 .. (the slot keeps its sentinel), n_0 overwritten,
                                                      ||bx - G'dz|| = n_last
  4 p = z + beta p without the `first` test,          71 fail: every run with a sweep on the fused form (MBFIR_FUSE=0 and np = 1088
    k_fold_cg_start                                   run k_cg_start and pass): group 5, p = z (the sentinel p went in with), then
                                                      everything behind it
  5 hz < 0 -> hz > 0 in S_PINF, k_scal_resid          96 fail: every test that checks the residual kernels: pinf = 1e300 on the 15
                                                      runs with h'z > 0, its value on the run with h'z < 0
  6 mask_row(it + 2) -> mask_row(it + 1), kkt_solve   6 fail: the four units with unequal sweep counts, the unit with a masked lane
                                                      and the unit of two orders: S_CG_RZ at the end is not what the lane's own last
                                                      start left (a lane restarts once more than it sweeps); single designs pass
  7 bz2[1] = s - rz -> s + rz, k_resid_rows           96 fail: every test that checks the residual kernels: bz2[1] = fl(s - rz)"""
import numpy as np
import pytest

import kkt_ref as K
import lattice_ref as lr
import mbfir

pytestmark = pytest.mark.gpu
RUNS = K.RUNS
SWITCHES = ("MBFIR_FUSE", "MBFIR_HSOLVE", "MBFIR_LANEPAIR")
_IN, _DEV, _TWIN = {}, {}, {}
BLOCKS = ("res_r", "res_x", "res_sc", "M", "out_x", "out_r", "sc")


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def inputs(run, seed=0):
    if (run, seed) not in _IN:
        _IN[(run, seed)] = K.run_inputs(run, seed)
    return _IN[(run, seed)]


def call(lanes, ns, mask=None, **kw):
    """The hook on a unit whose lanes are (run, seed) pairs of one design, nv and entry."""
    run = lanes[0][0]
    Is = [inputs(*ln)[1] for ln in lanes]
    P = inputs(*lanes[0])[0]
    own = run[2] == "own"
    o = mbfir.test_unit_kkt([K.designs()[run[0]]["job"]] * len(lanes), np.stack([I["s"] for I in Is]), np.stack([I["z"] for I in Is]),
                            np.stack([I["x"] for I in Is]), np.array([[I["tau"], I["kappa"]] for I in Is]), ns, P["nq3"],
                            bx=None if own else np.stack([I["bx"] for I in Is]), bz=None if own else np.stack([I["bz"] for I in Is]),
                            nv=run[3], wbz_ready=run[4], mask=mask, opts=kw.pop("opts", None) or K.make_opts_of(run[0]), **kw)
    live = [n for b, n in enumerate(ns) if mask is None or mask[b]]
    assert o["report"]["lanes"] == len(lanes) and o["report"]["nv"] == run[3] and o["report"]["nsweep_max"] == max(live)
    return o


def single(run, ns, seed=0, form=0):
    """one run alone on the device, once per module"""
    key = (run, ns, seed, form)
    if key not in _DEV:
        _DEV[key] = call([(run, seed)], [ns], form=form)
    return _DEV[key]


def twin_sc(run, D, bx, bz, seed=0):
    """the float64 twin's norms of a run (8 sweeps contain the shorter solves), once per module"""
    if (run, seed) not in _TWIN:
        P, I = inputs(run, seed)
        Gm = K.model_G(P, bool(K.designs()[run[0]].get("dense")))
        Wm = K.oracle_scaling(P, I["s"], I["z"])
        M, Lc = K.factor64(P, Gm, Wm)
        _TWIN[(run, seed)] = K.twin(P, Gm, Wm, M, bx, bz, 8)["sc"]
    return _TWIN[(run, seed)]


def same(a, b, la, lb, skip=()):
    """lane la of result a and lane lb of result b are bit-identical (sentinels included)"""
    return [k for k in BLOCKS if k not in skip and not np.array_equal(a[k][la], b[k][lb], equal_nan=True)]


def held(run, o, ns, b=0, seed=0, form=0, tag="", P=None, I=None, sentinel=np.nan, refine=True):
    if P is None:
        P, I = inputs(run, seed)
    nv, rep = run[3], o["report"]
    D = K.unpack(o, b, P, nv)
    O = K.ops_of(run, I) if run[0] in K.designs() else K.Ops(P, I["s"], I["z"])
    assert D["flag"] == 0, "pivots replaced: the factor is not the one of H"
    rec, rf = K.check_residuals(P, O, D, I, form, sentinel=sentinel)
    bx, bz = K.rhs_of(run, I, D["res"])
    rec, facts = K.check_solve(P, O, D, bx, bz, ns, nv, bool(rep["z_written"]), rec, sentinel)
    print("\n%-44s %s" % (K.run_id(run) + " ns %d%s" % (ns, tag), "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.over(), rec.over()
    assert not rec.failed, rec.failed
    assert not facts["undecided"], facts["undecided"]
    bad = K.untouched(P, D, ns, nv, bool(rep["z_written"]), sentinel)
    assert not bad, bad
    if refine:
        worse = K.refines(facts, twin_sc(run, D, bx, bz, seed), ns)
        assert not worse, worse
    if run[2] == "zero":        # the all-zero column comes back all zero: alpha = beta = 0 in every sweep and no NaN
        for k in list(mbfir.UNIT_KKT_OUT_X) + list(mbfir.UNIT_KKT_OUT_R):
            q = int(k[-1]) if k[-1].isdigit() else -1
            if q < ns and not (k[0] == "z" and not rep["z_written"]):
                assert np.all(D[k][1] == 0.0), k
        assert all(D["sc"]["step%d" % q]["alpha1"] == 0.0 and D["sc"]["start%d" % q]["rz1"] == 0.0 for q in range(ns))
        assert facts["pHp_pos"][1::2] == [False] * ns and facts["beta_zero"][1::2] == [True] * max(ns - 1, 0)
    return rec, facts


def check_report(run, rep, form=0, fuse=1, hsolve=1, two=0):
    P = K.program_of(run[0])
    hsolve = hsolve if -(-P["N"] // 64) * 64 <= 1024 else 0            # (past np = 1024: the two triangular products)
    dense = bool(K.designs()[run[0]].get("dense"))
    assert (rep["N"], rep["R"], rep["np"], rep["big"], rep["l"], rep["nq3"]) == (P["N"], P["R"], -(-P["N"] // 64) * 64, P["big"], P["l"], P["nq3"])
    assert rep["fused_hsolve"] == hsolve and rep["fuse"] == fuse and rep["form"] == form and rep["two"] == two
    assert rep["lattice"] == (0 if dense else 1) and rep["hetero"] == 0 and rep["initial"] == 0 and rep["wbz_ready"] == int(run[4])
    assert rep["gt_finish_blocks"] == -(-P["Nt"] // 32) + 1 and rep["z_written"] == (0 if fuse and hsolve else 1)
    assert rep["resid_blocks"] >= -(-P["R"] // 256)


@pytest.mark.parametrize("ns", K.SWEEPS)
@pytest.mark.parametrize("run", RUNS, ids=K.run_id)
def test_stages(run, ns):
    o = single(run, ns)
    check_report(run, o["report"])
    # the passes: the residual kernels' G x and G'z; the solve's 2 + 2 and two per sweep
    if not K.designs()[run[0]].get("dense"):
        assert o["report"]["gtv_passes"] == 1 + 2 + ns
    held(run, o, ns)


@pytest.mark.parametrize("run", [r for r in RUNS if r[2] == "own"], ids=K.run_id)
def test_residual_kernels_two_phase_form(run):
    """form = 1: k_scal_resid in phases 0 and 1 (the kernels of a row-sharded solve, the mailbox behind G'z) on one rank.  The same
    bounds, the same decisions; both forms fold the row partials and the columns with SCAL_T threads in one order, so every vector
    and every one of the scalars is bit-identical -- only the mailbox differs, which form 0 does not write."""
    a, b = single(run, 1), single(run, 1, form=1)
    check_report(run, b["report"], form=1)
    held(run, b, 1, form=1, tag=" form 1")
    assert not same(a, b, 0, 0, skip=("res_sc",))
    assert np.array_equal(a["res_sc"][0][:19], b["res_sc"][0][:19])
    P, I = inputs(run)
    f = K.check_residuals(P, K.ops_of(run, I), K.unpack(b, 0, P, run[3]), I, 1)[1]
    assert f["hz_neg"] == run[5] and f["hz_margin"] >= 1e-3 and f["cx_margin"] >= 1e-3


def test_residual_decisions_on_both_sides():
    got = set()
    for run in RUNS:
        P, I = inputs(run)
        f = K.check_residuals(P, K.ops_of(run, I), K.unpack(single(run, 1), 0, P, run[3]), I, 0)[1]
        got.add((f["hz_neg"], f["cx_neg"]))
    assert {g[0] for g in got} == {True, False} and {g[1] for g in got} == {True, False}


@pytest.mark.parametrize("switch", ["MBFIR_FUSE", "MBFIR_HSOLVE"])
@pytest.mark.parametrize("run", [RUNS[0], RUNS[1], RUNS[3], RUNS[4], RUNS[5]], ids=K.run_id)
def test_switches(run, switch, monkeypatch):
    monkeypatch.setenv(switch, "0")
    ns = 3
    o = call([(run, 0)], [ns])
    check_report(run, o["report"], fuse=0 if switch == "MBFIR_FUSE" else 1, hsolve=0 if switch == "MBFIR_HSOLVE" else 1)
    held(run, o, ns, tag=" %s=0" % switch)
    if switch == "MBFIR_FUSE":
        # stage for stage the default's bits: k_resid_norm against the tail fused into k_gt_finish, k_hsolve_fold + k_cg_start against
        # k_fold_cg_start; z is the one block only this form writes, and p of the first start is that z
        a = single(run, ns)
        zs = [i for i, k in enumerate(mbfir.UNIT_KKT_OUT_X) if k[0] == "z"]
        keep = [i for i in range(len(mbfir.UNIT_KKT_OUT_X)) if i not in zs]
        assert not same(a, o, 0, 0, skip=("out_x",))
        assert np.array_equal(a["out_x"][0][keep], o["out_x"][0][keep], equal_nan=True)
        assert np.all(np.isnan(a["out_x"][0][zs])) and np.array_equal(o["out_x"][0][zs[0]], o["out_x"][0][zs[0] - 1], equal_nan=True)


@pytest.mark.parametrize("run", [RUNS[0], RUNS[1], RUNS[2], RUNS[5], RUNS[7], RUNS[8], RUNS[15]], ids=K.run_id)
def test_sharded_cg_form_on_one_rank(run):
    """two = 1: the sweep's update by k_cg_step + k_cg_update_r, the two launches of a row-sharded solve."""
    ns = 3
    o = call([(run, 0)], [ns], two=True)
    check_report(run, o["report"], two=1)
    rec, facts = held(run, o, ns, tag=" two launches")
    sc = K.unpack(o, 0, K.program_of(run[0]), run[3])["sc"]
    print("alpha of the vectors, sweep by sweep:", [(sc["step%d" % q]["alpha0"], sc["step%d" % q]["alpha1"]) for q in range(ns)])


@pytest.mark.parametrize("run,counts", [(RUNS[0], [0, 3, 1, 8]), (RUNS[3], [2, 0, 8]), (RUNS[8], [1, 3, 0]), (RUNS[2], [8, 1])], ids=lambda v: K.run_id(v) if isinstance(v, tuple) else "-".join(map(str, v)))
def test_lanes_are_their_single_runs(run, counts):
    """several lanes of one design, every lane its own iterate, right-hand sides and sweep count: each is bit-identical to the same
    lane alone with its own count -- so the blocks of the sweeps it does not run and its norm slots past its count hold their
    sentinels, as the single run's do -- and is held to the reference."""
    lanes = [(run, b) for b in range(len(counts))]
    o = call(lanes, counts)
    for b, n in enumerate(counts):
        assert not same(o, single(run, n, seed=b), b, 0), (b, n)
        held(run, o, n, b=b, seed=b, tag=" lane %d" % b)


def test_masked_lane_keeps_everything():
    run, counts = RUNS[0], [3, 8, 1]
    o = call([(run, b) for b in range(3)], counts, mask=[1, 0, 1])
    assert o["report"]["nsweep_max"] == 3
    for k in BLOCKS:
        assert np.all(np.isnan(o[k][1])), k
    assert o["flag"][1] == -1
    for b in (0, 2):
        assert not same(o, single(run, counts[b], seed=b), b, 0), b


def test_heterogeneous_unit():
    """two orders in one unit (lattice_ref.hetero_jobs): per-lane dimensions; each lane is held to the reference, is bit-identical to
    its single design, and returns the sentinel past its own N / R.  (A finite sentinel: M'(M b) reads its operand over all np
    entries, where a shorter lane's G'v leaves the sentinel; its factor is the identity there, and 0 x NaN would not be 0.)"""
    jobs, grid_m = lr.hetero_jobs()
    Ps = [lr.program(fn, args, grid_m) for fn, args in jobs]
    assert Ps[0]["R"] != Ps[1]["R"] and Ps[0]["N"] != Ps[1]["N"] and -(-Ps[0]["N"] // 64) == -(-Ps[1]["N"] // 64)
    run = ("hetero", "wide", "own", 2, True, False)
    sent, counts = -7.25e77, [3, 1]
    Is = []
    for b, P in enumerate(Ps):
        rng = np.random.default_rng(70 + b)
        s, z = K.CR.iterate(P, ("wide", "late")[b], rng)
        Is.append(dict(s=s, z=z, x=rng.standard_normal(P["N"]), tau=1.25, kappa=0.5))

    def pad(v, n):
        return np.concatenate([v, np.zeros(n - len(v))])

    def go(bs):
        R, N, nq3 = max(Ps[b]["R"] for b in bs), max(Ps[b]["N"] for b in bs), max(Ps[b]["nq3"] for b in bs)
        return mbfir.test_unit_kkt([jobs[b] for b in bs], np.stack([pad(Is[b]["s"], R) for b in bs]), np.stack([pad(Is[b]["z"], R) for b in bs]),
                                   np.stack([pad(Is[b]["x"], N) for b in bs]), np.array([[Is[b]["tau"], Is[b]["kappa"]] for b in bs]),
                                   [counts[b] for b in bs], nq3, wbz_ready=True, opts=mbfir.make_opts(grid_m=grid_m), sentinel=sent)
    o = go([0, 1])
    assert o["report"]["hetero"] == 1 and o["report"]["lanes"] == 2
    for b, P in enumerate(Ps):
        held(run, o, counts[b], b=b, P=P, I=Is[b], sentinel=sent, refine=False, tag=" lane %d" % b)
        alone = go([b])
        assert alone["report"]["hetero"] == 0
        n, r = P["N"], P["R"]
        npd = -(-n // 64) * 64
        assert np.array_equal(o["out_x"][b][..., :n], alone["out_x"][0][..., :n]) and np.array_equal(o["out_r"][b][..., :r], alone["out_r"][0][..., :r])
        assert np.array_equal(o["sc"][b], alone["sc"][0]) and np.array_equal(o["res_sc"][b], alone["res_sc"][0])
        assert np.array_equal(o["M"][b][:npd, :npd], alone["M"][0][:npd, :npd])


@pytest.mark.parametrize("name", ["c8_dup12", "c4_qphs21", "c6_qp25"])
def test_initial_point(name):
    """mode = initial: k_unit_scaling, k_init_rhs, the solve from the winv2 entry with W = I, the copies and the cone shifts."""
    run = (name, "centred", "own", 2, False, False)
    P, I = inputs(run)
    ns = 3
    o = mbfir.test_unit_kkt([K.designs()[name]["job"]], I["s"][None], I["z"][None], I["x"][None], np.array([[I["tau"], I["kappa"]]]), [ns],
                            P["nq3"], initial=True, opts=K.make_opts_of(name))
    assert o["report"]["initial"] == 1 and o["report"]["wbz_ready"] == 0
    D = K.unpack(o, 0, P, 2)
    ini, l = D["init"], P["l"]
    zN, zR = np.zeros(P["N"]), np.zeros(P["R"])
    assert np.array_equal(ini["ibx2a"], zN) and np.array_equal(ini["ibx2b"], -P["c"]) and np.array_equal(ini["bz2a"], P["h"]) and np.array_equal(ini["bz2b"], zR)
    assert np.all(ini["dl"][:l] == 1.0) and np.all(ini["wl"][:l] == 1.0) and np.all(np.isnan(ini["dl"][l:])) and np.all(np.isnan(ini["wl"][l:]))
    if P["nq3"]:
        assert np.array_equal(ini["w3"][:P["nq3"]], np.tile([1.0, 1.0, 0.0, 0.0], (P["nq3"], 1)))
    if P["big"]:
        assert ini["wbb"][0] == 1.0 and np.all(ini["wbb"][1:P["big"]] == 0.0)
    O = K.Ops(P, None, None, dense=bool(K.designs()[name].get("dense")), unit=True)
    bx, bz = np.stack([zN, -P["c"]]), np.stack([P["h"], zR])
    rec, facts = K.check_solve(P, O, D, bx, bz, ns, 2, bool(o["report"]["z_written"]))
    assert not K.untouched(P, D, ns, 2, bool(o["report"]["z_written"]))
    # x, s, z: the solve's dx2[0], and -dz2[0], dz2[1] through the cone shift
    rec.exact("init", "x = dx2[0]", np.array_equal(ini["x_x"], D["dx_end"][0]))
    K.check_shift(P, -D["dz_end"][0], ini["s"], rec, "s")
    K.check_shift(P, D["dz_end"][1], ini["z"], rec, "z")
    print("\n%-44s %s" % (name + " initial point", "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.over(), rec.over()
    assert not rec.failed, rec.failed


def test_refused_units_and_the_context_after():
    run = RUNS[0]
    P, I = inputs(run)
    a = (I["s"][None], I["z"][None], I["x"][None], np.array([[I["tau"], I["kappa"]]]))
    job = K.designs()["c8_dup12"]["job"]
    with pytest.raises(ValueError, match="row-sharded"):
        mbfir.test_unit_kkt([job], *a, [1], P["nq3"], opts=mbfir.make_opts(shard_size=2))
    P6, I6 = inputs(RUNS[10])
    with pytest.raises(ValueError, match="extended-precision"):
        mbfir.test_unit_kkt([K.designs()["c6_qp25"]["job"]], I6["s"][None], I6["z"][None], I6["x"][None], np.array([[1.0, 1.0]]), [1], P6["nq3"])
    with pytest.raises(ValueError, match="form"):
        mbfir.test_unit_kkt([job], *a, [1], P["nq3"], form=2)
    with pytest.raises(ValueError, match="sweep count"):
        mbfir.test_unit_kkt([job], *a, [9], P["nq3"])
    with pytest.raises(ValueError, match="wbz_ready"):
        mbfir.test_unit_kkt([job], *a, [1], P["nq3"], nv=1, wbz_ready=True, bx=np.zeros((1, 1, P["N"])), bz=np.zeros((1, 1, P["R"])))
    # the context still solves, and the hook after a solve gives what it gave before
    fn, args = job
    h, status = getattr(mbfir, fn)(*args)
    assert status == "Solved" and len(h) == args[0]
    assert not same(call([(run, 0)], [3]), single(run, 3), 0, 0)
