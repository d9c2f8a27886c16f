"""The cone kernels of one interior-point iteration (mbfir_test_unit_cone: the stages launch_iteration runs between its KKT solves,
at an iterate and with "solutions" the test chooses) against the high-precision reference of tests/cone_ref.py, stage by stage,
within the bounds derived there and validated on the CPU by tests/test_cone_cpu.py.  Every stage is handed the device's own earlier
outputs, so a wrong kernel fails alone; every decision (alpha = 1 at a zero bound, the caps, the corrector's projections and floor,
the pick, the shift test) must be the reference's exactly; every entry of every output of every live lane is checked, and what no
kernel writes must come back holding the sentinel it went in with.

Runs (cone_ref.RUNS): five designs -- 3-row cones in a partly filled last block, orthant only, no orthant rows with the big
cone's partial row in front, a quad program with 50 blocks, and a big cone longer than its 1024-thread workgroup -- at a well-centred
pair, at orthant weights spread over 1e8, and at a late-iteration pair (complementary, boundary gap 1e-6, s'z / degree 1e-8); the
binding term of the affine, the combined and the corrected step bound is in turn an orthant row of the last block, a 3-row cone, the
big cone, -dtau/tau, -dkappa/kappa and nothing.  No designer yields all three cone kinds at once (test_cone_cpu asserts it), so no
run has them.  pytest -s prints the worst error / bound per stage and run; DESIGN.md tabulates them.

That the tests can fail -- six arithmetic-only changes, each built apart and this file run once on it (54 tests; fractions are
error / bound; every other test passed, none faulted):
  1 (sb1 - zb1) -> (sb1 + zb1), soc3_scaling      23 fail: test_stages and test_two_phase_form on all 7 c8_dup12 and 4 c6_qp25 runs
                                                  (the designs with 3-row cones), the unit of two orders; first at scaling: lam = W^-1 s
                                                  (1e14), then affine W^-1 ds_a (1e13 .. 5e14), alpha_0, the end state
  2 1 + lb0 -> 2 + lb0, soc3_step                 11 fail: both forms of 4 c8_dup12 runs and 1 c6_qp25 run (a 3-row cone near or at the
                                                  bound), the unit of two orders; S_TMAX of the affine step and alpha_0 (1e12), the end state
  3 part + (P.big ? 2 : 0) -> part, k_dir_post    4 fail: both forms of the 2 c6_qp25 runs whose binding 3-row cone sits in block 0
                                                  (k_big_dir_post then overwrites that block's maxima): S_TMAX (4e13), the end state;
                                                  c4_qphs21 and n600 bind in the last block or the big cone and do not see it
  4 STEP / tm -> 1.0 / tm, k_update's fused branch  4 fail: test_stages on the runs without corrector whose step bound exceeds 1
                                                  (3 c6_qp25, 1 c3_lin64): alpha (5e13), the end state; form 1 does not run that branch
  5 CORR_BMIN <-> CORR_BMAX, corr_target          6 fail: both forms of 2 c4_qphs21 runs and 1 n600 run: the big cone's rows of bz_k (2e9 .. 1e12)
  6 pick ? dsk[t] : ds[t] -> ds[t], k_update_pick 15 fail: both forms of the 6 runs that pick the corrected direction, MBFIR_CORR_BIG=0,
                                                  the unit of two orders, the context test: s after the update (4e14 .. 6e15), the end state"""
import numpy as np
import pytest

import cone_ref as CR
import lattice_ref as lr
import mbfir

pytestmark = pytest.mark.gpu
RUNS = CR.RUNS
CORR_RUNS = [r for r in RUNS if r[6]]
SWITCHES = ("MBFIR_FUSE", "MBFIR_CORR_BIG", "MBFIR_CORRECTOR", "MBFIR_LANEPAIR")
_IN, _DEV = {}, {}


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def inputs(run):
    if run not in _IN:
        _IN[run] = CR.run_inputs(run)
    return _IN[run]


def call(runs, form=0, mask=None, jobs=None, progs=None, opts=None):
    """The hook on a unit whose lanes carry the inputs of `runs` (all of one design unless jobs / progs say otherwise)."""
    name = runs[0][0]
    Ps = progs or [inputs(r)[0] for r in runs]
    Is = [inputs(r)[1] for r in runs]
    R, N, nq3 = max(P["R"] for P in Ps), max(P["N"] for P in Ps), max(P["nq3"] for P in Ps)
    in_r, in_x, in_sc = CR.pack(Is, R, N)
    o = mbfir.test_unit_cone(jobs or [CR.designs()[name]["job"]] * len(runs), in_r, in_x, in_sc, nq3, form=form, corrector=runs[0][6],
                             mask=mask, opts=opts or CR.make_opts_of(name))
    assert o["report"]["lanes"] == len(runs) and o["report"]["form"] == form
    return o


def single(run, form=0):
    """one run alone on the device, once per module"""
    if (run, form) not in _DEV:
        _DEV[(run, form)] = call([run], form)
    return _DEV[(run, form)]


def same(a, b, la, lb, P):
    """lane la of result a and lane lb of result b are bit-identical on the lane's own rows (sentinels included)"""
    R, N = P["R"], P["N"]
    return (np.array_equal(a["out_r"][la][:, :R], b["out_r"][lb][:, :R], equal_nan=True) and
            np.array_equal(a["out_x"][la][:, :N], b["out_x"][lb][:, :N], equal_nan=True) and
            np.array_equal(a["w3"][la][:max(P["nq3"], 1)], b["w3"][lb][:max(P["nq3"], 1)], equal_nan=True) and
            np.array_equal(a["sc"][la], b["sc"][lb], equal_nan=True))


def held(run, o, b=0, form=0, corr_big=True, P=None, I=None):
    if P is None:
        P, I = inputs(run)
    D = CR.unpack(o, b, P)
    rec, facts = CR.check_lane(P, I, D, run[6], corr_big=corr_big)
    if corr_big:
        CR.check_end_to_end(P, I, D, run[6], rec, facts)
    print("\n%-50s %s" % (CR.run_id(run) + (" form 1" if form else ""), "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.over(), rec.over()
    assert not rec.failed, rec.failed
    assert not CR.untouched(P, D, run[6], form), CR.untouched(P, D, run[6], form)
    return rec, facts


@pytest.mark.parametrize("run", RUNS, ids=CR.run_id)
def test_stages(run):
    o = single(run)
    P = inputs(run)[0]
    rep = o["report"]
    assert (rep["l"], rep["nq3"], rep["big"], rep["N"], rep["R"]) == (P["l"], P["nq3"], P["big"], P["N"], P["R"])
    blocks = max(1, -(-(P["l"] + P["nq3"]) // 256))
    assert rep["cone_blocks"] == blocks and rep["ns_affine"] == rep["ns_combined"] == blocks + (1 if P["big"] else 0)
    assert rep["fuse"] == 1 and rep["corr_big"] == 1 and rep["hetero"] == 0
    held(run, o)


@pytest.mark.parametrize("run", RUNS, ids=CR.run_id)
def test_two_phase_form(run):
    """form = 1: k_scal_dtau / k_scal_step in phases 0 and 1 (the kernels of a row-sharded solve) on one rank.  Same bounds, the same
    decisions; the maxima are bit-identical, the sums are folded by another thread count."""
    a, b = single(run), single(run, 1)
    held(run, b, form=1)
    sa, sb = a["sc"][0], b["sc"][0]
    names = mbfir.UNIT_CONE_SC
    for snap in ("comb_rhs", "corr_rhs", "update"):
        i = mbfir.UNIT_CONE_SNAPS.index(snap)
        if np.isnan(sa[i][0]):
            continue
        # S_TMAX is a maximum of per-row values that depend on the folded sums only through dtau; where dtau agrees to the bit so does it
        for k in ("pick", "ncorr", "npick"):
            assert sa[i][names.index(k)] == sb[i][names.index(k)], (snap, k)
        same_dtau = all(sa[i][names.index(k)] == sb[i][names.index(k)] for k in ("dtau_a", "dtau", "dtau_c"))
        if same_dtau:
            assert sa[i][names.index("tmax")] == sb[i][names.index("tmax")], snap
    i = mbfir.UNIT_CONE_SNAPS.index("shift")
    assert sa[i][names.index("rb0")] == sb[i][names.index("rb0")]
    # phase 0 leaves the folded maxima in RB, the identity all-reduce leaves them there: the last step's maxima
    i = mbfir.UNIT_CONE_SNAPS.index("update")
    assert max(0.0, sb[i][names.index("rb0")], sb[i][names.index("rb1")]) <= sb[i][names.index("tmax")]


@pytest.mark.parametrize("run", [RUNS[0], RUNS[5], RUNS[14], RUNS[17]], ids=CR.run_id)
def test_fuse_off_is_bit_identical(run, monkeypatch):
    """MBFIR_FUSE=0 (the step length by k_scal_step instead of inside k_update) changes no bit."""
    monkeypatch.setenv("MBFIR_FUSE", "0")
    o = call([run])
    assert o["report"]["fuse"] == 0
    P = inputs(run)[0]
    a = single(run)
    keep = [i for i, k in enumerate(mbfir.UNIT_CONE_SC) if k not in ("tau0", "kap0")]      # (the snapshot only the fused update reads)
    assert np.array_equal(a["out_r"], o["out_r"], equal_nan=True) and np.array_equal(a["out_x"], o["out_x"], equal_nan=True)
    assert np.array_equal(a["w3"], o["w3"], equal_nan=True) and np.array_equal(a["sc"][0][:, keep], o["sc"][0][:, keep], equal_nan=True)
    assert P["R"] == o["report"]["R"]


@pytest.mark.parametrize("run", [r for r in CORR_RUNS if r[0] in ("c4_qphs21", "n600")][:3], ids=CR.run_id)
def test_corr_big_off(run, monkeypatch):
    """MBFIR_CORR_BIG=0: the big cone's rows of the corrector's right-hand side are exact zeros; everything else as before."""
    monkeypatch.setenv("MBFIR_CORR_BIG", "0")
    o = call([run])
    assert o["report"]["corr_big"] == 0
    held(run, o, corr_big=False)


@pytest.mark.parametrize("name,nl", [("c8_dup12", 2), ("c8_dup12", 4), ("c4_qphs21", 3), ("c3_lin64", 2)])
def test_lanes_are_their_single_runs(name, nl):
    """2 - 4 lanes of one design, every lane with its own iterate and directions: each is bit-identical to the same lane alone."""
    runs = [r for r in CORR_RUNS if r[0] == name][:nl]
    assert len(runs) == nl
    o = call(runs)
    for b, r in enumerate(runs):
        assert same(o, single(r), b, 0, inputs(r)[0]), (name, b)


def test_masked_lane_keeps_its_sentinels():
    runs = [r for r in CORR_RUNS if r[0] == "c8_dup12"][:3]
    o = call(runs, mask=[1, 0, 1])
    assert np.all(np.isnan(o["out_r"][1])) and np.all(np.isnan(o["out_x"][1])) and np.all(np.isnan(o["w3"][1])) and np.all(np.isnan(o["sc"][1]))
    for b in (0, 2):
        assert same(o, single(runs[b]), b, 0, inputs(runs[b])[0]), b


def test_heterogeneous_unit():
    """two orders in one unit (lattice_ref.hetero_jobs): per-lane dimensions and block counts; each lane is held to the reference
    and is bit-identical to its single design."""
    jobs, grid_m = lr.hetero_jobs()
    Ps = [lr.program(fn, args, grid_m) for fn, args in jobs]
    assert Ps[0]["R"] != Ps[1]["R"] and Ps[0]["N"] != Ps[1]["N"]
    run = ("hetero", "wide", ("orth", "q3", "tau"), "step", 3.0, "outside", True)
    Is = []
    for b, P in enumerate(Ps):
        rng = np.random.default_rng(40 + b)
        s, z = CR.iterate(P, ("wide", "late")[b], rng)
        Is.append(CR.draw_inputs(P, s, z, rng, bind=(("orth", "q3", "tau"), ("q3", "tau", "orth"))[b], pick=("step", "guard")[b]))
    R, N, nq3 = max(P["R"] for P in Ps), max(P["N"] for P in Ps), max(P["nq3"] for P in Ps)
    opts = mbfir.make_opts(grid_m=grid_m)
    o = mbfir.test_unit_cone(jobs, *CR.pack(Is, R, N), nq3, corrector=True, opts=opts)
    assert o["report"]["hetero"] == 1 and o["report"]["lanes"] == 2
    for b, P in enumerate(Ps):
        held(run, o, b=b, P=P, I=Is[b])
        alone = mbfir.test_unit_cone([jobs[b]], *CR.pack([Is[b]], P["R"], P["N"]), P["nq3"], corrector=True, opts=opts)
        assert alone["report"]["hetero"] == 0
        assert same(o, alone, b, 0, P), b
        # past the lane's own rows: the sentinel, or -- the blocks updated in place -- the zero padding of the input
        inplace_r = [mbfir.UNIT_CONE_OUT_R.index(k) for k in ("kzsum", "kgsum", "s", "z", "shift")]
        rest_r = [i for i in range(len(mbfir.UNIT_CONE_OUT_R)) if i not in inplace_r and mbfir.UNIT_CONE_OUT_R[i] != "wbb"]
        assert np.all(np.isnan(o["out_r"][b][rest_r][:, P["R"]:])) and np.all(o["out_r"][b][inplace_r][:, P["R"]:] == 0.0)
        assert np.all(np.isnan(o["out_x"][b][0, P["N"]:])) and np.all(o["out_x"][b][1:, P["N"]:] == 0.0)


def test_refused_units_and_the_context_after():
    run = RUNS[0]
    P, I = inputs(run)
    a = CR.pack([I], P["R"], P["N"])
    with pytest.raises(ValueError, match="row-sharded"):
        mbfir.test_unit_cone([CR.designs()["c8_dup12"]["job"]], *a, P["nq3"], opts=mbfir.make_opts(shard_size=2))
    run6 = [r for r in RUNS if r[0] == "c6_qp25"][0]
    P6, I6 = inputs(run6)
    with pytest.raises(ValueError, match="extended-precision"):
        mbfir.test_unit_cone([CR.designs()["c6_qp25"]["job"]], *CR.pack([I6], P6["R"], P6["N"]), P6["nq3"])
    with pytest.raises(ValueError, match="form"):
        mbfir.test_unit_cone([CR.designs()["c8_dup12"]["job"]], *a, P["nq3"], form=2)
    # the context still solves, and the hook after a solve gives what it gave before
    fn, args = CR.designs()["c8_dup12"]["job"]
    h, status = getattr(mbfir, fn)(*args)
    assert status == "Solved" and len(h) == args[0]
    assert same(call([run]), single(run), 0, 0, P)
