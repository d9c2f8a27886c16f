"""The fused forms of the corrector's cone stages -- the trial step inside k_corr_rhs, k_corr_add inside k_dots_r (programs without a
big cone), the pick and the final step inside k_update_pick -- against the launches they replace: mbfir_test_unit_cone by default and
under MBFIR_FUSE=0 must agree bit for bit on every output and on every exported scalar except the snapshots tau0 / kap0, on every run
of cone_ref.RUNS that has a corrector.  Between them those runs pick the corrected direction and leave it, bind the corrected step at
an orthant row of the last, partly filled block, at a 3-row cone, at -dtau/tau, at -dkappa/kappa and at nothing (alpha = 1 at a zero
bound), and have a big cone (whose rows have no thread in k_dots_r: k_corr_add must still be launched, or the candidate's rows there
differ).  The fused default is held to the reference bounds of cone_ref.check_lane as tests/test_cone_gpu.py holds it."""
import numpy as np
import pytest

import cone_ref as CR
import lattice_ref as lr
import mbfir
import test_cone_gpu as T

pytestmark = pytest.mark.gpu
CORR_RUNS = T.CORR_RUNS
KEEP = [i for i, k in enumerate(mbfir.UNIT_CONE_SC) if k not in ("tau0", "kap0")]
SNAP_UPDATE = mbfir.UNIT_CONE_SNAPS.index("update")


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in T.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def bitwise(a, b, la, lb, P):
    """lane la of a and lane lb of b: every output on the lane's own rows, every exported scalar but tau0 / kap0"""
    R, N = P["R"], P["N"]
    return (np.array_equal(a["out_r"][la][:, :R], b["out_r"][lb][:, :R], equal_nan=True) and
            np.array_equal(a["out_x"][la][:, :N], b["out_x"][lb][:, :N], equal_nan=True) and
            np.array_equal(a["w3"][la][:max(P["nq3"], 1)], b["w3"][lb][:max(P["nq3"], 1)], equal_nan=True) and
            np.array_equal(a["sc"][la][:, KEEP], b["sc"][lb][:, KEEP], equal_nan=True))


def scalar(o, name, b=0, snap=SNAP_UPDATE):
    return o["sc"][b][snap][mbfir.UNIT_CONE_SC.index(name)]


def test_the_runs_cover_the_cases():
    binders = {r[2][2] for r in CORR_RUNS}
    assert {"orth", "q3", "tau", "kappa", "none", "big"} <= binders
    picks = {scalar(T.single(r), "pick") for r in CORR_RUNS}
    assert picks == {0.0, 1.0}
    # the orthant binder of c8_dup12 sits in the last block, which is partly filled
    P = T.inputs([r for r in CORR_RUNS if r[0] == "c8_dup12" and r[2][2] == "orth"][0])[0]
    assert (P["l"] + P["nq3"]) % 256 != 0 and P["l"] + P["nq3"] > 256
    # nothing binds: the corrected direction's bound is zero and its step is 1
    for r in CORR_RUNS:
        if r[2][2] == "none" and scalar(T.single(r), "pick") == 1.0:
            assert scalar(T.single(r), "tmax") == 0.0 and scalar(T.single(r), "alpha") == 1.0
    assert any(T.inputs(r)[0]["big"] for r in CORR_RUNS) and any(not T.inputs(r)[0]["big"] and T.inputs(r)[0]["nq3"] for r in CORR_RUNS)


@pytest.mark.parametrize("run", CORR_RUNS, ids=CR.run_id)
def test_fused_is_the_unfused_bit_for_bit(run, monkeypatch):
    a = T.single(run)
    assert a["report"]["fuse"] == 1 and a["report"]["form"] == 0
    monkeypatch.setenv("MBFIR_FUSE", "0")
    o = T.call([run])
    assert o["report"]["fuse"] == 0
    P = T.inputs(run)[0]
    assert np.array_equal(a["out_r"], o["out_r"], equal_nan=True) and np.array_equal(a["out_x"], o["out_x"], equal_nan=True)
    assert np.array_equal(a["w3"], o["w3"], equal_nan=True)
    assert bitwise(a, o, 0, 0, P)
    assert scalar(a, "ncorr") == 1.0 and scalar(a, "npick") == scalar(a, "pick")


@pytest.mark.parametrize("run", CORR_RUNS, ids=CR.run_id)
def test_fused_default_holds_the_reference_bounds(run):
    T.held(run, T.single(run))


def test_masked_middle_lane():
    runs = [r for r in CORR_RUNS if r[0] == "c8_dup12"][:3]
    o = T.call(runs, mask=[1, 0, 1])
    assert np.all(np.isnan(o["out_r"][1])) and np.all(np.isnan(o["out_x"][1])) and np.all(np.isnan(o["w3"][1])) and np.all(np.isnan(o["sc"][1]))
    for b in (0, 2):
        assert T.same(o, T.single(runs[b]), b, 0, T.inputs(runs[b])[0]), b
    assert {scalar(o, "pick", 0), scalar(o, "pick", 2)} == {0.0, 1.0}      # (one lane takes the corrected direction, one leaves it)


def test_heterogeneous_unit(monkeypatch):
    """the unit of two orders of tests/test_cone_gpu.py (lattice_ref.hetero_jobs): fused against unfused lane by lane, each lane its single design"""
    jobs, grid_m = lr.hetero_jobs()
    Ps = [lr.program(fn, args, grid_m) for fn, args in jobs]
    Is = []
    for b, P in enumerate(Ps):
        rng = np.random.default_rng(40 + b)
        s, z = CR.iterate(P, ("wide", "late")[b], rng)
        Is.append(CR.draw_inputs(P, s, z, rng, bind=(("orth", "q3", "tau"), ("q3", "tau", "orth"))[b], pick=("step", "guard")[b]))
    R, N, nq3 = max(P["R"] for P in Ps), max(P["N"] for P in Ps), max(P["nq3"] for P in Ps)
    opts = mbfir.make_opts(grid_m=grid_m)
    o = mbfir.test_unit_cone(jobs, *CR.pack(Is, R, N), nq3, corrector=True, opts=opts)
    assert o["report"]["hetero"] == 1 and o["report"]["fuse"] == 1
    alone = [mbfir.test_unit_cone([jobs[b]], *CR.pack([Is[b]], P["R"], P["N"]), P["nq3"], corrector=True, opts=opts) for b, P in enumerate(Ps)]
    monkeypatch.setenv("MBFIR_FUSE", "0")
    o0 = mbfir.test_unit_cone(jobs, *CR.pack(Is, R, N), nq3, corrector=True, opts=opts)
    assert o0["report"]["fuse"] == 0
    for b, P in enumerate(Ps):
        assert bitwise(o, o0, b, b, P), b
        assert T.same(o, alone[b], b, 0, P), b
