"""k_fold_cg_start<2> with one workgroup per vector (grid (2, 1, lanes)) against the launches it stands for: a two-vector plain KKT
solve (mbfir_test_unit_kkt) by default and under MBFIR_FUSE=0 -- k_hsolve_fold + k_cg_start, one workgroup, the vectors one after the
other -- must agree bit for bit on everything but the z blocks only the unfused form writes: p, H p, dx, r, G p, W^-2 G p, gdx, dz of
every sweep, the end state, and every scalar snapshot (the residual norms n_0 .., rz and alpha of both vectors).
np = 64 (c8_dup12: every thread past np folds zeros) and np = 320 (c2_ap150: not a multiple of 256, N > SCAL_T), 2 and 3 sweeps (one
restart and two), one design and a unit of three lanes whose middle lane needs fewer sweeps (its mask row switches it off for the last
restarts while both workgroups of the others go on)."""
import numpy as np
import pytest

import kkt_ref as K
import mbfir
import test_kkt_gpu as T

pytestmark = pytest.mark.gpu
RUNS = [r for r in K.RUNS if r[0] in ("c8_dup12", "c2_ap150") and r[2] == "own" and r[3] == 2 and r[1] == "centred"]
NP = {"c8_dup12": 64, "c2_ap150": 320}
ZS = [i for i, k in enumerate(mbfir.UNIT_KKT_OUT_X) if k[0] == "z"]
KEEP_X = [i for i in range(len(mbfir.UNIT_KKT_OUT_X)) if i not in ZS]


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in T.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def equal_but_z(a, o, b):
    bad = T.same(a, o, b, b, skip=("out_x",))
    if not np.array_equal(a["out_x"][b][KEEP_X], o["out_x"][b][KEEP_X], equal_nan=True):
        bad.append("out_x")
    return bad


def test_the_runs_are_the_sizes():
    assert sorted(r[0] for r in RUNS) == ["c2_ap150", "c8_dup12"]
    for r in RUNS:
        rep = T.single(r, 2)["report"]
        assert rep["np"] == NP[r[0]] and rep["nv"] == 2 and rep["fused_hsolve"] == 1 and rep["fuse"] == 1 and rep["two"] == 0
    assert NP["c2_ap150"] % 256 != 0


@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("run", RUNS, ids=K.run_id)
def test_one_design(run, ns, monkeypatch):
    a = T.single(run, ns)
    monkeypatch.setenv("MBFIR_FUSE", "0")
    o = T.call([(run, 0)], [ns])
    assert o["report"]["fuse"] == 0 and a["report"]["fuse"] == 1
    assert not equal_but_z(a, o, 0)
    # the sweeps ran: both vectors' rz of every start and the norms n_0 .. n_ns are numbers, the slots past them sentinels
    sc, names = a["sc"][0], mbfir.UNIT_KKT_SC
    end = mbfir.UNIT_KKT_SNAPS.index("end")
    assert np.all(np.isfinite(sc[end][:ns + 1])) and np.all(np.isnan(sc[end][ns + 1:9]))
    for q in range(ns):
        st = mbfir.UNIT_KKT_SNAPS.index("start%d" % q)
        assert np.isfinite(sc[st][names.index("rz0")]) and np.isfinite(sc[st][names.index("rz1")])


@pytest.mark.parametrize("run", RUNS, ids=K.run_id)
def test_unit_of_three_with_a_shorter_lane(run, monkeypatch):
    counts = [3, 1, 2]
    lanes = [(run, b) for b in range(3)]
    a = T.call(lanes, counts)
    for b, n in enumerate(counts):
        assert not T.same(a, T.single(run, n, seed=b), b, 0), (b, n)
    monkeypatch.setenv("MBFIR_FUSE", "0")
    o = T.call(lanes, counts)
    assert o["report"]["fuse"] == 0
    for b in range(3):
        assert not equal_but_z(a, o, b), b
