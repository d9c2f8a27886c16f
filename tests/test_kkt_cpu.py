"""The reference and the bounds of tests/kkt_ref.py, checked without a GPU on every run tests/test_kkt_gpu.py uses:
  - the float64 twin of kkt_solve and of the residual kernels (kkt_ref.twin, twin_residuals: NumPy on lattice_ref's float64 model of
    the lattice products, the oracle's float64 NT scaling, an explicit M = L^-1 of the padded H) stays inside every bound with a
    margin of 4, at 8 sweeps (which contain the shorter solves) and with z read back; pytest -s prints the ratios;
  - every decision of the runs has both outcomes: h'z and c'x on either side of zero with a margin of 1e-3 sum |.|, so that the
    reference's sign is not in doubt; p'Hp <= 0 reached through an all-zero column, p'Hp > 0 everywhere else; beta = 0 at rz_old = 0;
  - the spread of the twin's norms n_q under two summation orders and the two preconditioner forms, which sets kkt_ref.FACTOR;
  - the sentinel and masking rules on a NumPy stand-in of the hook's output layout: a unit with sweep counts [0, 3, 1, 8] and a masked
    lane passes kkt_ref.untouched, and a write past a lane's count, a z in the fused form or a second vector at nv = 1 is reported.

Measured over the 16 runs (worst twin error / bound; pytest -s prints every run): 0.24 at group 0 (the orthant's two roundings against
8 u), below 0.25 at groups 1 - 7 and at the end, 0.999 at groups 8 and 9 and 0.97 at the residual kernels, all three on bounds
that count roundings (kkt_ref.COUNTED); the spread of the norms is 1.000 (kkt_ref's docstring says why)."""
import numpy as np
import pytest

import kkt_ref as K
import mbfir

RUNS = K.RUNS
_RES = {}


def result(run, ns=8, order="device", precond="M"):
    key = (run, ns, order, precond)
    if key not in _RES:
        P, I = K.run_inputs(run)
        dense = bool(K.designs()[run[0]].get("dense"))
        Gm = K.model_G(P, dense)
        Wm = K.oracle_scaling(P, I["s"], I["z"])
        M, Lc = K.factor64(P, Gm, Wm)
        res = K.twin_residuals(P, Gm, I, 0)
        bx, bz = K.rhs_of(run, I, res)
        D = K.twin(P, Gm, Wm, M, bx, bz, ns, order, precond, Lc)
        D["res"] = res
        _RES[key] = (P, I, D, bx, bz)
    return _RES[key]


@pytest.mark.parametrize("run", RUNS, ids=K.run_id)
def test_twin_within_bounds(run):
    P, I, D, bx, bz = result(run)
    O = K.ops_of(run, I)
    rec, facts = K.check_solve(P, O, D, bx, bz, 8, run[3], True)
    K.check_residuals(P, O, D, I, 0, rec)
    print("\n%-40s %s" % (K.run_id(run), "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.failed, rec.failed
    low = sorted((k, v) for k, v in rec.frac.items() if not v <= (1.0 if k in K.COUNTED else 0.25))
    assert not low, low
    assert not facts["undecided"]


@pytest.mark.parametrize("form", [0, 1])
def test_twin_residuals_both_forms(form):
    run = RUNS[0]
    P, I, D, bx, bz = result(run)
    Gm = K.model_G(P)
    rec, facts = K.check_residuals(P, K.ops_of(run, I), dict(res=K.twin_residuals(P, Gm, I, form)), I, form)
    assert not rec.failed and not [k for k, v in rec.frac.items() if not v <= (1.0 if k in K.COUNTED else 0.25)]


def test_both_outcomes_of_every_decision():
    hz, cx, php, beta0 = set(), set(), set(), set()
    for run in RUNS:
        P, I, D, bx, bz = result(run)
        O = K.ops_of(run, I)
        _, f = K.check_residuals(P, O, D, I, 0)
        assert f["hz_margin"] >= 1e-3 and f["cx_margin"] >= 1e-3, (K.run_id(run), f)
        assert f["hz_neg"] == run[5]
        hz.add(f["hz_neg"]), cx.add(f["cx_neg"])
        _, g = K.check_solve(P, O, D, bx, bz, 8, run[3], True)
        php.update(g["pHp_pos"]), beta0.update(g["beta_zero"])
        if run[2] == "zero":                                 # the zero column: alpha = beta = 0 in every sweep, nothing but zeros, no NaN
            assert g["pHp_pos"][1::2] == [False] * 8 and g["beta_zero"][1::2] == [True] * 7
            for k, v in D.items():
                if k not in ("sc", "M", "res"):
                    assert np.all(v[1] == 0.0), k
            assert all(D["sc"]["step%d" % q]["alpha1"] == 0.0 for q in range(8))
    assert hz == {True, False} and cx == {True, False} and php == {True, False} and beta0 == {True, False}


def test_twin_spread_sets_the_factor():
    """n_q of the twin under two summation orders x two preconditioner forms: the largest ratio between any two variants, over every
    run and every q whose norms are above the floor (stage 4's bound of r)."""
    worst = 1.0
    for run in RUNS:
        P, I, D, bx, bz = result(run)
        _, f = K.check_solve(P, K.ops_of(run, I), D, bx, bz, 8, run[3], True)
        seqs, raw = [], []
        for order in ("device", "seq"):
            for precond in ("M", "chol"):
                Dv = result(run, 8, order, precond)[2]
                seqs.append([max(Dv["sc"]["end"]["n%d" % q], f["floor"]) for q in range(9)])
                raw.append([Dv["sc"]["end"]["n%d" % q] for q in range(9)])
        a = np.array(seqs)
        sp = float((a.max(0) / a.min(0)).max())
        print("%-40s spread %.3g  (floor %.2g; the twin's own n_0 %.2g, n_1 %.2g, n_2 %.2g)" % (K.run_id(run), sp, f["floor"], raw[0][0], raw[0][1], raw[0][2]))
        worst = max(worst, sp)
    print("largest spread %.3g: FACTOR %.0f" % (worst, K.FACTOR))
    assert worst <= K.SPREAD_MEASURED and K.FACTOR >= 4 * K.SPREAD_MEASURED


def test_designs_reach_their_branches():
    P = K.program_of("c8_dup12")
    assert P["Nt"] <= 32 and P["nq3"] > 0 and P["l"] == 900                  # k_gt_finish: one column workgroup and the y block
    P = K.program_of("c2_ap150")
    assert P["N"] > K.SCAL_T and -(-P["Nt"] // 32) + 1 > 2                    # a second pass of the strided loops; several column workgroups
    assert K.program_of("c3_lin64")["nq3"] == K.program_of("c3_lin64")["big"] == 0
    P = K.program_of("c4_qphs21")
    assert P["quad"] and P["big"] == 43
    P = K.program_of("c6_qp25")
    assert P["l"] == 0 and P["nq3"] and P["big"]
    npd = {n: -(-K.program_of(n)["N"] // 64) * 64 for n in K.designs()}
    assert npd["n512_ap"] == 1024 and npd["n512_qphs"] == 1088 and K.program_of("n512_qphs")["big"] > 1024   # either side of the one-pass M'(M b)
    assert all(v <= 1024 for k, v in npd.items() if k != "n512_qphs")


# ---- the sentinel and masking rules on a stand-in of the hook's output ----------------------------------------------------------------
def standin(N, R, ns, live, nv, z_written):
    """what mbfir.test_unit_kkt returns for one lane by the rules of include/mbfir.h: NaN where nothing writes, 1 elsewhere."""
    X, Rn, S = mbfir.UNIT_KKT_OUT_X, mbfir.UNIT_KKT_OUT_R, mbfir.UNIT_KKT_SNAPS
    ox, orr, sc = np.full((len(X), 2, N), np.nan), np.full((len(Rn), 2, R), np.nan), np.full((len(S), len(mbfir.UNIT_KKT_SC)), np.nan)
    if not live:
        return dict(raw_x=ox, raw_r=orr, raw_sc=sc)
    for names, a in ((X, ox), (Rn, orr)):
        for i, k in enumerate(names):
            q = int(k[-1]) if k[-1].isdigit() else None
            if q is None:
                a[i, :nv] = 1.0
            elif q < ns and not (k[0] == "z" and not z_written):
                a[i, :nv] = 1.0
    for i, sn in enumerate(S):
        q = int(sn[-1]) if sn[-1].isdigit() else None
        if q is None or q < ns:
            sc[i, :ns + 1] = 1.0
    return dict(raw_x=ox, raw_r=orr, raw_sc=sc)


def test_sentinel_rules_on_a_stand_in():
    N, R = 24, 933
    for nv in (1, 2):
        for zw in (True, False):
            for b, (ns, live) in enumerate([(0, True), (3, True), (1, False), (8, True), (1, True)]):
                D = standin(N, R, ns, live, nv, zw)
                if live:
                    assert K.untouched(None, D, ns, nv, zw) == [], (nv, zw, ns)
                else:
                    assert all(np.all(np.isnan(v)) for v in D.values())
    # a lane that took one sweep too many, a z in the fused form, a second vector at nv = 1, a snapshot past the count: all reported
    D = standin(N, R, 4, True, 2, True)
    bad = K.untouched(None, D, 3, 2, True)
    assert {"hp3", "dx3", "r3", "p3", "z3", "gp3", "wp3", "gdx3", "dz3", "snapshot start3", "snapshot step3"} == set(bad)
    assert set(K.untouched(None, standin(N, R, 2, True, 2, True), 2, 2, False)) == {"z0", "z1"}
    assert "gtwbz vector 1" in K.untouched(None, standin(N, R, 2, True, 2, True), 2, 1, True)
