"""The reference and the bounds of tests/cone_ref.py, checked without a GPU on every input tests/test_cone_gpu.py uses:
  - the float64 NumPy formulas of oracle/conic_ipm.py (cone_ref.twin) stay inside every bound and reproduce every decision;
  - the reference satisfies its defining properties to 1e-40 (the NT scaling of the second-order cones in mpmath: W z = W^-1 s,
    w'Jw = 1, W^-1 W = I, the dense forms of W and Arw against the structured ones, the first root of the step's quadratic, the
    eigenvalues of a Jordan product from its dense arrow matrix);
  - every run binds the step bounds it is there for, holds its decisions with a relative margin of 1e-6, and both outcomes of
    every decision occur among the runs;
  - every design has the cone composition and block counts it is there for.
pytest -s prints the twin's worst error / bound per stage and run."""
import mpmath as mp
import numpy as np
import pytest

import cone_ref as CR

RUNS = CR.RUNS
_RES = {}


def result(run):
    if run not in _RES:
        P, I = CR.run_inputs(run)
        rec, facts = CR.check_lane(P, I, CR.twin(P, I, run[6]), run[6])
        _RES[run] = (P, I, rec, facts)
    return _RES[run]


@pytest.mark.parametrize("name", sorted(CR.designs()))
def test_designs_have_their_edges(name):
    d = CR.designs()[name]
    P = CR.program_of(name)
    assert (P["l"], P["nq3"], P["big"]) == d["dims"] and P["R"] == P["l"] + 3 * P["nq3"] + P["big"]
    blocks = max(1, -(-(P["l"] + P["nq3"]) // 256))
    if name == "c8_dup12":          # the 3-row cones sit in the last, partly filled block
        assert blocks == 4 and P["l"] // 256 == 3 and (P["l"] + P["nq3"]) % 256 != 0
    if name == "c3_lin64":
        assert blocks == 8 and P["nq3"] == 0 and P["big"] == 0
    if name == "c6_qp25":           # no orthant rows; the big cone's partial row in front of two block rows
        assert blocks == 2 and P["l"] == 0
    if name == "c4_qphs21":
        assert blocks == 50 and P["quad"]
    if name == "n600":              # the big cone is longer than its 1024-thread workgroup; np = 1216
        assert P["big"] > 1024 and -(-P["N"] // 64) * 64 == 1216
    assert not (P["l"] and P["nq3"] and P["big"]), "a designer with all three cone kinds: add it to the runs"


@pytest.mark.parametrize("run", RUNS, ids=CR.run_id)
def test_twin_within_bounds(run):
    P, I, rec, facts = result(run)
    print("\n%-50s %s" % (CR.run_id(run), "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.over(), rec.over()
    assert not rec.failed, rec.failed


@pytest.mark.parametrize("run", RUNS, ids=CR.run_id)
def test_run_binds_and_decides_with_margin(run):
    P, I, rec, facts = result(run)
    got = tuple(facts[k]["label"] for k in ("affine", "combined", "corrector") if k in facts)
    assert got == run[2][:len(got)], got
    if "orth" in got:                                        # ... a row of the LAST cone block
        k = ("affine", "combined", "corrector")[got.index("orth")]
        assert facts[k]["row"] >= 256 * (max(1, -(-(P["l"] + P["nq3"]) // 256)) - 1)
    low = {k: v for k, v in facts["margins"].items() if not v >= CR.MARGIN}
    assert not low, low
    for (r0, m, kind, c) in CR.socs(P):                      # the iterate is what the run says
        gs, gz = CR.gap(I["s"][r0:r0 + m]), CR.gap(I["z"][r0:r0 + m])
        assert (0.5e-6 < gs < 2e-6 and 0.5e-6 < gz < 2e-6) if run[1] == "late" else min(gs, gz) > 1e-3
    if run[1] == "late":
        l = P["l"]
        deg = l + P["nq3"] + (1 if P["big"] else 0)
        assert 1e-9 < float(I["s"] @ I["z"]) / deg < 1e-7
    if run[1] == "wide" and P["l"]:
        r = I["z"][:P["l"]] / I["s"][:P["l"]]
        assert r.max() / r.min() >= 1e8


@pytest.mark.parametrize("run", RUNS, ids=CR.run_id)
def test_twin_end_to_end(run):
    """the twin's end state against the chain without hand-over, within the carried-forward bound"""
    P, I, rec, facts = result(run)
    r2 = CR.Rec()
    CR.check_end_to_end(P, I, CR.twin(P, I, run[6]), run[6], r2, facts)
    print("\n%-50s %s" % (CR.run_id(run), "  ".join("%s %.3f" % (k[1], v) for k, v in r2.frac.items())))
    assert not r2.over(), r2.over()


def test_both_outcomes_of_every_decision():
    F = [result(run)[3] for run in RUNS]
    D = [f["decisions"] for f in F]
    labels = {k: {f[k]["label"] for f in F if k in f} for k in ("affine", "combined", "corrector")}
    assert labels["affine"] == {"orth", "q3", "big", "tau", "kappa"}       # ('none' cannot be: -dkappa_a/kappa = 1 + dtau_a/tau)
    assert labels["combined"] == labels["corrector"] == {"orth", "q3", "big", "tau", "kappa", "none"}
    assert {d["affine_alpha1"] for d in D} == {True, False} and {d["sigma_capped"] for d in D} == {True, False}
    for k in ("combined", "corrector"):                       # alpha = 1 at a zero bound, min(1, STEP / t) on both sides
        ts = [f[k]["t"] for f in F if k in f]
        assert any(t == 0 for t in ts) and any(0 < t < CR.STEP for t in ts) and any(t > CR.STEP for t in ts)
    assert {int(b) for d in D for b in d.get("corr_branches", [])} == {0, 1, 2, 3}
    assert {int(b) for d in D for b in d.get("corr_big_branches", [])} >= {0, 1, 3}
    picks = {(bool(d["pick_by_step"]), bool(d["pick_by_guard"])) for d in D if "pick" in d}
    assert picks == {(True, True), (True, False), (False, True)}
    assert all(d["directions_differ"] for d in D if "pick" in d)
    assert {d["shifted"] for d in D} == {True, False}
    barely = [f for run, f in zip(RUNS, F) if run[5] == "barely"]
    assert barely and all(f["decisions"]["shifted"] and f["shift_t"] < 0 for f in barely)


def test_reference_meets_its_definitions():
    tol = mp.mpf(10) ** -40
    for name, kind in (("c8_dup12", "late"), ("c6_qp25", "late"), ("c4_qphs21", "centred")):
        P = CR.program_of(name)
        s, z = CR.iterate(P, kind, np.random.default_rng(5))
        rng = np.random.default_rng(6)
        for (r0, m, knd, c) in CR.socs(P)[-3:]:
            sm, zm = CR.mpv(s[r0:r0 + m]), CR.mpv(z[r0:r0 + m])
            eta, w, sb, zb, gamma = CR.nt_ref(sm, zm)
            W = CR.Soc(1.0, np.ones(m))
            W.eta, W.w = eta, w
            lam, lam2 = W.mul(zm), W.inv(sm)
            scale = max(abs(x) for x in lam)
            assert abs(CR.jf(w, w) - 1) < tol
            assert max(abs(a - b) for a, b in zip(lam, lam2)) < tol * scale
            u = CR.mpv(rng.standard_normal(m))
            assert max(abs(a - b) for a, b in zip(W.inv(W.mul(u)), u)) < tol * 1e6
            Wd = W.dense()
            assert max(abs(a - b) for a, b in zip(list(Wd * mp.matrix(u)), W.mul(u))) < tol * float(eta) * 1e3
            assert max(abs(a - b) for a, b in zip(list(mp.lu_solve(Wd, mp.matrix(u))), W.inv(u))) < tol / float(eta) * 1e9
            # the step bound: at alpha = 1 / t the point is on the boundary, inside before it
            d = CR.mpv(rng.standard_normal(m) * float(scale))
            t = CR.soc_t(lam, d)
            if t > 0:
                p = [x + y / t for x, y in zip(lam, d)]
                assert abs(CR.jf(p, p)) < tol * scale ** 2 * 1e6 and p[0] > 0
                q = [x + y / (2 * t) for x, y in zip(lam, d)]
                assert CR.jf(q, q) > 0 and q[0] > 0
            # lam \ d by elimination against the dense arrow matrix, and the Jordan eigenvalues against its spectrum
            x = CR.arw_solve(lam, d)
            back = CR.jprod(lam, x)
            assert max(abs(a - b) for a, b in zip(back, d)) < tol * scale ** 2 * 1e9
            if m > CR.DENSE:
                continue
            x0 = (d[0] - CR.mdot(lam[1:], d[1:]) / lam[0]) / (lam[0] - CR.mdot(lam[1:], lam[1:]) / lam[0])
            assert abs(x0 - x[0]) < tol * abs(x[0]) * 1e9
            A = mp.matrix(m, m)
            for i in range(m):
                A[i, i] = d[0]
                if i:
                    A[0, i] = A[i, 0] = d[i]
            ev = mp.eigsy(A, eigvals_only=True)
            n1 = CR.mnorm(d[1:])
            assert abs(max(ev) - (d[0] + n1)) < tol * scale * 1e6 and abs(min(ev) - (d[0] - n1)) < tol * scale * 1e6


def test_oracle_scaling_loses_one_over_the_gap():
    """the float64 scaling formulas against the 60-digit scaling: a few u where the pair is centred, ~ u / gap near the boundary --
    the bound must carry 1 / gap (cone_ref.rcond), no constant could."""
    from oracle import conic_ipm as O
    rng = np.random.default_rng(11)
    for g, lo, hi in ((1e-3, 30, 3e4), (1e-6, 3e4, 3e7)):
        worst = 0.0
        for _ in range(20):
            u = rng.standard_normal(2)
            u /= np.linalg.norm(u)
            s, z = np.concatenate([[1 + g], u]), np.concatenate([[1 + g], -u]) * 0.3
            eta, w = O._Scaling._soc(s[None], z[None])
            _, wr, *_ = CR.nt_ref(CR.mpv(s), CR.mpv(z))
            worst = max(worst, float(max(abs(mp.mpf(float(a)) - b) / abs(b) for a, b in zip(w[0], wr) if b != 0)) / CR.U)
        print("gap %.0e: the float64 scaling misses by %.3g u" % (g, worst))
        assert lo < worst < hi
