"""The double-double dense kernels of csrc/ddlin.hip (mbfir_test_ddstages: dd_syrk_launch, dd_chol_launch, then dd_trsv_launch in a
chosen form, every group of launches read back at the padded size) against the reference of tests/ddlin_ref.py, stage by stage, within
the bounds derived there and held on the CPU by tests/test_ddlin_ref_cpu.py.  Every stage is handed the device's own earlier outputs,
so a wrong kernel fails alone; every entry a launch writes is checked and must be finite; what no launch writes must come back holding
the sentinel (NaN) it went in with: the low words of the tiles strictly above the diagonal tiles, the strict lower part of Lt, dinv in
the forms without block inverses, the second solution row of a single right-hand side.

Cases (ddlin_ref.CASES): n = 30 (np = 64, padding inside the first pair of panels), 64 (one inverse block, two panels, no rows below the
last), 65 (np = 128, a block that is almost all padding), 150 (np = 192: a block waiting on two predecessors, several update tiles and
trailing panels); k = 0, 1, 7, 8, 9 (either side of the update's chunk of 8 rows) and 20, every n at two of them and every k at n = 150;
X = 10^U(8, 16), a third of the rows nearly dependent, exact zeros in U.  Every case in the three solve forms (single: k_dd_trsv, which no
other test reaches; mw; bi), the solve forms again with nrhs = 1, an all-zero second column and three solves on one flag array (epochs
1 .. 3); both tile sizes at n = 150; replaced pivots at j = 0 (never replaced: the first pivot is d0 itself), 31, 32, 63, 64, n - 1 and
31 with 64, with k = 0 and k = 9: the count equals the reference's plan and the oracle twin's.  pytest -s prints the worst error / bound
per stage and case.

That the tests can fail -- eight arithmetic-only changes of ddlin.hip, each built apart, this file and the double-double tests of
test_kernels_gpu.py (the solve against the oracle's kernels, block inverses against substitution, 32 against 64 wide tiles, one against
two right-hand sides: 7 tests) run once on it; fractions are error / bound at worst:
  1 k_ddchol_diag: e1 = fma(-p.l, t2.h, e1) dropped    40 of 41 fail, stage factor alone: ri (4.8e13), diagonal, off the diagonal; every
                                                       later stage takes the device's wrong ri and factor as given and passes
  2 k_dd_syrk: ax[p].h alone in the product            31 fail (every case with k > 0), stage update alone (5.4e13)
  3 k_ddchol_update: product of the high words only    35 fail (every case but n = 30, whose rows below the first panel are all padding),
                                                       stage factor alone: diagonal and off the diagonal (6.3e12)
  4 k_ddchol_trsm: ril taken as 0                      35 fail (the same cases), stage factor alone: off the diagonal (4.2e13)
  5 k_dd_blockinv: ril taken as 0                      32 fail (every call in form bi), stage blockinv alone: X (5.4e13) and "the
                                                       diagonal is ri bit for bit"; the bi solve takes the wrong inverse as given and passes
  6 k_dd_trsv_bi: the inverse's low word as 0          32 fail (every call in form bi), stage solve alone (1.8e11)
  7 k_dd_trsv_mw: factor's low word 0 off the diagonal 27 fail (every case but n = 30 in form mw), stage solve alone (3.1e11)
  8 k_dd_trsv: the same                                27 fail (every case but n = 30 in form single), stage solve alone (3.1e11)
None faulted; every test not named passed.  The older tests: test_double_double_solve_matches_the_oracles_dd_kernels fails on 1, 3, 4,
5 and 6 in all four cases and on 2 in the three with k > 0 -- its bound 1e-24 max|x| max(1, X_max) is 1e-24 relative at k = 0 and the
errors planted are 1e-17, and with k > 0 the weak directions amplify them -- so it does notice a lost low word, without saying where;
the other three pass on all eight (they compare the device with itself).  7 and 8 pass all seven older tests: nothing reached
k_dd_trsv, and k_dd_trsv_mw ran only against the block-inverse form at 1e-22 X_max and against itself.
(Before the solve stage took rho = |ri L_qq - 1| from the device's own ri, mutant 1 also failed solve in single and mw, 5.3e11.)
"""
import numpy as np
import pytest

import ddlin_ref as R
import mbfir

pytestmark = pytest.mark.gpu
PLAIN = [c for c in R.CASES if "_p" not in c]
PIVOT = [c for c in R.CASES if "_p" in c]
_DEV = {}


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    monkeypatch.delenv("MBFIR_DD_TILE", raising=False)


def dev(name, form, nrhs=2, rhs="random", nsolve=1, tile=None, monkeypatch=None):
    """the hook's result for a case (one call per distinct argument list)"""
    key = (name, form, nrhs, rhs, nsolve, tile)
    if key not in _DEV:
        if tile:
            monkeypatch.setenv("MBFIR_DD_TILE", str(tile))
        inp = R.inputs(name, rhs)
        _DEV[key] = mbfir.test_ddstages(inp["H"], inp["U"], inp["X"], inp["b"][:nrhs], inp["bl"][:nrhs], pivtol=R.PIVTOL, form=form, nsolve=nsolve)
        if tile:
            monkeypatch.delenv("MBFIR_DD_TILE")
    return _DEV[key]


def held(name, form, nrhs=2, rhs="random", nsolve=1, tile=None, monkeypatch=None, twin_count=None):
    inp = R.inputs(name, rhs)
    o = dev(name, form, nrhs, rhs, nsolve, tile, monkeypatch)
    assert o["xh"].shape == (nsolve, 2, R.npad(inp["n"]))
    rec, facts = R.check_all(inp, o, form, nrhs, tile or 32, twin_count=twin_count)
    R.assert_held(rec, "%s %s nv%d %s x%d%s" % (name, form, nrhs, rhs, nsolve, " tile %d" % tile if tile else ""))
    return o, facts


@pytest.mark.parametrize("name", PLAIN)
def test_every_stage_in_every_form(name):
    """update, d0, factor (with ri and Lt), block inverses, solve, counter; the factor is the same bit for bit whatever the form"""
    outs = [held(name, form)[0] for form in R.FORMS]
    for o in outs[1:]:
        for key in ("Hh", "Hl", "d0", "Lh", "Ll", "Lth", "Ltl", "ri"):
            assert R.same_bits(o[key], outs[0][key]), key


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("name", ["n30_k9", "n64_k8", "n65_k20", "n150_k20"])
def test_solve_forms(name, form):
    """nrhs = 2 and 1, low words in b, an all-zero second column, three solves on one flag array; one right-hand side reproduces column 0
    of two bit for bit"""
    o2, _ = held(name, form, nsolve=3)
    o1, _ = held(name, form, nrhs=1, nsolve=3)
    oz, _ = held(name, form, rhs="zero", nsolve=3)
    assert np.array_equal(o1["xh"][0, 0], o2["xh"][0, 0]) and np.array_equal(o1["xl"][0, 0], o2["xl"][0, 0])
    assert np.array_equal(oz["xh"][0, 0], o2["xh"][0, 0]) and np.array_equal(oz["xl"][0, 0], o2["xl"][0, 0])
    assert np.any(o2["xl"][0] != 0.0)


@pytest.mark.parametrize("name", ["n150_k9", "n150_k20"])
def test_both_tile_sizes_are_held_to_the_reference(name, monkeypatch):
    """MBFIR_DD_TILE = 32 and 64 (k_dd_syrk<2|4>, k_ddchol_update<2|4>): each against the reference; only the sentinel's region differs"""
    o32, _ = held(name, "bi", tile=32, monkeypatch=monkeypatch)
    o64, _ = held(name, "bi", tile=64, monkeypatch=monkeypatch)
    low = R.tile_mask(len(o32["Hh"]), 64)
    tri = np.tril(np.ones(low.shape, dtype=bool))
    assert np.array_equal(o32["Hh"][tri], o64["Hh"][tri]) and np.array_equal(o32["Hl"][tri], o64["Hl"][tri])
    for key in ("d0", "ri", "dinv", "xh", "xl"):
        assert R.same_bits(o32[key], o64[key]), key
    assert np.array_equal(o32["Lh"][tri], o64["Lh"][tri]) and np.array_equal(o32["Ll"][tri], o64["Ll"][tri])
    between = low & ~R.tile_mask(len(low), 32)              # written with 64-wide tiles, untouched with 32-wide ones
    assert R.is_sent(o32["Hl"][between]) and np.isfinite(o64["Hl"][between]).all()


@pytest.mark.parametrize("name", PIVOT)
def test_replaced_pivots(name):
    """the branch of k_ddchol_diag that replaces a pivot not above pivtol d0 by d0 and counts it: the count is the reference's plan and the
    oracle twin's, the factor passes its stage with the rule applied, the solves go through"""
    inp = R.inputs(name)
    tw = R.twin(inp, "mw")
    want = [j for j in R.CASES[name][2] if j > 0]
    for form in R.FORMS:
        o, facts = held(name, form, twin_count=int(tw["counter"][0]))
        assert facts["replaced"] == want and int(o["counter"][0]) == len(want)


def test_bad_arguments_are_refused_before_anything_runs():
    inp = R.inputs("n30_k9")
    with pytest.raises(ValueError):
        mbfir.test_ddstages(inp["H"], inp["U"], inp["X"], inp["b"], inp["bl"], form="fast")
    with pytest.raises(ValueError):
        mbfir.test_ddstages(inp["H"], inp["U"], inp["X"], inp["b"], inp["bl"], nsolve=0)
    with pytest.raises(ValueError):
        mbfir.test_ddstages(inp["H"], inp["U"], inp["X"], np.zeros((3, 30)), np.zeros((3, 30)))
