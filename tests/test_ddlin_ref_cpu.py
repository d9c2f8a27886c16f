"""tests/ddlin_ref.py held without a GPU: every stage check of tests/test_ddlin_gpu.py on the outputs of the oracle's C twin
(oracle/ddlin.c: rank_k, chol, cho_solve) and of the NumPy double-double restatement of the block-inverse form, for every case of the
device tests -- all fractions below 1, the worst per stage printed; planted errors fail their own stage and no other; the replaced-pivot
inputs decide every pivot far from rounding; the exact integer sums agree with plain mpmath sums at 240 bits.

The reference of the largest case (n150_k20, np = 192, all stages, form bi) takes 0.3 s on one core here: the sums are integer products
on the mantissas, not mpmath operations (a plain mpmath Cholesky of that size is about 3 s)."""
import time

import numpy as np
import pytest

import ddlin_ref as R

_TW = {}


def twin(name, form, **kw):
    key = (name, form) + tuple(sorted(kw.items()))
    if key not in _TW:
        _TW[key] = R.twin(R.inputs(name, kw.pop("rhs", "random")), form, **kw)
    return _TW[key]


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_twin_passes_every_stage(name):
    worst = {}
    for form in R.FORMS:
        o = twin(name, form)
        rec, facts = R.check_all(R.inputs(name), o, form, twin_count=int(o["counter"][0]))
        R.assert_held(rec, "twin %s %s" % (name, form))
        assert facts["replaced"] == [j for j in R.CASES[name][2] if j > 0]
        for st, v in rec.worst().items():
            worst[st] = max(worst.get(st, 0.0), v)
    assert all(v < 1.0 for v in worst.values())


@pytest.mark.parametrize("form", R.FORMS)
def test_one_right_hand_side_an_all_zero_column_and_the_wide_tile(form):
    name = "n65_k20"
    for kw in (dict(nrhs=1), dict(rhs="zero"), dict(tile=64), dict(nsolve=3)):
        o = twin(name, form, **kw)
        rec, _ = R.check_all(R.inputs(name, kw.get("rhs", "random")), o, form, kw.get("nrhs", 2), kw.get("tile", 32))
        R.assert_held(rec, "twin %s %s %s" % (name, form, kw))


# what is planted, where, on which case and form: each must fail exactly the stage CORRUPTIONS names.  (A column past the strong rows of
# a case with k > 0 is no place for the factor's: its entries are what is left of 1e16 after fourteen digits cancel, a low word there is
# below what double-double arithmetic itself delivers, and the bound -- rightly -- lets it pass: 0.3 at column 33 or 40 of n150_k9.)
PLANTED = [("update_low", 0, "n150_k9", "bi"), ("pivot_low", 40, "n150_k0", "bi"), ("pivot_low", 3, "n30_k9", "single"),
           ("column_low", 33, "n150_k0", "bi"), ("column_low", 0, "n64_k8", "mw"), ("inverse_low", 1, "n150_k9", "bi"),
           ("inverse_low", 0, "n30_k9", "bi"), ("solve_low", 0, "n150_k9", "bi"), ("solve_low", 0, "n150_k9", "mw"), ("solve_low", 0, "n64_k8", "single")]


@pytest.mark.parametrize("what,at,name,form", PLANTED)
def test_a_planted_error_fails_its_own_stage_alone(what, at, name, form):
    """low words of the update zeroed; a pivot's low word ignored in the diagonal; the low words of one factor column zeroed; one inverse
    block's low words zeroed; the factor's low words zeroed in the solve -- each where a wrong kernel would make it, everything
    downstream computed from the wrong values"""
    o = R.twin(R.inputs(name), form, corrupt=what, at=at)
    rec, _ = R.check_all(R.inputs(name), o, form)
    R.report(rec, "planted %s@%d %s %s" % (what, at, name, form))
    assert R.failing(rec) == [R.CORRUPTIONS[what]], (R.failing(rec), rec.over(), rec.failed)
    assert max(v for (st, _), v in rec.frac.items() if st == R.CORRUPTIONS[what]) > 1e6


def test_a_wrong_count_a_lost_hand_off_and_a_touched_sentinel_are_seen():
    name, form = "n150_k0_p31", "mw"
    inp = R.inputs(name)
    base = twin(name, form)
    for key, edit, stage in (("counter", lambda a: a.__setitem__(slice(None), 0), "counter"),
                             ("counter", lambda a: a.__setitem__(1, a[1] + R.SYNC_LOST), "counter"),
                             ("Ltl", lambda a: a.__setitem__((5, 2), 0.0), "factor"),
                             ("Hl", lambda a: a.__setitem__((0, 40), 0.0), "update"),
                             ("dinv", lambda a: a.__setitem__((0, 0, 0, 0), 1.0), "blockinv"),
                             ("d0", lambda a: a.__setitem__(7, np.nextafter(a[7], 0)), "d0")):
        o = {k: v.copy() for k, v in base.items()}
        edit(o[key])
        rec, _ = R.check_all(inp, o, form, twin_count=int(base["counter"][0]))
        assert stage in R.failing(rec), (key, R.failing(rec))


@pytest.mark.parametrize("name", [c for c in R.CASES if "_p" in c])
def test_the_replaced_pivot_inputs_decide_far_from_rounding(name):
    """every pivot the reference keeps exceeds pivtol d0[j] by a factor of at least 1e10; every one it replaces is negative by half a
    diagonal entry (p = -d0[j] up to the column's noise): neither the device nor the twin can part from the plan through rounding"""
    o = twin(name, "mw")
    rec, facts = R.check_all(R.inputs(name), o, "mw")
    want = [j for j in R.CASES[name][2] if j > 0]
    assert facts["replaced"] == want and int(o["counter"][0]) == len(want)
    assert facts["keep"] >= 1e10
    if want:
        assert facts["drop"] <= -0.9
        d0 = o["d0"][want]
        assert np.all(d0 > 0.1 * np.median(np.diag(R.inputs(name)["H"]))) and np.all(d0 < np.abs(R.inputs(name)["H"]).max())
    assert np.isfinite(o["Lh"][np.tril_indices(len(o["Lh"]))]).all()


def test_the_exact_sums_agree_with_mpmath():
    """the integer sums of the factor stage and of the update against plain mpmath sums at 240 bits, entry by entry (n30_k9)"""
    mp = R.mpm()
    inp = R.inputs("n30_k9")
    o = twin("n30_k9", "mw")
    Hp, Up, _, _ = R.padded(inp)
    f = lambda a, b=0.0: mp.mpf(float(a)) + mp.mpf(float(b))
    n = inp["n"]
    Lx, el = R.xdd(np.tril(o["Lh"]), np.tril(o["Ll"]))
    for i in range(0, n, 3):
        for j in range(0, i + 1, 2):
            ref = mp.fsum(f(o["Lh"][i, c], o["Ll"][i, c]) * f(o["Lh"][j, c], o["Ll"][j, c]) for c in range(j))
            got = mp.ldexp(mp.mpf(int(Lx[i, :j] @ Lx[j, :j]) if j else 0), 2 * el)
            assert abs(got - ref) <= mp.mpf(2) ** -200 * (abs(ref) + 1)
            ref = f(Hp[i, j]) + mp.fsum(f(inp["X"][r]) * f(Up[r, i]) * f(Up[r, j]) for r in range(inp["k"]))
            err = abs(f(o["Hh"][i, j], o["Hl"][i, j]) - ref)
            env = abs(Hp[i, j]) + float(np.sum(inp["X"] * np.abs(Up[:, i]) * np.abs(Up[:, j])))
            assert err <= R.k_dd(inp["k"] + 1) * R.EPS_DD * env


def test_the_reference_of_the_largest_case_is_quick():
    name = "n150_k20"
    o = twin(name, "bi")
    R._CACHE.clear()
    t = time.perf_counter()
    R.check_all(R.inputs(name), o, "bi")
    dt = time.perf_counter() - t
    print("ddlin reference %s bi: %.2f s" % (name, dt))
    assert dt < 5.0
