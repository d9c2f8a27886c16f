"""The capacitance-form KKT kernels (capkkt.hip: k_cap_gemm<0/1/2>, k_cap_fold<0/1/2>, k_cap_add, k_cap_uy, k_cap_dx) and the
consumers of their output (chol.hip: k_hsolve<NV, U>, the k_trigemv pair) stage by stage against tests/capkkt_ref.py, through
mbfir.test_capsolve -- the launches of a solve's capacitance branch on caller-supplied problems, NaN written wherever the kernels
claim not to read.  Each stage takes the device's own earlier outputs as exact input and is held to a bound derived from its
summation (capkkt_ref's docstring); the final dx is also held to the double-double solution of the un-eliminated system.

Measured on an MI355X (worst over the cases of this file, as a fraction of the bound; printed by every case with -s): DESIGN.md
section 2b keeps the table."""
import numpy as np
import pytest

import capkkt_ref as ref
import mbfir

pytestmark = pytest.mark.gpu

# (n, k): one tile, every MODE 0 span 1 (three of the four split parts empty) | n < np | - | kp = 128, np = 192: odd tile count,
# k_hsolve U = 2 with its j < np guard | kp = 192 | k = kp, no padding row | np = 1088: the k_trigemv pair
SHAPES = [(64, 1), (60, 3), (100, 7), (191, 65), (320, 129), (449, 64), (1030, 70)]
_problems, _solved = {}, {}


def problem(n, k, nrhs=2, t_mode="scaled", seed=None):
    key = (n, k, nrhs, t_mode, seed)
    if key not in _problems:
        _problems[key] = ref.family(n, k, nrhs, t_mode, seed)
    return _problems[key]


def solve(keys, kp, form=-1, mask=None):
    """The problems `keys` (arguments of problem()) as one call of the hook; cached, the arrays are not to be written to."""
    keys = tuple(tuple(q) + (2, "scaled", None)[len(q) - 2:] for q in keys)
    ck = (keys, kp, form, tuple(mask) if mask is not None else None)
    if ck not in _solved:
        H, U, X, a, b, t, k = ref.pack([problem(*q) for q in keys], kp)
        _solved[ck] = mbfir.test_capsolve(H, U, X, a, b, t, k, kp, mask=mask, hsolve_form=form)
    return _solved[ck]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def upper_tiles(q):
    t = np.arange(q) // 64
    return t[None, :] > t[:, None]


def check_lane(p, kp, out, label):
    """Stage checks of one lane; the poison above the diagonal is still there; no pivot was replaced.  Returns the Report."""
    assert out["flag"] == 0
    for name in ("M", "S", "Ms"):
        assert np.isnan(out[name][upper_tiles(len(out[name]))]).all(), "a tile above the diagonal of %s was written" % name
    rep = ref.stage_checks(p, kp, out)
    print("CAPKKT stages %s: %s" % (label, " ".join("%s %.3g" % (s, rep.fractions.get(s, np.nan)) for s in ref.STAGES)))
    assert not rep.failures, rep.failures
    assert set(rep.fractions) == set(ref.STAGES)
    return rep


@pytest.mark.parametrize("t_mode", ["zero", "scaled"])
@pytest.mark.parametrize("nrhs", [1, 2])
@pytest.mark.parametrize("n,k", SHAPES)
def test_every_stage_within_its_bound_and_dx_against_the_double_double_solution(n, k, nrhs, t_mode):
    kp = ref.pad64(k)
    p = problem(n, k, nrhs, t_mode)
    out = ref.lane(solve([(n, k, nrhs, t_mode)], kp), 0)
    check_lane(p, kp, out, "n %d k %d nrhs %d t %s" % (n, k, nrhs, t_mode))
    err_dev, err_restate, cond_s, spd = ref.end_to_end(p, out["dx"][:, :n])
    print("CAPKKT e2e n %d k %d nrhs %d t %s: device %.3g restatement %.3g ratio %.3g cond(S) %.3g"
          % (n, k, nrhs, t_mode, err_dev, err_restate, err_dev / err_restate, cond_s))
    assert spd and cond_s <= ref.COND_S_MAX and err_restate <= ref.RESTATE_TOL        # what the reference itself must meet
    assert err_dev <= ref.E2E_FACTOR * err_restate


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n,k", [(191, 65), (320, 129)])
def test_both_forms_of_the_solve_with_M_pass_the_stage_bounds(n, k, form):
    """np = 192 and 320: y by the one-pass k_hsolve (1) and by the k_trigemv pair (0, with the stored transpose); what does not
    depend on y's form is the same bit for bit."""
    kp = ref.pad64(k)
    out = ref.lane(solve([(n, k)], kp, form=form), 0)
    check_lane(problem(n, k), kp, out, "n %d k %d form %d" % (n, k, form))
    auto = ref.lane(solve([(n, k)], kp), 0)
    for name in ("M", "Yt", "Zt", "S", "Ms", "rhs_w"):
        assert same(out[name], auto[name]), name
    if form == 1:                                              # (a solve of this size takes the one-pass form)
        assert all(same(out[name], auto[name]) for name in ref.STAGES)


def test_the_largest_size_takes_the_gemv_pair():
    n, k = 1030, 70
    auto, pair = solve([(n, k)], 128), solve([(n, k)], 128, form=0)
    assert all(same(auto[name], pair[name]) for name in ref.STAGES)


def test_padding_changes_no_bit_of_the_lanes_own_rows():
    """(191, 65) carried by launches of kp = 128, 192 and 512 (k_hsolve<., 1 / 2 / 4> on Ms): the rows below k of Yt, Zt, S, zeta
    and all of dx are the same bit for bit, the padding rows zero with a unit diagonal (stage checks at every kp)."""
    n, k = 191, 65
    outs = {kp: ref.lane(solve([(n, k)], kp), 0) for kp in (128, 192, 512)}
    for kp, out in outs.items():
        check_lane(problem(n, k), kp, out, "n %d k %d kp %d" % (n, k, kp))
    base = outs[128]
    low = ~upper_tiles(128)[:k, :k]
    for kp in (192, 512):
        out = outs[kp]
        assert same(out["Yt"][:k], base["Yt"][:k]) and same(out["Zt"][:k], base["Zt"][:k])
        assert same(out["S"][:k, :k][low], base["S"][:k, :k][low]) and same(out["Ms"][:k, :k][low], base["Ms"][:k, :k][low])
        assert same(out["w"][:, :k], base["w"][:, :k])
        assert same(out["zeta"][:, :k], base["zeta"][:, :k])
        assert same(out["dx"], base["dx"])


LANES = [(191, 65), (191, 1), (191, 40), (191, 65, 2, "scaled", 7)]


def test_a_unit_of_four_lanes_equals_the_single_solves_and_leaves_a_masked_lane_alone():
    """Four different problems at n = 191 with k = (65, 1, 40, 65) as one unit at kp = 128 (launches sized to kp, every lane's count
    read from its arena; the factorisations in the unit's single-launch form): every output of every lane equals its single solve's bit
    for bit.  With lane 1 masked its outputs keep the sentinel (and the poison), the other lanes' do not change."""
    kp = 128
    unit = solve(LANES, kp)
    for q, key in enumerate(LANES):
        single, mine = ref.lane(solve([key], kp), 0), ref.lane(unit, q)
        check_lane(problem(*key), kp, mine, "unit lane %d k %d" % (q, key[1]))
        for name in ref.STAGES + ("flag",):
            assert same(np.asarray(mine[name]), np.asarray(single[name])), (q, name)
    masked = solve(LANES, kp, mask=(1, 0, 1, 1))
    for q in range(len(LANES)):
        mine = ref.lane(masked, q)
        for name in ref.STAGES:
            if q != 1:
                assert same(mine[name], unit[name][q]), (q, name)
                continue
            keep = ~upper_tiles(len(mine[name])) if name in ("M", "S", "Ms") else np.ones(mine[name].shape, dtype=bool)
            assert (mine[name][keep] == mbfir.CAP_SENTINEL).all(), name
        assert masked["flag"][q] == (unit["flag"][q] if q != 1 else -1)


def test_bad_arguments_are_refused_with_a_message_before_anything_runs():
    n, kp = 60, 64
    H, U, X, a, b, t, k = ref.pack([problem(n, 3)], kp)
    good = mbfir.test_capsolve(H, U, X, a, b, t, k, kp)

    def refused(word, **kw):
        args = dict(k=k, kp=kp)
        args.update(kw)
        kk, kq = args.pop("k"), args.pop("kp")
        with pytest.raises(ValueError, match=word):
            mbfir.test_capsolve(H, U, X, a, b, t, kk, kq, **args)
    refused("k = 0", k=[0])
    refused("k = 65", k=[65])
    big = ref.pack([problem(n, 3)], 1088)
    with pytest.raises(ValueError, match="kp must be"):
        mbfir.test_capsolve(*big[:6], big[6], 1088)
    U100, X100, t100 = np.zeros((1, 100, n)), np.ones((1, 100)), np.zeros((1, 2, 100))
    with pytest.raises(ValueError, match="kp must be"):
        mbfir.test_capsolve(H, U100, X100, a, b, t100, k, 100)
    refused("nrhs", nrhs=0)
    a3, t3 = np.zeros((1, 3, n)), np.zeros((1, 3, kp))
    with pytest.raises(ValueError, match="nrhs"):
        mbfir.test_capsolve(H, U, X, a3, a3, t3, k, kp)
    refused("nlanes", nlanes=0)
    refused("hsolve_form", hsolve_form=2)
    Hb, Ub, Xb, ab, bb, tb, kb = ref.pack([problem(1030, 70)], 128)
    with pytest.raises(ValueError, match="one-pass"):
        mbfir.test_capsolve(Hb, Ub, Xb, ab, bb, tb, kb, 128, hsolve_form=1)
    again = mbfir.test_capsolve(H, U, X, a, b, t, k, kp)                  # the context is as it was
    assert all(same(good[name], again[name]) for name in ref.STAGES)
