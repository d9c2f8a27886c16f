"""CPU checks of tests/lattice_ref.py, the reference tests/test_latticeops_gpu.py holds a unit's operators to: the longdouble G
against the product's float64 assembly, the Nesterov-Todd blocks against their defining identities, the facts about the grids
the device tests rely on, and the error bounds against a float64 model of the lattice recurrences (seeds by sincos at segment
and run starts, the rotation recurrence in between, the folded grid).  The model, not the device, is what the bounds are measured
against: its worst error over the longdouble reference must stay a factor 4 below the bound (the margin is for the freedom in
FMA contraction and summation order the device has and the model has not).

Measured (worst model error / bound; pytest -s prints them; K_G, K_GT, K_H in units of u = 2^-53):
    case        K_G    K_GT   K_H    G v     G v, |G| form   G e_j   G'u     H trig block (centred | wide draw)
    c1_ap24      876   1413   2080   0.021   0.031           0.109   0.002   0.003 | 0.005
    c2_ap150    5421   5006   9235   0.012   0.019           0.111   0.003   0.005 | 0.006
    c3_lin64    1157   1652   2562   0.003   0.005           0.011   0.002   0.003 | 0.002
    c4_qphs21    483   1096   1400   0.020   0.036           0.116   0.000   0.002 | 0.003
    c5_qphs22    506   1096   1417   0.018   0.033           0.120   0.000   0.002 | 0.001
    c6_qp25      917   1438   2185   0.017   0.027           0.113   0.003   0.002 | 0.003
    c7_ap58     2144   2406   4033   0.016   0.026           0.120   0.002   0.003 | 0.005
    c8_dup12     429   1064   1391   0.024   0.036           0.120   0.002   0.005 | 0.003
    c1_ap24, MBFIR_FOLD=0 grid       0.003   0.005           0.019   0.002   0.002 | 0.004
    c2_ap150, MBFIR_FOLD=0 grid      0.001   0.001           0.003   0.004   0.005 | 0.005
The bounds are worst-case sums of roundings and the errors add up like a random walk, hence ratios of 1e-2 for the sums; a single
entry (the unit vectors e_j) comes to 1 / 9 of its bound, which is the seed's rounded argument X u against the 9 X of trig().  A
kernel that is wrong in an index, a sign, a factor or a seed is off by 1e10 bounds and more."""
import numpy as np
import pytest
from conftest import WHICH

import lattice_ref as lr
import mbfir

LD = lr.LD
CASES = lr.unit_cases()
_cache = {}


def _prog(name):
    if name not in _cache:
        c = CASES[name]
        _cache[name] = lr.program(c["job"][0], c["job"][1], c["grid_m"])
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_longdouble_G_equals_the_products_assembly(name):
    c, P = CASES[name], _prog(name)
    fn, args = c["job"]
    rc, Q = mbfir.assemble_dense(WHICH[fn], args[0], args[1], args[2], args[3], lr._params(fn, args), grid_m=c["grid_m"])
    assert rc == 0, Q
    G = lr.G_ref(P)
    assert G.dtype == LD and np.finfo(LD).eps < 2e-19
    assert G.shape == Q["G"].shape and (P["l"], P["nq3"], P["big"]) == (Q["l"], Q["nq3"], Q["big"])
    # A float64 assembly rounds the argument w tau before the cosine, which moves an entry by up to |w tau| u times its amplitude
    # (1.4e-14 at n = 24, 1e-13 at n = 150): with the argument rounded the same way the reference meets the literal of
    # test_product_assembly_equals_oracle, and with the exact argument it differs by no more than that rounding explains
    assert np.abs(lr.G_ref(P, round_arg=True) - Q["G"].astype(LD)).max() <= 4e-15 * np.abs(Q["G"]).max()
    assert np.all(np.abs(G - Q["G"].astype(LD)).astype(np.float64) <= (lr.grid_facts(P)["X"] + 4) * lr.U * lr.G_hat(P))
    # the envelope dominates G entry by entry (to the rounding of the float64 amplitudes)
    assert np.all(np.abs(G).astype(np.float64) <= lr.G_hat(P) * (1 + 1e-15))


@pytest.mark.parametrize("name", ["c1_ap24", "c4_qphs21", "c6_qp25", "c7_ap58"])
@pytest.mark.parametrize("wide", [False, True])
def test_scaling_blocks_satisfy_their_definitions(name, wide):
    """W^-2 = (W^-1)^2 and W^-1 s = W z (= lambda), block by block, to longdouble rounding: both sides are a few dozen longdouble
    operations on numbers of the block's size, so 256 eps_longdouble of the largest entry involved."""
    P = _prog(name)
    s, z = lr.draw_sz(P, np.random.default_rng(5), wide)
    S = lr.Scaling(P, s, z)
    eps = float(np.finfo(LD).eps)
    l, o3 = P["l"], P["l"] + 3 * P["nq3"]
    if l:
        wl = np.sqrt(S.s[:l] / S.z[:l])                  # W = diag(sqrt(s / z)) on the orthant
        assert np.abs(S.d - 1 / wl ** 2).max() <= 8 * eps * np.abs(S.d).max()
        assert np.abs(S.s[:l] / wl - wl * S.z[:l]).max() <= 8 * eps * np.abs(wl * S.z[:l]).max()
        if wide:
            assert float(S.d.max() / S.d.min()) >= 1e8
    blocks = []
    if P["nq3"]:
        blocks += [(S.W3[c], S.Wi3[c], S.B3[c], S.s[l + 3 * c:l + 3 * c + 3], S.z[l + 3 * c:l + 3 * c + 3]) for c in range(P["nq3"])]
    if P["big"]:
        blocks.append((S.Wb, S.Wib, S.Bb, S.s[o3:], S.z[o3:]))
    for W, Wi, B, sb, zb in blocks:
        tol = 256 * eps * len(sb)
        assert np.abs(Wi @ Wi - B).max() <= tol * np.abs(B).max()
        assert np.abs(W @ Wi - np.eye(len(sb))).max() <= tol * np.abs(W).max() * np.abs(Wi).max()
        lam = W @ zb
        assert np.abs(Wi @ sb - lam).max() <= tol * np.abs(lam).max() * max(1.0, float(np.abs(Wi).max() * np.abs(sb).max() / np.abs(lam).max()))
    # ... and the blocks act where they belong
    x = np.random.default_rng(6).standard_normal(P["R"])
    y = S.winv2(x)
    assert y.dtype == LD
    if l:
        assert np.array_equal(y[:l], S.d * x[:l].astype(LD))
    if P["big"]:
        assert np.array_equal(y[o3:], S.Bb @ x[o3:].astype(LD))
    assert np.all(S.abs_winv2(np.abs(x)) >= np.abs(y).astype(np.float64) * (1 - 1e-12))


@pytest.mark.parametrize("name", sorted(CASES))
def test_grids_are_lattice_usable_and_have_the_edges_the_device_tests_name(name):
    P, ex = _prog(name), CASES[name]["expect"]
    for fold in (True, False):
        tf, L = mbfir.test_fold(P["w"], fold=fold), lr.analyse(P, fold)
        assert tf["ok"] == 1 and tf["bad"] == 0
        # the model's port of the grid analysis cuts the grid as the product does
        assert (tf["nfold"], tf["runs"]) == (len(L["wf"]), len(L["chunks"]))
        assert tf["longest"] == max(c[1] for c in L["chunks"]) <= lr.CHUNK_LEN
        assert tf["pairs"] == int(((L["pos"] >= 0) & (L["neg"] >= 0)).sum())
    tf, L, F = mbfir.test_fold(P["w"]), lr.analyse(P), lr.grid_facts(P)
    assert np.allclose(P["tau"] - L["tmin"], L["lat"], atol=1e-9, rtol=0) and L["D1"] == F["D1"]
    assert L["tmin"] == ex["tmin"] and F["useg"] == ex["useg"] and P["quad"] == ex["quad"]
    assert -(-(3 * L["D1"] - 1) // lr.MPTS) == ex["mom_blocks"]
    assert tf["runs"] > lr.CGRP                                        # nchunk > cgrp: a second chunk group in every moment launch
    nwv, nvb = (3, 2 * P["Ne"]) if P["quad"] else (1, P["Ne"])
    assert int(P["Ne"] > 0 and L["tmin"] == 0.0 and nwv + nvb <= 4) == ex["one_pass"]
    empty = int(((L["pos"] < 0) | (L["neg"] < 0)).sum())
    if "nfold_above" in ex:
        assert tf["nfold"] > ex["nfold_above"]
    if "rows_per_freq_above" in ex:
        assert F["rows_per_freq"] > ex["rows_per_freq_above"]
    if "empty_side_above" in ex:
        assert 0 < empty < tf["nfold"]
    if ex.get("no_pairs"):
        assert tf["pairs"] == 0 and empty == tf["nfold"]
    if ex.get("big"):
        assert P["big"] > 0 and P["nq3"] > 0
    if "nq3_above" in ex:
        assert P["nq3"] > 0 and np.any(P["col"] >= 0) and P["Ne"] > 0       # spike cones, identity rows, a slack column
    if ex.get("duplicates"):
        assert len(np.unique(P["w"])) < P["Mf"]
    if ex.get("lone_runs"):
        assert sum(1 for c in L["chunks"] if c[1] == 1) >= 1
    if name == "c4_qphs21":
        assert L["tmin"] == round(L["tmin"])
    if name == "c5_qphs22":
        assert L["tmin"] - np.floor(L["tmin"]) == 0.5


def test_hetero_unit_shares_a_class_but_not_an_order():
    jobs, grid_m = lr.hetero_jobs()
    Ps = [lr.program(fn, args, grid_m) for fn, args in jobs]
    assert Ps[0]["Nt"] != Ps[1]["Nt"] and Ps[0]["Ne"] == Ps[1]["Ne"] and -(-Ps[0]["N"] // 64) == -(-Ps[1]["N"] // 64)
    assert all(mbfir.test_fold(P["w"])["ok"] == 1 for P in Ps)


def _ratio(err, bound):
    return float(np.max(np.asarray(err, dtype=np.float64) / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("name,fold", [(n, True) for n in sorted(CASES)] + [("c1_ap24", False), ("c2_ap150", False)])
def test_bounds_hold_on_the_recurrence_model_with_margin_4(name, fold):
    P = _prog(name)
    L = lr.analyse(P, fold)
    rng = np.random.default_rng(11)
    G, Gh = lr.G_ref(P), lr.G_hat(P)
    v, u = rng.standard_normal((P["N"], 2)), rng.standard_normal((P["R"], 2))
    E = np.zeros((P["N"], len(lr.unit_columns(P))))
    E[lr.unit_columns(P), np.arange(E.shape[1])] = 1.0
    # G v through the row response's recurrence (segments along the lattice), G'u through the runs' (along the frequencies)
    Ge = lr.model_G(P, *lr.model_eval_trig(P, L), L)
    Gc = lr.model_G(P, *lr._unfold(P, L, *lr.chunk_trig(L, L["tmin"] + np.arange(L["D1"]))), L)
    kg, kgt, kh = lr.K_G(P) * lr.U, lr.K_GT(P) * lr.U, lr.K_H(P) * lr.U
    r_gv = _ratio(np.abs(Ge @ v - G @ v.astype(LD)), kg * (Gh @ np.abs(v)))
    r_gv_lit = _ratio(np.abs(Ge @ v - G @ v.astype(LD)), kg * (np.abs(G).astype(np.float64) @ np.abs(v)))
    r_ge = _ratio(np.abs(Ge @ E - G @ E.astype(LD)), kg * (Gh @ E))
    r_gt = _ratio(np.abs(Gc.T @ u - G.T @ u.astype(LD)), kgt * (Gh.T @ np.abs(u)))
    r_h = []
    for wide in (False, True):
        S = lr.Scaling(P, *lr.draw_sz(P, rng, wide))
        D = lr.freq_blocks(P, S)
        Hm, Hr, He = lr.model_H_trig(P, L, D), lr.H_trig_ref(P, D), lr.H_trig_ref(P, D, amplitude=True)
        r_h.append(_ratio(np.abs(Hm - Hr), kh * He))
    print("\n%-10s fold=%d  G v %.4f  G v (|G| form) %.4f  G e_j %.4f  G'u %.4f  H %.4f | %.4f   (K_G %.0f K_GT %.0f K_H %.0f)"
          % (name, fold, r_gv, r_gv_lit, r_ge, r_gt, r_h[0], r_h[1], lr.K_G(P), lr.K_GT(P), lr.K_H(P)))
    for r in (r_gv, r_gv_lit, r_ge, r_gt, r_h[0], r_h[1]):
        assert r <= 0.25
