"""A lock-step unit's operators G v, G'u, W^-2 G v - sub and H = G'W^-2 G (mbfir_test_unit_ops: the stages and launch code of a
solve, at an iterate the test chooses) against the dense longdouble reference of tests/lattice_ref.py, within the bounds derived
there and checked on the CPU by tests/test_latticeops_cpu.py.  Every test asserts from the hook's report which path it ran.

Cases (lattice_ref.unit_cases): the smallest designs at which each edge of the lattice kernels exists.  Two findings about the
shapes: D1 = 150 gives THREE evaluation segments, not two (the segment length is 64 until D1 passes 1024; 128 = SEGMAX is its
cap), and the golden n = 22 fir_qprog_phs spec folds without an empty side, so case 5 moves two band edges off the mirror image.
Lanes of a case: lane 0 well centred, lane 1 with orthant weights z / s spread over 1e8, lanes 2 and 3 centred; every lane has its
own v, u, sub and (s, z).  Inputs per lane: run A two random vectors (NV = 2), run B two unit vectors (one per column kind / row
kind), run C one vector (NV = 1; the slack column's unit vector where there is one) without `sub`.
pytest -s prints, per unit and lane, the report and the worst error / bound of the four outputs.

Measured on one MI355X (worst error / bound over all lanes, runs and forms of a case; lattice = 1, cgrp = 4, seg = 64 in all;
units of 2 - 4 lanes: pair_passes = 4, single designs and the unit of two orders: 0):
    case        one_pass  tmin   D1  useg  nfold  nchunk   np  empty sides   G v     G'u     W^-2 G v - sub   H
    c1_ap24     1           0.0   24  1      265  21       64     8          0.110   0.004   0.396            0.007
    c2_ap150    1           0.0  150  3     1033  40      320     8          0.111   0.011   0.311            0.012
    c3_lin64    0           0.5   32  1      964  28       64   964          0.011   0.010   0.430            0.004
    c4_qphs21   0         -10.0   21  1      318  19       64     0          0.115   0.008   0.470            0.026
    c5_qphs22   0         -10.5   22  1      336  18       64     6          0.120   0.005   0.460            0.015
    c6_qp25     0           0.0   25  1      128  10       64     0          0.110   0.061   0.406            0.111
    c7_ap58     1           0.0   58  1      879  39      128     8          0.115   0.003   0.355            0.007
    c8_dup12    1           0.0   12  1      186  16       64     6          0.111   0.054   0.416            0.008
G v peaks on the unit vectors (one entry: the seed's rounded argument, 1 / 9 of trig()), W^-2 G v - sub where `sub` dwarfs the product
(the subtraction's own rounding against 2 u |sub|).  The draws with orthant weights spread over 1e8 keep H within 0.03 of its bound:
the moment-assembled H loses no digits the envelope does not account for.  Dense twins (opts.dense_trig): 0.01 / 0.000 / 0.15 / 0.002.

That the tests can fail -- four arithmetic-only changes to solver.hip, each built apart and this file run once on it:
    sign of sdv in lat_T                      19 of 23 fail, first on H (2e10 .. 2e11 bounds); pass: c3 (cosine columns only), dense_trig, context
    0.5 -> 0.25 in lat_T's return             20 fail, first on H (5e11 .. 3e12); pass: dense_trig, context
    C - S -> C + S at fold_neg, k_trig_eval   17 fail, first on G v (4e11 .. 2e13), the units on `==` with the lane alone (their own
                                              kernel is the paired twin); pass: c3 and MBFIR_FOLD=0 (no negative side), dense_trig, context
    chunk 0's seeds in every chunk            20 fail, first on G'u (1e11 .. 1e12); pass: dense_trig, context"""
import numpy as np
import pytest

import lattice_ref as lr
import mbfir

pytestmark = pytest.mark.gpu
LD, U = lr.LD, lr.U
CASES = lr.unit_cases()
NAMES = sorted(CASES)
SWITCHES = ("MBFIR_LANEPAIR", "MBFIR_FUSE", "MBFIR_CGRP", "MBFIR_FOLD")
_P, _G, _IN, _REF = {}, {}, {}, {}


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def prog(name):
    if name not in _P:
        c = CASES[name]
        _P[name] = lr.program(c["job"][0], c["job"][1], c["grid_m"])
    return _P[name]


def mats(name):
    if name not in _G:
        P = prog(name)
        _G[name] = (lr.G_ref(P), lr.G_hat(P))
    return _G[name]


def h_rows(P):
    """The rows of H compared with the reference: all of them, or (N > 128: a longdouble product of that size takes many seconds) the
    rows next to every 64 x 64 tile edge and kind boundary, the first and the last, and sixteen drawn ones -- all columns of each."""
    N = P["N"]
    if N <= 128:
        return np.arange(N)
    fixed = [0, 1, N - 2, N - 1, P["Nt"] // 2 - 1, P["Nt"] // 2, P["Nt"] // 2 + 1, P["Nt"] - 1] + [e + d for e in range(64, N, 64) for d in (-1, 0)]
    drawn = np.random.default_rng(3).choice(N, 16, replace=False)
    return np.unique(np.clip(np.concatenate([fixed, drawn]), 0, N - 1))


def inputs(name, b):
    """Lane b of case `name`: (s, z) and the runs' vectors; the same whenever asked for."""
    if (name, b) not in _IN:
        P = prog(name)
        rng = np.random.default_rng([NAMES.index(name), b])
        N, R = P["N"], P["R"]
        s, z = lr.draw_sz(P, rng, wide=(b == 1))
        cols = lr.unit_columns(P)
        eb = np.zeros((2, N))
        eb[0, cols[0]] = 1.0
        eb[1, cols[1] if len(cols) > 1 and cols[1] < P["Nt"] else 0] = 1.0
        fr, idr = np.nonzero(P["freq"] >= 0)[0], np.nonzero(P["col"] >= 0)[0]
        ub = np.zeros((2, R))
        ub[0, fr[len(fr) // 2]] = 1.0
        ub[1, idr[len(idr) // 2] if len(idr) else R - 1] = 1.0
        ec = rng.standard_normal((1, N))
        if P["Ne"]:
            ec[:] = 0.0
            ec[0, N - 1] = 1.0
        _IN[(name, b)] = dict(s=s, z=z, A=dict(v=rng.standard_normal((2, N)), u=rng.standard_normal((2, R)), sub=rng.standard_normal((2, R))),
                              B=dict(v=eb, u=ub, sub=rng.standard_normal((2, R))), C=dict(v=ec, u=rng.standard_normal((1, R)), sub=None))
    return _IN[(name, b)]


def ref(name, b, run):
    """Reference values and envelopes of lane b's run, computed once."""
    P = prog(name)
    G, Gh = mats(name)
    I = inputs(name, b)
    if (name, b) not in _REF:
        S = lr.Scaling(P, I["s"], I["z"])
        rows = h_rows(P)
        _REF[(name, b)] = dict(S=S, rows=rows, H=lr.H_ref(G, S, rows), E=lr.H_env(Gh, S, rows))
    Rf = _REF[(name, b)]
    if run not in Rf:
        x = I[run]
        v, u = x["v"].T.astype(LD), x["u"].T.astype(LD)
        gv = G @ v
        wgv = Rf["S"].winv2(gv) - (x["sub"].T.astype(LD) if x["sub"] is not None else 0)
        env_gv = Gh @ np.abs(x["v"].T)
        Rf[run] = dict(gv=gv.T, gtu=(G.T @ u).T, wgv=wgv.T, env_gv=env_gv.T, env_gv_lit=(np.abs(G).astype(np.float64) @ np.abs(x["v"].T)).T,
                       env_gtu=(Gh.T @ np.abs(x["u"].T)).T, env_wgv=Rf["S"].abs_winv2(env_gv).T)
    return Rf, Rf[run]


def call(name, lanes, run="A", mask=None, jobs=None, **opt):
    """The hook on a unit whose lane q carries the inputs of pool lane lanes[q].  The outputs go in holding a sentinel."""
    c = CASES[name]
    P = prog(name)
    I = [inputs(name, b) for b in lanes]
    nl, nv = len(lanes), I[0][run]["v"].shape[0]
    npad = -(-P["N"] // 64) * 64
    init = (np.full((nl, nv, P["R"]), 7.25), np.full((nl, nv, P["N"]), -3.5), np.full((nl, nv, P["R"]), 1.75), np.full((nl, npad, npad), -9.125))
    sub = np.stack([x[run]["sub"] for x in I]) if I[0][run]["sub"] is not None else None
    opts = mbfir.make_opts(grid_m=c["grid_m"], ddkkt=c.get("ddkkt", 0), **opt)
    out = mbfir.test_unit_ops(jobs or [c["job"]] * nl, np.stack([x[run]["v"] for x in I]), np.stack([x[run]["u"] for x in I]),
                              np.stack([x["s"] for x in I]), np.stack([x["z"] for x in I]), sub=sub, mask=mask, opts=opts, init=init)
    return out, init


def check_lane(name, b, run, gv, gtu, wgv, H, dense=False, tag=""):
    """One lane's four outputs within the bounds; H's padding exact.  Returns the worst error / bound of each."""
    P = prog(name)
    Rf, r = ref(name, b, run)
    N, rows = P["N"], Rf["rows"]
    kg, kgt, kwg, kh = [K(P, dense) * U for K in (lr.K_G, lr.K_GT, lr.K_WG, lr.K_H)]

    def ratio(got, want, bound):
        assert np.all(np.isfinite(got))
        return float(np.max(np.abs(got.astype(LD) - want).astype(np.float64) / np.maximum(bound, 1e-300)))
    sub = inputs(name, b)[run]["sub"]
    q = dict(gv=ratio(gv, r["gv"], kg * r["env_gv"]), gtu=ratio(gtu, r["gtu"], kgt * r["env_gtu"]),
             wgv=ratio(wgv, r["wgv"], kwg * r["env_wgv"] + 2 * U * (np.abs(sub) if sub is not None else 0.0)))
    if run == "A":                                          # (no zeros in v: the |G| |v| form of the bound as well)
        q["gv_lit"] = ratio(gv, r["gv"], kg * r["env_gv_lit"])
    low = np.tril(np.ones((len(rows), N), dtype=bool), 0) if len(rows) == N else (np.arange(N)[None, :] <= rows[:, None])
    q["H"] = float(np.max(np.where(low, np.abs(H[rows, :N].astype(LD) - Rf["H"]).astype(np.float64) / np.maximum(kh * Rf["E"], 1e-300), 0.0)))
    assert np.all(np.isfinite(H[rows, :N][low]))
    print("    %-10s lane %d run %s %s  " % (name, b, run, tag) + "  ".join("%s %.3f" % kv for kv in q.items()))
    for k, x in q.items():
        assert x <= 1.0, "%s lane %d run %s: %s is %.3g times its bound" % (name, b, run, k, x)
    check_padding(H, N)
    return q


def check_padding(H, N):
    """Rows and columns past N (lower triangle): exactly pad_diag = 1 on the diagonal and 0 elsewhere."""
    npad = H.shape[0]
    pad = np.tril(H)[N:, :]
    want = np.zeros_like(pad)
    want[np.arange(npad - N), N + np.arange(npad - N)] = 1.0
    assert np.array_equal(pad, want)


def check_report(name, rep, lanes=1, nv=2, dense=False, paired=None, **sw):
    """The path the unit took, from the hook's report, against what the case is there for."""
    P, ex = prog(name), CASES[name]["expect"]
    tf = mbfir.test_fold(P["w"], fold=sw.get("fold", 1) != 0)
    assert rep["lanes"] == lanes and rep["np"] == -(-P["N"] // 64) * 64 and rep["gv_passes"] == 2 and rep["gtv_passes"] == 1
    if dense:
        assert rep["lattice"] == 0 and rep["pair_passes"] == 0 and rep["one_pass"] == 0
        return
    L = lr.analyse(P, sw.get("fold", 1) != 0)
    assert rep["lattice"] == 1 and rep["hetero"] == 0 and rep["tmin"] == ex["tmin"] and rep["D1"] == L["D1"]
    assert rep["useg"] == ex["useg"] and rep["seg"] == lr.seg_of(L["D1"]) and rep["one_pass"] == ex["one_pass"]
    assert rep["nfold"] == tf["nfold"] and rep["nchunk"] == tf["runs"] and rep["cgrp"] == sw.get("cgrp", 4)
    assert rep["nchunk"] > rep["cgrp"] and -(-(3 * rep["D1"] - 1) // lr.MPTS) == ex["mom_blocks"]
    assert rep["empty_side"] == int(((L["pos"] < 0) | (L["neg"] < 0)).sum())
    if "empty_side_above" in ex and sw.get("fold", 1):
        assert 0 < rep["empty_side"] < rep["nfold"]
    if "nfold_above" in ex:
        assert rep["nfold"] > ex["nfold_above"]
    # paired passes: both row responses, G'u where the paired moment kernel takes its operand count, the build's moment launches
    if paired is None:
        paired = lanes >= 2 and sw.get("lanepair", 1) != 0
    assert rep["seeds_shared"] == (1 if lanes >= 2 else 0)
    gt = 1 if sw.get("fuse", 1) and ((not P["quad"] and nv <= 2) or (P["quad"] and nv == 1)) else 0
    mom = 1 if rep["one_pass"] else 1 + (1 if P["Ne"] else 0)
    assert rep["pair_passes"] == (2 + gt + mom if paired else 0)


@pytest.mark.parametrize("name", NAMES)
def test_single_design_both_draws_all_runs(name):
    for b in (0, 1):
        for run in "ABC":
            (gv, gtu, wgv, H, rep), _ = call(name, [b], run)
            if b == 0:
                print("  %s report %s" % (name, rep))
            check_report(name, rep, 1, nv=gv.shape[1])
            check_lane(name, b, run, gv[0], gtu[0], wgv[0], H[0])


def _single(name, b):
    (gv, gtu, wgv, H, _), _ = call(name, [b], "A")
    return gv[0], gtu[0], wgv[0], np.tril(H[0])


@pytest.mark.parametrize("name", ["c1_ap24", "c2_ap150", "c4_qphs21"])
def test_units_of_two_three_and_four_with_a_masked_lane(name):
    single = {b: _single(name, b) for b in range(4)}
    for lanes, mask in (([0, 1], None), ([0, 1, 2], None), ([0, 3, 2, 1], [1, 0, 1, 1])):
        (gv, gtu, wgv, H, rep), init = call(name, lanes, "A", mask=mask)
        print("  %s unit %s mask %s report %s" % (name, lanes, mask, rep))
        check_report(name, rep, len(lanes))
        for q, b in enumerate(lanes):
            if mask and not mask[q]:
                # a masked lane: every output as it went in, bit for bit (H: the whole buffer)
                for got, was in zip((gv, gtu, wgv, H), init):
                    assert np.array_equal(got[q], was[q])
                continue
            check_lane(name, b, "A", gv[q], gtu[q], wgv[q], H[q], tag="unit of %d" % len(lanes))
            # ... and the lane alone with the same inputs, bit for bit
            for got, alone in zip((gv[q], gtu[q], wgv[q], np.tril(H[q])), single[b]):
                assert np.array_equal(got, alone)


def test_heterogeneous_unit_of_two_orders():
    """n = 20 and n = 24 in one unit: per-lane dimensions, nothing pairs; each lane within its own bounds and equal to itself alone."""
    jobs, grid_m = lr.hetero_jobs()
    Ps = [lr.program(fn, args, grid_m) for fn, args in jobs]
    N, R = max(P["N"] for P in Ps), max(P["R"] for P in Ps)
    rng = np.random.default_rng(77)
    v, u, sub, s, z = np.zeros((2, 2, N)), np.zeros((2, 2, R)), np.zeros((2, 2, R)), np.ones((2, R)), np.ones((2, R))
    for b, P in enumerate(Ps):
        v[b, :, :P["N"]], u[b, :, :P["R"]], sub[b, :, :P["R"]] = rng.standard_normal((2, P["N"])), rng.standard_normal((2, P["R"])), rng.standard_normal((2, P["R"]))
        s[b, :P["R"]], z[b, :P["R"]] = lr.draw_sz(P, rng, wide=(b == 1))
    opts = mbfir.make_opts(grid_m=grid_m)
    gv, gtu, wgv, H, rep = mbfir.test_unit_ops(jobs, v, u, s, z, sub=sub, opts=opts)
    print("  hetero report %s" % rep)
    assert rep["lattice"] == 1 and rep["hetero"] == 1 and rep["pair_passes"] == 0 and rep["seeds_shared"] == 0 and rep["lanes"] == 2
    assert rep["D1"] == 24 and rep["one_pass"] == 1
    for b, P in enumerate(Ps):
        n_, r_ = P["N"], P["R"]
        G, Gh, S = lr.G_ref(P), lr.G_hat(P), lr.Scaling(P, s[b, :r_], z[b, :r_])
        vb, ub = v[b, :, :n_].T, u[b, :, :r_].T
        gref = G @ vb.astype(LD)
        env = Gh @ np.abs(vb)
        def ratio(got, want, bound):
            return float(np.max(np.abs(got.astype(LD) - want).astype(np.float64) / np.maximum(bound, 1e-300)))
        q = dict(gv=ratio(gv[b, :, :r_].T, gref, lr.K_G(P) * U * env), gtu=ratio(gtu[b, :, :n_].T, G.T @ ub.astype(LD), lr.K_GT(P) * U * (Gh.T @ np.abs(ub))),
                 wgv=ratio(wgv[b, :, :r_].T, S.winv2(gref) - sub[b, :, :r_].T.astype(LD), lr.K_WG(P) * U * S.abs_winv2(env) + 2 * U * np.abs(sub[b, :, :r_].T)),
                 H=ratio(np.tril(H[b, :n_, :n_]), np.tril(lr.H_ref(G, S)), lr.K_H(P) * U * lr.H_env(Gh, S)))
        print("    hetero lane %d (n = %d)  " % (b, P["args"][0]) + "  ".join("%s %.3f" % kv for kv in q.items()))
        assert all(x <= 1.0 for x in q.values()), q
        check_padding(H[b], n_)                               # (the shorter lane: identity from ITS N on)
        alone = mbfir.test_unit_ops([jobs[b]], v[b:b + 1, :, :n_], u[b:b + 1, :, :r_], s[b:b + 1, :r_], z[b:b + 1, :r_], sub=sub[b:b + 1, :, :r_], opts=opts)
        assert alone[4]["hetero"] == 0
        for got, one in ((gv[b, :, :r_], alone[0][0]), (gtu[b, :, :n_], alone[1][0]), (wgv[b, :, :r_], alone[2][0]), (np.tril(H[b]), np.tril(alone[3][0]))):
            assert np.array_equal(got, one)


TOGGLES = [("MBFIR_LANEPAIR", "0", dict(lanepair=0)), ("MBFIR_FUSE", "0", dict(fuse=0)), ("MBFIR_CGRP", "1", dict(cgrp=1)),
           ("MBFIR_FOLD", "0", dict(fold=0)), ("dense_trig", "1", {})]


@pytest.mark.parametrize("name", ["c1_ap24", "c2_ap150"])
@pytest.mark.parametrize("switch,value,sw", TOGGLES, ids=[t[0] for t in TOGGLES])
def test_one_switch_at_a_time(name, switch, value, sw, monkeypatch):
    """Each switch against the default, on a single design and on a unit of two: within the bounds on its own path (the report
    says which), and where the product promises the same bits (MBFIR_LANEPAIR, MBFIR_FUSE) the same bits."""
    base1, base2 = call(name, [0], "A")[0], call(name, [0, 1], "A")[0]
    dense = switch == "dense_trig"
    opt = dict(dense_trig=1) if dense else {}
    if not dense:
        monkeypatch.setenv(switch, value)
    (g1, t1, w1, H1, rep1), _ = call(name, [0], "A", **opt)
    (g2, t2, w2, H2, rep2), _ = call(name, [0, 1], "A", **opt)
    print("  %s %s=%s report %s" % (name, switch, value, rep2))
    check_report(name, rep1, 1, dense=dense, **sw)
    check_report(name, rep2, 2, dense=dense, **sw)
    check_lane(name, 0, "A", g1[0], t1[0], w1[0], H1[0], dense=dense, tag=switch)
    for q in (0, 1):
        check_lane(name, q, "A", g2[q], t2[q], w2[q], H2[q], dense=dense, tag=switch + " unit of 2")
    if switch in ("MBFIR_LANEPAIR", "MBFIR_FUSE"):
        for got, was in zip((g1, t1, w1, np.tril(H1[0])), (base1[0], base1[1], base1[2], np.tril(base1[3][0]))):
            assert np.array_equal(got, was)
        for got, was in zip((g2, t2, w2, np.tril(H2[0]), np.tril(H2[1])), (base2[0], base2[1], base2[2], np.tril(base2[3][0]), np.tril(base2[3][1]))):
            assert np.array_equal(got, was)


def test_context_solves_as_before_after_the_hook_and_out_of_scope_units_are_refused():
    from conftest import CASES as GOLDEN
    fn, args = CASES["c1_ap24"]["job"]
    ctx = mbfir.get_context()
    h0, st0 = mbfir.fir_ap_cvx(*GOLDEN["ap_lowpass20"][1], ctx=ctx)
    call("c1_ap24", [0, 1, 2], "A")
    h1, st1 = mbfir.fir_ap_cvx(*GOLDEN["ap_lowpass20"][1], ctx=ctx)
    assert st0 == st1 == "Solved" and np.array_equal(h0, h1)
    I = inputs("c1_ap24", 0)
    with pytest.raises(ValueError, match="row-sharded"):
        mbfir.test_unit_ops([(fn, args)], I["A"]["v"][None], I["A"]["u"][None], I["s"][None], I["z"][None], opts=mbfir.make_opts(grid_m=512, shard_size=2))
    J = inputs("c6_qp25", 0)
    with pytest.raises(ValueError, match="extended-precision"):
        mbfir.test_unit_ops([CASES["c6_qp25"]["job"]], J["A"]["v"][None], J["A"]["u"][None], J["s"][None], J["z"][None])
