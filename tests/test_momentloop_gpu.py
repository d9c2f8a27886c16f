"""The paired lattice kernels take their operands by row broadcast: k_trig_moments_pair (G'v and the normal-matrix moments, one
or two operands per lane) and k_trig_eval_pair (G v) run their recurrences in blocks of 16 steps, lane r of every row of 16 lanes loads the operands of
step r and each step's FMAs read them from that lane; the last block of a chunk (of a segment) runs past its end on zeros.  k_fold_partials runs in
256-thread workgroups.  Not one bit may move: a lane of a unit equals its single solve, which runs the unpaired kernels.

Solves (taps, status, iteration count and objective compared with ==, MBFIR_LANEPAIR on and off; the designs are those of test_lanepair2_gpu.py,
all "Solved" in the CPU oracle, iteration counts in that file's docstring).  What the shapes are for, asserted from the mbfir_test_unit_ops report:
  n = 24, grid_m = 512     nchunk = 25, cgrp = 4: seven chunk groups, the last one ragged (one chunk); chunks of 1, 2, 4, 8, 16, 32, 63 and 64
                           frequencies, so blocks of 16 steps that end past the chunk; D1 = 24: a partly filled wave with rows of 16 lanes that
                           hold no point at all
  ... MBFIR_CGRP = 1, 3    25 and 9 groups: other trip counts of the chunk loop (one chunk alone; a pair and a lone third), k_fold_partials
                           with 25 partials (more than its 16 groups, no multiple of them) and 9 (fewer)
  three lanes              the last pair runs the one-lane body
  loose and tight ripples  a lane finishes (is masked) long before its partner
  fir_qprog_phs n = 21     several rows per frequency in the gather, a quad program
  fir_linprog n = 64       two plain operands per lane in every G'v
Operators against the longdouble reference of lattice_ref.py (its bounds; no solve): n = 300 at grid_m = 512, D1 = 300 > 256, so G'v has two moment
blocks and the build's 899 points four, G v five segments of 64 the last of which holds 44 points (no multiple of 16); units of two and of three lanes
and a unit with one lane masked, every live lane also == itself alone.  n = 24 at grid_m = 4096 under MBFIR_CGRP = 1 (56 chunks: k_fold_partials
folds more than 48 partials, its unrolled loop) and the dense twin of n = 24, grid_m = 512 (dense_trig: k_fold_partials on the border products
A1'BB of the slack column, ld = 128, five partials).
Shapes the product cannot produce are not tested: k_fold_partials' leading dimension is a multiple of 256 on the lattice path and of 128 on the
dense one, never an odd multiple of 16.
"""
import os

import numpy as np
import pytest

import lattice_ref as lr
import mbfir

pytestmark = pytest.mark.gpu
LD, U = lr.LD, lr.U
LOOSE, MID, TIGHT = (0.1, 0.05), (0.05, 0.03), (0.02, 0.01)
SWITCHES = ("MBFIR_LANEPAIR", "MBFIR_FUSE", "MBFIR_CGRP", "MBFIR_FOLD")


def c13(ripple, peak, n=24):
    f, a, d = mbfir.spec.spec_c13_bssfp(n, T=2.0, d1=ripple[0], d2=ripple[1])
    return ("fir_ap_cvx", (n, f, a, d, 0.1, peak))


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def ctx():
    c = mbfir.Context(0)
    yield c
    c.close()


_single = {}


def single(ctx, job, grid_m):
    """The design's single solve under the switches in force, computed once per module."""
    name, args = job
    key = (name, grid_m, os.environ.get("MBFIR_CGRP")) + tuple(np.asarray(x, dtype=complex).tobytes() for x in args)
    if key not in _single:
        _single[key] = mbfir.solve_batch([job], ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=1, grid_m=grid_m))[0]
    return _single[key]


def same(r, ref):
    (h, s, i), (h0, s0, i0) = r, ref
    assert s == s0 == "Solved"
    assert i["iters"] == i0["iters"] and i["pcost"] == i0["pcost"]
    assert np.array_equal(h, h0)


def report(jobs, grid_m):
    """The path a unit of these designs takes, from the hook (any interior iterate)."""
    P = lr.program(jobs[0][0], jobs[0][1], grid_m)
    nl = len(jobs)
    s, z = lr.draw_sz(P, np.random.default_rng(7), wide=False)
    rep = mbfir.test_unit_ops(jobs, np.ones((nl, 1, P["N"])), np.ones((nl, 1, P["R"])), np.tile(s, (nl, 1)), np.tile(z, (nl, 1)), opts=mbfir.make_opts(grid_m=grid_m))[4]
    print("  report %s" % rep)
    return rep


def unit_equals_singles(ctx, jobs, grid_m, monkeypatch):
    refs = [single(ctx, j, grid_m) for j in jobs]
    assert all(r[2]["pair_passes"] == 0 for r in refs)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MBFIR_LANEPAIR", mode)
        out[mode] = mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=len(jobs), grid_m=grid_m))
        print("MBFIR_LANEPAIR=%s: iters %s, pair_passes %s" % (mode, [r[2]["iters"] for r in out[mode]], [r[2]["pair_passes"] for r in out[mode]]))
        assert all(r[2]["lanes"] == len(jobs) for r in out[mode])
        assert all((r[2]["pair_passes"] > r[2]["gv_passes"]) if mode == "1" else (r[2]["pair_passes"] == 0) for r in out[mode])
    monkeypatch.delenv("MBFIR_LANEPAIR")
    for r1, r0 in zip(out["1"], out["0"]):
        same(r1, r0)
    for mode in ("1", "0"):
        for r, ref in zip(out[mode], refs):
            same(r, ref)
    return refs


FOUR = [c13(LOOSE, 1e-2), c13(MID, 1e-2), c13(LOOSE, 1e-3), c13(MID, 1e-3)]


@pytest.mark.parametrize("cgrp", [None, "1", "3"])
def test_ragged_last_chunk_group(ctx, monkeypatch, cgrp):
    if cgrp:
        monkeypatch.setenv("MBFIR_CGRP", cgrp)
    rep = report(FOUR, 512)
    g = int(cgrp or 4)
    assert rep["lattice"] == 1 and rep["cgrp"] == g and rep["D1"] == 24 and rep["pair_passes"] > 0
    ngroups = -(-rep["nchunk"] // g)
    assert ngroups >= 3 and ngroups % 16 != 0 and (rep["nchunk"] % g != 0 or g != 4)
    assert (ngroups > 16) == (g == 1)                       # k_fold_partials: more partials than groups, and fewer
    assert mbfir.test_fold(lr.program(*FOUR[0], 512)["w"])["longest"] == 64
    unit_equals_singles(ctx, FOUR, 512, monkeypatch)


def test_odd_unit(ctx, monkeypatch):
    unit_equals_singles(ctx, FOUR[:3], 512, monkeypatch)


def test_lane_finishes_early(ctx, monkeypatch):
    refs = unit_equals_singles(ctx, [c13(TIGHT, 0.1), c13(LOOSE, 0.1), c13(LOOSE, 1e-2), c13(TIGHT, 0.3)], 512, monkeypatch)
    it = [r[2]["iters"] for r in refs]
    assert it[0] - it[1] >= 5 and it[3] - it[2] >= 5, it


def test_several_rows_per_frequency(ctx, monkeypatch):
    f, a, d = [-0.6, -0.3, -0.1, 0.1, 0.3, 0.6], [0, 0, 1, 1, 0, 0], [0.02, 0.05 * np.exp(0.3j), 0.02]
    jobs = [("fir_qprog_phs", (21, f, [v * s for v in a], d)) for s in (1.0, 0.97, 1.03, 0.94)]
    P = lr.program(*jobs[0], 0)
    assert P["quad"] and np.bincount(P["freq"][P["freq"] >= 0]).max() > 2
    unit_equals_singles(ctx, jobs, 0, monkeypatch)
    unit_equals_singles(ctx, jobs[:3], 0, monkeypatch)


def test_two_operands(ctx, monkeypatch):
    jobs = [("fir_linprog", (64, [0, .2, .3, 1], [1, 1, 0, 0], [.01, .01])), ("fir_linprog", (64, [0, .2, .3, 1], [1, 1, 0, 0], [.02, .015]))]
    refs = unit_equals_singles(ctx, jobs, 512, monkeypatch)
    assert not lr.program(*jobs[0], 512)["quad"] and all(r[2]["gtv_passes"] > 0 for r in refs)


# ---- operators against the dense reference ---------------------------------------------------------------------------------
BIG = dict(job=lr._c13(300), grid_m=512)
FINE = dict(job=lr._c13(24), grid_m=4096)
SMALL = dict(job=lr._c13(24), grid_m=512)
_P, _IN, _REF = {}, {}, {}


def prog(c):
    k = id(c)
    if k not in _P:
        _P[k] = lr.program(c["job"][0], c["job"][1], c["grid_m"])
    return _P[k]


def inputs(c, b):
    """Lane b's iterate and vectors (two per space; lane 1 with orthant weights spread over 1e8): the same whenever asked for."""
    if (id(c), b) not in _IN:
        P = prog(c)
        rng = np.random.default_rng([41, b])
        s, z = lr.draw_sz(P, rng, wide=(b == 1))
        _IN[(id(c), b)] = dict(s=s, z=z, v=rng.standard_normal((2, P["N"])), u=rng.standard_normal((2, P["R"])), sub=rng.standard_normal((2, P["R"])))
    return _IN[(id(c), b)]


def h_rows(P):
    N = P["N"]
    if N <= 128:
        return np.arange(N)
    fixed = [0, 1, N - 2, N - 1, P["Nt"] // 2 - 1, P["Nt"] // 2, P["Nt"] - 1] + [e + d for e in range(64, N, 64) for d in (-1, 0)]
    return np.unique(np.clip(np.concatenate([fixed, np.random.default_rng(3).choice(N, 8, replace=False)]), 0, N - 1))


def ref(c, b):
    """Reference values and envelopes of lane b, computed once."""
    k = (id(c), b)
    if k not in _REF:
        P, I = prog(c), inputs(c, b)
        if ("G", id(c)) not in _REF:
            _REF[("G", id(c))] = (lr.G_ref(P), lr.G_hat(P))
        G, Gh = _REF[("G", id(c))]
        S, rows = lr.Scaling(P, I["s"], I["z"]), h_rows(P)
        _REF[k] = dict(rows=rows, H=lr.H_ref(G, S, rows), E=lr.H_env(Gh, S, rows), gv=(G @ I["v"].T.astype(LD)).T, env_gv=(Gh @ np.abs(I["v"].T)).T,
                       gtu=(G.T @ I["u"].T.astype(LD)).T, env_gtu=(Gh.T @ np.abs(I["u"].T)).T)
    return _REF[k]


def call(c, lanes, mask=None, **opt):
    P = prog(c)
    I = [inputs(c, b) for b in lanes]
    nl, npad = len(lanes), -(-P["N"] // 64) * 64
    init = (np.full((nl, 2, P["R"]), 7.25), np.full((nl, 2, P["N"]), -3.5), np.full((nl, 2, P["R"]), 1.75), np.full((nl, npad, npad), -9.125))
    out = mbfir.test_unit_ops([c["job"]] * nl, np.stack([x["v"] for x in I]), np.stack([x["u"] for x in I]), np.stack([x["s"] for x in I]),
                              np.stack([x["z"] for x in I]), sub=np.stack([x["sub"] for x in I]), mask=mask,
                              opts=mbfir.make_opts(grid_m=c["grid_m"], **opt), init=init)
    return out, init


def check_lane(c, b, gv, gtu, H, dense=False, tag=""):
    """G v, G'u and the compared rows of H within lattice_ref's bounds; returns the worst error / bound of each."""
    P, r = prog(c), ref(c, b)
    N, rows = P["N"], r["rows"]

    def ratio(got, want, bound):
        assert np.all(np.isfinite(got))
        return float(np.max(np.abs(got.astype(LD) - want).astype(np.float64) / np.maximum(bound, 1e-300)))
    low = np.arange(N)[None, :] <= rows[:, None]
    q = dict(gv=ratio(gv, r["gv"], lr.K_G(P, dense) * U * r["env_gv"]), gtu=ratio(gtu, r["gtu"], lr.K_GT(P, dense) * U * r["env_gtu"]),
             H=float(np.max(np.where(low, np.abs(H[rows, :N].astype(LD) - r["H"]).astype(np.float64) / np.maximum(lr.K_H(P, dense) * U * r["E"], 1e-300), 0.0))))
    print("    lane %d %s  " % (b, tag) + "  ".join("%s %.3f" % kv for kv in q.items()))
    for k, x in q.items():
        assert x <= 1.0, "lane %d %s: %s is %.3g times its bound" % (b, tag, k, x)


_alone = {}


def alone(c, b, key=None, **opt):
    if (id(c), b, key) not in _alone:
        (gv, gtu, wgv, H, rep), _ = call(c, [b], **opt)
        assert rep["pair_passes"] == 0
        _alone[(id(c), b, key)] = (gv[0], gtu[0], wgv[0], np.tril(H[0]))
    return _alone[(id(c), b, key)]


def unit_against_reference(c, lanes, mask=None, key=None, dense=False, **opt):
    (gv, gtu, wgv, H, rep), init = call(c, lanes, mask=mask, **opt)
    print("  unit %s mask %s report %s" % (lanes, mask, rep))
    for q, b in enumerate(lanes):
        if mask and not mask[q]:
            for got, was in zip((gv, gtu, wgv, H), init):       # a masked lane: every output as it went in
                assert np.array_equal(got[q], was[q])
            continue
        check_lane(c, b, gv[q], gtu[q], H[q], dense=dense, tag="unit of %d" % len(lanes))
        for got, one in zip((gv[q], gtu[q], wgv[q], np.tril(H[q])), alone(c, b, key, **opt)):
            assert np.array_equal(got, one)
    return rep


@pytest.mark.parametrize("lanes,mask", [([0, 1], None), ([0, 1, 2], None), ([0, 2, 1], [1, 0, 1])], ids=["two", "three", "masked"])
def test_operators_two_moment_blocks(lanes, mask):
    rep = unit_against_reference(BIG, lanes, mask)
    assert rep["lattice"] == 1 and rep["D1"] == 300 and rep["cgrp"] == 4 and rep["seg"] == 64 and rep["useg"] == 5 and rep["nchunk"] > 3 * rep["cgrp"]
    assert rep["pair_passes"] == (4 if rep["one_pass"] else 5) and rep["lanes"] == len(lanes)      # both row responses, G'u, the build's moment passes


def test_operators_fold_more_than_48_partials(monkeypatch):
    monkeypatch.setenv("MBFIR_CGRP", "1")
    rep = unit_against_reference(FINE, [0, 1], key="cgrp1")
    assert rep["cgrp"] == 1 and rep["nchunk"] > 48 and rep["nchunk"] % 16 != 0 and rep["pair_passes"] == (4 if rep["one_pass"] else 5)


def test_operators_dense_border_products():
    P = prog(SMALL)
    assert P["Ne"] > 0 and -(-P["Mf"] // 128) < 16              # the slack column: build_H folds the five partials of A1'BB
    rep = unit_against_reference(SMALL, [0, 1], key="dense", dense=True, dense_trig=1)
    assert rep["lattice"] == 0 and rep["pair_passes"] == 0
