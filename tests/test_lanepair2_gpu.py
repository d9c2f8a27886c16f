"""Lane pairs, second part: the normal-matrix moment pass (k_trig_moments_pair<NV, false>) and the residual's G x
(k_trig_eval_pair<1> through trig_eval) run paired as well, and the paired moment kernels gather their operands side by side and load
their seeds ahead of the staging.  As in test_lanepair_gpu.py not one bit may move: each design of a unit equals its single solve
(lanes=1) with MBFIR_LANEPAIR on and off -- taps, status, iteration count and objective, compared with ==.

What the sizes are for: the H-build runs 3 D1 - 1 moment points in workgroups of 256, G'v runs D1.  n = 24 (71 and 24 points) and n = 64
(191 and 64) stay inside one partly filled workgroup; n = 150 (449 and 150 points, D1 no multiple of 64) gives the build two workgroups
along the moment axis, the second partly filled.

The designs were checked in the CPU oracle first (all "Solved"; iteration counts there: the n = 24 bSSFP designs 17 ... 21, the tight
pair of the uneven unit 41 and 43 against 17 for the loose one; fir_linprog 15 and 16; the spec_rand draws 15 and 18; the n = 64 sweep
23 ... 34; the four n = 150, T = 2 ms designs at grid_m = 2048: 30, 30, 30 and 27; the four fir_qprog_phs designs 19 each).
"""
import os
import sys

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu

LOOSE, MID, TIGHT = (0.1, 0.05), (0.05, 0.03), (0.02, 0.01)


def c13(ripple, peak, n=24):
    f, a, d = mbfir.spec.spec_c13_bssfp(n, T=2.0, d1=ripple[0], d2=ripple[1])
    return ("fir_ap_cvx", (n, f, a, d, 0.1, peak))


class lanepair:
    def __init__(self, mode):
        self.mode = str(mode)

    def __enter__(self):
        self.old = os.environ.get("MBFIR_LANEPAIR")
        os.environ["MBFIR_LANEPAIR"] = self.mode

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MBFIR_LANEPAIR", None)
        else:
            os.environ["MBFIR_LANEPAIR"] = self.old


@pytest.fixture(scope="module")
def ctx():
    c = mbfir.Context(0)
    yield c
    c.close()


_single = {}


def single(ctx, job, grid_m):
    """The design's single solve, computed once per module."""
    name, args = job
    key = (name, grid_m) + tuple(np.asarray(x, dtype=complex).tobytes() for x in args)
    if key not in _single:
        _single[key] = mbfir.solve_batch([job], ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=1, grid_m=grid_m))[0]
    return _single[key]


def same(r, ref):
    (h, s, i), (h0, s0, i0) = r, ref
    assert s == s0 == "Solved"
    assert i["iters"] == i0["iters"] and i["pcost"] == i0["pcost"]
    assert np.array_equal(h, h0)


def new_passes_counted(infos, all_gtv_pair):
    """pair_passes is the unit's count.  Every G v of a paired unit runs k_trig_eval_pair, the residual's included, and every iteration
    builds the normal matrix once through at least one paired moment pass: pair_passes >= gv_passes + iterations of the unit + 1 (the G'v
    of the residual, one operand, pairs in every program).  Where every G'v pairs as well (one or two operands: a program without the
    quadratic rows) the paired passes outnumber G v and G'v together -- without the build's passes they could not."""
    for i in infos:
        print("pair_passes %d, gv_passes %d, gtv_passes %d, iters %d" % (i["pair_passes"], i["gv_passes"], i["gtv_passes"], i["iters"]))
    unit_iters = max(i["iters"] for i in infos)
    for i in infos:
        assert i["pair_passes"] > i["gv_passes"]
        assert i["pair_passes"] >= i["gv_passes"] + unit_iters + 1
        if all_gtv_pair:
            assert i["pair_passes"] > i["gv_passes"] + i["gtv_passes"]


def unit_equals_singles(ctx, jobs, grid_m, modes=("1", "0"), unit=None, paired=True, all_gtv_pair=False):
    """info["pair_passes"] counts the passes of the unit that launched the paired kernels: > 0 where the test is about them
    (switch on, `paired`), 0 with the switch off, in the fallback units and in every single solve."""
    refs = [single(ctx, j, grid_m) for j in jobs]
    assert all(r[2]["pair_passes"] == 0 for r in refs)
    out = {}
    for mode in modes:
        with lanepair(mode):
            out[mode] = mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=len(jobs), grid_m=grid_m))
        print("MBFIR_LANEPAIR=%s: lanes %s, iters %s" % (mode, [r[2]["lanes"] for r in out[mode]], [r[2]["iters"] for r in out[mode]]))
        assert all(r[2]["lanes"] == (unit or len(jobs)) for r in out[mode])
        if paired and mode == "1":
            new_passes_counted([r[2] for r in out[mode]], all_gtv_pair)
        else:
            assert all(r[2]["pair_passes"] == 0 for r in out[mode]), [r[2]["pair_passes"] for r in out[mode]]
    if len(modes) == 2:                                     # paired against unpaired first: what the switch itself must not move
        for r1, r0 in zip(out["1"], out["0"]):
            same(r1, r0)
    for mode in modes:
        for r, ref in zip(out[mode], refs):
            same(r, ref)
    return refs


def test_even_unit(ctx):
    """Four designs on one grid (a quad program): two full pairs through the paired H-build and the paired residual pass."""
    unit_equals_singles(ctx, [c13(LOOSE, 1e-2), c13(MID, 1e-2), c13(LOOSE, 1e-3), c13(MID, 1e-3)], 512)


def test_odd_unit(ctx):
    """Three designs: the last pair has no partner and runs the one-lane body of both passes."""
    unit_equals_singles(ctx, [c13(LOOSE, 1e-2), c13(MID, 1e-2), c13(LOOSE, 1e-3)], 512)


def test_uneven_finish(ctx):
    """A loose and a tight ripple pair: in both pairs one lane is done (masked off) long before its partner -- the second lane of the
    first pair, the first lane of the second -- so the build's moment pass and the residual run their one-live-lane body."""
    jobs = [c13(TIGHT, 0.1), c13(LOOSE, 0.1), c13(LOOSE, 1e-2), c13(TIGHT, 0.3)]
    refs = unit_equals_singles(ctx, jobs, 512)
    it = [r[2]["iters"] for r in refs]
    assert it[0] - it[1] >= 5 and it[3] - it[2] >= 5, it


def test_non_quad_program(ctx):
    """Other operand counts in moments_array; every G'v of this program has one or two operands and pairs."""
    jobs = [("fir_linprog", (64, [0, .2, .3, 1], [1, 1, 0, 0], [.01, .01])), ("fir_linprog", (64, [0, .2, .3, 1], [1, 1, 0, 0], [.02, .015]))]
    unit_equals_singles(ctx, jobs, 512, all_gtv_pair=True)


def test_several_rows_per_frequency(ctx):
    """fir_qprog_phs at n = 21 (the pass-band amplitude varies, the ripples and with them the half-planes per frequency stay): every
    frequency carries several rows, so the gathered operands of G'v are sums of several terms -- the only place where the order and the
    fusing of the gather's own sums show (with one row per frequency every sum starts at 0 and has one term)."""
    f, a, d = [-0.6, -0.3, -0.1, 0.1, 0.3, 0.6], [0, 0, 1, 1, 0, 0], [0.02, 0.05 * np.exp(0.3j), 0.02]
    jobs = [("fir_qprog_phs", (21, f, [v * s for v in a], d)) for s in (1.0, 0.97, 1.03, 0.94)]
    unit_equals_singles(ctx, jobs, 0)                       # (the designer's own grid, as the oracle ran them)
    unit_equals_singles(ctx, jobs[:3], 0)                   # (the last pair without a partner: the one-lane body's gather)


def test_two_workgroups_along_the_moment_axis(ctx):
    """n = 150, grid_m = 2048: D1 between 128 and 256 and no multiple of 64 -- the build's 449 moment points fill one workgroup and part
    of a second, G'v's 150 part of one."""
    unit_equals_singles(ctx, [c13(LOOSE, 1e-2, n=150), c13(MID, 1e-2, n=150), c13(LOOSE, 1e-3, n=150), c13(MID, 1e-3, n=150)], 2048)


def test_fallback_other_grids_same_order(ctx):
    """Lanes that do not share a grid run unpaired."""
    jobs = []
    for seed in (5, 8):
        f, a, d = mbfir.spec.spec_rand(24, seed)
        jobs.append(("fir_ap_cvx", (24, f, a, d, 0.1, 1e-2)))
    unit_equals_singles(ctx, jobs, 512, modes=("1",), paired=False)


def test_fallback_two_orders(ctx):
    """A unit across two orders (per-lane dimensions) runs unpaired."""
    unit_equals_singles(ctx, [c13(LOOSE, 1e-2, n=20), c13(LOOSE, 1e-2, n=24)], 512, modes=("1",), paired=False)


def test_unit_of_sixteen(ctx):
    """The bench's sweep (16 Peak values) as one unit of 16 at n = 64, grid_m = 1024: eight pairs, paired against unpaired."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from bench import sweep_jobs
    finally:
        sys.path.pop(0)
    jobs = sweep_jobs(mbfir, 64, 16)
    out = {}
    for mode in ("1", "0"):
        with lanepair(mode):
            out[mode] = mbfir.solve_batch(jobs, ctxs=[ctx], info=True, opts=mbfir.make_opts(lanes=16, grid_m=1024))
    assert all(r[2]["lanes"] == 16 for r in out["1"])
    new_passes_counted([r[2] for r in out["1"]], False)
    assert all(r[2]["pair_passes"] == 0 for r in out["0"])
    for r1, r0 in zip(out["1"], out["0"]):
        same(r1, r0)
