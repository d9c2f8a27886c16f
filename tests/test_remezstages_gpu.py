"""k_remez iterate by iterate, and k_fmp at its small tiers, against the long-double reference of tests/remez_ref.py (checked on the
host by tests/test_remezstages_cpu.py).

One launch per maxiter = 1 .. K and grid density, every spec of remez_ref.SPECS in it (K = the largest iteration count of the
long-double replay, 16): with maxiter = k the kernel returns the set it solved on in iteration k, that iteration's delta and the taps
of its interpolant, so the sweep shows every iterate through the public remez_batch.  Per spec and k (remez_ref.check_sweep): the
start set, status and iteration count, delta_k within its envelope, ext_{k+1} equal to exchange(solve(ext_k)) index for index (a
near-tie allowance exists and is counted), h_k within its bound and exactly symmetric, the certificate at K_s, and the default
maxiter = 25 bit-identical to maxiter = K_s.  The taps use the FALLBACK bound (ten times the distance of the restatement
remez_ref.Kern64 from the reference for the same set, floor 1e-15 max|h|): the derived envelope lies a median of 120 times, and up
to 7000 times, above what the restatement achieves.  pytest -s prints the worst error / bound per spec.

Measured on one MI355X (worst over the iterates of a spec; 208 (spec, iteration) pairs, 3 launches per k, the file in 20 s):
    spec                 taps  G     K_s  delta err/env  env / |delta|  amplification  taps err/bound
    tiny3 .. tiny6       3-6   22-33 2-3  0.009 - 0.054  5e-15 - 2e-14  1 - 8          0.10 - 0.21
    frexp29 .. frexp32   29-32 215-  5-6  0.037 - 0.077  1e-13 - 2e-13  42 - 50        0.16 - 0.37
    nodes509 .. nodes513 509-  4039- 7-15 0.011 - 0.045  1e-10          3e3 - 4e3      0.15 - 0.32
    bp60_type2_below1    60    288   14   0.078          4e-12          9e2            0.35
    hp41                 41    302   6    0.041          4e-12          1e3            0.11
    point45              45    333   7    0.069          1e-12          3e2            0.20
    oneband21            21    176   5    0.047          4e-13          1e2            0.30
    eight121             121   770   12   0.044          6e-12          7e2            0.22
    comb64               513   1216  16   0.047          5e-9           2e5            0.30
    w1e4_101             101   735   13   0.033          2e-11          3e3            0.43
    G255 .. G513         33    255-  4-5  0.038 - 0.078  2e-13          51 - 71        0.22 - 0.33
    density 8 / 32       31,60 116-  6-14 0.041 - 0.099  1e-13 - 4e-12  44 - 9e2       0.20 - 0.47
The near-tie allowance was used in 0 of the 208 pairs: every exchange of the device equals the reference's index for index.
fmp: 3e-15 .. 1.5e-12 max|h| (bound 1e-9); dzrf at np = 64: 2e-15 (ex) and 1e-10 (se) of max|rf| (bound 1e-7).

What the first run of this file found: on w1e4_101 the certificate stood at 1.24e-8 |delta| against
CERT_TOL = 1e-8, because the taps were recovered from fp64 weights and fp64 barycentric sums (8e-15 in the taps, times W / delta =
1.5e6).  The tap recovery of k_remez now redoes weights, delta and node values in double-double; the certificate on that spec stands
at 4.7e-10, and the exchange, delta, ext and iteration counts of every design are bit for bit what they were.

That the tests can fail -- four arithmetic-only changes to remez.hip, each built apart and this file (44 tests) run once on it:
    sign of sgn in delta's denominator      41 fail: all 28 sweeps on `delta` at iteration 1; the fmp inputs, dzrf and the valid call of
                                            the rejection test no longer converge; pass: near-tie count, batch independence, fmp l = 1
    >= to > in run_winner's backward scan   0 fail.  Two candidates of one run never have the same |E| to the last bit in any of the
                                            208 pairs (between two nodes of equal sign there is always a candidate of the other sign),
                                            so no spec can show it; tests/test_remezstages_cpu.py pins the rule on planted equal maxima
    0.5 a[k] -> a[k] in the type I taps     20 fail: the 20 type I sweeps on `taps` at iteration 1; pass: the 8 type II sweeps, fmp
                                            (a scaled input), dzrf at even np
    delf from density (L + 1)               30 fail: all 28 sweeps on `ext` (not a grid point), dzrf (2e-3, 7e-3); pass: fmp, rejections
"""
import ctypes as C

import numpy as np
import pytest

import mbfir
import remez_ref as rr
from mbfir import slrclassic
from oracle import slr

pytestmark = pytest.mark.gpu
_RUNS = {}
FMP_LENGTHS, fmp_input = rr.FMP_LENGTHS, rr.fmp_input


def _launch(names, density, maxiter):
    res = mbfir.remez_batch([rr.SPECS[n][:4] for n in names], grid_density=density, maxiter=maxiter)
    return {n: dict(h=h, status=i["status"], iterations=i["iterations"], delta=i["delta"], ext=i["ext"]) for n, (h, i) in zip(names, res)}


def device_runs():
    """runs[name][k] for k = 1 .. K and runs[name][0] at the default maxiter: one launch per k and density."""
    if not _RUNS:
        K = max(rr.replay(n)[1] for n in rr.NAMES)
        assert K <= 25
        for n in rr.NAMES:
            _RUNS[n] = {}
        for dens in sorted(set(s[4] for s in rr.SPECS.values())):
            names = [n for n in rr.NAMES if rr.SPECS[n][4] == dens]
            for k in list(range(1, K + 1)) + [25]:
                for n, r in _launch(names, dens, k).items():
                    _RUNS[n][0 if k == 25 else k] = r
    return _RUNS


def sweep(name, stats=None):
    runs = dict(device_runs()[name])
    default = runs.pop(0)
    return rr.check_sweep(name, runs, default_run=default, stats=stats)


@pytest.mark.parametrize("name", rr.NAMES)
def test_every_iterate(name):
    st = {}
    try:
        sweep(name, st)
    finally:
        print("%-18s K %2d  delta err/env %.3f (env %.1e of |delta|, amplification %.1e)  taps err/bound %.3f  near-ties %d of %d"
              "  delta bits as the restatement's %d" % (name, st["K"], st["delta"], st["env_rel"], st["amp"], st["taps"], st["ties"],
                                                        st["pairs"], st["same_delta"]))


def test_near_tie_allowance_is_rare():
    """At most one (spec, iteration) pair in twenty may use the allowance (check_sweep grants none below 40 taps)."""
    pairs = ties = 0
    for n in rr.NAMES:
        st = {}
        try:
            sweep(n, st)
        except rr.Miss:
            pass                                                # (test_every_iterate reports it; the pairs before it count)
        pairs, ties = pairs + st["pairs"], ties + st["ties"]
    print("near-ties: %d of %d (spec, iteration) pairs" % (ties, pairs))
    assert 20 * ties <= pairs, (ties, pairs)


def _same(a, b):
    return (np.array_equal(a["h"], b["h"]) and a["delta"] == b["delta"] and np.array_equal(a["ext"], b["ext"])
            and a["status"] == b["status"] and a["iterations"] == b["iterations"])


def test_batch_independence():
    """Every spec of the table in one batch is bit-identical to the spec alone and to the batch reversed."""
    runs = device_runs()
    for dens in sorted(set(s[4] for s in rr.SPECS.values())):
        names = [n for n in rr.NAMES if rr.SPECS[n][4] == dens]
        rev = _launch(names[::-1], dens, 25)
        for n in names:
            assert _same(runs[n][0], rev[n]), ("reversed", n)
            assert _same(runs[n][0], _launch([n], dens, 25)[n]), ("alone", n)


# ---- the C-level argument checks ------------------------------------------------------------------------------------------
def _raw(ctx, numtaps, edges, desired, weight, nband=None, kind=0, density=16, maxiter=25):
    e, d, w = (np.ascontiguousarray(v, dtype=np.float64) for v in (edges, desired, weight))
    h, ext = np.zeros(4096), np.zeros(4096)
    job = (mbfir.RemezJob * 1)()
    job[0].numtaps, job[0].nband, job[0].type = numtaps, len(w) if nband is None else nband, kind
    job[0].edges, job[0].desired, job[0].weight = (v.ctypes.data_as(mbfir._dp) for v in (e, d, w))
    job[0].h, job[0].ext = h.ctypes.data_as(mbfir._dp), ext.ctypes.data_as(mbfir._dp)
    opts = mbfir.RemezOpts(density, maxiter)
    rc = mbfir.load_library().mbfir_remez_batch(ctx._h, job, 1, C.byref(opts))
    return rc, ctx.last_error(), h[:max(numtaps, 0)], job[0].status


def test_argument_rejections_leave_the_context_usable():
    ctx = mbfir.get_context()
    lp = ([0, .2, .3, 1], [1, 1, 0, 0], [1, 1])
    good = mbfir.remez(21, *lp)
    e65 = [v for b in range(65) for v in (2 * b / 131, (2 * b + 1) / 131)]
    J = "remez job 0: "
    for what, args, kw, msg in (
            ("grid smaller than L + 1", (33, [0, .02, .05, .08], [1, 1, 0, 0], [1, 1]), {}, J + "dense grid smaller than L + 1"),
            ("touching bands", (21, [0, .2, .2, 1], [1, 1, 0, 0], [1, 1]), {}, J + "bands must not touch"),
            ("nband = 65", (513, e65, [1.0] * 130, [1.0] * 65), {}, J + "nband must be in [1, 64]"),
            ("zero weight", (21, lp[0], lp[1], [1, 0]), {}, J + "weights must be positive"),
            ("non-finite desired", (21, lp[0], [1, np.inf, 0, 0], lp[2]), {}, J + "desired amplitude not finite"),
            ("NaN desired", (21, lp[0], [1, 1, np.nan, 0], lp[2]), {}, J + "desired amplitude not finite"),
            ("numtaps 2", (2,) + lp, {}, J + "numtaps must be in [3, 2047]"),
            ("numtaps 2048", (2048,) + lp, {}, J + "numtaps must be in [3, 2047]"),
            ("density 1025", (21,) + lp, dict(density=1025), "remez: bad batch or options"),
            ("maxiter 10001", (21,) + lp, dict(maxiter=10001), "remez: bad batch or options"),
            ("type 1", (21,) + lp, dict(kind=1), J + "only symmetric (bandpass) filters"),
            ("type 2", (21,) + lp, dict(kind=2), J + "only symmetric (bandpass) filters")):
        rc, err, _, _ = _raw(ctx, *args, **kw)
        assert rc == mbfir.E_ARG and err.startswith(msg), (what, rc, err)
        rc, err, h, status = _raw(ctx, 21, *lp)                 # a valid call still works, and gives the same bits
        assert rc == 0 and status == 0 and np.array_equal(h, good), what


# ---- fmp at its small tiers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", (3, 5) + FMP_LENGTHS)
def test_fmp_small_tiers(l):
    """lp = 32, 64 (l = 3, 5) and 256 .. 4096, on the device's own design; real taps and taps modulated to complex ones with a
    real spectrum; against fmp.m restated in long double (dense DFT, lp <= 512; fp64 fmp_np beyond): 1e-9 max|h|."""
    h = mbfir.remez(*fmp_input(l))
    assert len(h) == l
    for name, hh in (("real", h), ("modulated", h * np.exp(0.7j * (np.arange(l) - (l - 1) / 2)))):
        got, ref = mbfir.fmp(hh), rr.fmp_ref(hh)
        err = float(np.abs(got - ref).max() / np.abs(h).max())
        print("fmp l = %3d %-9s err %.2e" % (l, name, err))
        assert got.shape == ((l + 1) // 2,) and err <= 1e-9, (l, name, err)


def test_fmp_single_tap():
    got, ref = mbfir.fmp([0.25]), rr.fmp_ref([0.25])
    assert got.shape == (1,) and np.isfinite(got).all() and abs(got[0] - ref[0]) <= 1e-9 * 0.25, (got, ref)


# ---- dzrf on the type II dzlp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", ("ex", "se"))
def test_dzrf_even_np_matches_reference_chain(ptype):
    n, tb = 64, 6.0
    d1, d2, bsf = slrclassic.ptype_ripples(ptype, 0.01, 0.01)
    b = rr.replay_taps(*slrclassic.dzlp_spec(n, tb, d1, d2))
    r = slr.b2rf(bsf * np.asarray(b, dtype=np.complex128))
    rf = mbfir.dzrf(n, tb, ptype, "pm", 0.01, 0.01)
    err = np.abs(rf - r).max() / np.abs(r).max()
    print("dzrf np = 64 %s pm: %.2e" % (ptype, err))
    assert len(rf) == n and err <= 1e-7, (ptype, err)
