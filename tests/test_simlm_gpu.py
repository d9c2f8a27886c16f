"""The Levenberg-Marquardt step solved on the device (mbfir.abr_lm_step_batch / abr2_lm_step_batch: k_lm_init, k_abr_lm_sweep,
k_abr2_lm_sweep, k_lm_step, k_lm_trial and the shipped lsq kernels on the trial rf) and mbfir.refine_batch(solver="device") on it.

Exact, without a tolerance: the trial's loss and gradient are abr_lsq_batch's at rf + d; a pulse's outputs do not depend on the
batch, its order, or when its neighbours stop.  Against the dense solve: the project's 1e-4 max|d|
(test_first_step_is_the_dense_levenberg_marquardt_step).  Against the recurrence of tests/simlm_ref.py run on the shipped
abr_gn_batch as the operator: ncg equal, and for d a bound that is measured on code that is not under test.  The same recurrence
run on tests/simgn_ref.py's gn and on the shipped device gn differs by exactly an operator's rounding carried through the
recurrence; the device's CG adds dots summed in another order, which CG carries like an operator perturbation, so
    |d - d_ref| <= max(100 max over the shape's cg of |d_ref(simgn_ref) - d_ref(device gn)|, 1e-13 max|d_ref|)
For rr the same measurement does not serve: the two references' rr agree far better than their d (their d differ along
directions that H + mu I damps, which leave r alone; 4e-14 of rr against 2e-10 of max|d| at 257 samples, hard pulse, 'st'), so a
multiple of it says nothing about what a d inside the bound above may do to rr.  The recurrence keeps r = b - (H + mu I) d up to
rounding, so a d that is off by dd has r off by (H + mu I) dd, of norm at most dr = (trace(H) + mu) sqrt(2n) max|dd| (H is positive
semidefinite: its largest eigenvalue is at most its trace, taken from 2n shipped gn products), and
    |rr - rr_ref| <= 2 sqrt(rr_ref) dr + dr^2 + 2e-13 sqrt(rr_ref gg) + 1e-26 gg      with max|dd| the bound on d above,
the last two terms being the same with |dr| <= 1e-13 |b|, the floor.  DESIGN 8n has the figures measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1.0, 0.0, 0.9]
KINDS = ("ex", "se", "inv", "st")

_spec = importlib.util.spec_from_file_location("simlm_ref", os.path.join(ROOT, "tests", "simlm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
ref = lmref.gnref


def _pulses(seed, lengths, flips, two_d):
    """rf alone and (rf, g) in turn (g complex in 2D); total flip about flips[q]; for n >= 3 one rf sample is exactly zero"""
    rng = np.random.default_rng(seed)
    out = []
    for q, (n, flip) in enumerate(zip(lengths, flips)):
        rf = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (flip / n)
        if n >= 3:
            rf[n // 3] = 0.0
        g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n
        if two_d:
            g = g + 1j * rng.uniform(-1.5, 1.5, n) * 1e-2
        out.append((rf, g) if q % 2 or two_d else rf)
    return out


def _split(p):
    return p if isinstance(p, tuple) else (p, None)


def _moved(p, d):
    return (p[0] + d, p[1]) if isinstance(p, tuple) else p + d


def _grid(nx, span):
    x = np.linspace(-span, span, nx)
    x[nx // 2] = 0.0
    return x


def _fit(seed, shape, kind):
    """a target of the profile's size and weights a third of which are zero (and not all of them)"""
    rng = np.random.default_rng(seed)
    t = 0.5 * (rng.standard_normal(shape) + (0 if kind == "inv" else 1j) * rng.standard_normal(shape))
    w = rng.uniform(0.5, 2.0, shape) * (rng.uniform(size=shape) > 1 / 3)
    w[0].flat[0] = 1.0
    return t, w


def _dot(u, v):
    return float((np.conj(u) * v).real.sum())


def _call(two_d, which, pulses, xs, ys, *rest, **kw):
    fn = getattr(mbfir, ("abr2_" if two_d else "abr_") + which + "_batch")
    return fn(pulses, *((xs, ys) if two_d else (xs,)), *rest, **kw)


LENGTHS = [1, 7, 255, 256, 257]              # below, at and above the 256-sample tile and the step kernel's 256-thread stride
NXS = [1, 257, 257, 1, 257]                  # one point; two chunks, the last one partial
FLIPS = [0.3, 1.0, 0.5, 1.5, 2.0]
LEN2 = [7, 257]
COMBOS = ([(False, hard, kind) for kind in KINDS for hard in (False, True)]
          + [(True, k % 2 == 1, kind) for k, kind in enumerate(KINDS)])


@functools.lru_cache(maxsize=None)
def _case(two_d, hard, kind):
    """pulses, grids, fits, and per pulse b = -gradient at rf and mu = 1e-3 times the Rayleigh quotient of H at b (refine_batch's
    first mu), from the shipped device calls"""
    if two_d:
        pulses = _pulses(8, LEN2, [1.0, 2.0], True)
        xs, ys = [_grid(5, 3.0), _grid(5, 2.0)], [_grid(7, 30.0), _grid(7, 20.0)]
    else:
        pulses = _pulses(7, LENGTHS, FLIPS, False)
        xs, ys = [_grid(nx, 4.0 + q) for q, nx in enumerate(NXS)], None
    P = len(pulses)
    shapes = [(len(SCALES), len(xs[q])) + ((len(ys[q]),) if two_d else ()) for q in range(P)]
    fits = [_fit(100 + q, shapes[q], kind) for q in range(P)]
    ts, ws = [f[0] for f in fits], [f[1] for f in fits]
    kw = dict(profile=kind, scales=SCALES, hard_pulse=hard)
    at_rf = _call(two_d, "lsq", pulses, xs, ys, ts, ws, **kw)
    bs = [-g for _, g in at_rf]
    assert all(_dot(b, b) > 0 for b in bs)
    hb = _call(two_d, "gn", pulses, xs, ys, bs, ws, **kw)
    mus = [1e-3 * _dot(b, h) / _dot(b, b) for b, h in zip(bs, hb)]
    assert all(m > 0 for m in mus)
    return pulses, xs, ys, ts, ws, bs, mus, at_rf, kw


def _same(a, b):
    """every output of a pulse, bit for bit"""
    (da, ia), (db, ib) = a, b
    keys = set(ia) & set(ib)
    assert {"ncg", "rr", "gg", "status"} <= keys
    return np.array_equal(da, db) and all(np.array_equal(ia[k], ib[k]) for k in keys)


@pytest.mark.parametrize("two_d,hard,kind", COMBOS)
def test_trial_is_the_shipped_lsq_call_at_rf_plus_d(two_d, hard, kind):
    """rtol = 1e300: nothing runs, d = 0 and the loss and gradient are abr_lsq_batch's at rf; otherwise they are abr_lsq_batch's at
    rf + d with the returned d, bit for bit.  Solve-only returns the same d."""
    pulses, xs, ys, ts, ws, bs, mus, at_rf, kw = _case(two_d, hard, kind)
    idle = _call(two_d, "lm_step", pulses, xs, ys, bs, ws, mus, targets=ts, rtol=1e300, **kw)
    for (d, i), (L, g), b in zip(idle, at_rf, bs):
        assert np.array_equal(d, np.zeros_like(d)) and i["ncg"] == 0 and i["status"] == "rtol"
        assert i["loss"] == L and np.array_equal(i["grad"], g)
        assert i["rr"] == i["gg"] and abs(i["gg"] - _dot(b, b)) <= 1e-14 * _dot(b, b)
    for cg in (0, 3):
        got = _call(two_d, "lm_step", pulses, xs, ys, bs, ws, mus, targets=ts, cg=cg, rtol=0.0, **kw)
        want = _call(two_d, "lsq", [_moved(p, d) for p, (d, _) in zip(pulses, got)], xs, ys, ts, ws, **kw)
        solve = _call(two_d, "lm_step", pulses, xs, ys, bs, ws, mus, cg=cg, rtol=0.0, **kw)
        for (d, i), (L, g), (d0, i0), p in zip(got, want, solve, pulses):
            n = len(d)
            # rtol = 0 stops a pulse before the cap only at a residual of exact zeros (one sample at one point converges so)
            assert (i["ncg"] == cg and i["status"] == "cg") or (0 < i["ncg"] < cg and i["rr"] == 0.0 and i["status"] == "rtol"), (n, cg)
            assert cg == 0 or np.abs(d).max() > 0
            assert i["loss"] == L and np.array_equal(i["grad"], g), (n, cg)
            assert "loss" not in i0 and "grad" not in i0 and _same((d, i), (d0, i0)), (n, cg)


def test_outputs_have_the_same_bits_alone_in_17_reversed_repeated_and_beside_neighbours_that_stop_earlier_or_later():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 300, 17)]
    lengths[3], lengths[11] = 256, 257
    flips = list(np.linspace(0.1, 3.0, 17))
    sc = SCALES
    every, stops = list(range(17)), set()
    for two_d, hard, kind in ((False, False, "ex"), (False, True, "se"), (True, False, "inv"), (True, True, "st")):
        p = _pulses(53 + two_d, lengths, flips, two_d)
        x = [_grid(5 + 40 * q, 6.0) for q in every] if not two_d else [_grid(5 + 3 * q, 3.0) for q in every]
        y = [_grid(3 + 5 * (q % 7), 25.0) for q in every]
        shapes = [(len(sc), len(x[q])) + ((len(y[q]),) if two_d else ()) for q in every]
        fits = [_fit(300 + q, shapes[q], kind) for q in every]
        t, w = [f[0] for f in fits], [f[1] for f in fits]
        kw = dict(profile=kind, scales=sc, hard_pulse=hard)
        b = [-g for _, g in _call(two_d, "lsq", p, x, y, t, w, **kw)]
        mu = [1e-3 * _dot(v, h) / _dot(v, v) for v, h in zip(b, _call(two_d, "gn", p, x, y, b, w, **kw))]

        def lm(idx, bb=None, mm=None, targets=True, cg=6, rtol=1e-3):
            return _call(two_d, "lm_step", [p[q] for q in idx], [x[q] for q in idx], [y[q] for q in idx],
                         bb if bb is not None else [b[q] for q in idx], [w[q] for q in idx], mm if mm is not None else [mu[q] for q in idx],
                         targets=[t[q] for q in idx] if targets else None, cg=cg, rtol=rtol, **kw)

        full, again, rev, bare = lm(every), lm(every), lm(every[::-1])[::-1], lm(every, targets=False)
        stops |= set(i["ncg"] for _, i in full)
        print("%s hard %s %s: iterations per pulse %s" % ("2D" if two_d else "1D", hard, kind, [i["ncg"] for _, i in full]))
        for q in every:
            assert _same(full[q], again[q]) and _same(full[q], rev[q]) and _same(full[q], bare[q]), (two_d, hard, q)
            assert "loss" in full[q][1] and "loss" not in bare[q][1]
        longest = int(np.argmax(lengths))
        for q in (0, 3, 11, 16):
            alone, = lm([q])
            first, second = lm([q, q])
            assert _same(alone, full[q]) and _same(first, full[q]) and _same(second, full[q]), (two_d, hard, q)
            # neighbours that stop at once (b = 0), after one iteration (a huge mu), and later (the longest pulse, a tiny mu, no
            # tolerance): the pulse in the middle
            idx = [q, q, q, longest]
            n = lengths[q]
            bb = [np.zeros(n, dtype=complex), b[q], b[q], b[longest]]
            mm = [mu[q], 1e12 * mu[q], mu[q], 1e-9 * mu[longest]]
            for rtol, cg in ((1e-3, 6), (0.0, 9)):
                res = lm(idx, bb, mm, cg=cg, rtol=rtol)
                want, = lm([q], cg=cg, rtol=rtol)
                assert res[0][1]["ncg"] == 0 and res[0][1]["status"] == "rtol"
                assert _same(res[2], want), (two_d, hard, q, rtol)
            assert res[3][1]["ncg"] == 9
    assert len(stops) > 1                                            # the pulses of a batch do not all stop together


@pytest.mark.parametrize("two_d,hard,kind", [(False, False, "ex"), (False, True, "inv"), (True, True, "se"), (True, False, "st")])
def test_a_pulse_that_reaches_rtol_at_iteration_k_reports_k(two_d, hard, kind):
    """rr / gg after 1, 2, 3 iterations from three runs without a tolerance; an rtol just above the smallest of them stops the
    run with cg = 8 at the first iteration that reaches it, with that run's bits"""
    pulses, xs, ys, ts, ws, bs, mus, _, kw = _case(two_d, hard, kind)
    runs = [_call(two_d, "lm_step", pulses, xs, ys, bs, ws, mus, cg=k, rtol=0.0, **kw) for k in (1, 2, 3)]
    for q in range(len(pulses)):
        ratio = [runs[k][q][1]["rr"] / runs[k][q][1]["gg"] for k in range(3)]
        rtol = min(ratio) * (1 + 1e-9)
        k = 1 + min(j for j in range(3) if ratio[j] <= rtol)
        (d, i), = _call(two_d, "lm_step", pulses[q:q + 1], xs[q:q + 1], ys[q:q + 1] if two_d else None, bs[q:q + 1], ws[q:q + 1],
                        mus[q:q + 1], cg=8, rtol=rtol, **kw)
        print("n %d: rr / gg %s, rtol %.3g, stops after %d (%s)" % (len(d), ["%.3g" % v for v in ratio], rtol, i["ncg"], i["status"]))
        assert i["ncg"] == k and k < 8 and i["status"] == "rtol"
        assert np.array_equal(d, runs[k - 1][q][0]) and i["rr"] == runs[k - 1][q][1]["rr"] and i["gg"] == runs[k - 1][q][1]["gg"]


def _device_sum(v):
    """the step kernel's sum of one real per sample: thread t adds samples t, t + 256, ... in order, then the fixed tree over 256"""
    part = np.zeros(256)
    for t in range(min(256, len(v))):
        for m in range(t, len(v), 256):
            part[t] = part[t] + v[m]
    o = 128
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return float(part[0])


def _device_dot(u, v):
    return _device_sum(u.real * v.real + u.imag * v.imag)


@pytest.mark.parametrize("two_d,hard,kind", COMBOS)
def test_first_iteration_has_the_bits_of_the_shipped_product(two_d, hard, kind):
    """cg = 1: H p of a running pulse is abr_gn_batch's on p = b, bit for bit, so gg, rr and d follow exactly from one shipped
    product and the step kernel's arithmetic restated in NumPy (every product and sum rounded once, the sums in the kernel's
    order).  This pins the sweep's partial layout and the fold to the shipped ones, not to within a rounding spread."""
    pulses, xs, ys, ts, ws, bs, mus, _, kw = _case(two_d, hard, kind)
    got = _call(two_d, "lm_step", pulses, xs, ys, bs, ws, mus, cg=1, rtol=0.0, **kw)
    for (d, i), b, hb, mu in zip(got, bs, _call(two_d, "gn", pulses, xs, ys, bs, ws, **kw), mus):
        gg = _device_dot(b, b)
        ap = hb + mu * b
        alpha = gg / _device_dot(b, ap)
        r = b + (-alpha) * ap
        assert i["gg"] == gg and i["ncg"] == 1, len(b)
        assert np.array_equal(d, 0.0 + alpha * b), len(b)
        assert i["rr"] == _device_dot(r, r), len(b)


def _realform(v):
    return np.concatenate([v.real, v.imag])


@pytest.mark.parametrize("two_d,hard,kind", COMBOS)
def test_step_is_the_dense_solve_at_n_7(two_d, hard, kind):
    """H from 2n shipped gn products, mu = 1e-2 trace(H) / 2n, cg = 4n, rtol = 1e-16: within 1e-4 of max|d|"""
    pulses, xs, ys, ts, ws, bs, _, _, kw = _case(two_d, hard, kind)
    q = [len(_split(p)[0]) for p in pulses].index(7)
    n = 7
    one = lambda v: v[q:q + 1]
    basis = np.concatenate([np.eye(n), 1j * np.eye(n)])
    cols, = _call(two_d, "gn", one(pulses), one(xs), one(ys) if two_d else None, [basis], one(ws), **kw)
    H = np.stack([_realform(c) for c in cols], axis=1)
    if not np.trace(H) > 0:
        pytest.fail("H vanishes: the case has no weight on a point that the pulse excites")
    mu = 1e-2 * np.trace(H) / (2 * n)
    want = np.linalg.solve(H + mu * np.eye(2 * n), _realform(bs[q]))
    (d, i), = _call(two_d, "lm_step", one(pulses), one(xs), one(ys) if two_d else None, one(bs), one(ws), mu, cg=4 * n, rtol=1e-16, **kw)
    err = np.abs(_realform(d) - want).max() / np.abs(want).max()
    print("%s hard %s %s: step against the dense solve %.3g after %d iterations (%s), condition number %.0f"
          % ("2D" if two_d else "1D", hard, kind, err, i["ncg"], i["status"], np.linalg.cond(H + mu * np.eye(2 * n))))
    assert err <= 1e-4


CGS = (1, 2, 3, 8)


RECUR = ([(False, k % 2 == 1, kind, q) for k, kind in enumerate(KINDS) for q in range(len(LENGTHS))]
         + [(True, k % 2 == 0, kind, q) for k, kind in enumerate(KINDS) for q in range(len(LEN2))])


@pytest.mark.parametrize("two_d,hard,kind,q", RECUR)
def test_step_is_the_recurrence_on_the_shipped_operator(two_d, hard, kind, q):
    """cg in 1, 2, 3, 8 with rtol = 0 (the module's docstring has the bounds); one pulse per case, since the NumPy operator takes
    a third of a second per product at 257 samples"""
    pulses, xs, ys, ts, ws, bs, mus, _, kw = _case(two_d, hard, kind)
    p, x, y = pulses[q], xs[q], ys[q] if two_d else None
    rf, g = _split(p)
    got = {cg: _call(two_d, "lm_step", [p], [x], [y], [bs[q]], [ws[q]], mus[q], cg=cg, rtol=0.0, **kw)[0] for cg in CGS}

    @functools.lru_cache(maxsize=None)
    def shipped_of(key):
        return _call(two_d, "gn", [p], [x], [y], [np.frombuffer(key, dtype=complex)], [ws[q]], **kw)[0]

    @functools.lru_cache(maxsize=None)
    def numpy_of(key):
        return ref.gn(rf, g, x, np.frombuffer(key, dtype=complex), ws[q], SCALES, kind, y, hard)

    def shipped(v):                                                  # the runs with a smaller cg repeat the first products of cg = 8
        return shipped_of(v.tobytes())

    def numpy(v):
        return numpy_of(v.tobytes())

    on_dev = {cg: lmref.cg_solve(shipped, bs[q], mus[q], cg, 0.0) for cg in CGS}
    on_ref = {cg: lmref.cg_solve(numpy, bs[q], mus[q], cg, 0.0) for cg in CGS}
    scale = max(np.abs(on_dev[cg][0]).max() for cg in CGS)
    spread = max(np.abs(on_dev[cg][0] - on_ref[cg][0]).max() for cg in CGS)
    bound = max(100 * spread, 1e-13 * scale)
    n = len(rf)
    cols, = _call(two_d, "gn", [p], [x], [y], [np.concatenate([np.eye(n), 1j * np.eye(n)])], [ws[q]], **kw)
    trace = float(sum(cols[j][j].real + cols[n + j][j].imag for j in range(n)))
    dr = (trace + mus[q]) * np.sqrt(2 * n) * bound
    for cg in CGS:
        (d, i), (d0, i0) = got[cg], on_dev[cg]
        err = float(np.abs(d - d0).max())
        rr_spread = abs(on_ref[cg][1]["rr"] - i0["rr"])
        rr_bound = 2 * np.sqrt(i0["rr"]) * dr + dr * dr + 2e-13 * np.sqrt(i0["rr"] * i0["gg"]) + 1e-26 * i0["gg"]
        rr_err = abs(i["rr"] - i0["rr"])
        print("%s hard %s %s n %d points %s cg %d: |d - recurrence| %.3g, the two references apart %.3g, bound %.3g (max|d| %.3g); "
              "rr %.6g, |rr - recurrence| %.3g, references apart %.3g, bound %.3g; ncg %d (%d)"
              % ("2D" if two_d else "1D", hard, kind, len(d), ws[q].shape[1:], cg, err, spread, bound, scale, i0["rr"], rr_err,
                 rr_spread, rr_bound, i["ncg"], i0["ncg"]))
        assert i["ncg"] == i0["ncg"] and i["status"] == i0["status"], cg
        assert abs(i["gg"] - i0["gg"]) <= 1e-14 * i0["gg"], cg
        assert err <= bound, cg
        assert rr_err <= rr_bound, cg


@pytest.mark.parametrize("hard", [False, True])
def test_2d_at_y0_with_a_real_g_is_the_1d_call(hard):
    """the two form om differently (fma(x, gx, 0 gy) against x g): within the recurrence's bound of the 1D call, whose two
    references are run here"""
    kind = "ex"
    pulses, xs, _, ts, ws, bs, mus, _, kw = _case(False, hard, kind)
    p2 = [rf if g is None else (rf, g + 0j) for rf, g in map(_split, pulses)]
    one = mbfir.abr_lm_step_batch(pulses, xs, bs, ws, mus, cg=3, rtol=0.0, **kw)
    two = mbfir.abr2_lm_step_batch(p2, xs, [0.0], bs, [w[..., None] for w in ws], mus, cg=3, rtol=0.0, **kw)
    for q, ((d1, i1), (d2, i2)) in enumerate(zip(one, two)):
        rf, g = _split(pulses[q])
        a, _ = lmref.cg_solve(lambda v: mbfir.abr_gn_batch([pulses[q]], [xs[q]], [v], [ws[q]], **kw)[0], bs[q], mus[q], 3, 0.0)
        b, _ = lmref.cg_solve(lambda v: ref.gn(rf, g, xs[q], v, ws[q], SCALES, kind, None, hard), bs[q], mus[q], 3, 0.0)
        bound = max(100 * np.abs(a - b).max(), 1e-13 * np.abs(a).max())
        err = np.abs(d1 - d2).max()
        print("hard %s n %d points %d: |d(2D) - d(1D)| %.3g, bound %.3g" % (hard, len(d1), len(xs[q]), err, bound))
        assert err <= bound and i1["ncg"] == i2["ncg"] == 3


def test_a_huge_mu_gives_b_over_mu_and_zero_weights_without_mu_break_down():
    for two_d, hard, kind in ((False, False, "ex"), (False, True, "inv"), (True, True, "se"), (True, False, "st")):
        pulses, xs, ys, ts, ws, bs, mus, _, kw = _case(two_d, hard, kind)
        huge = [1e15 * m for m in mus]                              # mus hold 1e-3 times the Rayleigh quotient
        for (d, i), b, m in zip(_call(two_d, "lm_step", pulses, xs, ys, bs, ws, huge, **kw), bs, huge):
            assert np.abs(d - b / m).max() <= 1e-9 * np.abs(b / m).max() and i["ncg"] >= 1
        zero_w = [np.zeros_like(w) for w in ws]
        for d, i in _call(two_d, "lm_step", pulses, xs, ys, bs, zero_w, 0.0, targets=ts, **kw):
            assert i["status"] == "breakdown" and i["ncg"] == 0 and np.array_equal(d, np.zeros_like(d))
            assert i["loss"] == 0.0 and np.array_equal(i["grad"], np.zeros_like(d))
        for d, i in _call(two_d, "lm_step", pulses, xs, ys, [np.zeros_like(b) for b in bs], ws, mus, **kw):
            assert i["status"] == "rtol" and i["ncg"] == 0 and i["rr"] == 0.0 and i["gg"] == 0.0
            assert np.array_equal(d, np.zeros_like(d)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()


def test_refine_batch_on_the_device_solver(monkeypatch):
    """the 64-sample pulse at 90 degrees, 65 points, three gains of tests/test_simgn_gpu.py, two outer iterations"""
    n, x, sc = 64, np.linspace(-8, 8, 65), (0.9, 1.0, 1.1)
    win = np.hanning(n + 2)[1:-1] * np.sinc(np.linspace(-2, 2, n))
    probs = []
    for k, flip in enumerate((np.pi / 2, 0.45 * np.pi, 0.55 * np.pi)):
        rf = win * (flip / win.sum()) + 0j
        (a, b), = mbfir.abr_batch([rf], x, scales=(1.0,))
        phase = np.exp(1j * np.angle(2 * np.conj(a[0, 32]) * b[0, 32]))
        band, stop = np.abs(x) <= 0.6, np.abs(x) >= 2.5
        t = np.stack([np.where(band, phase * np.sin(s * flip), 0.0) for s in sc])
        probs.append((rf, t, (band | stop).astype(float)))
    kw = dict(scales=sc, iters=2)
    args = ([p[0] for p in probs], x, [p[1] for p in probs], [p[2] for p in probs])
    steps, trials = [], []
    honest_lm, honest_lsq = mbfir.abr_lm_step_batch, mbfir.abr_lsq_batch

    def lm(*a, **k):
        res = honest_lm(*a, **k)
        steps.append([d for d, _ in res])
        return res

    def lsq(pulses, *a, **k):
        trials.append([np.array(_split(p)[0]) for p in pulses])
        return honest_lsq(pulses, *a, **k)

    monkeypatch.setattr(mbfir, "abr_lm_step_batch", lm)
    rfs, infos = mbfir.refine_batch(*args, solver="device", **kw)
    first = steps[0]
    for q, (rf, t, w) in enumerate(probs):
        L = infos[q]["losses"]
        print("pulse %d: losses %s, refused %d, calls %s" % (q, ["%.6g" % v for v in L], infos[q]["refused"], infos[q]["calls"]))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), q
        c = infos[q]["calls"]
        assert c["lsq"] == 1 and c["gn"] == 1 and c["lm"] == len(L) - 1 + infos[q]["refused"]
        (r1,), (i1,) = mbfir.refine_batch([rf], x, [t], [w], solver="device", **kw)
        assert np.array_equal(r1, rfs[q]) and i1 == infos[q], q
        (Lend, _), = honest_lsq([rfs[q]], x, [t], [w], scales=sc)
        assert Lend == L[-1]
    monkeypatch.setattr(mbfir, "abr_lm_step_batch", honest_lm)
    monkeypatch.setattr(mbfir, "abr_lsq_batch", lsq)
    mbfir.refine_batch(*args, **kw)
    for q, (rf, _, _) in enumerate(probs):
        d_host = trials[1][q] - rf                                  # the host solver's second lsq call tries rf + d
        err = np.abs(first[q] - d_host).max() / np.abs(d_host).max()
        print("pulse %d: first step of the device solver against the host solver's %.3g" % (q, err))
        assert err <= 1e-4


def test_errors_through_the_raw_calls_in_their_order():
    """the MBFIR_E_ARG messages: the forward calls' and the gn checks first, then a null array of the step's own, mu, cg, rtol"""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    def pp(vs):
        return [(v.ctypes.data_as(mbfir._ip) if v.dtype == np.int32 else p(v)) if v is not None else None for v in vs]

    d, o = np.ones(64), [np.zeros(64) for _ in range(7)]
    k = [np.zeros(4, dtype=np.int32) for _ in range(2)]
    neg, nan, inf = np.ones(64), np.ones(64), np.ones(64)
    neg[0], nan[0], inf[0] = -1.0, np.nan, np.inf

    def outs(out):
        return pp([o[0], o[1], k[0], o[2], o[3], k[1]] + list(out))

    def lm1(roff=L(0, 3), xoff=L(0, 2), nscale=3, mode=0, npulse=1, nxgrid=1, profile=0, w=d, b=(d, d), mu=d, cg=2, rtol=1e-6,
            t=(d, d), out=(o[4], o[5], o[6]), first=None, **_):
        res = outs(out)
        if first is not None:
            res[first] = None
        return lib.mbfir_abr_lm_step_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, nxgrid, lp(xoff), p(d), nscale, p(d), mode,
                                           profile, *pp((w,) + tuple(b) + (mu,)), cg, rtol, *pp(t), *res)

    def lm2(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 1), nscale=3, mode=0, npulse=1, nxgrid=1, nygrid=1, profile=0, w=d, b=(d, d), mu=d,
            cg=2, rtol=1e-6, t=(d, d), out=(o[4], o[5], o[6]), first=None, **_):
        res = outs(out)
        if first is not None:
            res[first] = None
        return lib.mbfir_abr2_lm_step_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid, lp(yoff),
                                            p(d), nscale, p(d), mode, profile, *pp((w,) + tuple(b) + (mu,)), cg, rtol, *pp(t), *res)

    wneg = np.ones(64)
    wneg[5] = -1.0
    cases = ((dict(roff=L(0, 0)), "no samples"), (dict(xoff=L(0, 0)), "empty item"), (dict(nscale=0), "scale list is empty"),
             (dict(mode=2), "mode"), (dict(npulse=0), "no pulses"), (dict(nxgrid=2), "1 or npulse"), (dict(w=None), "null"),
             (dict(profile=4), "profile"), (dict(w=wneg), "weight"),
             (dict(b=(None, d)), "null"), (dict(b=(d, None)), "null"), (dict(mu=None), "null"), (dict(first=0), "null"),
             (dict(first=2), "null"), (dict(first=5), "null"), (dict(out=(None, o[5], o[6])), "null"),
             (dict(out=(o[4], o[5], None)), "null"), (dict(t=(None, d)), "null"),
             (dict(mu=neg), "mu is negative or not finite"), (dict(mu=nan), "mu is negative or not finite"),
             (dict(mu=inf), "mu is negative or not finite"), (dict(cg=-1), "cg must be at least 0"),
             (dict(rtol=-1e-300), "rtol is negative or not a number"), (dict(rtol=float("nan")), "rtol is negative or not a number"),
             # the order: each check hides the later ones
             (dict(profile=9, b=(None, d), mu=neg), "profile"), (dict(w=wneg, mu=None), "weight"), (dict(mu=None, cg=-1), "null"),
             (dict(mu=neg, cg=-1, rtol=-1.0), "mu is negative"), (dict(cg=-1, rtol=-1.0), "cg must be"), (dict(nscale=0, cg=-1), "scale list"))
    for call, who in ((lm1, "abr_lm_step_batch:"), (lm2, "abr2_lm_step_batch:")):
        assert call() == 0, ctx.last_error()
        for kw, why in cases:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call(t=(d, None)) == 0                               # a real target
        assert call(t=(None, None), out=(None, None, None)) == 0   # solve only
        assert call(cg=0) == 0 and call(rtol=float("inf")) == 0 and call(mu=np.zeros(4)) == 0
    # 2^22 + 8 pulses of 2^31 - 1 samples at one point and one scale pass the gn checks (2^53 partials); the step's own eight
    # sections per sample do not fit.  Only roff, the weights and mu are read before that is found.
    many = 2 ** 22 + 8
    roff, big = np.arange(many + 1, dtype=np.int64) * (2 ** 31 - 1), np.ones(many)
    for call, who in ((lm1, "abr_lm_step_batch:"), (lm2, "abr2_lm_step_batch:")):
        assert call(npulse=many, roff=roff, xoff=L(0, 1), nscale=1, w=big, mu=big) == mbfir.E_ARG
        assert ctx.last_error().startswith(who) and "overflows" in ctx.last_error(), ctx.last_error()
    rf, xx = np.full(8, 0.1 + 0.05j), np.array([0.0, 1.0])
    t, w = np.array([[0.1, 0.2j]]), np.ones((1, 2))
    (L0, g0), = mbfir.abr_lsq_batch([rf], xx, [t], [w])              # the context still works
    (dd, i), = mbfir.abr2_lm_step_batch([rf], xx, [0.0], [-g0], [w[..., None]], 0.1, targets=[t[..., None]], cg=2)
    assert i["ncg"] >= 1 and i["loss"] < L0
