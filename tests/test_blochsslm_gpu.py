"""The Levenberg-Marquardt step of the steady state solved on the device (mbfir.bloch_ss_lm_step_batch: k_lm_init,
k_bloch_ss_lm_prep, k_bloch_ss_lm_sweep, k_bloch_lm_step, k_bloch_lm_trial and the shipped k_bloch_ss_lsq_batch / k_bloch_gn_fold on
the trial rows) and mbfir.refine_bloch_ss_batch(solver="device") on it.

Exact, without a tolerance: the trial's loss and gradient are bloch_ss_lsq_batch's at b1 + d; the first iteration follows from one
shipped bloch_ss_gn_batch product and the step kernel's arithmetic restated in NumPy (this is what holds pass 0, hoisted out of the
rounds into k_bloch_ss_lm_prep, to the bits of the pass 0 inlined in k_bloch_ss_gn_batch); a pulse's outputs do not depend on the
batch, its order, or when its neighbours stop.  Against the dense solve: the project's 1e-4 max|d|.  Against the recurrence of
tests/simlm_ref.py (cg_solve) run on the shipped bloch_ss_gn_batch as the operator: ncg and status equal, and for d and rr the
bounds that tests/test_blochlm_gpu.py derives in its docstring, measured on code that is not under test:
    |d - d_ref| <= max(100 max over the case's cg of |d_ref(blochssgn_ref) - d_ref(device gn)|, 1e-13 max|d_ref|)
    |rr - rr_ref| <= 2 sqrt(rr_ref) dr + dr^2 + 2e-13 sqrt(rr_ref gg) + 1e-26 gg,   dr = (trace(H) + mu) sqrt(2n) (the bound on d)
gg is within 1e-14 relative.  DESIGN 8v has the figures measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochsslm_ref", os.path.join(ROOT, "tests", "blochsslm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
ref = lmref.gnref
ssref = ref.ssref
SCALES = lmref.SCALES
_dot = lmref.dot


def _moved(p, d):
    return (p[0] + d,) + tuple(p[1:])


@functools.lru_cache(maxsize=None)
def _case(shared):
    """blochsslm_ref.cases(shared) with, per pulse, b = -gradient at b1 and mu = 1e-3 times the Rayleigh quotient of H at b
    (refine_bloch_ss_batch's first mu), from the shipped device calls.  On its own 1 x 1 grid the 255-sample period, weighted on mz
    alone, has weight zero at both scales that are not 0: its gradient and its H are exact zeros.  It takes b = b1 and mu = 1, and
    the solve is then d = b exactly after one iteration (alpha = <b, b> / <b, b>, r = b - b), which every test below allows for."""
    pulses, dfs, dps, tgs, wts = lmref.cases(shared)
    D, P = (dfs[0], dps[0]) if shared else (dfs, dps)
    kw = dict(scales=SCALES)
    at_b1 = mbfir.bloch_ss_lsq_batch(pulses, D, P, tgs, wts, **kw)
    flat = [q for q, (_, g) in enumerate(at_b1) if _dot(g, g) == 0.0]
    assert flat == ([] if shared else [4]) and all(float(np.sum(wts[q][2][[0, 2]])) == 0.0 for q in flat)
    rhs = [(L, -np.asarray(pulses[q][0], dtype=complex)) if q in flat else (L, g) for q, (L, g) in enumerate(at_b1)]
    bs, mus = lmref.rhs_and_mu(lambda: rhs, lambda v: mbfir.bloch_ss_gn_batch(pulses, D, P, v, wts, **kw))
    for q in flat:
        assert mus[q] == 0.0
        mus[q] = 1.0
    assert all(_dot(b, b) > 0 for b in bs) and all(m > 0 for m in mus)
    return pulses, dfs, dps, D, P, tgs, wts, bs, mus, at_b1, kw


def _one(shared, q):
    """pulse q of the case as a batch of one: (args of the calls up to dp, keywords, targets, weights, b, mu)"""
    pulses, dfs, dps, D, P, tgs, wts, bs, mus, _, kw = _case(shared)
    return ([pulses[q]], dfs[q], dps[q]), kw, [tgs[q]], [wts[q]], [bs[q]], [mus[q]]


def _same(a, b):
    """every output of a pulse, bit for bit"""
    (da, ia), (db, ib) = a, b
    keys = set(ia) & set(ib)
    assert {"ncg", "rr", "gg", "status"} <= keys
    return np.array_equal(da, db) and all(np.array_equal(ia[k], ib[k]) for k in keys)


@pytest.mark.parametrize("shared", [False, True])
def test_trial_is_the_shipped_lsq_call_at_b1_plus_d(shared):
    """rtol = 1e300: nothing runs, d = 0 and the loss and gradient are bloch_ss_lsq_batch's at b1; otherwise they are
    bloch_ss_lsq_batch's at b1 + d with the returned d, bit for bit.  Solve-only returns the same d and state.  With the targets
    set to bloch_batch(mode=1)'s output at b1 + d the trial's loss and gradient are exact zeros."""
    pulses, dfs, dps, D, P, tgs, wts, bs, mus, at_b1, kw = _case(shared)
    idle = mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, targets=tgs, rtol=1e300, **kw)
    for (d, i), (L, g), b in zip(idle, at_b1, bs):
        assert np.array_equal(d, np.zeros_like(d)) and i["ncg"] == 0 and i["status"] == "rtol"
        assert i["loss"] == L and np.array_equal(i["grad"], g)
        assert i["rr"] == i["gg"] and abs(i["gg"] - _dot(b, b)) <= 1e-14 * _dot(b, b)
    for cg in (0, 3):
        got = mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, targets=tgs, cg=cg, rtol=0.0, **kw)
        moved = [_moved(p, d) for p, (d, _) in zip(pulses, got)]
        want = mbfir.bloch_ss_lsq_batch(moved, D, P, tgs, wts, **kw)
        solve = mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, cg=cg, rtol=0.0, **kw)
        there = mbfir.bloch_batch(moved, D, P, mode=1, **kw)
        at_rest = mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, targets=there, cg=cg, rtol=0.0, **kw)
        for (d, i), (L, g), (d0, i0), (dz, iz) in zip(got, want, solve, at_rest):
            n = len(d)
            # rtol = 0 stops a pulse before the cap only at a residual of exact zeros
            assert (i["ncg"] == cg and i["status"] == "cg") or (0 < i["ncg"] < cg and i["rr"] == 0.0 and i["status"] == "rtol"), (n, cg)
            assert cg == 0 or np.abs(d).max() > 0
            assert i["loss"] == L and np.array_equal(i["grad"], g), (n, cg)
            assert "loss" not in i0 and "grad" not in i0 and _same((d, i), (d0, i0)), (n, cg)
            assert np.array_equal(dz, d) and iz["loss"] == 0.0 and np.array_equal(iz["grad"], np.zeros(n)), (n, cg)


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


@pytest.mark.parametrize("shared", [False, True])
def test_first_iteration_has_the_bits_of_the_shipped_product(shared):
    """cg = 1, rtol = 0: H p of a running pulse is bloch_ss_gn_batch's on p = b, bit for bit, so gg, rr and d follow exactly from
    one shipped product and the step kernel's arithmetic restated in NumPy (every product and sum rounded once, the sums in the
    kernel's order).  The shipped product runs pass 0 inline; the step reads M and (I - A)^-1 back from k_bloch_ss_lm_prep's
    plane: this is the test that decides whether pass 0 may be hoisted out of the rounds."""
    pulses, dfs, dps, D, P, tgs, wts, bs, mus, _, kw = _case(shared)
    got = mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, cg=1, rtol=0.0, **kw)
    for (d, i), b, hb, mu in zip(got, bs, mbfir.bloch_ss_gn_batch(pulses, D, P, bs, wts, **kw), mus):
        gg = _device_dot(b, b)
        ap = hb + mu * b
        alpha = gg / _device_dot(b, ap)
        r = b + (-alpha) * ap
        assert i["gg"] == gg and i["ncg"] == 1, len(b)
        assert np.array_equal(d, 0.0 + alpha * b), len(b)
        assert i["rr"] == _device_dot(r, r), len(b)


def test_outputs_have_the_same_bits_alone_in_17_reversed_repeated_and_beside_neighbours_that_stop_earlier_or_later():
    pulses, dfs, dps, tgs, wts = lmref.batch17()
    lengths = [len(p[0]) for p in pulses]
    assert 256 in lengths and 257 in lengths and min(lengths) >= 1 and max(lengths) <= 300
    sc, every = lmref.SC17, list(range(17))

    def args(idx):
        return [pulses[q] for q in idx], [dfs[q] for q in idx], [dps[q] for q in idx]

    b, mu = lmref.rhs_and_mu(lambda: mbfir.bloch_ss_lsq_batch(*args(every), tgs, wts, scales=sc),
                             lambda v: mbfir.bloch_ss_gn_batch(*args(every), v, wts, scales=sc))

    def lm(idx, bb=None, mm=None, targets=True, cg=lmref.CG17, rtol=lmref.RTOL17):
        return mbfir.bloch_ss_lm_step_batch(*args(idx), bb if bb is not None else [b[q] for q in idx], [wts[q] for q in idx],
                                            mm if mm is not None else [mu[q] for q in idx],
                                            targets=[tgs[q] for q in idx] if targets else None, cg=cg, rtol=rtol, scales=sc)

    full, again, rev, bare = lm(every), lm(every), lm(every[::-1])[::-1], lm(every, targets=False)
    stops = set(i["ncg"] for _, i in full)
    print("iterations per pulse %s" % [i["ncg"] for _, i in full])
    for q in every:
        assert _same(full[q], again[q]) and _same(full[q], rev[q]) and _same(full[q], bare[q]), q
        assert "loss" in full[q][1] and "loss" not in bare[q][1]
    longest = int(np.argmax(lengths))
    for q in (0, 3, 11, 16):
        alone, = lm([q])
        first, second = lm([q, q])
        assert _same(alone, full[q]) and _same(first, full[q]) and _same(second, full[q]), q
        # neighbours that stop at once (b = 0), after one iteration (a huge mu), and later (the longest pulse, a tiny mu, no
        # tolerance): the pulse in the middle
        idx = [q, q, q, longest]
        n = lengths[q]
        bb = [np.zeros(n, dtype=complex), b[q], b[q], b[longest]]
        mm = [mu[q], 1e12 * mu[q], mu[q], 1e-9 * mu[longest]]
        for rtol, cg in ((lmref.RTOL17, lmref.CG17), (0.0, 9)):
            res = lm(idx, bb, mm, cg=cg, rtol=rtol)
            want, = lm([q], cg=cg, rtol=rtol)
            assert res[0][1]["ncg"] == 0 and res[0][1]["status"] == "rtol"
            assert _same(res[2], want), (q, rtol)
        assert res[1][1]["ncg"] >= 1 and res[3][1]["ncg"] == 9
    assert len(stops) > 1                                            # the pulses of a batch do not all stop together


@pytest.mark.parametrize("shared", [False, True])
def test_a_pulse_of_the_cases_alone_has_its_bits_in_the_batch(shared):
    """the cases at the three scales 1, 0, 0.9: every pulse alone against the batch of seven"""
    pulses, dfs, dps, D, P, tgs, wts, bs, mus, _, kw = _case(shared)
    full = mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, targets=tgs, cg=3, rtol=1e-3, **kw)
    for q in range(len(pulses)):
        a, k1, t, w, b, m = _one(shared, q)
        alone, = mbfir.bloch_ss_lm_step_batch(*a, b, w, m, targets=t, cg=3, rtol=1e-3, **k1)
        assert _same(alone, full[q]), q


@pytest.mark.parametrize("shared", [False, True])
def test_a_pulse_that_reaches_rtol_at_iteration_k_reports_k(shared):
    """rr / gg after 1, 2, 3 iterations from three runs without a tolerance; an rtol just above the smallest of them stops the
    run with cg = 8 at the first iteration that reaches it, with that run's bits"""
    pulses, dfs, dps, D, P, tgs, wts, bs, mus, _, kw = _case(shared)
    runs = [mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, mus, cg=k, rtol=0.0, **kw) for k in (1, 2, 3)]
    for q in range(len(pulses)):
        ratio = [runs[k][q][1]["rr"] / runs[k][q][1]["gg"] for k in range(3)]
        rtol = min(ratio) * (1 + 1e-9)
        k = 1 + min(j for j in range(3) if ratio[j] <= rtol)
        a, k1, _, w, b, m = _one(shared, q)
        (d, i), = mbfir.bloch_ss_lm_step_batch(*a, b, w, m, cg=8, rtol=rtol, **k1)
        print("n %d: rr / gg %s, rtol %.3g, stops after %d (%s)" % (len(d), ["%.3g" % v for v in ratio], rtol, i["ncg"], i["status"]))
        assert i["ncg"] == k and k < 8 and i["status"] == "rtol"
        assert np.array_equal(d, runs[k - 1][q][0]) and i["rr"] == runs[k - 1][q][1]["rr"] and i["gg"] == runs[k - 1][q][1]["gg"]


def _realform(v):
    return np.concatenate([v.real, v.imag])


def _dense_h(a, w, k1, n):
    """H of one pulse from 2n shipped gn products, real form"""
    cols, = mbfir.bloch_ss_gn_batch(*a, [np.concatenate([np.eye(n), 1j * np.eye(n)])], w, **k1)
    return np.stack([_realform(c) for c in cols], axis=1)


@pytest.mark.parametrize("shared", [False, True])
def test_step_is_the_dense_solve_at_n_7(shared):
    """H from 2n shipped gn products, mu = 1e-2 trace(H) / 2n, cg = 4n, rtol = 1e-16: within 1e-4 of max|d|"""
    n, q = 7, 1
    a, k1, _, w, b, _ = _one(shared, q)
    assert len(a[0][0][0]) == n
    H = _dense_h(a, w, k1, n)
    assert np.trace(H) > 0
    mu = 1e-2 * np.trace(H) / (2 * n)
    want = np.linalg.solve(H + mu * np.eye(2 * n), _realform(b[0]))
    (d, i), = mbfir.bloch_ss_lm_step_batch(*a, b, w, mu, cg=4 * n, rtol=1e-16, **k1)
    err = np.abs(_realform(d) - want).max() / np.abs(want).max()
    print("shared %s: step against the dense solve %.3g after %d iterations (%s), condition number %.0f"
          % (shared, err, i["ncg"], i["status"], np.linalg.cond(H + mu * np.eye(2 * n))))
    assert err <= 1e-4


CGS = (1, 2, 3, 8)


@pytest.mark.parametrize("shared,q", [(s, q) for s in (False, True) for q in range(lmref.NCASE)])
def test_step_is_the_recurrence_on_the_shipped_operator(shared, q):
    """cg in 1, 2, 3, 8 with rtol = 0 (the module's docstring has the bounds); one pulse per case"""
    pulses, dfs, dps, _, _, _, wts, _, _, _, _ = _case(shared)
    a, k1, _, w, (b,), (mu,) = _one(shared, q)
    p = pulses[q]
    got = {cg: mbfir.bloch_ss_lm_step_batch(*a, [b], w, mu, cg=cg, rtol=0.0, **k1)[0] for cg in CGS}

    @functools.lru_cache(maxsize=None)
    def shipped_of(key):
        return mbfir.bloch_ss_gn_batch(*a, [np.frombuffer(key, dtype=complex)], w, **k1)[0]

    @functools.lru_cache(maxsize=None)
    def numpy_of(key):
        return ref.gn(p, dfs[q], dps[q], np.frombuffer(key, dtype=complex), wts[q], SCALES)

    def shipped(v):                                                  # the runs with a smaller cg repeat the first products of cg = 8
        return shipped_of(v.tobytes())

    def numpy(v):
        return numpy_of(v.tobytes())

    on_dev = {cg: lmref.cg_solve(shipped, b, mu, cg, 0.0) for cg in CGS}
    on_ref = {cg: lmref.cg_solve(numpy, b, mu, cg, 0.0) for cg in CGS}
    scale = max(np.abs(on_dev[cg][0]).max() for cg in CGS)
    spread = max(np.abs(on_dev[cg][0] - on_ref[cg][0]).max() for cg in CGS)
    bound = max(100 * spread, 1e-13 * scale)
    n = len(b)
    H = _dense_h(a, w, k1, n)
    trace = float(np.trace(H))
    dr = (trace + mu) * np.sqrt(2 * n) * bound
    for cg in CGS:
        (d, i), (d0, i0) = got[cg], on_dev[cg]
        err = float(np.abs(d - d0).max())
        rr_spread = abs(on_ref[cg][1]["rr"] - i0["rr"])
        rr_bound = 2 * np.sqrt(i0["rr"]) * dr + dr * dr + 2e-13 * np.sqrt(i0["rr"] * i0["gg"]) + 1e-26 * i0["gg"]
        rr_err = abs(i["rr"] - i0["rr"])
        print("shared %s n %d points %dx%d cg %d: |d - recurrence| %.3g, the two references apart %.3g, bound %.3g, share %.3g "
              "(max|d| %.3g); rr %.6g, |rr - recurrence| %.3g, references apart %.3g, bound %.3g, share %.3g; ncg %d (%d)"
              % (shared, n, len(dfs[q]), np.shape(dps[q])[0], cg, err, spread, bound, err / bound if bound else 0.0, scale, i0["rr"],
                 rr_err, rr_spread, rr_bound, rr_err / rr_bound if rr_bound else 0.0, i["ncg"], i0["ncg"]))
        assert i["ncg"] == i0["ncg"] and i["status"] == i0["status"], cg
        assert abs(i["gg"] - i0["gg"]) <= 1e-14 * i0["gg"], cg
        assert err <= bound, cg
        assert rr_err <= rr_bound, cg


@pytest.mark.parametrize("shared", [False, True])
def test_a_huge_mu_gives_b_over_mu_and_a_vanishing_operator_without_mu_breaks_down(shared):
    pulses, dfs, dps, D, P, tgs, wts, bs, mus, _, kw = _case(shared)
    huge = [1e15 * m for m in mus]                                  # mus hold 1e-3 times the Rayleigh quotient
    for (d, i), b, m in zip(mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, wts, huge, **kw), bs, huge):
        assert np.abs(d - b / m).max() <= 1e-9 * np.abs(b / m).max() and i["ncg"] >= 1
    zero = [(0.0, 0.0, 0.0)] * len(pulses)
    for d, i in mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, zero, 0.0, targets=tgs, **kw):
        assert i["status"] == "breakdown" and i["ncg"] == 0 and np.array_equal(d, np.zeros_like(d))
        assert i["loss"] == 0.0 and np.array_equal(i["grad"], np.zeros_like(d))

    # the scale list (0,) alone: the fold's factor makes H an exact zero, and the loss (that of M = [0 0 1]) does not depend on b1
    def first_scale(tri):
        return tuple(x[:1] if np.ndim(x) else x for x in tri)

    w0, t0 = [first_scale(tri) for tri in wts], [first_scale(tri) for tri in tgs]
    want = mbfir.bloch_ss_lsq_batch(pulses, D, P, t0, w0, scales=(0.0,))
    for (d, i), (L, g) in zip(mbfir.bloch_ss_lm_step_batch(pulses, D, P, bs, w0, 0.0, targets=t0, scales=(0.0,)), want):
        assert i["status"] == "breakdown" and i["ncg"] == 0 and np.array_equal(d, np.zeros_like(d))
        assert i["loss"] == L and np.isfinite(L) and np.array_equal(i["grad"], np.zeros_like(d)) and np.array_equal(g, np.zeros_like(d))
    for d, i in mbfir.bloch_ss_lm_step_batch(pulses, D, P, [np.zeros_like(b) for b in bs], wts, mus, **kw):
        assert i["status"] == "rtol" and i["ncg"] == 0 and i["rr"] == 0.0 and i["gg"] == 0.0
        assert np.array_equal(d, np.zeros_like(d)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()


def test_refine_bloch_ss_batch_on_the_device_solver(monkeypatch):
    """tests/test_blochssgn_gpu.py's refine case: a 64-sample pulse and a dead time (a period of 2 ms, T1 = 0.2 s, T2 = 0.05 s),
    3 x 33 points, three gains, two outer iterations; the target is the steady state of the pulse's smooth part at 1.15 times its
    amplitude.  The first step is the host solver's within 1e-12 of max|d|: the same operator bits, the dots summed in another
    order."""
    sc, n, dt = (0.9, 1.0, 1.1), 64, 1e-5
    df, dp = ref._grid(3, 100.0), ref._grid(33, 3.0)
    tp, gr = np.append(np.full(n, dt), 2e-3 - n * dt), np.append(np.full(n, 0.05), 0.0)
    probs = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        smooth = np.hanning(n + 2)[1:-1] * (np.pi / 4 / (ssref.GAMMA_H1 * dt * np.hanning(n + 2).sum()))
        b1 = np.append(smooth * (1 + 0.1 * rng.standard_normal(n)), 0.0) + 0j
        t, = mbfir.bloch_batch([(np.append(1.15 * smooth, 0.0) + 0j, gr, tp, 0.2, 0.05, "H-1")], df, dp, mode=1)
        probs.append(((b1, gr, tp, 0.2, 0.05, "H-1"), tuple(c[0] for c in t), (1.0, 1.0, 1.0)))
    kw = dict(scales=sc, iters=2, cg=4)
    args = ([p for p, _, _ in probs], df, dp, [t for _, t, _ in probs], [w for _, _, w in probs])
    steps, trials = [], []
    honest_lm, honest_lsq = mbfir.bloch_ss_lm_step_batch, mbfir.bloch_ss_lsq_batch

    def lm(*a, **k):
        res = honest_lm(*a, **k)
        steps.append([d for d, _ in res])
        return res

    def lsq(pulses, *a, **k):
        trials.append([np.array(p[0]) for p in pulses])
        return honest_lsq(pulses, *a, **k)

    monkeypatch.setattr(mbfir, "bloch_ss_lm_step_batch", lm)
    b1s, infos = mbfir.refine_bloch_ss_batch(*args, solver="device", **kw)
    first = steps[0]
    for q, (p, t, w) in enumerate(probs):
        L = infos[q]["losses"]
        print("pulse %d: losses %s, refused %d, calls %s" % (q, ["%.6g" % v for v in L], infos[q]["refused"], infos[q]["calls"]))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), q
        c = infos[q]["calls"]
        assert c["lsq"] == 1 and c["gn"] == 1 and c["lm"] == len(L) - 1 + infos[q]["refused"]
        (r1,), (i1,) = mbfir.refine_bloch_ss_batch([p], df, dp, [t], [w], solver="device", **kw)
        assert np.array_equal(r1, b1s[q]) and i1 == infos[q], q
        (Lend, _), = honest_lsq([(b1s[q],) + p[1:]], df, dp, [t], [w], scales=sc)
        assert Lend == L[-1]
    monkeypatch.setattr(mbfir, "bloch_ss_lm_step_batch", honest_lm)
    monkeypatch.setattr(mbfir, "bloch_ss_lsq_batch", lsq)
    mbfir.refine_bloch_ss_batch(*args, **kw)
    for q, (p, _, _) in enumerate(probs):
        d_host = trials[1][q] - p[0]                                # the host solver's second lsq call tries b1 + d
        err = np.abs(first[q] - d_host).max() / np.abs(d_host).max()
        print("pulse %d: first step of the device solver against the host solver's %.3g" % (q, err))
        assert err <= 1e-12


def test_errors_through_the_raw_call_in_their_order():
    """the MBFIR_E_ARG messages: the forward call's at mode 1 and the gn checks first, then a null array of the step's own, targets
    only partly given, mu, cg, rtol, the overflow; a good call before and after"""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    who = "bloch_ss_lm_step_batch:"

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    def pp(vs):
        return [(v.ctypes.data_as(mbfir._ip) if v.dtype == np.int32 else p(v)) if v is not None else None for v in vs]

    d, one, neg, nan, inf = np.full(64, 1e-5), np.ones(64), np.ones(64), np.ones(64), np.ones(64)
    neg[0], nan[0], inf[0] = -1.0, np.nan, np.inf
    wneg = np.ones(64)
    wneg[5] = -1.0
    o = [np.zeros(64) for _ in range(7)]
    k = [np.zeros(4, dtype=np.int32) for _ in range(2)]

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, t2=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
             w=(one, one, one), b=(d, d), mu=one, cg=2, rtol=1e-6, t=(d, d, d), out=(o[4], o[5], o[6]), first=None):
        res = pp([o[0], o[1], k[0], o[2], o[3], k[1]] + list(out))
        if first is not None:
            res[first] = None
        return lib.mbfir_bloch_ss_lm_step_batch(ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None,
                                                lp(tsoff), p(d), p(t1), p(t2), p(t2), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d),
                                                None, None, nscale, p(one), *pp(w), *pp(b), *pp((mu,)), cg, rtol, *pp(t), *res)

    big = 2 ** 31 - 1
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
             (dict(tsoff=L(0, 2)), "neither 1 nor"), (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"),
             (dict(nfgrid=2), "1 or npulse"), (dict(b1=None), "required array is null"),
             (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"),
             (dict(w=(one, None, one)), "plane is null"), (dict(w=(one, wneg, one)), "a weight is negative or not finite"),
             (dict(b=(None, d)), "required array is null"), (dict(b=(d, None)), "required array is null"),
             (dict(mu=None), "required array is null"), (dict(first=0), "required array is null"),
             (dict(first=2), "required array is null"), (dict(first=5), "required array is null"),
             (dict(out=(None, o[5], o[6])), "required array is null"), (dict(out=(o[4], o[5], None)), "required array is null"),
             (dict(t=(None, d, d)), "tx, ty and tz"), (dict(t=(d, d, None)), "tx, ty and tz"),
             (dict(t=(None, d, None), out=(None, None, None)), "required array is null"),
             (dict(mu=neg), "mu is negative or not finite"), (dict(mu=nan), "mu is negative or not finite"),
             (dict(mu=inf), "mu is negative or not finite"), (dict(cg=-1), "cg must be at least 0"),
             (dict(rtol=-1e-300), "rtol is negative or not a number"), (dict(rtol=float("nan")), "rtol is negative or not a number"),
             # the order: each check hides the later ones
             (dict(nscale=0, cg=-1), "scale list"), (dict(w=(one, None, one), b=(None, d)), "plane is null"),
             (dict(w=(wneg, one, one), mu=None), "a weight is negative"),
             (dict(mu=None, t=(None, d, d)), "required array is null"), (dict(t=(d, None, d), mu=neg), "tx, ty and tz"),
             (dict(mu=neg, cg=-1, rtol=-1.0), "mu is negative"), (dict(cg=-1, rtol=-1.0), "cg must be"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
    assert call(t=(None, None, None), out=(None, None, None)) == 0      # solve only
    assert call(cg=0) == 0 and call(rtol=float("inf")) == 0 and call(mu=np.zeros(4)) == 0
    # 257 pulses of 2^31 - 1 samples at one point and one scale: every array that is read before the sizes are found wanting (the
    # offsets, t1, t2, the 257 weights per plane) is there; the per-sample sections' workgroups (more than 2^31 - 1 chunks of 256
    # samples, for the fold of H p as for the trial rows) do not fit
    many = 257
    toff, ones = np.arange(many + 1, dtype=np.int64) * big, np.ones(many + 1)
    tsoff = np.arange(many + 1, dtype=np.int64)
    assert call(npulse=many, toff=toff, tsoff=tsoff, t1=ones, t2=ones, foff=L(0, 1), poff=L(0, 1), w=(ones, ones, ones), mu=ones) == mbfir.E_ARG
    assert ctx.last_error().startswith(who) and "overflows" in ctx.last_error(), ctx.last_error()
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)                 # the context still works
    pulse = (np.full(8, 1e-2 + 5e-3j), None, 1e-4, 1.0, 1.0, "H-1")
    t, w = (0.0, 0.0, 0.5), (0.0, 0.0, 1.0)
    (L0, g0), = mbfir.bloch_ss_lsq_batch([pulse], df, dp, [t], [w])
    (dd, i), = mbfir.bloch_ss_lm_step_batch([pulse], df, dp, [-g0], [w], 0.1 * _dot(g0, g0) ** 0.5, targets=[t], cg=2)
    assert i["ncg"] >= 1 and np.isfinite(i["loss"])
