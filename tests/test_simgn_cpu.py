"""The NumPy reference of the least-squares products (tests/simgn_ref.py, no GPU): its gradient against central differences of
its loss, its Gauss-Newton operator assembled densely; the argument errors that mbfir.abr_lsq_batch / abr_gn_batch and their 2D
twins raise before any device work; and the logic of mbfir.refine_batch with the four device wrappers replaced by the reference."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("simgn_ref", os.path.join(ROOT, "tests", "simgn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

SCALES = (1.0, 0.0, 0.9)
CASES = [(n, hard, two_d, kind) for n in (1, 7, 300) for hard in (False, True) for two_d in (False, True) for kind in ref.KINDS]
SMALL = [c for c in CASES if c[0] == 7]


@functools.lru_cache(maxsize=None)
def _case(n, hard, two_d, kind):
    """A pulse of flip 2 rad with, for n > 1, one rf sample exactly zero; x = 0 (and y = 0) on the grid, so phi = 0 occurs; a 5 x 7
    grid in 2D; a third of the weights zero.  Returns rf, g, x, y, target, weights."""
    rng = np.random.default_rng(20 + n)
    rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (2.0 / n)
    g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n + 1j * rng.uniform(-1.5, 1.5, n) * 1e-2
    if n > 1:
        rf[n // 2] = 0.0
    x = np.linspace(-2, 2, 5) if two_d else np.linspace(-3, 3, 7)
    y = np.linspace(-30, 30, 7) if two_d else None
    assert 0.0 in x and (y is None or 0.0 in y)
    shape = (len(SCALES),) + ((5, 7) if two_d else (7,))
    t = 0.5 * (rng.standard_normal(shape) + (0 if kind == "inv" else 1j) * rng.standard_normal(shape))
    w = rng.uniform(0.5, 2.0, shape) * (rng.uniform(size=shape) > 1 / 3)
    assert (w == 0).any() and (w > 0).any()
    return rf, (g if two_d else g.real), x, y, t, w


@pytest.mark.parametrize("n,hard,two_d,kind", CASES)
def test_gradient_is_the_central_difference_of_the_loss(n, hard, two_d, kind):
    """h = 1e-6 along Re and Im of single samples (all of them up to n = 7; at n = 300 the first, the last, the zero sample and
    three more): within 1e-7 max|g|, the bound of tests/test_simgrad_cpu.py."""
    rf, g, x, y, t, w = _case(n, hard, two_d, kind)
    L, grad = ref.lsq(rf, g, x, t, w, SCALES, kind, y, hard)
    assert L > 0 and grad.shape == (n,)
    h, worst = 1e-6, 0.0
    for m in (range(n) if n <= 7 else (0, n // 2, n - 1, 17, 101, 256)):
        for d in (1.0, 1j):
            e = np.zeros(n, dtype=complex)
            e[m] = d
            fd = (ref.loss(rf + h * e, g, x, t, w, SCALES, kind, y, hard) - ref.loss(rf - h * e, g, x, t, w, SCALES, kind, y, hard)) / (2 * h)
            worst = max(worst, abs(fd - (grad[m].real if d == 1.0 else grad[m].imag)))
    bound = 1e-7 * float(np.abs(grad).max())
    print("n %d hard %s 2D %s %s: gradient against central differences %.3g, bound %.3g" % (n, hard, two_d, kind, worst, bound))
    assert worst <= bound


def _realform(v):
    return np.concatenate([v.real, v.imag])


def _dense_h(rf, g, x, y, w, kind, hard):
    n = len(rf)
    cols = []
    for j in range(2 * n):
        e = np.zeros(n, dtype=complex)
        e[j % n] = 1.0 if j < n else 1j
        cols.append(_realform(ref.gn(rf, g, x, e, w, SCALES, kind, y, hard)))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("n,hard,two_d,kind", SMALL)
def test_dense_gauss_newton_operator_is_symmetric_positive_semidefinite(n, hard, two_d, kind):
    rf, g, x, y, _, w = _case(n, hard, two_d, kind)
    H = _dense_h(rf, g, x, y, w, kind, hard)
    norm = np.linalg.norm(H, 2)
    asym = np.abs(H - H.T).max() / np.abs(H).max()
    lo = np.linalg.eigvalsh(0.5 * (H + H.T)).min()
    rng = np.random.default_rng(5)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    quad = float((np.conj(v) * ref.gn(rf, g, x, v, w, SCALES, kind, y, hard)).real.sum())
    direct = float((w * np.abs(ref.jac(rf, g, x, v, SCALES, kind, y, hard)) ** 2).sum())
    rel = abs(quad - direct) / direct
    print("hard %s 2D %s %s: asymmetry %.3g, smallest eigenvalue / norm %.3g, <v, H v> against sum w |F J v|^2 %.3g"
          % (hard, two_d, kind, asym, lo / norm, rel))
    assert asym <= 1e-13
    assert lo >= -1e-13 * norm
    assert rel <= 1e-13


def test_seed_is_the_adjoint_of_dprofile():
    rng = np.random.default_rng(3)
    a, b, da, db, c = (rng.standard_normal(6) + 1j * rng.standard_normal(6) for _ in range(5))
    for kind in ref.KINDS:
        la, lb = ref.seed(kind, a, b, c)
        lhs = (np.conj(c) * ref.dprofile(kind, a, b, da, db)).real.sum()
        rhs = (np.conj(la) * da + np.conj(lb) * db).real.sum()
        assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), abs(rhs))
        h = 1e-6
        fd = (ref.profile(kind, a + h * da, b + h * db) - ref.profile(kind, a - h * da, b - h * db)) / (2 * h)
        assert np.abs(fd - ref.dprofile(kind, a, b, da, db)).max() <= 1e-8
    assert np.array_equal(ref.profile("sat", a, b), ref.profile("inv", a, b))
    assert mbfir.PROFILES == {"ex": 0, "se": 1, "inv": 2, "sat": 2, "st": 3}
    assert np.abs(ref.profile("ex", a, b) - mbfir.ab2ex(a, b)).max() <= 1e-15
    assert np.abs(ref.profile("se", a, b) - mbfir.ab2se(a, b)).max() <= 1e-15
    assert np.abs(ref.profile("st", a, b) - mbfir.ab2st(a, b)).max() <= 1e-15
    assert np.abs(ref.profile("inv", a, b) - mbfir.ab2inv(a, b)).max() <= 1e-15


def test_gn_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym, nargs in (("mbfir_abr_lsq_batch", 19), ("mbfir_abr2_lsq_batch", 23), ("mbfir_abr_gn_batch", 19),
                       ("mbfir_abr2_gn_batch", 23)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert len(mbfir.SYMBOLS[sym][1]) == nargs
        assert getattr(mbfir.load_library(), sym) is not None           # the library exports it
    for name in ("abr_lsq_batch", "abr2_lsq_batch", "abr_gn_batch", "abr2_gn_batch", "refine_batch"):
        assert callable(getattr(mbfir, name))


def test_argument_errors_come_before_any_device_work():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    rf, v = np.ones(4), np.ones(4, dtype=complex)
    t1, w1 = np.zeros((2, 5), dtype=complex), np.ones((2, 5))
    t2, w2 = np.zeros((2, 5, 3), dtype=complex), np.ones((2, 5, 3))
    sc = (1.0, 0.9)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr_lsq_batch([], x, [], [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr_gn_batch([rf], x, [v], [w1], scales=())
    with pytest.raises(ValueError, match="profile must be one of"):
        mbfir.abr_lsq_batch([rf], x, [t1], [w1], scales=sc, profile="xy")
    with pytest.raises(ValueError, match="profile must be one of"):
        mbfir.abr2_gn_batch([rf], x, y, [v], [w2], scales=sc, profile=0)
    with pytest.raises(ValueError, match=r"target of pulse 0 has shape \(5,\)"):
        mbfir.abr_lsq_batch([rf], x, [t1[0]], [w1], scales=sc)
    with pytest.raises(ValueError, match=r"weights of pulse 0 have shape \(2, 4\)"):
        mbfir.abr_lsq_batch([rf], x, [t1], [w1[:, :4]], scales=sc)
    with pytest.raises(ValueError, match=r"weights of pulse 0 have shape \(3,\)"):
        mbfir.abr2_gn_batch([rf], x, y, [v], [np.ones(3)], scales=sc)
    with pytest.raises(ValueError, match="2 weight arrays for 1 pulses"):
        mbfir.abr_gn_batch([rf], x, [v], [w1, w1], scales=sc)
    with pytest.raises(ValueError, match="2 targets for 1 pulses"):
        mbfir.abr2_lsq_batch([rf], x, y, [t2, t2], [w2], scales=sc)
    for bad in (-1e-300, np.nan, np.inf):
        w = w1.copy()
        w[1, 2] = bad
        with pytest.raises(ValueError, match="negative or not finite"):
            mbfir.abr_lsq_batch([rf], x, [t1], [w], scales=sc)
        with pytest.raises(ValueError, match="negative or not finite"):
            mbfir.abr_gn_batch([rf], x, [v], [w], scales=sc)
    with pytest.raises(ValueError, match="'inv' is real"):
        mbfir.abr_lsq_batch([rf], x, [t1 + 1j], [w1], scales=sc, profile="inv")
    with pytest.raises(ValueError, match="'inv' is real"):
        mbfir.abr2_lsq_batch([rf], x, y, [t2 + 1j], [w2], scales=sc, profile="sat")
    with pytest.raises(ValueError, match="the same K"):                             # ragged K
        mbfir.abr_gn_batch([rf, rf], x, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)], [w1, w1], scales=sc)
    with pytest.raises(ValueError, match="the same K"):
        mbfir.abr2_gn_batch([rf, rf], x, y, [np.ones((1, 4), dtype=complex), v], [w2, w2], scales=sc)
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        mbfir.abr_gn_batch([rf], x, [v[:3]], [w1], scales=sc)
    with pytest.raises(ValueError, match="an empty y"):
        mbfir.abr2_lsq_batch([rf], x, np.zeros(0), [t2], [w2], scales=sc)
    with pytest.raises(ValueError, match="takes"):
        mbfir.refine_batch([rf], x)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.refine_batch([], x, [], [])
    with pytest.raises(ValueError, match="2 targets and 1 weight arrays for 1 pulses"):
        mbfir.refine_batch([rf], x, [t1, t1], [w1])


def test_c_calls_refuse_a_null_context():
    """The C calls' own checks need a context, which needs a device (tests/test_simgn_gpu.py has their messages); without one they
    return MBFIR_E_ARG, as every call does."""
    lib = mbfir.load_library()
    d = np.ones(8)
    off = np.array([0, 2], dtype=np.int64)
    lp, p = off.ctypes.data_as(mbfir._lp), mbfir._ptr(d)
    assert lib.mbfir_abr_lsq_batch(None, 1, lp, p, p, None, 1, lp, p, 1, p, 0, 0, p, p, p, p, p, p) == mbfir.E_ARG
    assert lib.mbfir_abr2_lsq_batch(None, 1, lp, p, p, None, None, 1, lp, p, 1, lp, p, 1, p, 0, 0, p, p, p, p, p, p) == mbfir.E_ARG
    assert lib.mbfir_abr_gn_batch(None, 1, lp, p, p, None, 1, lp, p, 1, p, 0, 0, p, 1, p, p, p, p) == mbfir.E_ARG
    assert lib.mbfir_abr2_gn_batch(None, 1, lp, p, p, None, None, 1, lp, p, 1, lp, p, 1, p, 0, 0, p, 1, p, p, p, p) == mbfir.E_ARG


# ---- refine_batch on the reference ------------------------------------------------------------------------------------------------
N, NX = 5, 9
RSC = (0.9, 1.0, 1.1)


def _split(p):
    return p if isinstance(p, tuple) else (p, None)


def _grid(v, k):
    """the grid of pulse k: a list holds one per pulse"""
    return v[k] if isinstance(v, list) else v


@pytest.fixture
def on_reference(monkeypatch):
    """The four device wrappers replaced by the reference; returns the log of the calls: (name, the rf of every pulse)."""
    log = []

    def lsq1(pulses, x, targets, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        log.append(("lsq", [np.array(_split(p)[0]) for p in pulses]))
        return [ref.lsq(*_split(p), _grid(x, k), t, w, scales, profile, None, hard_pulse)
                for k, (p, t, w) in enumerate(zip(pulses, targets, weights))]

    def lsq2(pulses, x, y, targets, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        log.append(("lsq", [np.array(_split(p)[0]) for p in pulses]))
        return [ref.lsq(*_split(p), _grid(x, k), t, w, scales, profile, _grid(y, k), hard_pulse)
                for k, (p, t, w) in enumerate(zip(pulses, targets, weights))]

    def gn1(pulses, x, tangents, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        log.append(("gn", [np.array(_split(p)[0]) for p in pulses]))
        return [ref.gn(*_split(p), _grid(x, k), v, w, scales, profile, None, hard_pulse)
                for k, (p, v, w) in enumerate(zip(pulses, tangents, weights))]

    def gn2(pulses, x, y, tangents, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        log.append(("gn", [np.array(_split(p)[0]) for p in pulses]))
        return [ref.gn(*_split(p), _grid(x, k), v, w, scales, profile, _grid(y, k), hard_pulse)
                for k, (p, v, w) in enumerate(zip(pulses, tangents, weights))]

    monkeypatch.setattr(mbfir, "abr_lsq_batch", lsq1)
    monkeypatch.setattr(mbfir, "abr2_lsq_batch", lsq2)
    monkeypatch.setattr(mbfir, "abr_gn_batch", gn1)
    monkeypatch.setattr(mbfir, "abr2_gn_batch", gn2)
    return log


def _problem(seed, kind="ex", hard=False):
    """A pulse near 60 degrees, its profile at gain 1 perturbed as the target, weights with zeros"""
    rng = np.random.default_rng(seed)
    rf = (np.hanning(N + 2)[1:-1] + 0.1 * rng.standard_normal(N)) * (np.pi / 3 / np.hanning(N + 2).sum()) + 0j
    x = np.linspace(-2, 2, NX)
    a, b = ref.forward(rf, None, x, None, hard)
    f = ref.profile(kind, a, b)
    t = np.stack([f * (1 + 0.2 * rng.standard_normal(NX)) for _ in RSC])
    w = np.ones((len(RSC), NX))
    w[:, 1] = 0.0
    return rf, x, t, w


@pytest.mark.parametrize("kind,hard", [("ex", False), ("se", True), ("inv", False), ("st", True)])
def test_first_step_is_the_dense_levenberg_marquardt_step(on_reference, kind, hard):
    """cg = 2 (2n) iterations at a fixed mu = 1e-2 trace(H) / 2n: the step that is tried first is the dense solution of
    (H + mu I) d = -g within 1e-4 of max|d|.  rtol = 1e-16 stops CG at a residual of 1e-8 |g|, so that the bound tests the
    recurrence and not the default stop (1e-3 |g|, which alone leaves up to 1e-3 cond)."""
    rf, x, t, w = _problem(1, kind, hard)
    H = _dense_h_sc(rf, x, w, kind, hard)
    _, g = ref.lsq(rf, None, x, t, w, RSC, kind, None, hard)
    mu = 1e-2 * np.trace(H) / (2 * N)
    d = np.linalg.solve(H + mu * np.eye(2 * N), -_realform(g))
    mbfir.refine_batch([rf], x, [t], [w], profile=kind, scales=RSC, hard_pulse=hard, iters=1, cg=2 * 2 * N, mu0=mu, rtol=1e-16)
    trial = [c for c in on_reference if c[0] == "lsq"][1][1][0]                  # the second lsq call tries rf + d
    err = np.abs(_realform(trial - rf) - d).max() / np.abs(d).max()
    print("%s hard %s: first step against the dense solve %.3g (condition number %.0f)" % (kind, hard, err, np.linalg.cond(H + mu * np.eye(2 * N))))
    assert err <= 1e-4


def _dense_h_sc(rf, x, w, kind, hard):
    cols = []
    for j in range(2 * N):
        e = np.zeros(N, dtype=complex)
        e[j % N] = 1.0 if j < N else 1j
        cols.append(_realform(ref.gn(rf, None, x, e, w, RSC, kind, None, hard)))
    return np.stack(cols, axis=1)


def test_accepted_losses_strictly_decrease(on_reference):
    rf, x, t, w = _problem(2)
    (out,), (info,) = mbfir.refine_batch([rf], x, [t], [w], scales=RSC, iters=4)
    L = info["losses"]
    assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:]))
    assert L[0] == ref.lsq(rf, None, x, t, w, RSC)[0] and L[-1] == ref.lsq(out, None, x, t, w, RSC)[0]
    assert info["calls"]["lsq"] == 1 + (len(L) - 1) + info["refused"]
    assert info["calls"]["gn"] == sum(1 for c in on_reference if c[0] == "gn")
    assert info["status"] in ("iters", "converged", "gave_up")


def test_a_refused_step_changes_only_mu(on_reference, monkeypatch):
    """The first trial step is refused by force (its loss reported as infinite): the run then continues as the run that started
    from four times the mu, from the same rf and gradient."""
    rf, x, t, w = _problem(3)
    mu = 0.05
    (want,), (winfo,) = mbfir.refine_batch([rf], x, [t], [w], scales=RSC, iters=2, mu0=4 * mu)
    honest, count = mbfir.abr_lsq_batch, [0]

    def refusing(*a, **k):
        count[0] += 1
        res = honest(*a, **k)
        return [(np.inf, g) for _, g in res] if count[0] == 2 else res

    monkeypatch.setattr(mbfir, "abr_lsq_batch", refusing)
    del on_reference[:]
    (got,), (ginfo,) = mbfir.refine_batch([rf], x, [t], [w], scales=RSC, iters=2, mu0=mu)
    assert ginfo["refused"] == winfo["refused"] + 1
    assert ginfo["losses"] == winfo["losses"] and ginfo["mu"] == winfo["mu"]
    assert np.array_equal(got, want)
    second = [k for k, c in enumerate(on_reference) if c[0] == "lsq"][1]
    gn_after = on_reference[second + 1]
    assert gn_after[0] == "gn" and np.array_equal(gn_after[1][0], rf)           # the next CG runs at the unchanged rf


def test_a_pulse_in_a_batch_has_the_bits_of_the_pulse_alone(on_reference):
    probs = [_problem(s) for s in (4, 5, 6)]
    x = probs[0][1]
    kw = dict(scales=RSC, iters=3, cg=4)
    alone = [mbfir.refine_batch([p[0]], x, [p[2]], [p[3]], **kw) for p in probs]
    for order in ((0, 1, 2), (2, 1, 0)):
        rfs, infos = mbfir.refine_batch([probs[q][0] for q in order], x, [probs[q][2] for q in order], [probs[q][3] for q in order],
                                        **kw)
        for k, q in enumerate(order):
            assert np.array_equal(rfs[k], alone[q][0][0])
            assert infos[k] == alone[q][1][0]


def test_refine_batch_in_two_dimensions_with_per_pulse_grids(on_reference):
    rng = np.random.default_rng(9)
    rf = [0.2 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) for _ in range(2)]
    g = np.full(N, 2 * np.pi / N) + 0.3j
    xs, ys = [np.linspace(-1, 1, 3), np.linspace(-2, 2, 4)], [np.linspace(-1, 1, 2), np.linspace(-1, 1, 2)]
    t = [np.zeros((1, 3, 2), dtype=complex), np.zeros((1, 4, 2), dtype=complex)]
    w = [np.ones((3, 2)), np.ones((4, 2))]
    rfs, infos = mbfir.refine_batch([(r, g) for r in rf], xs, ys, t, w, iters=2)
    for q in range(2):
        (r1,), (i1,) = mbfir.refine_batch([(rf[q], g)], xs[q], ys[q], [t[q]], [w[q]], iters=2)
        assert np.array_equal(rfs[q], r1) and infos[q] == i1
        assert infos[q]["losses"][-1] < infos[q]["losses"][0]
