"""The NumPy reference of the least-squares products of the Bloch simulator's steady state (tests/blochssgn_ref.py, no GPU): its
float64 results against its long-double ones on the cases of tests/test_blochssgn_gpu.py, the gradient against central differences
of the loss, the dense Gauss-Newton operator, the two products against the compositions of blochss_ref.ss_vjp_scaled and
blochss_ref.ss_jvp they fuse, and the bindings, the argument errors and the Levenberg-Marquardt loop of mbfir.bloch_ss_lsq_batch /
mbfir.bloch_ss_gn_batch / mbfir.refine_bloch_batch(steady_state=True), none of which needs a device."""
import ctypes
import functools
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochssgn_ref", os.path.join(ROOT, "tests", "blochssgn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
ssref = ref.ssref
K = 2


@functools.lru_cache(maxsize=None)
def _case(shared):
    return ref.cases(shared, K)


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_is_the_longdouble_one_to_a_hundredth_of_the_device_bounds(shared):
    """The shares measured here, before any device run: at most 6.8e-6 of the bound of L, 3.2e-7 of g's and 1.1e-6 of H v's (the
    kappa^3 term of the seed's error dominates both bounds: against bound_b1 of the exact cotangent alone the float64 reference
    reaches 5.1e-4 for g and 5.6e-3 for H v)."""
    pulses, dfs, dps, tgs, wts, vs = _case(shared)
    for q, (p, df, dp, t, w, v) in enumerate(zip(pulses, dfs, dps, tgs, wts, vs)):
        k = ref.kappa(p, df, dp, ref.SCALES)
        L64, g64 = ref.lsq(p, df, dp, t, w, ref.SCALES)
        Lld, gld, li = ref.lsq(p, df, dp, t, w, ref.SCALES, dtype=np.longdouble, parts=True)
        h64 = ref.gn(p, df, dp, v, w, ref.SCALES)
        hld, hi = ref.gn(p, df, dp, v, w, ref.SCALES, dtype=np.longdouble, parts=True)
        bg, bh, bl = ref.bound_g(p, li, ref.SCALES, k), ref.bound_h(p, v, hi, ref.SCALES, k), ref.bound_L(li, k)
        eg, eh, el = np.abs(g64 - gld).astype(np.float64), np.abs(h64 - hld).astype(np.float64), abs(float(L64 - Lld))
        print("shared %s n %d points %dx%d kappa %.4g: worst shares of the bounds: g %.3g, H v %.3g, L %.3g"
              % (shared, len(p[0]), len(df), np.shape(dp)[0], k, (eg / bg).max(), (eh / bh).max(), el / bl))
        assert np.all(eg <= bg / 100) and np.all(eh <= bh / 100) and el <= bl / 100, q


def _fd_problem():
    """tests/test_blochss_cpu.py's: 64 samples of 10 us and a dead time of 160 us (a period of 0.8 ms) at T1 = 0.1 s, T2 = 0.03 s on
    5 x 7 points, kappa = 119; weights with a third zero and targets in [-1, 1] at scales 0.9, 1.0, 1.1"""
    rng = np.random.default_rng(7)
    n, gamma = 65, ssref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 / (gamma * 64e-5))
    b1[20], b1[-1] = 0.0, 0.0
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.1
    gr[-1] = 0.0
    tp = np.full(n, 1e-5)
    tp[-1] = 1.6e-4
    pulse = (b1, gr, tp, 0.1, 0.03, "H-1")
    df, dp = ref._grid(5, 150.0), np.stack([ref._grid(7, 2.0), ref._grid(7, 1.0)], 1)
    w = rng.uniform(0, 1, (3, 3, 5, 7))
    w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
    return pulse, df, dp, tuple(rng.uniform(-1, 1, (3, 3, 5, 7))), tuple(w), (0.9, 1.0, 1.1)


# The central difference of the long-double loss with DESIGN 8t's step, FD_STEP |b1|, reaches 1.8e-8 of max|g| per real coordinate on
# this problem and 1.5e-8 of |g| along g / |g| (the truncation of the dead-time entry, whose gamma dt is 16 times the others'; it
# falls with the square of the step, but the float64 loss of the device test could not follow a smaller one).  8t's 1e-7 would keep
# a factor of 5.5 over that; the tolerance is 2e-7, a factor of ten.  tests/test_blochssgn_gpu.py uses the same step and tolerance
# along g / |g|.
FD_STEP, FD_TOL = 1e-5, 2e-7


def test_gradient_is_the_central_difference_of_the_loss_in_every_real_coordinate():
    p, df, dp, t, w, sc = _fd_problem()
    assert abs(ref.kappa(p, df, dp, sc) - 119) < 1
    _, g = ref.lsq(p, df, dp, t, w, sc)
    n, h = len(p[0]), FD_STEP * float(np.linalg.norm(p[0]))
    fd = np.zeros(n, dtype=complex)
    for j in range(2 * n):
        e = np.zeros(n, dtype=complex)
        e[j % n] = 1.0 if j < n else 1j
        lp = ref.lsq((p[0] + h * e,) + p[1:], df, dp, t, w, sc, dtype=np.longdouble)[0]
        lm = ref.lsq((p[0] - h * e,) + p[1:], df, dp, t, w, sc, dtype=np.longdouble)[0]
        fd[j % n] += (1 if j < n else 1j) * float((lp - lm) / (2 * h))
    rel = float(np.abs(fd - g).max() / np.abs(g).max())
    nrm = float(np.linalg.norm(g))
    d = g / nrm
    along = float((ref.lsq((p[0] + h * d,) + p[1:], df, dp, t, w, sc, dtype=np.longdouble)[0]
                   - ref.lsq((p[0] - h * d,) + p[1:], df, dp, t, w, sc, dtype=np.longdouble)[0]) / (2 * h))
    print("max|g| %.6g, |central difference - g| / max|g| %.3g; along g / |g|: relative difference %.3g"
          % (np.abs(g).max(), rel, abs(along - nrm) / nrm))
    assert rel <= FD_TOL / 10 and abs(along - nrm) <= FD_TOL / 10 * nrm          # the factor of ten the tolerance keeps


def _realform(v):
    return np.concatenate([np.real(v), np.imag(v)], -1)


def _dense_h(p, df, dp, w, sc, dtype=np.float64):
    n = len(p[0])
    e = np.concatenate([np.eye(n), 1j * np.eye(n)])
    return _realform(ref.gn(p, df, dp, e, w, sc, dtype=dtype)).T


def _small(n, seed=3):
    """n samples and a dead time on 3 x 5 points, T1 = 50 periods"""
    rng = np.random.default_rng(seed)
    gamma, dt = ssref.GAMMA_H1, 2e-5
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 / (gamma * n * dt))
    b1[-1] = 0.0
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.1
    tp = np.full(n, dt)
    tp[-1] = 4 * n * dt
    tr = float(tp.sum())
    df, dp = ref._grid(3, 200.0), np.stack([ref._grid(5, 2.0), ref._grid(5, 1.0)], 1)
    w = rng.uniform(0, 1, (3, 3, 3, 5))
    w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
    return (b1, gr, tp, 50 * tr, 10 * tr, "H-1"), df, dp, tuple(rng.uniform(-1, 1, (3, 3, 3, 5))), tuple(w), (0.9, 1.0, 1.1)


def test_dense_gauss_newton_operator_is_symmetric_positive_semidefinite():
    p, df, dp, _, w, sc = _small(7)
    n = 7
    H = _dense_h(p, df, dp, w, sc)
    size = np.linalg.norm(H, 2)
    asym, low = np.abs(H - H.T).max() / size, np.linalg.eigvalsh((H + H.T) / 2).min() / size
    print("|H - H'| / |H| %.3g, smallest eigenvalue / |H| %.3g" % (asym, low))
    assert asym <= 1e-13 and low >= -1e-13
    rng = np.random.default_rng(8)
    v = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    hv, info = ref.gn(p, df, dp, v, w, sc, dtype=np.longdouble, parts=True)
    for k in range(2):
        quad = float((np.conj(v[k]) * hv[k]).real.sum())
        assert abs(quad - float(info["E"][k])) <= 1e-13 * abs(quad), k       # Re <v, H v> = sum w |J v|^2
        assert np.abs(_realform(hv[k]).astype(np.float64) - H @ _realform(v[k])).max() <= 1e-12 * size * np.abs(v[k]).sum()


def test_the_products_are_the_compositions_they_fuse():
    """blochss_ref.ss_scaled -> residual -> ss_vjp_scaled, and ss_jvp -> weights -> ss_vjp_scaled direction by direction: within a
    thousandth of the device bounds (the sums over the points may run in another order), on the 3 x 5 cases"""
    pulses, dfs, dps, tgs, wts, vs = _case(True)
    for q in (0, 1, 3, 4):
        p, df, dp, t, w, v = pulses[q], dfs[q], dps[q], tgs[q], wts[q], vs[q]
        k = ref.kappa(p, df, dp, ref.SCALES)
        L, g, li = ref.lsq(p, df, dp, t, w, ref.SCALES, parts=True)
        h, hi = ref.gn(p, df, dp, v, w, ref.SCALES, parts=True)
        M = ssref.ss_scaled(p, df, dp, ref.SCALES)
        r = [M[c] - t[c] for c in range(3)]
        L2 = sum((w[c] * r[c] * r[c]).sum() for c in range(3)) / 2
        g2, _ = ssref.ss_vjp_scaled(p, df, dp, [w[c] * r[c] for c in range(3)], ref.SCALES)
        _, dM = ssref.ss_jvp(p, df, dp, v, ref.SCALES)
        h2 = np.stack([ssref.ss_vjp_scaled(p, df, dp, [w[c] * dM[c][j] for c in range(3)], ref.SCALES)[0] for j in range(len(v))])
        assert all(np.array_equal(a, b) for a, b in zip(li["M"], M)), q
        assert abs(L - L2) <= ref.bound_L(li, k) / 1000
        assert np.all(np.abs(g - g2) <= ref.bound_g(p, li, ref.SCALES, k) / 1000), q
        assert np.all(np.abs(h - h2) <= ref.bound_h(p, v, hi, ref.SCALES, k) / 1000), q


# ---- the bindings ------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_bloch_ss_lsq_batch\s*\(", hdr) and re.search(r"\bmbfir_bloch_ss_gn_batch\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_bloch_ss_lsq_batch"][1]) == 35
    assert len(mbfir.SYMBOLS["mbfir_bloch_ss_gn_batch"][1]) == 31
    for name, count in (("mbfir_bloch_ss_lsq_batch", 35), ("mbfir_bloch_ss_gn_batch", 31)):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        assert len(decl.split(",")) == count, name
    lib = mbfir.load_library()
    assert getattr(lib, "mbfir_bloch_ss_lsq_batch") is not None and getattr(lib, "mbfir_bloch_ss_gn_batch") is not None
    assert callable(mbfir.bloch_ss_lsq_batch) and callable(mbfir.bloch_ss_gn_batch)
    assert "steady_state" in inspect.signature(mbfir.refine_bloch_batch).parameters
    src = open(os.path.join(ROOT, "multiband-rf-pulse-design_amd", "csrc", "blochssgn.hip")).read()
    assert "k_bloch_ss_lsq_batch" in src and "k_bloch_ss_gn_batch" in src and "atomic" not in src.replace("No atomics", "")
    assert "blochssgn.o" in open(os.path.join(ROOT, "multiband-rf-pulse-design_amd", "csrc", "Makefile")).read()


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    v, z, one = np.ones(4, dtype=complex), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for fn, who, arg in ((mbfir.bloch_ss_lsq_batch, "bloch_ss_lsq_batch", z), (mbfir.bloch_ss_gn_batch, "bloch_ss_gn_batch", v)):
        with pytest.raises(ValueError, match=who + ": no pulses"):
            fn([], df, dp, [], [])
        with pytest.raises(ValueError, match="scale list is empty"):
            fn([p], df, dp, [arg], [one], scales=())
        with pytest.raises(ValueError, match="empty grid"):
            fn([p], np.zeros(0), dp, [arg], [one])
        with pytest.raises(ValueError, match="2 weight triples for 1 pulses"):
            fn([p], df, dp, [arg], [one, one])
        with pytest.raises(ValueError, match="must be a triple"):
            fn([p], df, dp, [arg], [(1.0, 1.0)])
        with pytest.raises(ValueError, match="has shape"):
            fn([p], df, dp, [arg], [(1.0, 1.0, np.ones((3, 4)))])
        with pytest.raises(ValueError, match="has shape"):                                # two scales' worth of weights for one scale
            fn([p], df, dp, [arg], [(1.0, 1.0, np.ones((2, 3, 5)))])
        with pytest.raises(ValueError, match="negative or not finite"):
            fn([p], df, dp, [arg], [(1.0, -1.0, 1.0)])
        with pytest.raises(ValueError, match="negative or not finite"):
            fn([p], df, dp, [arg], [(1.0, np.full((3, 5), np.nan), 1.0)])
        with pytest.raises(TypeError):                                                    # the steady state takes no m0
            fn([p], df, dp, [arg], [one], m0=(0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="2 target triples for 1 pulses"):
        mbfir.bloch_ss_lsq_batch([p], df, dp, [z, z], [one])
    with pytest.raises(ValueError, match="must be a triple"):
        mbfir.bloch_ss_lsq_batch([p], df, dp, [np.zeros((3, 5))], [one])
    with pytest.raises(ValueError, match="has shape"):
        mbfir.bloch_ss_lsq_batch([p], df, dp, [(0.0, 0.0, np.zeros(5))], [one])
    with pytest.raises(ValueError, match="2 tangents for 1 pulses"):
        mbfir.bloch_ss_gn_batch([p], df, dp, [v, v], [one])
    with pytest.raises(ValueError, match="has shape"):
        mbfir.bloch_ss_gn_batch([p], df, dp, [v[:3]], [one])
    with pytest.raises(ValueError, match="every pulse takes the same K"):                 # a ragged K
        mbfir.bloch_ss_gn_batch([p, p], df, dp, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)], [one, one])
    with pytest.raises(ValueError, match="refine_bloch_batch: no pulses"):
        mbfir.refine_bloch_batch([], df, dp, [], [], steady_state=True)
    with pytest.raises(ValueError, match="2 target and 1 weight triples for 1 pulses"):
        mbfir.refine_bloch_batch([p], df, dp, [z, z], [one], steady_state=True)
    with pytest.raises(ValueError, match="iters must be at least 0 and cg at least 1"):
        mbfir.refine_bloch_batch([p], df, dp, [z], [one], cg=0, steady_state=True)
    with pytest.raises(ValueError, match="does not depend on m0"):
        mbfir.refine_bloch_batch([p], df, dp, [z], [one], m0=(0.0, 0.0, 1.0), steady_state=True)
    with pytest.raises(ValueError, match="steady-state device step is not built"):
        mbfir.refine_bloch_batch([p], df, dp, [z], [one], solver="device", steady_state=True)


def test_c_calls_refuse_a_null_context():
    """before they read anything else (the checks that need a context: tests/test_blochssgn_gpu.py)"""
    for name in ("mbfir_bloch_ss_lsq_batch", "mbfir_bloch_ss_gn_batch"):
        args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
        assert getattr(mbfir.load_library(), name)(*args) == mbfir.E_ARG


# ---- refine_bloch_batch(steady_state=True) on the calls stubbed by the reference -------------------------------------------------
N, RSC = 5, (0.9, 1.0, 1.1)


def _grid_of(v, k):
    return v[k] if isinstance(v, list) else v


@pytest.fixture
def on_reference(monkeypatch):
    """The two device wrappers replaced by the reference, and the transient ones by calls that fail; returns the log of the calls:
    (name, the b1 of every pulse)."""
    log = []

    def lsq(pulses, df, dp, targets, weights, *, scales=(1.0,), steady=False, ctx=None):
        log.append(("lsq", [np.array(p[0]) for p in pulses]))
        return [tuple(ref.lsq(p, _grid_of(df, k), _grid_of(dp, k), t, w, scales)) for k, (p, t, w) in enumerate(zip(pulses, targets, weights))]

    def gn(pulses, df, dp, tangents, weights, *, scales=(1.0,), ctx=None):
        log.append(("gn", [np.array(p[0]) for p in pulses]))
        return [ref.gn(p, _grid_of(df, k), _grid_of(dp, k), v, w, scales) for k, (p, v, w) in enumerate(zip(pulses, tangents, weights))]

    def transient(*a, **k):
        raise AssertionError("steady_state=True called a transient product")

    monkeypatch.setattr(mbfir, "bloch_ss_lsq_batch", lsq, raising=False)
    monkeypatch.setattr(mbfir, "bloch_ss_gn_batch", gn, raising=False)
    monkeypatch.setattr(mbfir, "bloch_lsq_batch", transient)
    monkeypatch.setattr(mbfir, "bloch_gn_batch", transient)
    return log


def _problem(seed):
    """A period of 5 samples (four of b1 near 40 degrees in all, then a dead time) on 3 x 3 points at T1 = 40 periods; the target is
    its own steady state at gain 1, perturbed; weights with zeros, none on mx at all"""
    rng = np.random.default_rng(seed)
    gamma, dt = ssref.GAMMA_H1, 1e-4
    b1 = np.append((np.hanning(N + 1)[1:-1] + 0.1 * rng.standard_normal(N - 1)) * (0.7 / (gamma * dt * np.hanning(N + 1).sum())), 0.0) + 0j
    tp = np.append(np.full(N - 1, dt), 1.6e-3)
    p = (b1, np.append(rng.uniform(0.5, 1.5, N - 1) * 0.05, 0.0), tp, 40 * 2e-3, 10 * 2e-3, "H-1")
    df, dp = ref._grid(3, 100.0), ref._grid(3, 2.0)
    m = ssref.ss(p, df, dp)
    t = (0.0, m[1] * (1 + 0.2 * rng.standard_normal((3, 3))), np.stack([m[2] + 0.1 * rng.standard_normal((3, 3)) for _ in RSC]))
    w = np.ones((3, 3))
    w[1, 1] = 0.0
    return p, df, dp, t, (0.0, w, np.stack([w] * 3))


def test_first_step_is_the_dense_levenberg_marquardt_step(on_reference):
    """cg = 2 (2n) iterations at a fixed mu = 1e-2 trace(H) / 2n and rtol = 1e-16: the step that is tried first is the dense
    solution of (H + mu I) d = -g within 1e-4 of max|d|"""
    p, df, dp, t, w = _problem(1)
    H = _dense_h(p, df, dp, w, RSC)
    _, g = ref.lsq(p, df, dp, t, w, RSC)
    mu = 1e-2 * np.trace(H) / (2 * N)
    d = np.linalg.solve(H + mu * np.eye(2 * N), -_realform(g))
    mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=1, cg=2 * 2 * N, mu0=mu, rtol=1e-16, steady_state=True)
    trial = [c for c in on_reference if c[0] == "lsq"][1][1][0]                  # the second lsq call tries b1 + d
    err = np.abs(_realform(trial - p[0]) - d).max() / np.abs(d).max()
    print("first step against the dense solve %.3g (condition number %.0f)" % (err, np.linalg.cond(H + mu * np.eye(2 * N))))
    assert err <= 1e-4


def test_accepted_losses_strictly_decrease(on_reference):
    p, df, dp, t, w = _problem(2)
    (out,), (info,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=4, steady_state=True)
    L = info["losses"]
    assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:]))
    assert L[0] == ref.lsq(p, df, dp, t, w, RSC)[0] and L[-1] == ref.lsq((out,) + p[1:], df, dp, t, w, RSC)[0]
    assert info["calls"]["lsq"] == 1 + (len(L) - 1) + info["refused"]
    assert info["calls"]["gn"] == sum(1 for c in on_reference if c[0] == "gn")
    assert info["status"] in ("iters", "converged", "gave_up")
    assert out.shape == (N,) and out.dtype == np.complex128


def test_a_pulse_in_a_batch_has_the_bits_of_the_pulse_alone(on_reference):
    probs = [_problem(s) for s in (4, 5, 6)]
    df, dp = probs[0][1], probs[0][2]
    kw = dict(scales=RSC, iters=3, cg=4, steady_state=True)
    alone = [mbfir.refine_bloch_batch([p[0]], df, dp, [p[3]], [p[4]], **kw) for p in probs]
    for order in ((0, 1, 2), (2, 1, 0)):
        b1s, infos = mbfir.refine_bloch_batch([probs[q][0] for q in order], df, dp, [probs[q][3] for q in order],
                                              [probs[q][4] for q in order], **kw)
        for k, q in enumerate(order):
            assert np.array_equal(b1s[k], alone[q][0][0])
            assert infos[k] == alone[q][1][0]


def test_the_default_path_calls_the_transient_products(monkeypatch):
    """steady_state=False (the default) goes to bloch_lsq_batch / bloch_gn_batch with m0, as before"""
    seen = []

    def lsq(pulses, df, dp, targets, weights, *, scales=(1.0,), m0=None, ctx=None):
        seen.append(("lsq", m0))
        return [(1.0, np.zeros(len(p[0]), dtype=complex)) for p in pulses]

    def steady(*a, **k):
        raise AssertionError("the default path called a steady-state product")
    monkeypatch.setattr(mbfir, "bloch_lsq_batch", lsq)
    monkeypatch.setattr(mbfir, "bloch_ss_lsq_batch", steady, raising=False)
    monkeypatch.setattr(mbfir, "bloch_ss_gn_batch", steady, raising=False)
    p, df, dp, t, w = _problem(1)
    _, (info,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, m0=(0.0, 0.0, 1.0))
    assert seen == [("lsq", (0.0, 0.0, 1.0))] and info["status"] == "converged"
