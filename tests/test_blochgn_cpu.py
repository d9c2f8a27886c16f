"""The NumPy reference of the Bloch simulator's least-squares products (tests/blochgn_ref.py, no GPU): its float64 results against
its long-double ones on the cases of tests/test_blochgn_gpu.py, the gradient against central differences of the loss, the dense
Gauss-Newton operator, the two products against the compositions of blochgrad_ref.vjp and blochjvp_ref.jvp they fuse, and the
bindings, the argument errors and the Levenberg-Marquardt loop of mbfir.bloch_lsq_batch / mbfir.bloch_gn_batch /
mbfir.refine_bloch_batch, none of which needs a device."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochgn_ref", os.path.join(ROOT, "tests", "blochgn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
K = 2


@functools.lru_cache(maxsize=None)
def _case(shared):
    return ref.cases(shared, K)


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_is_the_longdouble_one_to_a_twentieth_of_the_device_bounds(shared):
    pulses, dfs, dps, m0s, tgs, wts, vs = _case(shared)
    for q, (p, df, dp, m0, t, w, v) in enumerate(zip(pulses, dfs, dps, m0s, tgs, wts, vs)):
        L64, g64 = ref.lsq(p, df, dp, t, w, ref.SCALES, m0)
        Lld, gld, li = ref.lsq(p, df, dp, t, w, ref.SCALES, m0, dtype=np.longdouble, parts=True)
        h64 = ref.gn(p, df, dp, v, w, ref.SCALES, m0)
        hld, hi = ref.gn(p, df, dp, v, w, ref.SCALES, m0, dtype=np.longdouble, parts=True)
        bg, bh, bl = ref.bound_g(p, li, ref.SCALES), ref.bound_h(p, v, hi, ref.SCALES), ref.bound_L(li)
        eg, eh, el = np.abs(g64 - gld).astype(np.float64), np.abs(h64 - hld).astype(np.float64), abs(float(L64 - Lld))
        print("shared %s n %d points %dx%d: worst shares of the bounds: g %.3g, H v %.3g, L %.3g"
              % (shared, len(p[0]), len(df), np.shape(dp)[0], (eg / bg).max(), (eh / bh).max(), el / bl if bl else 0.0))
        assert np.all(eg <= bg / 20) and np.all(eh <= bh / 20) and el <= bl / 20, q


def _small(t2, n=16, seed=3):
    rng = np.random.default_rng(seed)
    dur, gamma = 4e-3, ref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.5 / (gamma * dur))
    b1[n // 3] = 0.0
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.1
    df, dp = ref._grid(3, 200.0), np.stack([ref._grid(5, 2.0), ref._grid(5, 1.0)], 1)
    m0 = tuple(rng.uniform(-0.5, 0.5, (3, 3, 5)))
    sc = (0.9, 1.0, 1.1)
    w = rng.uniform(0, 1, (3, 3, 3, 5))
    w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
    t = rng.uniform(-1, 1, (3, 3, 3, 5))
    return (b1, gr, dur / n, 1.0, t2, "H-1"), df, dp, m0, sc, tuple(t), tuple(w)


@pytest.mark.parametrize("t2", [40e-3, 1e-3])
def test_gradient_is_the_central_difference_of_the_loss(t2):
    """16 samples on 3 x 5 points at three scales, every real coordinate of b1 moved by h = 1e-6 of max|b1| (truncation h^2, the
    loss in long double so that rounding does not count): within 1e-7 of max|g|"""
    p, df, dp, m0, sc, t, w = _small(t2)
    _, g = ref.lsq(p, df, dp, t, w, sc, m0)
    n, size, h = len(p[0]), np.abs(p[0]).max(), 1e-6
    fd = np.zeros(n, dtype=complex)
    for j in range(2 * n):
        e = np.zeros(n, dtype=complex)
        e[j % n] = size if j < n else 1j * size
        lp = ref.lsq((p[0] + h * e,) + p[1:], df, dp, t, w, sc, m0, dtype=np.longdouble)[0]
        lm = ref.lsq((p[0] - h * e,) + p[1:], df, dp, t, w, sc, m0, dtype=np.longdouble)[0]
        fd[j % n] += (1 if j < n else 1j) * float((lp - lm) / (2 * h)) / size
    rel = float(np.abs(fd - g).max() / np.abs(g).max())
    print("T2 %.0e: max|g| %.6g, |central difference - g| / max|g| %.3g" % (t2, np.abs(g).max(), rel))
    assert rel <= 1e-7


def _realform(v):
    return np.concatenate([np.real(v), np.imag(v)], -1)


def _dense_h(p, df, dp, w, sc, m0):
    n = len(p[0])
    e = np.concatenate([np.eye(n), 1j * np.eye(n)])
    return _realform(ref.gn(p, df, dp, e, w, sc, m0)).T


def test_dense_gauss_newton_operator_is_symmetric_positive_semidefinite():
    p, df, dp, m0, sc, _, w = _small(40e-3, n=7)
    n = 7
    H = _dense_h(p, df, dp, w, sc, m0)
    size = np.linalg.norm(H, 2)
    asym, low = np.abs(H - H.T).max() / size, np.linalg.eigvalsh((H + H.T) / 2).min() / size
    print("|H - H'| / |H| %.3g, smallest eigenvalue / |H| %.3g" % (asym, low))
    assert asym <= 1e-13 and low >= -1e-13
    rng = np.random.default_rng(8)
    v = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    hv, info = ref.gn(p, df, dp, v, w, sc, m0, parts=True)
    for k in range(2):
        quad = float((np.conj(v[k]) * hv[k]).real.sum())
        assert abs(quad - float(info["E"][k])) <= 1e-13 * abs(quad), k       # Re <v, H v> = sum w |J v|^2
        assert np.abs(_realform(hv[k]) - H @ _realform(v[k])).max() <= 1e-13 * size * np.abs(v[k]).sum()


def _compose_lsq(p, df, dp, t, w, sc, m0):
    """bloch forward -> residual -> blochgrad_ref.vjp, scale by scale"""
    b1, gr, tp, t1, t2, nuc = p
    L, g = 0.0, 0
    for k, s in enumerate(sc):
        m = ref.forward(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nuc), s, m0)
        r = [m[c] - t[c][k] for c in range(3)]
        L += sum((w[c][k] * r[c] * r[c]).sum() for c in range(3)) / 2
        g = g + ref.vjp(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nuc), s, m0, [w[c][k] * r[c] for c in range(3)])[0]
    return L, g


def _compose_gn(p, df, dp, v, w, sc, m0):
    """blochjvp_ref.jvp -> weights -> blochgrad_ref.vjp, scale by scale and direction by direction"""
    b1, gr, tp, t1, t2, nuc = p
    h = np.zeros(np.shape(v), dtype=complex)
    for k, s in enumerate(sc):
        _, dm = ref.jvp(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nuc), s, m0, v)
        for j in range(len(v)):
            h[j] += ref.vjp(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nuc), s, m0, [w[c][k] * dm[c][j] for c in range(3)])[0]
    return h


def test_the_products_are_the_compositions_they_fuse():
    """Within a thousandth of the device bounds (the sums over the points may run in another order), on the 3 x 5 cases"""
    pulses, dfs, dps, m0s, tgs, wts, vs = _case(True)
    for q in (0, 1, 3, 4):
        p, df, dp, m0, t, w, v = pulses[q], dfs[q], dps[q], m0s[q], tgs[q], wts[q], vs[q]
        L, g, li = ref.lsq(p, df, dp, t, w, ref.SCALES, m0, parts=True)
        h, hi = ref.gn(p, df, dp, v, w, ref.SCALES, m0, parts=True)
        L2, g2 = _compose_lsq(p, df, dp, t, w, ref.SCALES, m0)
        h2 = _compose_gn(p, df, dp, v, w, ref.SCALES, m0)
        assert abs(L - L2) <= ref.bound_L(li) / 1000
        assert np.all(np.abs(g - g2) <= ref.bound_g(p, li, ref.SCALES) / 1000), q
        assert np.all(np.abs(h - h2) <= ref.bound_h(p, v, hi, ref.SCALES) / 1000), q


def test_scalar_and_per_scale_planes_broadcast():
    p, df, dp, m0, sc, t, w = _small(40e-3, n=5)
    full = ref.lsq(p, df, dp, (0.0, 0.0, t[2]), (0.0, 0.0, w[2][0]), sc, m0)
    wide = ref.lsq(p, df, dp, (np.zeros((3, 3, 5)), np.zeros((3, 5)), t[2]), (np.zeros((3, 5)), 0.0, np.stack([w[2][0]] * 3)), sc, m0)
    assert full[0] == wide[0] and np.array_equal(full[1], wide[1])


# ---- the bindings ------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_bloch_lsq_batch\s*\(", hdr) and re.search(r"\bmbfir_bloch_gn_batch\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_bloch_lsq_batch"][1]) == 35
    assert len(mbfir.SYMBOLS["mbfir_bloch_gn_batch"][1]) == 34
    lib = mbfir.load_library()
    assert getattr(lib, "mbfir_bloch_lsq_batch") is not None and getattr(lib, "mbfir_bloch_gn_batch") is not None
    assert callable(mbfir.bloch_lsq_batch) and callable(mbfir.bloch_gn_batch) and callable(mbfir.refine_bloch_batch)
    src = open(os.path.join(ROOT, "multiband-rf-pulse-design_amd", "csrc", "blochgn.hip")).read()
    assert "k_bloch_lsq_batch" in src and "k_bloch_gn_batch" in src and "atomic" not in src.replace("No atomics", "")


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    v, z, one = np.ones(4, dtype=complex), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for fn, who, arg in ((mbfir.bloch_lsq_batch, "bloch_lsq_batch", z), (mbfir.bloch_gn_batch, "bloch_gn_batch", v)):
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
    with pytest.raises(ValueError, match="2 target triples for 1 pulses"):
        mbfir.bloch_lsq_batch([p], df, dp, [z, z], [one])
    with pytest.raises(ValueError, match="must be a triple"):
        mbfir.bloch_lsq_batch([p], df, dp, [np.zeros((3, 5))], [one])
    with pytest.raises(ValueError, match="has shape"):
        mbfir.bloch_lsq_batch([p], df, dp, [(0.0, 0.0, np.zeros(5))], [one])
    with pytest.raises(ValueError, match="2 tangents for 1 pulses"):
        mbfir.bloch_gn_batch([p], df, dp, [v, v], [one])
    with pytest.raises(ValueError, match="has shape"):
        mbfir.bloch_gn_batch([p], df, dp, [v[:3]], [one])
    with pytest.raises(ValueError, match="every pulse takes the same K"):                 # a ragged K
        mbfir.bloch_gn_batch([p, p], df, dp, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)], [one, one])
    with pytest.raises(ValueError, match="refine_bloch_batch: no pulses"):
        mbfir.refine_bloch_batch([], df, dp, [], [])
    with pytest.raises(ValueError, match="2 target and 1 weight triples for 1 pulses"):
        mbfir.refine_bloch_batch([p], df, dp, [z, z], [one])
    with pytest.raises(ValueError, match="iters must be at least 0 and cg at least 1"):
        mbfir.refine_bloch_batch([p], df, dp, [z], [one], cg=0)


def test_c_calls_refuse_a_null_context():
    """before they read anything else (the checks that need a context: tests/test_blochgn_gpu.py)"""
    for name in ("mbfir_bloch_lsq_batch", "mbfir_bloch_gn_batch"):
        args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
        assert getattr(mbfir.load_library(), name)(*args) == mbfir.E_ARG


# ---- refine_bloch_batch on the calls stubbed by the reference -------------------------------------------------------------------
N, RSC = 5, (0.9, 1.0, 1.1)


def _grid_of(v, k):
    return v[k] if isinstance(v, list) else v


@pytest.fixture
def on_reference(monkeypatch):
    """The two device wrappers replaced by the reference; returns the log of the calls: (name, the b1 of every pulse)."""
    log = []

    def lsq(pulses, df, dp, targets, weights, *, scales=(1.0,), m0=None, ctx=None):
        log.append(("lsq", [np.array(p[0]) for p in pulses]))
        return [tuple(ref.lsq(p, _grid_of(df, k), _grid_of(dp, k), t, w, scales, m0[k] if isinstance(m0, list) else m0))
                for k, (p, t, w) in enumerate(zip(pulses, targets, weights))]

    def gn(pulses, df, dp, tangents, weights, *, scales=(1.0,), m0=None, ctx=None):
        log.append(("gn", [np.array(p[0]) for p in pulses]))
        return [ref.gn(p, _grid_of(df, k), _grid_of(dp, k), v, w, scales, m0[k] if isinstance(m0, list) else m0)
                for k, (p, v, w) in enumerate(zip(pulses, tangents, weights))]

    monkeypatch.setattr(mbfir, "bloch_lsq_batch", lsq)
    monkeypatch.setattr(mbfir, "bloch_gn_batch", gn)
    return log


def _problem(seed):
    """A 5-sample pulse near 60 degrees on 3 x 3 points with T2 twice its duration; the target is its own end point at gain 1,
    perturbed; weights with zeros, none on mx at all"""
    rng = np.random.default_rng(seed)
    dur, gamma = 2e-3, ref.GAMMA_H1
    b1 = (np.hanning(N + 2)[1:-1] + 0.1 * rng.standard_normal(N)) * (np.pi / 3 / (gamma * dur / N * np.hanning(N + 2).sum())) + 0j
    p = (b1, rng.uniform(0.5, 1.5, N) * 0.05, dur / N, 1.0, 2 * dur, "H-1")
    df, dp = ref._grid(3, 100.0), ref._grid(3, 2.0)
    m = ref.forward(*p[:5], df, dp, gamma, 1.0)
    t = (0.0, m[1] * (1 + 0.2 * rng.standard_normal((3, 3))), np.stack([m[2] + 0.1 * rng.standard_normal((3, 3)) for _ in RSC]))
    w = np.ones((3, 3))
    w[1, 1] = 0.0
    return p, df, dp, t, (0.0, w, np.stack([w] * 3))


def test_first_step_is_the_dense_levenberg_marquardt_step(on_reference):
    """cg = 2 (2n) iterations at a fixed mu = 1e-2 trace(H) / 2n and rtol = 1e-16: the step that is tried first is the dense
    solution of (H + mu I) d = -g within 1e-4 of max|d|"""
    p, df, dp, t, w = _problem(1)
    H = _dense_h(p, df, dp, w, RSC, None)
    _, g = ref.lsq(p, df, dp, t, w, RSC)
    mu = 1e-2 * np.trace(H) / (2 * N)
    d = np.linalg.solve(H + mu * np.eye(2 * N), -_realform(g))
    mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=1, cg=2 * 2 * N, mu0=mu, rtol=1e-16)
    trial = [c for c in on_reference if c[0] == "lsq"][1][1][0]                  # the second lsq call tries b1 + d
    err = np.abs(_realform(trial - p[0]) - d).max() / np.abs(d).max()
    print("first step against the dense solve %.3g (condition number %.0f)" % (err, np.linalg.cond(H + mu * np.eye(2 * N))))
    assert err <= 1e-4


def test_accepted_losses_strictly_decrease(on_reference):
    p, df, dp, t, w = _problem(2)
    (out,), (info,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=4)
    L = info["losses"]
    assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:]))
    assert L[0] == ref.lsq(p, df, dp, t, w, RSC)[0] and L[-1] == ref.lsq((out,) + p[1:], df, dp, t, w, RSC)[0]
    assert info["calls"]["lsq"] == 1 + (len(L) - 1) + info["refused"]
    assert info["calls"]["gn"] == sum(1 for c in on_reference if c[0] == "gn")
    assert info["status"] in ("iters", "converged", "gave_up")
    assert out.shape == (N,) and out.dtype == np.complex128


def test_a_refused_step_changes_only_mu(on_reference, monkeypatch):
    """The first trial step is refused by force (its loss reported as infinite): the run then continues as the run that started
    from four times the mu, from the same b1 and gradient."""
    p, df, dp, t, w = _problem(3)
    mu = 0.05 * np.trace(_dense_h(p, df, dp, w, RSC, None)) / (2 * N)
    (want,), (winfo,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=2, mu0=4 * mu)
    honest, count = mbfir.bloch_lsq_batch, [0]

    def refusing(*a, **k):
        count[0] += 1
        res = honest(*a, **k)
        return [(np.inf, g) for _, g in res] if count[0] == 2 else res

    monkeypatch.setattr(mbfir, "bloch_lsq_batch", refusing)
    del on_reference[:]
    (got,), (ginfo,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=2, mu0=mu)
    assert ginfo["refused"] == winfo["refused"] + 1
    assert ginfo["losses"] == winfo["losses"] and ginfo["mu"] == winfo["mu"]
    assert np.array_equal(got, want)
    second = [k for k, c in enumerate(on_reference) if c[0] == "lsq"][1]
    gn_after = on_reference[second + 1]
    assert gn_after[0] == "gn" and np.array_equal(gn_after[1][0], p[0])          # the next CG runs at the unchanged b1


def test_a_pulse_in_a_batch_has_the_bits_of_the_pulse_alone(on_reference):
    probs = [_problem(s) for s in (4, 5, 6)]
    df, dp = probs[0][1], probs[0][2]
    kw = dict(scales=RSC, iters=3, cg=4)
    alone = [mbfir.refine_bloch_batch([p[0]], df, dp, [p[3]], [p[4]], **kw) for p in probs]
    for order in ((0, 1, 2), (2, 1, 0)):
        b1s, infos = mbfir.refine_bloch_batch([probs[q][0] for q in order], df, dp, [probs[q][3] for q in order],
                                              [probs[q][4] for q in order], **kw)
        for k, q in enumerate(order):
            assert np.array_equal(b1s[k], alone[q][0][0])
            assert infos[k] == alone[q][1][0]


# ---- refine_batch keeps its bits: the loop it now shares with refine_bloch_batch -------------------------------------------------
def _abr_stubs(monkeypatch):
    """abr_lsq_batch / abr_gn_batch replaced by a model made of sums and products alone, f_i = u_i + 0.3 u_i^2 with u = C rf and
    C_ij = ((1 + i + 2 j) + (i - j) i / 2) / 8, so that the recorded values below do not depend on a libm"""
    def parts(rf, x):
        C = np.array([[((1 + i + 2 * j) + 0.5j * (i - j)) / 8 for j in range(len(rf))] for i in range(len(x))])
        u = np.array([sum(C[i, j] * rf[j] for j in range(len(rf))) for i in range(len(x))])
        return C, u

    def adj(C, u, c):
        return np.array([sum(np.conj(C[i, j] * (1 + 0.6 * u[i])) * c[i] for i in range(len(u))) for j in range(C.shape[1])])

    def lsq(pulses, x, targets, weights, **kw):
        out = []
        for rf, t, w in zip(pulses, targets, weights):
            C, u = parts(rf, x)
            r = u + 0.3 * u * u - t[0]
            out.append((float(sum(0.5 * w[i] * (r[i].real * r[i].real + r[i].imag * r[i].imag) for i in range(len(x)))), adj(C, u, w * r)))
        return out

    def gn(pulses, x, tangents, weights, **kw):
        out = []
        for rf, v, w in zip(pulses, tangents, weights):
            C, u = parts(rf, x)
            jv = np.array([(1 + 0.6 * u[i]) * sum(C[i, j] * v[j] for j in range(len(rf))) for i in range(len(x))])
            out.append(adj(C, u, w * jv))
        return out
    monkeypatch.setattr(mbfir, "abr_lsq_batch", lsq)
    monkeypatch.setattr(mbfir, "abr_gn_batch", gn)


# what the parent commit's refine_batch returned for _abr_scenario on the stubs above (float.hex)
RECORDED = dict(
    rf=[['-0x1.090a21e4be936p+0', '-0x1.0fdac79ff0eeap+0', '0x1.4aa49526e5b34p-3', '0x1.e507d9d354b61p-1', '0x1.725864e7f2ec8p-2',
         '0x1.12af695a24c51p-2', '0x1.33066dcc56a24p-2', '-0x1.2ca28dc17784dp-2'],
        ['-0x1.4af177d5e9bb7p-2', '-0x1.8c412e7c0c3e1p-4', '0x1.0268704bf1cefp-1', '-0x1.269be6626b6c7p-3', '-0x1.4e1fd88e9dc85p-4',
         '0x1.df1d4dd16c667p-3', '0x1.952a1fa89eba3p-5', '-0x1.14883dfd1d05ep-3']],
    losses=[['0x1.1e80eb46e9999p-1', '0x1.7d83a55e6a038p-4', '0x1.47f6b03c9f7a8p-4', '0x1.47ea682432e22p-4'],
            ['0x1.b7233165c28f6p-5', '0x1.ce015ee4ba12bp-6', '0x1.cc85e32cb5f82p-6', '0x1.cc84e44b69a5ap-6']],
    rest=[('0x1.869c087feec54p-12', 'iters', 0, {'gn': 7, 'lsq': 4}), ('0x1.2b1b8fb1c4b5bp-11', 'iters', 0, {'gn': 7, 'lsq': 4})])


def _abr_scenario():
    x = np.array([-1.0, -0.5, 0.25, 0.75, 1.5, 2.0])
    rfs = [np.array([0.25, -0.5 + 0.125j, 0.375j, 0.0625]), np.array([-0.125, 0.25j, 0.5, -0.25 - 0.25j])]
    tg = [np.array([[0.5, -0.25j, 0.125, 0.0, 0.25 + 0.25j, -0.5]]), np.array([[0.0, 0.25, -0.125j, 0.5, 0.0, 0.125]])]
    ws = [np.array([1.0, 0.5, 0.0, 1.0, 0.25, 1.0]), np.array([0.5, 1.0, 1.0, 0.0, 1.0, 0.75])]
    return mbfir.refine_batch(rfs, x, tg, ws, iters=3, cg=5)


def test_refine_batch_has_the_bits_it_had_before_the_loop_was_shared(monkeypatch):
    _abr_stubs(monkeypatch)
    rfs, infos = _abr_scenario()
    got = [[float(v).hex() for v in _realform(rf)] for rf in rfs]
    losses = [[float(v).hex() for v in i["losses"]] for i in infos]
    rest = [(float(i["mu"]).hex(), i["status"], i["refused"], i["calls"]) for i in infos]
    print(dict(rf=got, losses=losses, rest=rest))
    assert dict(rf=got, losses=losses, rest=rest) == RECORDED
