"""The NumPy reference of the Bloch simulator's steady state and of its adjoint and tangent in b1 (tests/blochss_ref.py, no GPU): its
M against the oracle's mode 1, its float64 results against its long-double ones on the cases of tests/test_blochss_gpu.py, against
central differences of its own forward and against each other through the dot-product identity, the cap on kappa, and the binding,
the argument errors and the torch plumbing of mbfir.bloch_ss_vjp_batch / mbfir.bloch_ss_jvp_batch /
mbfir.torchsim.bloch(steady_state=True), none of which needs a device."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir
from oracle import bloch as obloch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochss_ref", os.path.join(ROOT, "tests", "blochss_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
K = 2


@functools.lru_cache(maxsize=None)
def _case(shared):
    """The cases with two directions per pulse, their kappa and their float64 gradient, M and tangents"""
    pulses, dfs, dps, cots = ref.batch(shared)
    vs, _ = ref.directions(pulses, dfs, dps, K)
    ks = [ref.kappa(p, df, dp, ref.SCALES) for p, df, dp in zip(pulses, dfs, dps)]
    adj = [ref.ss_vjp_scaled(p, df, dp, c, ref.SCALES) for p, df, dp, c in zip(pulses, dfs, dps, cots)]
    tan = [ref.ss_jvp(p, df, dp, v, ref.SCALES) for p, df, dp, v in zip(pulses, dfs, dps, vs)]
    return pulses, dfs, dps, cots, vs, ks, adj, tan


def _pos3(dp):
    dp = np.asarray(dp, dtype=np.float64)
    dp = dp.reshape(-1, 1) if dp.ndim < 2 else dp
    return np.concatenate([dp, np.zeros((dp.shape[0], 3 - dp.shape[1]))], 1)


def test_kappa_spans_the_range_and_stays_under_the_cap():
    for shared in (False, True):
        ks = _case(shared)[5]
        print("shared %s: kappa %s" % (shared, " ".join("%.4g" % k for k in ks)))
        assert min(ks) < 10 and max(ks) > 2000 and max(ks) <= ref.KAPPA_CAP


def test_reference_steady_state_is_the_oracles_mode_1():
    """blochsimfz(mode=1) at scales 1.0 and 0.9 on the per-pulse grids, within 1e-13 kappa"""
    pulses, dfs, dps, _, _, ks, adj, _ = _case(False)
    for q, ((b1, gr, tp, t1, t2, nucleus), df, dp, k, (_, M)) in enumerate(zip(pulses, dfs, dps, ks, adj)):
        n = len(b1)
        g3 = np.concatenate([gr.reshape(n, -1), np.zeros((n, 3 - gr.reshape(n, -1).shape[1]))], 1)
        for si, s in enumerate(ref.SCALES):
            want = obloch.blochsimfz(b1 * s, g3, np.broadcast_to(tp, (n,)), t1, t2, df, _pos3(dp), mode=1, gamma=ref.gamma_of(nucleus))
            err = max(float(np.abs(M[c][si] - want[:, :, 0, c]).max()) for c in range(3))
            print("n %d scale %g: |ref - oracle| %.3g, 1e-13 kappa %.3g" % (n, s, err, 1e-13 * k))
            assert err <= 1e-13 * k, (q, s)


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_is_the_longdouble_one_to_a_hundredth_of_each_bound(shared):
    """Measured worst shares: M 6.4e-5, gradient 1.9e-3, tangent 5.9e-5 (of 1e-12 kappa^2, bound_b1 kappa, bound_jvp kappa^2); with the
    first power of kappa M reaches 1.8e-2 and the tangent 1.1e-1 on the 600-sample period (tests/blochss_ref.py)"""
    pulses, dfs, dps, cots, vs, ks, adj, tan = _case(shared)
    for q, (p, df, dp, c, v, k, (g64, M64), (_, d64)) in enumerate(zip(pulses, dfs, dps, cots, vs, ks, adj, tan)):
        gl, Ml = ref.ss_vjp_scaled(p, df, dp, c, ref.SCALES, np.longdouble)
        _, dl = ref.ss_jvp(p, df, dp, v, ref.SCALES, np.longdouble)
        sm = max(float(np.abs(a - b).max()) for a, b in zip(M64, Ml)) / ref.bound_m(k)
        sg = float((np.abs(g64 - gl).astype(np.float64) / ref.bound_b1(p, c, ref.SCALES, k)).max())
        bj = ref.bound_jvp(p, v, ref.SCALES, k)[:, None]
        sj = max(float((np.abs(a - b).astype(np.float64) / bj).max()) for a, b in zip(d64, dl))
        print("shared %s n %d points %s kappa %.4g: |f64 - ld| / bound: M %.3g, gradient %.3g, tangent %.3g"
              % (shared, len(p[0]), M64[0].shape[1:], k, sm, sg, sj))
        assert sm <= 0.01 and sg <= 0.01 and sj <= 0.01, q


def _fd_problem():
    """64 samples of 10 us and a dead time of 160 us (a period of 0.8 ms) at T1 = 0.1 s, T2 = 0.03 s on 5 x 7 points: kappa = 119.
    The dead-time sample's entry dominates the gradient (its gamma dt is 16 times the others'), and the central difference's
    truncation grows with the cube of that: 3.3e-8 here, 1e-6 with a dead time of 2.56 ms (and a hundredth of that at a tenth of
    the step)."""
    rng = np.random.default_rng(7)
    n, gamma = 65, ref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 / (gamma * 64e-5))
    b1[20], b1[-1] = 0.0, 0.0
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.1
    gr[-1] = 0.0
    tp = np.full(n, 1e-5)
    tp[-1] = 1.6e-4
    pulse = (b1, gr, tp, 0.1, 0.03, "H-1")
    df, dp = ref._grid(5, 150.0), np.stack([ref._grid(7, 2.0), ref._grid(7, 1.0)], 1)
    return pulse, df, dp, rng


def test_adjoint_and_tangent_are_the_central_differences_of_the_reference_forward():
    """L = 1/2 sum (w . M)^2 at scales 0.9, 1.0, 1.1: the derivative along g / |g| against a central difference with step 1e-5 |b1|,
    and the tangent along a direction of the pulse's size against the central difference of the long-double M (h = 1e-7; in float64 rounding and truncation meet at 2e-7 near h = 1e-6), both to 1e-7
    relative"""
    pulse, df, dp, rng = _fd_problem()
    sc = (0.9, 1.0, 1.1)
    k = ref.kappa(pulse, df, dp, sc)
    assert k <= 300
    w = rng.standard_normal((3, 3, 5, 7))

    def fwd(b):
        return ref.ss_scaled((b,) + pulse[1:], df, dp, sc)

    def loss(b):
        M = fwd(b)
        r = w[0] * M[0] + w[1] * M[1] + w[2] * M[2]
        return 0.5 * float((r * r).sum()), tuple(w[c] * r for c in range(3))
    _, cot = loss(pulse[0])
    g, _ = ref.ss_vjp_scaled(pulse, df, dp, cot, sc)
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, 1e-5 * float(np.linalg.norm(pulse[0]))
    fd = (loss(pulse[0] + eps * d)[0] - loss(pulse[0] - eps * d)[0]) / (2 * eps)
    print("kappa %.4g: |g| %.9g, central difference %.9g, relative difference %.3g" % (k, nrm, fd, abs(fd - nrm) / nrm))
    assert abs(fd - nrm) <= 1e-7 * nrm
    v = (rng.standard_normal(65) + 1j * rng.standard_normal(65)) * np.abs(pulse[0]).max()
    _, tan = ref.ss_jvp(pulse, df, dp, v, sc)
    tan, h = np.stack([t[0] for t in tan]), 1e-7
    ld = lambda b: np.stack(ref.ss_scaled((b,) + pulse[1:], df, dp, sc, np.longdouble))
    fdm = ((ld(pulse[0] + h * v) - ld(pulse[0] - h * v)) / (2 * h)).astype(np.float64)
    rel = float(np.abs(fdm - tan).max() / np.abs(tan).max())
    print("max|tangent| %.6g, |central difference - tangent| / max|tangent| %.3g" % (np.abs(tan).max(), rel))
    assert rel <= 1e-7


@pytest.mark.parametrize("shared", [False, True])
def test_tangent_and_adjoint_satisfy_the_dot_product_identity(shared):
    """<c, J v> = <J' c, v> to 1e-10 of the sum of the absolute terms of either side"""
    pulses, _, _, cots, vs, _, adj, tan = _case(shared)
    for q, (p, c, v, (g, _), (_, dM)) in enumerate(zip(pulses, cots, vs, adj, tan)):
        for k in range(K):
            lt = np.concatenate([(c[i] * dM[i][k]).ravel() for i in range(3)])
            rt = (np.conj(g) * v[k]).real
            lhs, rhs, size = float(lt.sum()), float(rt.sum()), max(float(np.abs(lt).sum()), float(np.abs(rt).sum()))
            print("shared %s n %d direction %d: lhs %.9g rhs %.9g |lhs - rhs| / size %.3g" % (shared, len(p[0]), k, lhs, rhs, abs(lhs - rhs) / size))
            assert abs(lhs - rhs) <= 1e-10 * size, (q, k)


def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for name in ("mbfir_bloch_ss_vjp_batch", "mbfir_bloch_ss_jvp_batch", "mbfir_test_bloch_ss_jvp_group"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(mbfir.load_library(), name) is not None                          # the library exports it
    assert len(mbfir.SYMBOLS["mbfir_bloch_ss_vjp_batch"][1]) == 31
    assert len(mbfir.SYMBOLS["mbfir_bloch_ss_jvp_batch"][1]) == 32
    assert mbfir.bloch_ss_jvp_group() in (4, 8)
    assert callable(mbfir.bloch_ss_vjp_batch) and callable(mbfir.bloch_ss_jvp_batch)


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    v, c = np.ones(4, dtype=complex), np.zeros((1, 3, 5))
    for who, call, arg in (("bloch_ss_vjp_batch", mbfir.bloch_ss_vjp_batch, (c, c, c)), ("bloch_ss_jvp_batch", mbfir.bloch_ss_jvp_batch, v)):
        with pytest.raises(ValueError, match=who + ": no pulses"):
            call([], df, dp, [])
        with pytest.raises(ValueError, match="scale list is empty"):
            call([p], df, dp, [arg], scales=())
        with pytest.raises(ValueError, match="pulse 1 has no samples"):
            call([p, (np.zeros(0),) + p[1:]], df, dp, [arg, arg])
        with pytest.raises(ValueError, match="empty grid"):
            call([p], np.zeros(0), dp, [arg])
    with pytest.raises(ValueError, match="2 cotangent triples for 1 pulses"):
        mbfir.bloch_ss_vjp_batch([p], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="triple"):
        mbfir.bloch_ss_vjp_batch([p], df, dp, [(c, c)])
    with pytest.raises(ValueError, match="have shapes"):
        mbfir.bloch_ss_vjp_batch([p], df, dp, [(c, c, c[:, :2])])
    with pytest.raises(ValueError, match="have shapes"):                                   # one scale's cotangents for two scales
        mbfir.bloch_ss_vjp_batch([p], df, dp, [(c, c, c)], scales=(1.0, 0.9))
    with pytest.raises(ValueError, match="2 tangents for 1 pulses"):
        mbfir.bloch_ss_jvp_batch([p], df, dp, [v, v])
    with pytest.raises(ValueError, match="has shape"):
        mbfir.bloch_ss_jvp_batch([p], df, dp, [v[:3]])
    with pytest.raises(ValueError, match="every pulse takes the same K"):
        mbfir.bloch_ss_jvp_batch([p, p], df, dp, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)])
    with pytest.raises(TypeError):                                                        # no m0: the steady state does not depend on it
        mbfir.bloch_ss_vjp_batch([p], df, dp, [(c, c, c)], m0=None)
    # the C calls refuse a null context before they read anything else (the checks that need a context: tests/test_blochss_gpu.py)
    for name in ("mbfir_bloch_ss_vjp_batch", "mbfir_bloch_ss_jvp_batch"):
        args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
        assert getattr(mbfir.load_library(), name)(*args) == mbfir.E_ARG


def _stub_device_calls(monkeypatch):
    """mbfir's Bloch calls replaced by the NumPy references, so that torchsim's plumbing runs without a device"""
    def bloch_batch(pulses, df, dp, *, scales, mode=0, m0=None):
        if mode == 1:
            return [ref.ss_scaled(pulses[0], df, dp, scales)]
        b1, gr, tp, t1, t2, nucleus = pulses[0]
        out = [ref.forward(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nucleus), s, m0) for s in scales]
        return [tuple(np.stack([o[c] for o in out]) for c in range(3))]

    def bloch_ss_vjp_batch(pulses, df, dp, cot, *, scales):
        return [ref.ss_vjp_scaled(pulses[0], df, dp, cot[0], scales)[0]]

    def bloch_ss_jvp_batch(pulses, df, dp, tangents, *, scales):
        assert np.ndim(tangents[0]) == 1                                                  # one direction, without the K axis
        M, tan = ref.ss_jvp(pulses[0], df, dp, tangents[0], scales)
        return [(M, tuple(t[0] for t in tan))]
    monkeypatch.setattr(mbfir, "bloch_batch", bloch_batch)
    monkeypatch.setattr(mbfir, "bloch_ss_vjp_batch", bloch_ss_vjp_batch, raising=False)
    monkeypatch.setattr(mbfir, "bloch_ss_jvp_batch", bloch_ss_jvp_batch, raising=False)


def test_torchsim_bloch_steady_state_on_stubbed_calls(monkeypatch):
    """gradcheck in b1, reverse and forward mode, on 6 samples plus a dead time and 2 x 3 points; torch.func.jvp equals the
    reference; an m0 raises ValueError; without forward_mode a tangent raises NotImplementedError; the default path is the
    transient end point, unchanged."""
    import torch
    _stub_device_calls(monkeypatch)
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(7) + 1j * rng.standard_normal(7)) * (0.5 / (gamma * dt))
    b0[-1] = 0.0
    gr = np.append(rng.uniform(0.5, 1.5, 6) * 0.05, 0.0)
    tp = np.append(np.full(6, dt), 2e-3)
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    sc = (1.0, 0.8)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)

    def f(b, forward_mode=True, **kw):
        return mbfir.torchsim.bloch(b, gr, tp, 0.1, 0.02, df, dp, nucleus="H-1", scales=sc, forward_mode=forward_mode,
                                    steady_state=True, **kw)
    assert torch.autograd.gradcheck(lambda b: f(b, False), (b1,))
    assert torch.autograd.gradcheck(f, (b1,), check_forward_ad=True)
    pulse = (b0, gr, tp, 0.1, 0.02, "H-1")
    v = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    out, tan = torch.func.jvp(f, (b1.detach(),), (torch.tensor(v),))
    wm, wt = ref.ss_jvp(pulse, df, dp, v, sc)
    assert tan[0].dtype == torch.float64 and tuple(tan[0].shape) == (2, 2, 3)
    assert all(np.array_equal(o.numpy(), w) for o, w in zip(out, wm))
    assert all(np.array_equal(t.numpy(), w[0]) for t, w in zip(tan, wt))
    with pytest.raises(ValueError, match="does not depend on m0"):
        f(b1, m0=(0.0, 0.0, 1.0))
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: f(b, False), (b1.detach(),), (torch.ones_like(b1),))
    got = mbfir.torchsim.bloch(b1.detach(), gr, tp, 0.1, 0.02, df, dp, nucleus="H-1", scales=sc)
    want = [ref.forward(b0, gr, tp, 0.1, 0.02, df, dp, gamma, s) for s in sc]
    assert all(np.array_equal(got[c].numpy(), np.stack([w[c] for w in want])) for c in range(3))
    assert not any(np.array_equal(got[c].numpy(), wm[c]) for c in range(3))              # and it is not the steady state
