"""The NumPy reference of the Bloch simulator's adjoint (tests/blochgrad_ref.py, no GPU): its forward against oracle.bloch.blochsimfz
on the cases of tests/test_blochgrad_gpu.py, its float64 adjoint against its long-double one on the same cases, its adjoint against
central differences of its own forward, and the binding, the argument errors and the torch plumbing of mbfir.bloch_vjp_batch /
mbfir.torchsim.bloch, none of which needs a device."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir
from oracle import bloch as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochgrad_ref", os.path.join(ROOT, "tests", "blochgrad_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


@functools.lru_cache(maxsize=None)
def _batch(shared):
    return ref.batch(shared)


@pytest.mark.parametrize("shared", [False, True])
def test_reference_forward_is_the_oracle(shared):
    """blochsimfz forms rotz in another order of the same products; 1e-13 absolute on |m| <= 1 (measured 1.5e-15)"""
    pulses, dfs, dps, m0s, _ = _batch(shared)
    worst = 0.0
    for (b1, gr, tp, t1, t2, nucleus), df, dp, m0 in zip(pulses, dfs, dps, m0s):
        gamma = ref.gamma_of(nucleus)
        pos = np.concatenate([dp, np.zeros((dp.shape[0], 3 - dp.shape[1]))], 1)
        for s in ref.SCALES:
            got = ref.forward(b1, gr, tp, t1, t2, df, dp, gamma, s, m0)
            want = ob.blochsimfz(b1 * s, gr, tp, t1, t2, df, pos, 0, np.stack(m0, -1), gamma=gamma)[:, :, 0, :]
            worst = max(worst, max(float(np.abs(got[c] - want[..., c]).max()) for c in range(3)))
    print("shared %s: reference forward against oracle.bloch.blochsimfz %.3g" % (shared, worst))
    assert worst <= 1e-13


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_adjoint_is_the_longdouble_one_to_a_hundredth_of_the_device_bound(shared):
    pulses, dfs, dps, m0s, cots = _batch(shared)
    for q, (p, df, dp, m0, cot) in enumerate(zip(pulses, dfs, dps, m0s, cots)):
        g64, l64 = ref.vjp_scaled(p, df, dp, cot, ref.SCALES, m0)
        gld, lld = ref.vjp_scaled(p, df, dp, cot, ref.SCALES, m0, dtype=np.longdouble)
        eb = np.abs(g64 - gld).astype(np.float64)
        bb = ref.bound_b1(p, cot, ref.SCALES)
        em, bm = max(float(np.abs(a - b).max()) for a, b in zip(l64, lld)), ref.bound_m0(cot)
        print("shared %s n %d points %s: b1 |f64 - ld| / bound %.3g (|f64 - ld| %.3g), m0 |f64 - ld| %.3g bound %.3g"
              % (shared, len(p[0]), cot[0].shape[1:], (eb / bb).max(), eb.max(), em, bm))
        assert np.all(eb <= bb / 100) and em <= bm / 100, q


@pytest.mark.parametrize("t2", [40e-3, 1e-3])
def test_reference_adjoint_is_the_central_difference_of_its_forward(t2):
    """L = sum w . m_n over three scales; the directional derivative along g / |g| equals |g| to 1e-7 relative, in b1 and in m0"""
    rng = np.random.default_rng(3)
    n, dur, gamma = 64, 4e-3, ref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.5 / (gamma * dur))
    b1[n // 3] = 0.0
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.1
    df, dp = ref._grid(3, 200.0), np.stack([ref._grid(5, 2.0), ref._grid(5, 1.0)], 1)
    m0 = tuple(rng.uniform(-0.5, 0.5, (3, 3, 5)))
    sc = (0.9, 1.0, 1.1)
    w = rng.standard_normal((3, 3, 3, 5))
    pulse = (b1, gr, dur / n, 1.0, t2, "H-1")

    def L(b, m):
        return float(sum((w[c][k] * ref.forward(b, gr, dur / n, 1.0, t2, df, dp, gamma, s, m)[c]).sum()
                         for k, s in enumerate(sc) for c in range(3)))
    g, gm = ref.vjp_scaled(pulse, df, dp, tuple(w), sc, m0)
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, 1e-5 * float(np.linalg.norm(b1))
    fd = (L(b1 + eps * d, m0) - L(b1 - eps * d, m0)) / (2 * eps)
    gm = np.stack([v.sum(0) for v in gm])
    nm = float(np.linalg.norm(gm))
    fm = (L(b1, tuple(np.stack(m0) + 1e-4 * gm / nm)) - L(b1, tuple(np.stack(m0) - 1e-4 * gm / nm))) / 2e-4
    print("T2 %.0e: |g| %.9g central difference %.9g relative %.3g; m0 |g| %.9g central difference %.9g relative %.3g"
          % (t2, nrm, fd, abs(fd - nrm) / nrm, nm, fm, abs(fm - nm) / nm))
    assert abs(fd - nrm) <= 1e-7 * nrm and abs(fm - nm) <= 1e-7 * nm


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_bloch_vjp_batch\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_bloch_vjp_batch"][1]) == 34
    assert getattr(mbfir.load_library(), "mbfir_bloch_vjp_batch") is not None           # the library exports it
    assert callable(mbfir.bloch_vjp_batch) and callable(mbfir.torchsim.bloch)


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    c = np.zeros((1, 3, 5))
    with pytest.raises(ValueError, match="bloch_vjp_batch: no pulses"):
        mbfir.bloch_vjp_batch([], df, dp, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.bloch_vjp_batch([p], df, dp, [(c, c, c)], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.bloch_vjp_batch([p, (np.zeros(0),) + p[1:]], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="2 cotangent triples for 1 pulses"):
        mbfir.bloch_vjp_batch([p], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="triple"):
        mbfir.bloch_vjp_batch([p], df, dp, [(c, c)])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.bloch_vjp_batch([p], df, dp, [(c, c, c[:, :, :4])])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.bloch_vjp_batch([p], df, dp, [(c, c, c)], scales=(1.0, 0.9))
    with pytest.raises(ValueError, match="empty grid"):
        mbfir.bloch_vjp_batch([p], np.zeros(0), dp, [(c, c, c)])
    # the C call refuses a null context before it reads anything else (the checks that need a context: tests/test_blochgrad_gpu.py)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS["mbfir_bloch_vjp_batch"][1][1:]]
    assert mbfir.load_library().mbfir_bloch_vjp_batch(*args) == mbfir.E_ARG


def _stub_device_calls(monkeypatch):
    """mbfir's two Bloch calls replaced by the NumPy reference, so that torchsim's plumbing runs without a device"""
    def bloch_batch(pulses, df, dp, *, scales, m0):
        b1, gr, tp, t1, t2, nucleus = pulses[0]
        out = [ref.forward(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nucleus), s, m0) for s in scales]
        return [tuple(np.stack([o[c] for o in out]) for c in range(3))]

    def bloch_vjp_batch(pulses, df, dp, cot, *, scales, m0, grad_m0):
        g, gm = ref.vjp_scaled(pulses[0], df, dp, cot[0], scales, m0)
        return [(g, gm) if grad_m0 else g]
    monkeypatch.setattr(mbfir, "bloch_batch", bloch_batch)
    monkeypatch.setattr(mbfir, "bloch_vjp_batch", bloch_vjp_batch)


def test_torchsim_bloch_passes_gradcheck_on_stubbed_calls(monkeypatch):
    """gradcheck in b1, in m0 and in both on 6 samples and 2 x 3 points with T2 of the order of the duration; a backward that needs
    only b1 does not ask for dL/dm0; a forward-mode tangent raises NotImplementedError."""
    import torch
    _stub_device_calls(monkeypatch)
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 6) * 0.05
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    sc = (1.0, 0.8)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 2, 3)), dtype=torch.float64, requires_grad=True)

    def f(b, m):
        return mbfir.torchsim.bloch(b, gr, dt, 1.0, 1e-3, df, dp, nucleus="H-1", scales=sc, m0=m)
    assert torch.autograd.gradcheck(lambda b: f(b, None), (b1,))
    assert torch.autograd.gradcheck(lambda m: f(b1.detach(), m), (m0,))
    assert torch.autograd.gradcheck(f, (b1, m0))
    mx, my, mz = f(b1, m0.detach())
    assert mx.dtype == torch.float64 and tuple(mx.shape) == (2, 2, 3)
    asked = []
    inner = mbfir.bloch_vjp_batch
    monkeypatch.setattr(mbfir, "bloch_vjp_batch", lambda *a, **k: asked.append(k["grad_m0"]) or inner(*a, **k))
    (mx * my + mz).sum().backward()
    assert asked == [False] and b1.grad is not None
    with pytest.raises(ValueError, match="complex128"):
        mbfir.torchsim.bloch(torch.ones(6), gr, dt, 1.0, 1e-3, df, dp)
    with pytest.raises(ValueError, match="shape"):
        mbfir.torchsim.bloch(b1, gr, dt, 1.0, 1e-3, df, dp, m0=torch.zeros(3, 6, dtype=torch.float64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: f(b, None), (b1.detach(),), (torch.ones_like(b1),))
