"""The NumPy reference of the Bloch simulator's tangent (tests/blochjvp_ref.py, no GPU): its primal against blochgrad_ref.forward,
its float64 tangent against its long-double one on the cases of tests/test_blochjvp_gpu.py, against central differences of the
forward and against the adjoint through the dot-product identity, and the binding, the argument errors and the torch plumbing of
mbfir.bloch_jvp_batch / mbfir.torchsim.bloch(forward_mode=True), none of which needs a device."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochjvp_ref", os.path.join(ROOT, "tests", "blochjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
K = 2


@functools.lru_cache(maxsize=None)
def _case(shared):
    """The cases with two directions per pulse and their float64 tangents"""
    pulses, dfs, dps, m0s, cots, vs, dms = ref.cases(shared, K)
    got = [ref.jvp_scaled(p, df, dp, v, ref.SCALES, m0, dm) for p, df, dp, m0, v, dm in zip(pulses, dfs, dps, m0s, vs, dms)]
    return pulses, dfs, dps, m0s, cots, vs, dms, got


@pytest.mark.parametrize("shared", [False, True])
def test_reference_primal_has_the_bits_of_the_adjoint_reference_forward(shared):
    pulses, dfs, dps, m0s, _, _, _, got = _case(shared)
    for q, ((b1, gr, tp, t1, t2, nucleus), df, dp, m0, (m, _)) in enumerate(zip(pulses, dfs, dps, m0s, got)):
        for k, s in enumerate(ref.SCALES):
            want = ref.forward(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nucleus), s, m0)
            assert all(np.array_equal(m[c][k], want[c]) for c in range(3)), (q, s)


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_tangent_is_the_longdouble_one_to_a_twentieth_of_the_device_bound(shared):
    """Measured worst 6.4e-3 of the bound (600 samples, 26 ms at T2 = 1 ms, on 3 x 200 points)"""
    pulses, dfs, dps, m0s, _, vs, dms, got = _case(shared)
    for q, (p, df, dp, m0, v, dm, (_, d64)) in enumerate(zip(pulses, dfs, dps, m0s, vs, dms, got)):
        _, dld = ref.jvp_scaled(p, df, dp, v, ref.SCALES, m0, dm, dtype=np.longdouble)
        bound = ref.bound_jvp(p, v, dm, ref.SCALES)[:, None]
        err = np.max([np.abs(a - b).astype(np.float64) for a, b in zip(d64, dld)], 0)
        print("shared %s n %d points %s: |f64 - ld| %.3g, bound %.3g, max |f64 - ld| / bound %.3g"
              % (shared, len(p[0]), d64[0].shape[2:], err.max(), bound.min(), (err / bound).max()))
        assert np.all(err <= bound / 20), q


@pytest.mark.parametrize("t2", [40e-3, 1e-3])
def test_reference_tangent_is_the_central_difference_of_the_forward(t2):
    """64 samples on 3 x 5 points at three scales: along a b1 direction of the pulse's size (h = 1e-6: truncation h^2, rounding
    eps / h) and along an m0 direction, in which the forward is affine; 1e-7 of the largest tangent entry"""
    rng = np.random.default_rng(3)
    n, dur, gamma = 64, 4e-3, ref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.5 / (gamma * dur))
    b1[n // 3] = 0.0
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.1
    df, dp = ref._grid(3, 200.0), np.stack([ref._grid(5, 2.0), ref._grid(5, 1.0)], 1)
    m0 = rng.uniform(-0.5, 0.5, (3, 3, 5))
    v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(b1).max()
    dm0 = rng.standard_normal((3, 3, 5))
    pulse, h = (b1, gr, dur / n, 1.0, t2, "H-1"), 1e-6

    def fwd(b, m):
        out = [ref.forward(b, gr, dur / n, 1.0, t2, df, dp, gamma, s, tuple(m)) for s in (0.9, 1.0, 1.1)]
        return np.stack([np.stack([o[c] for o in out]) for c in range(3)])
    for name, vv, dd in (("b1", v, None), ("m0", np.zeros(n), tuple(dm0[:, None])), ("both", v, tuple(dm0[:, None]))):
        _, tan = ref.jvp_scaled(pulse, df, dp, vv, (0.9, 1.0, 1.1), tuple(m0), dd)
        tan = np.stack([t[0] for t in tan])
        hm = 0 if dd is None else h * dm0
        fd = (fwd(b1 + h * vv, m0 + hm) - fwd(b1 - h * vv, m0 - hm)) / (2 * h)
        rel = float(np.abs(fd - tan).max() / np.abs(tan).max())
        print("T2 %.0e, %s: max|tangent| %.6g, |central difference - tangent| / max|tangent| %.3g" % (t2, name, np.abs(tan).max(), rel))
        assert rel <= 1e-7


@pytest.mark.parametrize("shared", [False, True])
def test_tangent_and_adjoint_satisfy_the_dot_product_identity(shared):
    """sum cot . dm = Re sum conj(g) v + sum gm0 . dm_0 against blochgrad_ref.vjp, within the two sides' own bounds"""
    pulses, dfs, dps, m0s, cots, vs, dms, got = _case(shared)
    for q, (p, df, dp, m0, cot, v, dm, (_, tan)) in enumerate(zip(pulses, dfs, dps, m0s, cots, vs, dms, got)):
        g, gm = ref.vjp_scaled(p, df, dp, cot, ref.SCALES, m0)
        for k in range(K):
            d0 = tuple(d[k] for d in dm)
            lhs = float(sum((cot[c] * tan[c][k]).sum() for c in range(3)))
            rhs = float((np.conj(g) * v[k]).real.sum()) + float(sum((gm[c] * d0[c]).sum() for c in range(3)))
            tol = ref.identity_tol(p, cot, v[k], d0, ref.SCALES)
            print("shared %s n %d direction %d: lhs %.9g rhs %.9g |lhs - rhs| / tolerance %.3g" % (shared, len(p[0]), k, lhs, rhs, abs(lhs - rhs) / tol))
            assert abs(lhs - rhs) <= tol, (q, k)


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_bloch_jvp_batch\s*\(", hdr) and re.search(r"\bmbfir_test_bloch_jvp_group\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_bloch_jvp_batch"][1]) == 38
    assert getattr(mbfir.load_library(), "mbfir_bloch_jvp_batch") is not None            # the library exports it
    assert mbfir.bloch_jvp_group() in (1, 2, 4, 8)
    assert callable(mbfir.bloch_jvp_batch)


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    v, d = np.ones(4, dtype=complex), np.zeros((3, 5))
    with pytest.raises(ValueError, match="bloch_jvp_batch: no pulses"):
        mbfir.bloch_jvp_batch([], df, dp, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.bloch_jvp_batch([p], df, dp, [v], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.bloch_jvp_batch([p, (np.zeros(0),) + p[1:]], df, dp, [v, v])
    with pytest.raises(ValueError, match="empty grid"):
        mbfir.bloch_jvp_batch([p], np.zeros(0), dp, [v])
    with pytest.raises(ValueError, match="2 tangents for 1 pulses"):
        mbfir.bloch_jvp_batch([p], df, dp, [v, v])
    with pytest.raises(ValueError, match="has shape"):                                    # a wrong length
        mbfir.bloch_jvp_batch([p], df, dp, [v[:3]])
    with pytest.raises(ValueError, match="has shape"):
        mbfir.bloch_jvp_batch([p], df, dp, [np.ones((2, 5), dtype=complex)])
    with pytest.raises(ValueError, match="every pulse takes the same K"):                 # a ragged K
        mbfir.bloch_jvp_batch([p, p], df, dp, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)])
    with pytest.raises(ValueError, match="2 m0 tangent triples for 1 pulses"):
        mbfir.bloch_jvp_batch([p], df, dp, [v], tangents_m0=[(d, d, d)] * 2)
    with pytest.raises(ValueError, match="triple"):
        mbfir.bloch_jvp_batch([p], df, dp, [v], tangents_m0=[(d, d)])
    with pytest.raises(ValueError, match="does not broadcast"):
        mbfir.bloch_jvp_batch([p], df, dp, [v], tangents_m0=[(d, d, d[:, :4])])
    with pytest.raises(ValueError, match="does not broadcast"):                           # two m0 directions for one b1 direction
        mbfir.bloch_jvp_batch([p], df, dp, [v], tangents_m0=[(d, d, np.zeros((2, 3, 5)))])
    # the C call refuses a null context before it reads anything else (the checks that need a context: tests/test_blochjvp_gpu.py)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS["mbfir_bloch_jvp_batch"][1][1:]]
    assert mbfir.load_library().mbfir_bloch_jvp_batch(*args) == mbfir.E_ARG


def _stub_device_calls(monkeypatch):
    """mbfir's three Bloch calls replaced by the NumPy references, so that torchsim's plumbing runs without a device"""
    def bloch_batch(pulses, df, dp, *, scales, m0):
        b1, gr, tp, t1, t2, nucleus = pulses[0]
        out = [ref.forward(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nucleus), s, m0) for s in scales]
        return [tuple(np.stack([o[c] for o in out]) for c in range(3))]

    def bloch_vjp_batch(pulses, df, dp, cot, *, scales, m0, grad_m0):
        g, gm = ref.vjp_scaled(pulses[0], df, dp, cot[0], scales, m0)
        return [(g, gm) if grad_m0 else g]

    def bloch_jvp_batch(pulses, df, dp, tangents, *, scales, m0, tangents_m0):
        assert np.ndim(tangents[0]) == 1                                                  # one direction, without the K axis
        m, tan = ref.jvp_scaled(pulses[0], df, dp, tangents[0], scales, m0, None if tangents_m0 is None else tangents_m0[0])
        return [(m, tuple(t[0] for t in tan))]
    monkeypatch.setattr(mbfir, "bloch_batch", bloch_batch)
    monkeypatch.setattr(mbfir, "bloch_vjp_batch", bloch_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_jvp_batch", bloch_jvp_batch)


def test_torchsim_bloch_forward_mode_on_stubbed_calls(monkeypatch):
    """gradcheck with forward AD in b1, in m0 and in both on 6 samples and 2 x 3 points; torch.func.jvp equals the reference; the
    default function still raises NotImplementedError."""
    import torch
    _stub_device_calls(monkeypatch)
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 6) * 0.05
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    sc = (1.0, 0.8)
    m00 = rng.uniform(-0.5, 0.5, (3, 2, 3))
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(m00, dtype=torch.float64, requires_grad=True)

    def f(b, m, forward_mode=True):
        return mbfir.torchsim.bloch(b, gr, dt, 1.0, 1e-3, df, dp, nucleus="H-1", scales=sc, m0=m, forward_mode=forward_mode)
    assert torch.autograd.gradcheck(lambda b: f(b, None), (b1,), check_forward_ad=True)
    assert torch.autograd.gradcheck(lambda m: f(b1.detach(), m), (m0,), check_forward_ad=True)
    assert torch.autograd.gradcheck(f, (b1, m0), check_forward_ad=True)
    v, dm = rng.standard_normal(6) + 1j * rng.standard_normal(6), rng.standard_normal((3, 2, 3))
    out, tan = torch.func.jvp(f, (b1.detach(), m0.detach()), (torch.tensor(v), torch.tensor(dm)))
    wm, wt = ref.jvp_scaled((b0, gr, dt, 1.0, 1e-3, "H-1"), df, dp, v, sc, tuple(m00), tuple(dm))
    assert tan[0].dtype == torch.float64 and tuple(tan[0].shape) == (2, 2, 3)
    assert all(np.array_equal(o.numpy(), w) for o, w in zip(out, wm))
    assert all(np.array_equal(t.numpy(), w[0]) for t, w in zip(tan, wt))
    _, tb = torch.func.jvp(lambda b: f(b, torch.tensor(m00)), (b1.detach(),), (torch.tensor(v),))      # m0 a constant tensor
    wb = ref.jvp_scaled((b0, gr, dt, 1.0, 1e-3, "H-1"), df, dp, v, sc, tuple(m00))[1]
    assert all(np.array_equal(t.numpy(), w[0]) for t, w in zip(tb, wb))
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: f(b, None, forward_mode=False), (b1.detach(),), (torch.ones_like(b1),))
