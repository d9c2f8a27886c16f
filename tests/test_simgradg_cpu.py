"""The NumPy reference of the simulators' adjoint with respect to rf and the gradient waveform (tests/simgradg_ref.py, no GPU): its
g-gradient against central differences of simgrad_ref.forward, its rf part against simgrad_ref.vjp to the bit, the scale sweep, and
the bindings and argument errors that mbfir.abr_vjp_rfg_batch / abr2_vjp_rfg_batch and mbfir.torchsim raise before any device
work."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("simgrad_ref", "simgrad_ref.py")
refg = _load("simgradg_ref", "simgradg_ref.py")


def _pulse(seed, n, flip=np.pi / 2):
    rng = np.random.default_rng(seed)
    rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (flip / n)
    g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n + 1j * rng.uniform(-1.5, 1.5, n) * 1e-2
    return rf, g


def _loss(rf, g, x, y, hard, wa, wb):
    """A real loss whose cotangents are not constant: L = sum Re(conj(wa) a) + |b|^2 Re(wb)"""
    a, b = ref.forward(rf, g, x, y, hard_pulse=hard)
    return float((np.conj(wa) * a).real.sum() + (np.abs(b) ** 2 * wb.real).sum()), a, b


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("two_d", [False, True])
def test_g_adjoint_is_the_central_difference_of_the_forward(n, hard, two_d):
    """h = 1e-6 on each g_m (1D) or on each of Re g_m, Im g_m (2D); bound 1e-7 max(max |gbar|, 1) absolute (the O(h^2) truncation
    term and the rounding of the difference, about eps L / h).  x = 0 and y = 0 are on the grid and, for n > 1, one rf sample is
    exactly zero, so phi = 0 occurs.  The rf part is simgrad_ref.vjp to the bit."""
    rf, g = _pulse(10 + n, n, flip=2.0)
    if n > 1:
        rf[n // 2] = 0.0
    x = np.linspace(-3, 3, 7)
    assert x[3] == 0.0
    y = np.array([-20.0, 0.0, 15.0]) if two_d else None
    g0 = g if two_d else g.real
    rng = np.random.default_rng(99)
    shape = (7, 3) if two_d else (7,)
    wa = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    wb = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    _, a, b = _loss(rf, g0, x, y, hard, wa, wb)
    grad, gbar = refg.vjp_rfg(rf, g0, x, wa, 2 * wb.real * b, y, hard_pulse=hard)
    assert np.array_equal(grad, ref.vjp(rf, g0, x, wa, 2 * wb.real * b, y, hard_pulse=hard))
    assert gbar.shape == (n,) and gbar.dtype == (np.complex128 if two_d else np.float64)
    h = 1e-6
    fd = np.zeros(n, dtype=np.complex128)
    idx = range(n) if n <= 7 else sorted({0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1} | set(range(3, n, 37)))
    for m in idx:
        for d in (1.0, 1j) if two_d else (1.0,):
            e = np.zeros(n, dtype=np.complex128 if two_d else np.float64)
            e[m] = h * d
            fd[m] += d * (_loss(rf, g0 + e, x, y, hard, wa, wb)[0] - _loss(rf, g0 - e, x, y, hard, wa, wb)[0]) / (2 * h)
    sel = np.array(list(idx))
    err, scale = float(np.abs(gbar[sel] - fd[sel]).max()), max(float(np.abs(gbar).max()), 1.0)
    print("n %d hard %s 2D %s: g adjoint against central differences %.3g absolute, max(max |gbar|, 1) %.3g"
          % (n, hard, two_d, err, scale))
    assert err <= 1e-7 * scale


@pytest.mark.parametrize("hard", [False, True])
def test_default_g_is_differentiated_at_two_pi_over_n(hard):
    rf, _ = _pulse(5, 7)
    x, y = np.linspace(-3, 3, 5), np.array([-2.0, 0.0, 1.0])
    rng = np.random.default_rng(6)
    ca, cb = (rng.standard_normal((5, 3)) + 1j * rng.standard_normal((5, 3)) for _ in range(2))
    g1 = np.full(7, 2 * np.pi / 7)
    for a, b in zip(refg.vjp_rfg(rf, None, x, ca[:, 0], cb[:, 0], hard_pulse=hard),
                    refg.vjp_rfg(rf, g1, x, ca[:, 0], cb[:, 0], hard_pulse=hard)):
        assert np.array_equal(a, b)
    for a, b in zip(refg.vjp_rfg(rf, None, x, ca, cb, y, hard_pulse=hard),
                    refg.vjp_rfg(rf, g1 + 0j, x, ca, cb, y, hard_pulse=hard)):
        assert np.array_equal(a, b)


def test_scale_sweep_adds_g_without_a_factor_and_rf_with_s():
    rf, g = _pulse(3, 9)
    x = np.linspace(-2, 2, 5)
    sc = [1.0, 0.0, 0.9]
    rng = np.random.default_rng(4)
    ca, cb = (rng.standard_normal((3, 5)) + 1j * rng.standard_normal((3, 5)) for _ in range(2))
    grad, gbar = refg.vjp_rfg_scaled(rf, g.real, x, (ca, cb), sc)
    assert np.array_equal(grad, ref.vjp_scaled(rf, g.real, x, (ca, cb), sc))
    parts = [refg.vjp_rfg(rf * s, g.real, x, ca[k], cb[k]) for k, s in enumerate(sc)]
    assert np.array_equal(gbar, parts[0][1] + parts[1][1] + parts[2][1])

    def L(gv):
        tot = 0.0
        for k, s in enumerate(sc):
            a, b = ref.forward(rf * s, gv, x)
            tot += float((np.conj(ca[k]) * a + np.conj(cb[k]) * b).real.sum())
        return tot
    h, fd = 1e-6, np.zeros(9)
    for m in range(9):
        e = np.zeros(9)
        e[m] = h
        fd[m] = (L(g.real + e) - L(g.real - e)) / (2 * h)
    assert np.abs(gbar - fd).max() <= 1e-7 * max(np.abs(gbar).max(), 1.0)


def test_rfg_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym, nargs in (("mbfir_abr_vjp_rfg_batch", 19), ("mbfir_abr2_vjp_rfg_batch", 24)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert len(mbfir.SYMBOLS[sym][1]) == nargs
        assert getattr(mbfir.load_library(), sym) is not None           # the library exports it
    assert callable(mbfir.abr_vjp_rfg_batch) and callable(mbfir.abr2_vjp_rfg_batch)


def test_rfg_argument_errors_come_before_any_device_work():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    c1, c2 = np.zeros((1, 5), dtype=complex), np.zeros((1, 5, 3), dtype=complex)
    with pytest.raises(ValueError, match="abr_vjp_rfg_batch: no pulses"):
        mbfir.abr_vjp_rfg_batch([], x, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr_vjp_rfg_batch([np.ones(4)], x, [(c1, c1)], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.abr_vjp_rfg_batch([np.ones(4), np.zeros(0)], x, [(c1, c1), (c1, c1)])
    with pytest.raises(ValueError, match="one entry per rf sample"):
        mbfir.abr_vjp_rfg_batch([(np.ones(4), np.ones(3))], x, [(c1, c1)])
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr_vjp_rfg_batch([np.ones(4)], x, [(c1, c1)], convention="abx")
    with pytest.raises(ValueError, match="cotangent pairs"):
        mbfir.abr_vjp_rfg_batch([np.ones(4)], x, [(c1, c1), (c1, c1)])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr_vjp_rfg_batch([np.ones(4)], x, [(c1, c1[:, :4])])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr_vjp_rfg_batch([np.ones(4)], x, [(c1, c1)], scales=(1.0, 0.9))
    with pytest.raises(ValueError, match="abr2_vjp_rfg_batch: no pulses"):
        mbfir.abr2_vjp_rfg_batch([], x, y, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr2_vjp_rfg_batch([np.ones(4)], x, y, [(c2, c2)], scales=())
    with pytest.raises(ValueError, match="an empty y"):
        mbfir.abr2_vjp_rfg_batch([np.ones(4)], x, np.zeros(0), [(c2, c2)])
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr2_vjp_rfg_batch([np.ones(4)], x, y, [(c2, c2)], convention="abx")
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr2_vjp_rfg_batch([np.ones(4)], x, y, [(c2, c2.reshape(1, 3, 5))])
    # the C calls refuse a null context before they read anything else (the checks that need a context: tests/test_simgradg_gpu.py)
    lib = mbfir.load_library()
    for sym in ("mbfir_abr_vjp_rfg_batch", "mbfir_abr2_vjp_rfg_batch"):
        args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[sym][1][1:]]
        assert getattr(lib, sym)(*args) == mbfir.E_ARG


def _stub_device_calls(monkeypatch):
    """mbfir's one-pulse simulator calls replaced by the NumPy reference, so that torchsim's plumbing runs without a device"""
    def split(p):
        return p if isinstance(p, tuple) else (p, None)

    def abr_batch(pulses, x, *, scales, hard_pulse):
        rf, g = split(pulses[0])
        return [tuple(np.stack(v) for v in zip(*[ref.forward(rf * s, g, x, hard_pulse=hard_pulse) for s in scales]))]

    def abr2_batch(pulses, x, y, *, scales, hard_pulse):
        rf, g = split(pulses[0])
        return [tuple(np.stack(v) for v in zip(*[ref.forward(rf * s, g, x, y, hard_pulse=hard_pulse) for s in scales]))]

    def abr_vjp_batch(pulses, x, cot, *, scales, hard_pulse):
        rf, g = split(pulses[0])
        return [ref.vjp_scaled(rf, g, x, cot[0], scales, hard_pulse=hard_pulse)]

    def abr_vjp_rfg_batch(pulses, x, cot, *, scales, hard_pulse):
        rf, g = split(pulses[0])
        return [refg.vjp_rfg_scaled(rf, g, x, cot[0], scales, hard_pulse=hard_pulse)]

    def abr2_vjp_rfg_batch(pulses, x, y, cot, *, scales, hard_pulse):
        rf, g = split(pulses[0])
        return [refg.vjp_rfg_scaled(rf, g, x, cot[0], scales, y=y, hard_pulse=hard_pulse)]

    def no_device(*a, **k):
        raise AssertionError("a tangent call was made")
    for name, fn in (("abr_batch", abr_batch), ("abr2_batch", abr2_batch), ("abr_vjp_batch", abr_vjp_batch),
                     ("abr_vjp_rfg_batch", abr_vjp_rfg_batch), ("abr2_vjp_rfg_batch", abr2_vjp_rfg_batch),
                     ("abr_jvp_batch", no_device), ("abr2_jvp_batch", no_device)):
        monkeypatch.setattr(mbfir, name, fn)


@pytest.mark.parametrize("hard", [False, True])
def test_torchsim_routes_g_on_stubbed_calls(monkeypatch, hard):
    """torchsim with mbfir's calls stubbed by the reference (no device): gradcheck in g and in (rf, g); a backward that needs only rf
    makes the rf call; torch.func.jvp with a tangent for g raises NotImplementedError, in 1D and 2D, before any call."""
    import torch
    _stub_device_calls(monkeypatch)
    rng = np.random.default_rng(5)
    rf0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * 0.3
    g1 = rng.uniform(0.5, 1.5, 6)
    g2 = g1 + 1j * rng.uniform(-1, 1, 6)
    x, x2, y2 = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3), np.linspace(-2, 2, 4)
    sc = (1.0, 0.8)
    rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
    rfc = torch.tensor(rf0, dtype=torch.complex128)
    tg1 = torch.tensor(g1, dtype=torch.float64, requires_grad=True)
    tg2 = torch.tensor(g2, dtype=torch.complex128, requires_grad=True)
    assert torch.autograd.gradcheck(lambda g: mbfir.torchsim.abr(rfc, x, g, scales=sc, hard_pulse=hard), (tg1,))
    assert torch.autograd.gradcheck(lambda r, g: mbfir.torchsim.abr2(r, g, x2, y2, scales=sc, hard_pulse=hard), (rf, tg2))
    monkeypatch.setattr(mbfir, "abr_vjp_rfg_batch", None)           # rf alone: the rf call, never the rfg one
    a, b = mbfir.torchsim.abr(rf, x, torch.tensor(g1), scales=sc, hard_pulse=hard)
    (a.abs() ** 2 + b.real).sum().backward()
    assert rf.grad is not None
    with pytest.raises(ValueError, match="float64"):
        mbfir.torchsim.abr(rfc, x, torch.tensor(g1, dtype=torch.float32, requires_grad=True), scales=sc)
    with pytest.raises(ValueError, match="complex128"):
        mbfir.torchsim.abr2(rfc, tg1, x2, y2, scales=sc)
    with pytest.raises(NotImplementedError, match="tangent with respect to g"):
        torch.func.jvp(lambda r, g: mbfir.torchsim.abr(r, x, g, scales=sc, hard_pulse=hard), (rfc, torch.tensor(g1)),
                       (torch.ones_like(rfc), torch.ones(6, dtype=torch.float64)))
    with pytest.raises(NotImplementedError, match="tangent with respect to g"):
        torch.func.jvp(lambda g: mbfir.torchsim.abr2(rfc, g, x2, y2, scales=sc, hard_pulse=hard), (torch.tensor(g2),),
                       (torch.ones(6, dtype=torch.complex128),))
