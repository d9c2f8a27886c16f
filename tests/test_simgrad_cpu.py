"""The NumPy reference of the simulators' adjoint (tests/simgrad_ref.py, no GPU): its forward against the other restatements of the
model and against oracle.bloch, its adjoint against central differences of its own forward, and the bindings and argument errors
that mbfir.abr_vjp_batch / abr2_vjp_batch raise before any device work."""
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir
from oracle import bloch as obloch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("simgrad_ref", "simgrad_ref.py")


def _pulse(seed, n, flip=np.pi / 2):
    rng = np.random.default_rng(seed)
    rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (flip / n)
    g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n + 1j * rng.uniform(-1.5, 1.5, n) * 1e-2
    return rf, g


def test_forward_is_the_oracle_and_the_2d_restatement():
    abr2_np = _load("abr2batch_gpu", "test_abr2batch_gpu.py").abr2_np
    rf, g = _pulse(1, 60)
    x, y = np.linspace(-20, 20, 31), np.linspace(-30, 30, 5)
    a, b = ref.forward(rf, g.real, x)
    ao, bo = obloch.abrm(rf, g.real, x)
    assert np.abs(a - ao).max() <= 1e-14 and np.abs(b - bo).max() <= 1e-14
    a, b = ref.forward(rf, None, x, hard_pulse=True)
    ao, bo = obloch.hard_pulse_ab(rf, x)
    assert np.abs(a - ao).max() <= 1e-14 and np.abs(b - bo).max() <= 1e-14
    for hard in (False, True):
        a, b = ref.forward(rf, g, x, y, hard_pulse=hard)
        a2, b2 = abr2_np(rf, g, x, y, hard_pulse=hard)
        assert a.shape == (31, 5)
        assert np.abs(a - a2).max() <= 1e-14 and np.abs(b - b2).max() <= 1e-14
        a1, b1 = ref.forward(rf, g.real, x, hard_pulse=hard)              # 2D at y = 0 is 1D
        a, b = ref.forward(rf, g, x, [0.0], hard_pulse=hard)
        assert np.abs(a[:, 0] - a1).max() <= 1e-14 and np.abs(b[:, 0] - b1).max() <= 1e-14


def _loss(rf, g, x, y, hard, wa, wb):
    """A real loss whose cotangents are not constant: L = sum Re(conj(wa) a) + |b|^2 Re(wb)"""
    a, b = ref.forward(rf, g, x, y, hard_pulse=hard)
    return float((np.conj(wa) * a).real.sum() + (np.abs(b) ** 2 * wb.real).sum()), a, b


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("two_d", [False, True])
def test_adjoint_is_the_central_difference_of_the_forward(n, hard, two_d):
    """h = 1e-6 on each of Re rf_m, Im rf_m; bound 1e-7 relative to max |gbar| (the O(h^2) truncation term and the rounding of the
    difference, about eps L / h).  x = 0 is on the grid and, for n > 1, one rf sample is exactly zero, so phi = 0 occurs."""
    rf, g = _pulse(10 + n, n, flip=2.0)
    if n > 1:
        rf[n // 2] = 0.0
    x = np.linspace(-3, 3, 7)
    assert x[3] == 0.0
    y = np.array([-20.0, 0.0, 15.0]) if two_d else None
    gg = g if two_d else g.real
    rng = np.random.default_rng(99)
    shape = (7, 3) if two_d else (7,)
    wa = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    wb = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    _, a, b = _loss(rf, gg, x, y, hard, wa, wb)
    grad = ref.vjp(rf, gg, x, wa, 2 * wb.real * b, y, hard_pulse=hard)     # dL/da* convention: abar = wa, bbar = 2 Re(wb) b
    h = 1e-6
    fd = np.zeros(n, dtype=np.complex128)
    idx = range(n) if n <= 7 else sorted({0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1} | set(range(3, n, 37)))
    for m in idx:
        for d in (1.0, 1j):
            e = np.zeros(n, dtype=np.complex128)
            e[m] = h * d
            fd[m] += d * (_loss(rf + e, gg, x, y, hard, wa, wb)[0] - _loss(rf - e, gg, x, y, hard, wa, wb)[0]) / (2 * h)
    sel = np.array(list(idx))
    err = float(np.abs(grad[sel] - fd[sel]).max() / np.abs(grad).max())
    print("n %d hard %s 2D %s: adjoint against central differences %.3g" % (n, hard, two_d, err))
    assert err <= 1e-7


def test_scale_sweep_adjoint_is_the_chain_rule():
    rf, g = _pulse(3, 9)
    x = np.linspace(-2, 2, 5)
    sc = [1.0, 0.0, 0.9]
    rng = np.random.default_rng(4)
    ca, cb = (rng.standard_normal((3, 5)) + 1j * rng.standard_normal((3, 5)) for _ in range(2))
    grad = ref.vjp_scaled(rf, g.real, x, (ca, cb), sc)

    def L(r):
        tot = 0.0
        for k, s in enumerate(sc):
            a, b = ref.forward(r * s, g.real, x)
            tot += float((np.conj(ca[k]) * a + np.conj(cb[k]) * b).real.sum())
        return tot
    h, fd = 1e-6, np.zeros(9, dtype=np.complex128)
    for m in range(9):
        for d in (1.0, 1j):
            e = np.zeros(9, dtype=np.complex128)
            e[m] = h * d
            fd[m] += d * (L(rf + e) - L(rf - e)) / (2 * h)
    assert np.abs(grad - fd).max() <= 1e-7 * np.abs(grad).max()


def test_vjp_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym, nargs in (("mbfir_abr_vjp_batch", 18), ("mbfir_abr2_vjp_batch", 22)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert len(mbfir.SYMBOLS[sym][1]) == nargs
        assert getattr(mbfir.load_library(), sym) is not None           # the library exports it
    assert callable(mbfir.abr_vjp_batch) and callable(mbfir.abr2_vjp_batch)
    assert callable(mbfir.torchsim.abr) and callable(mbfir.torchsim.abr2)


def test_vjp_argument_errors_come_before_any_device_work():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    c1, c2 = np.zeros((1, 5), dtype=complex), np.zeros((1, 5, 3), dtype=complex)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr_vjp_batch([], x, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1)], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.abr_vjp_batch([np.ones(4), np.zeros(0)], x, [(c1, c1), (c1, c1)])
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1)], convention="abx")
    with pytest.raises(ValueError, match="cotangent pairs"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1), (c1, c1)])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1[:, :4])])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1)], scales=(1.0, 0.9))
    with pytest.raises(ValueError, match="pair"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [c1])
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr2_vjp_batch([], x, y, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr2_vjp_batch([np.ones(4)], x, y, [(c2, c2)], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.abr2_vjp_batch([np.ones(4), np.zeros(0)], x, y, [(c2, c2), (c2, c2)])
    with pytest.raises(ValueError, match="an empty y"):
        mbfir.abr2_vjp_batch([np.ones(4)], x, np.zeros(0), [(c2, c2)])
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr2_vjp_batch([np.ones(4)], x, y, [(c2, c2)], convention="abx")
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr2_vjp_batch([np.ones(4)], x, y, [(c2, c2.reshape(1, 3, 5))])
