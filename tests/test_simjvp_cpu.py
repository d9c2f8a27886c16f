"""The NumPy reference of the simulators' tangent (tests/simjvp_ref.py, no GPU): its primal against tests/simgrad_ref.py, its tangent
against central differences of that forward and, through the dot-product identity, against that adjoint; and the bindings and
argument errors that mbfir.abr_jvp_batch / abr2_jvp_batch raise before any device work."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("simjvp_ref", os.path.join(ROOT, "tests", "simjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

CASES = [(n, hard, two_d) for n in (1, 7, 300) for hard in (False, True) for two_d in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(n, hard, two_d):
    """A pulse of flip 2 rad with, for n > 1, one rf sample exactly zero; x = 0 is on the grid, so phi = 0 occurs.  Returns the
    inputs, a random direction and the reference's ((a, b), (da, db)) along it."""
    rng = np.random.default_rng(10 + n)
    rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (2.0 / n)
    g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n + 1j * rng.uniform(-1.5, 1.5, n) * 1e-2
    if n > 1:
        rf[n // 2] = 0.0
    x = np.linspace(-3, 3, 7)
    assert x[3] == 0.0
    y = np.array([-20.0, 0.0, 15.0]) if two_d else None
    gg = g if two_d else g.real
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return rf, gg, x, y, v, ref.jvp(rf, gg, x, v, y, hard_pulse=hard)


@pytest.mark.parametrize("n,hard,two_d", CASES)
def test_primal_is_the_forward_of_the_adjoint_reference(n, hard, two_d):
    rf, g, x, y, _, ((a, b), _) = _case(n, hard, two_d)
    a0, b0 = ref.forward(rf, g, x, y, hard_pulse=hard)
    assert a.shape == ((7, 3) if two_d else (7,))
    assert np.abs(a - a0).max() <= 1e-14 and np.abs(b - b0).max() <= 1e-14


@pytest.mark.parametrize("n,hard,two_d", CASES)
def test_tangent_is_the_central_difference_of_the_forward(n, hard, two_d):
    """h = 1e-6 along v; every entry within 1e-7 sum|v| (sum|v| bounds any tangent entry: the derivative of a rotation has norm
    <= 1; the O(h^2) truncation term and the rounding of the difference, about eps / h, are both far below 1e-7)."""
    rf, g, x, y, v, (_, (da, db)) = _case(n, hard, two_d)
    h = 1e-6
    ap, bp = ref.forward(rf + h * v, g, x, y, hard_pulse=hard)
    am, bm = ref.forward(rf - h * v, g, x, y, hard_pulse=hard)
    err = max(float(np.abs(da - (ap - am) / (2 * h)).max()), float(np.abs(db - (bp - bm) / (2 * h)).max()))
    bound = 1e-7 * float(np.abs(v).sum())
    print("n %d hard %s 2D %s: tangent against central differences %.3g, bound %.3g" % (n, hard, two_d, err, bound))
    assert err <= bound


@pytest.mark.parametrize("n,hard,two_d", CASES)
def test_tangent_and_adjoint_satisfy_the_dot_product_identity(n, hard, two_d):
    """Re sum(conj(ca) da + conj(cb) db) = Re sum(conj(gbar) v) for gbar = vjp(ca, cb): relative to the larger side at most 1e-12.
    Both sides are O(n) fp64 sums of O(1) terms, which leaves about three digits over rounding at n = 300."""
    rf, g, x, y, v, (_, (da, db)) = _case(n, hard, two_d)
    rng = np.random.default_rng(77)
    ca, cb = (rng.standard_normal(da.shape) + 1j * rng.standard_normal(da.shape) for _ in range(2))
    lhs = float((np.conj(ca) * da + np.conj(cb) * db).real.sum())
    rhs = float((np.conj(ref.vjp(rf, g, x, ca, cb, y, hard_pulse=hard)) * v).real.sum())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print("n %d hard %s 2D %s: <c, J v> %.15g, <J^H c, v> %.15g, relative difference %.3g" % (n, hard, two_d, lhs, rhs, rel))
    assert rel <= 1e-12


def test_scale_sweep_tangent_is_the_chain_rule():
    rf, g, x, _, v, _ = _case(7, False, False)
    sc = [1.0, 0.0, 0.9]
    (a, b), (da, db) = ref.jvp_scaled(rf, g, x, v, sc)
    assert a.shape == da.shape == (3, 7)
    assert np.array_equal(da[1], np.zeros(7)) and np.array_equal(db[1], np.zeros(7))       # dr = 0 v at scale 0
    h = 1e-6
    for k, s in enumerate(sc):
        ap, bp = ref.forward((rf + h * v) * s, g, x)
        am, bm = ref.forward((rf - h * v) * s, g, x)
        assert np.abs(da[k] - (ap - am) / (2 * h)).max() <= 1e-7 * np.abs(v).sum()
        assert np.abs(db[k] - (bp - bm) / (2 * h)).max() <= 1e-7 * np.abs(v).sum()


def test_jvp_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym, nargs in (("mbfir_abr_jvp_batch", 23), ("mbfir_abr2_jvp_batch", 27), ("mbfir_test_jvp_group", 0)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert len(mbfir.SYMBOLS[sym][1]) == nargs
        assert getattr(mbfir.load_library(), sym) is not None           # the library exports it
    assert callable(mbfir.abr_jvp_batch) and callable(mbfir.abr2_jvp_batch)
    assert mbfir.jvp_group() in (1, 2, 4, 8)


def test_jvp_argument_errors_come_before_any_device_work():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    rf, v = np.ones(4), np.ones(4, dtype=complex)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr_jvp_batch([], x, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr_jvp_batch([rf], x, [v], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.abr_jvp_batch([rf, np.zeros(0)], x, [v, v])
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr_jvp_batch([rf], x, [v], convention="abx")
    with pytest.raises(ValueError, match="2 tangents for 1 pulses"):
        mbfir.abr_jvp_batch([rf], x, [v, v])
    with pytest.raises(ValueError, match=r"shape \(3,\)"):                          # the wrong length
        mbfir.abr_jvp_batch([rf], x, [v[:3]])
    with pytest.raises(ValueError, match=r"shape \(2, 5\)"):
        mbfir.abr_jvp_batch([rf], x, [np.ones((2, 5), dtype=complex)])
    with pytest.raises(ValueError, match=r"shape \(0, 4\)"):                        # K = 0
        mbfir.abr_jvp_batch([rf], x, [np.ones((0, 4), dtype=complex)])
    with pytest.raises(ValueError, match="the same K"):                             # ragged K
        mbfir.abr_jvp_batch([rf, rf], x, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)])
    with pytest.raises(ValueError, match="the same K"):
        mbfir.abr_jvp_batch([rf, rf], x, [np.ones((1, 4), dtype=complex), v])
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr2_jvp_batch([], x, y, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr2_jvp_batch([rf], x, y, [v], scales=())
    with pytest.raises(ValueError, match="an empty y"):
        mbfir.abr2_jvp_batch([rf], x, np.zeros(0), [v])
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr2_jvp_batch([rf], x, y, [v], convention="abx")
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        mbfir.abr2_jvp_batch([rf], x, y, [v[:3]])
    with pytest.raises(ValueError, match="the same K"):
        mbfir.abr2_jvp_batch([rf, rf], x, y, [np.ones((2, 4), dtype=complex), np.ones((3, 4), dtype=complex)])


def test_c_calls_refuse_a_null_context():
    """The C calls' own checks need a context, which needs a device (tests/test_simjvp_gpu.py has their messages); without one
    they return MBFIR_E_ARG, as every call does."""
    lib = mbfir.load_library()
    d = np.ones(8)
    off = np.array([0, 2], dtype=np.int64)
    lp, p = off.ctypes.data_as(mbfir._lp), mbfir._ptr(d)
    assert lib.mbfir_abr_jvp_batch(None, 1, lp, p, p, None, 1, lp, p, 1, p, 0, 1, p, p, p, p, p, p, p, p, p, p) == mbfir.E_ARG
    assert lib.mbfir_abr2_jvp_batch(None, 1, lp, p, p, None, None, 1, lp, p, 1, lp, p, 1, p, 0, 1, p, p, p, p, p, p, p, p, p,
                                    p) == mbfir.E_ARG
