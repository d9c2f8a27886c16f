"""NumPy restatement of the least-squares products of the Cayley-Klein simulators (helper of tests/test_simgn_cpu.py and
tests/test_simgn_gpu.py; not collected).  The forward model, its adjoint and its tangent are those of tests/simgrad_ref.py and
tests/simjvp_ref.py, loaded by path.

For a profile f(a, b), a real weight w >= 0 and a target t per point and scale, L = 1/2 sum w |f - t|^2.  With F = df / d(a, b)
and J = F d(a, b) / drf:
    lsq: g = J^H W (f - t): the adjoint with the seed lambda = F^H c, c = w (f - t)
    gn:  H v = J^H W J v:   the adjoint with the seed lambda = F^H c, c = w F dpsi, dpsi the tangent along v
    kind   f              F dpsi                          (lambda_a, lambda_b)
    ex     2 conj(a) b    2 (conj(da) b + conj(a) db)     (2 b conj(c), 2 a c)
    se     i b^2          2i b db                         (0, -2i conj(b) c)
    inv    1 - 2 |b|^2    -4 Re(conj(b) db)               (0, -4 b Re c)
    st     i a^2          2i a da                         (-2i conj(a) c, 0)"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("simjvp_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "simjvp_ref.py"))
_jvp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_jvp)
forward, vjp, vjp_scaled, jvp, jvp_scaled = _jvp.forward, _jvp.vjp, _jvp.vjp_scaled, _jvp.jvp, _jvp.jvp_scaled

KINDS = ("ex", "se", "inv", "st")


def _kind(kind):
    kind = "inv" if kind == "sat" else kind
    assert kind in KINDS, kind
    return kind


def profile(kind, a, b):
    kind = _kind(kind)
    if kind == "ex":
        return 2 * np.conj(a) * b
    if kind == "se":
        return 1j * b * b
    if kind == "inv":
        return 1 - 2 * np.abs(b) ** 2 + 0j
    return 1j * a * a


def dprofile(kind, a, b, da, db):
    kind = _kind(kind)
    if kind == "ex":
        return 2 * (np.conj(da) * b + np.conj(a) * db)
    if kind == "se":
        return 2j * b * db
    if kind == "inv":
        return -4 * (np.conj(b) * db).real + 0j
    return 2j * a * da


def seed(kind, a, b, c):
    """(lambda_a, lambda_b) = F^H c"""
    kind = _kind(kind)
    z = np.zeros_like(a)
    if kind == "ex":
        return 2 * b * np.conj(c), 2 * a * c
    if kind == "se":
        return z, -2j * np.conj(b) * c
    if kind == "inv":
        return z, -4 * b * c.real
    return -2j * np.conj(a) * c, z


def _weights(w, shape):
    w = np.asarray(w, dtype=np.float64)
    return np.broadcast_to(w, shape)


def loss(rf, g, x, t, w, scales, kind="ex", y=None, hard_pulse=False):
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    ab = [forward(rf * s, g, x, y, hard_pulse) for s in scales]
    f = np.stack([profile(kind, a, b) for a, b in ab])
    w = _weights(w, f.shape)
    return 0.5 * float(np.sum(w * np.abs(f - np.asarray(t).reshape(f.shape)) ** 2))


def lsq(rf, g, x, t, w, scales, kind="ex", y=None, hard_pulse=False, parts=False):
    """(L, grad); with parts also N = sum(|lambda_a| + |lambda_b|) of the seed and E = sum w (|f| + |t|)^2"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    ab = [forward(rf * s, g, x, y, hard_pulse) for s in scales]
    a, b = np.stack([p[0] for p in ab]), np.stack([p[1] for p in ab])
    f = profile(kind, a, b)
    w = _weights(w, f.shape)
    t = np.asarray(t, dtype=np.complex128).reshape(f.shape)
    c = w * (f - t)
    la, lb = seed(kind, a, b, c)
    L = 0.5 * float(np.sum(w * np.abs(f - t) ** 2))
    grad = vjp_scaled(rf, g, x, (la, lb), scales, y, hard_pulse)
    if parts:
        return L, grad, float(np.sum(np.abs(la) + np.abs(lb))), float(np.sum(w * (np.abs(f) + np.abs(t)) ** 2))
    return L, grad


def jac(rf, g, x, v, scales, kind="ex", y=None, hard_pulse=False):
    """F J v over (S, ...): the first-order change of the profile along v"""
    (a, b), (da, db) = jvp_scaled(rf, g, x, v, scales, y, hard_pulse)
    return dprofile(kind, a, b, da, db)


def gn(rf, g, x, v, w, scales, kind="ex", y=None, hard_pulse=False, parts=False):
    """H v = J^H W J v; with parts also N of the seed"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    (a, b), (da, db) = jvp_scaled(rf, g, x, v, scales, y, hard_pulse)
    d = dprofile(kind, a, b, da, db)
    w = _weights(w, d.shape)
    la, lb = seed(kind, a, b, w * d)
    hv = vjp_scaled(rf, g, x, (la, lb), scales, y, hard_pulse)
    if parts:
        return hv, float(np.sum(np.abs(la) + np.abs(lb)))
    return hv
