"""NumPy restatement of the tangent of the Cayley-Klein simulators with respect to rf (helper of tests/test_simjvp_cpu.py and
tests/test_simjvp_gpu.py; not collected), vectorised over the points.  The model, its angles and `half_sinc` are those of
tests/simgrad_ref.py, loaded by path.

Per point and sample m, with psi = (a, b), psi_m = Q_m psi_{m-1}, r = rf_m and dr = v_m for a direction v of the rf samples:
    dpsi_m = Q_m dpsi_{m-1} + (dQ_m[dr]) psi_{m-1},   dpsi_0 = 0
dQ_m[dr] is real-linear in (Re dr, Im dr); with inv = sin(phi/2)/phi, D = (d inv / d phi) / phi and r . dr = Re r Re dr + Im r Im dr:
    mode 0 (abrm.m)   d alpha = (r . dr)(-inv/2 - i om D),  d beta = D (r . dr)(-i r) + inv (-i dr)
                      da' = alpha da - conj(beta) db + d alpha a - conj(d beta) b,  db' = beta da + conj(alpha) db + d beta a + conj(d alpha) b
    mode 1 (hard)     d C = -(r . dr) inv / 2,  dS = D (r . dr)(i r) + inv (i dr),  w = exp(-i om) b,  dw = exp(-i om) db
                      da' = C da - conj(S) dw + dC a - conj(dS) w,  db' = S da + C dw + dS a + dC w"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("simgrad_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "simgrad_ref.py"))
_grad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_grad)
forward, vjp, vjp_scaled = _grad.forward, _grad.vjp, _grad.vjp_scaled


def jvp(rf, g, x, v, y=None, hard_pulse=False):
    """((a, b), (da, db)) over the grid for the direction v (n,): each of shape (nx,) in 1D, (nx, ny) in 2D"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    v = np.asarray(v, dtype=np.complex128).ravel()
    assert v.shape == rf.shape
    om = _grad._angles(len(rf), g, x, y)
    a = np.ones(om.shape[1:], dtype=np.complex128)
    b = np.zeros(om.shape[1:], dtype=np.complex128)
    da, db = np.zeros_like(a), np.zeros_like(a)
    for r, dr, o in zip(rf, v, om):
        rd = r.real * dr.real + r.imag * dr.imag
        if hard_pulse:
            inv, D = _grad._half_sinc(np.abs(r))
            C, S, z = np.cos(np.abs(r) / 2), 1j * r * inv, np.exp(-1j * o)
            dC, dS = -rd * inv / 2, D * rd * (1j * r) + inv * (1j * dr)
            w, dw = z * b, z * db
            da, db = C * da - np.conj(S) * dw + dC * a - np.conj(dS) * w, S * da + C * dw + dS * a + dC * w
            a, b = C * a - np.conj(S) * w, S * a + C * w
        else:
            phi = np.sqrt(np.abs(r) ** 2 + o ** 2)
            inv, D = _grad._half_sinc(phi)
            al, be = np.cos(phi / 2) - 1j * o * inv, -1j * r * inv
            dal, dbe = rd * (-inv / 2 - 1j * o * D), D * rd * (-1j * r) + inv * (-1j * dr)
            da, db = (al * da - np.conj(be) * db + dal * a - np.conj(dbe) * b,
                      be * da + np.conj(al) * db + dbe * a + np.conj(dal) * b)
            a, b = al * a - np.conj(be) * b, be * a + np.conj(al) * b
    return (a, b), (da, db)


def jvp_scaled(rf, g, x, v, scales, y=None, hard_pulse=False):
    """The tangent of the scale sweep: ((a, b), (da, db)), each (S, ...): scale s simulates s rf and moves it along s v"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    v = np.asarray(v, dtype=np.complex128).ravel()
    res = [jvp(rf * s, g, x, v * s, y, hard_pulse) for s in scales]
    return ((np.stack([p[0] for p, _ in res]), np.stack([p[1] for p, _ in res])),
            (np.stack([t[0] for _, t in res]), np.stack([t[1] for _, t in res])))
