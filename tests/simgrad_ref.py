"""NumPy restatement of the Cayley-Klein simulators and of their adjoint with respect to rf (helper of tests/test_simgrad_cpu.py and
tests/test_simgrad_gpu.py; not collected), vectorised over the points.

Forward, per point and sample m: psi_m = Q_m psi_{m-1}, psi = (a, b), psi_0 = (1, 0), Q_m in SU(2) from r = rf_m and the precession
angle om (x g_m in 1D, x Re g_m + y Im g_m in 2D):
    mode 0 (abrm.m)   phi = sqrt(|r|^2 + om^2), alpha = cos(phi/2) - i om sin(phi/2)/phi, beta = -i r sin(phi/2)/phi,
                      a' = alpha a - conj(beta) b, b' = beta a + conj(alpha) b
    mode 1 (hard)     th = |r|, C = cos(th/2), S = i r sin(th/2)/th, w = exp(-i om) b,  a' = C a - conj(S) w, b' = S a + C w
Adjoint: with the cotangents (abar, bbar) of (a_n, b_n), dL = Re(conj(abar) da + conj(bbar) db), the sweep over the samples in
reverse recomputes psi_{m-1} = Q_m^H psi_m, adds Re <lambda_m, (dQ_m/dp) psi_{m-1}> for p = Re r, Im r, summed over the points, to
gbar_m = dL/dRe rf_m + i dL/dIm rf_m, and steps lambda_{m-1} = Q_m^H lambda_m from lambda_n = (abar, bbar)."""
import numpy as np


def _angles(n, g, x, y):
    """om[m] over the grid: (n, nx) in 1D (y None), (n, nx, ny) in 2D; g None: 2 pi / n along x."""
    x = np.asarray(x, dtype=np.float64)
    if y is None:
        g = np.full(n, 2 * np.pi / n) if g is None else np.asarray(g, dtype=np.float64).ravel()
        return g[:, None] * x[None, :]
    g = np.full(n, 2 * np.pi / n + 0j) if g is None else np.asarray(g, dtype=np.complex128).ravel()
    X, Y = np.meshgrid(x, np.asarray(y, dtype=np.float64), indexing="ij")
    return g.real[:, None, None] * X[None] + g.imag[:, None, None] * Y[None]


def _half_sinc(phi):
    """sin(phi/2)/phi and (its derivative)/phi, with the limits 1/2 and -1/24 + phi^2/960 below 1e-4"""
    small = phi < 1e-4
    safe = np.where(small, 1.0, phi)
    inv = np.where(phi > 0, np.sin(phi / 2) / np.where(phi > 0, phi, 1.0), 0.5)
    D = np.where(small, -1.0 / 24 + phi * phi / 960, (0.5 * np.cos(safe / 2) - np.sin(safe / 2) / safe) / (safe * safe))
    return inv, D


def forward(rf, g, x, y=None, hard_pulse=False):
    """(a, b) over the grid: shape (nx,) in 1D, (nx, ny) in 2D"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    om = _angles(len(rf), g, x, y)
    a = np.ones(om.shape[1:], dtype=np.complex128)
    b = np.zeros(om.shape[1:], dtype=np.complex128)
    for r, o in zip(rf, om):
        if hard_pulse:
            inv, _ = _half_sinc(np.abs(r))
            C, S, w = np.cos(np.abs(r) / 2), 1j * r * inv, np.exp(-1j * o) * b
            a, b = C * a - np.conj(S) * w, S * a + C * w
        else:
            phi = np.sqrt(np.abs(r) ** 2 + o ** 2)
            inv, _ = _half_sinc(phi)
            al, be = np.cos(phi / 2) - 1j * o * inv, -1j * r * inv
            a, b = al * a - np.conj(be) * b, be * a + np.conj(al) * b
    return a, b


def vjp(rf, g, x, ca, cb, y=None, hard_pulse=False):
    """gbar (n,) for the cotangents ca, cb in forward's shapes"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    om = _angles(len(rf), g, x, y)
    a, b = forward(rf, g, x, y, hard_pulse)
    la = np.asarray(ca, dtype=np.complex128).reshape(a.shape)
    lb = np.asarray(cb, dtype=np.complex128).reshape(a.shape)
    grad = np.zeros(len(rf), dtype=np.complex128)
    for m in range(len(rf) - 1, -1, -1):
        r, o = rf[m], om[m]
        if hard_pulse:
            th = np.abs(r)
            inv, D = _half_sinc(th)
            C, S, sh, z = np.cos(th / 2), 1j * r * inv, 1j * r, np.exp(1j * o)
            u, w = C * a + np.conj(S) * b, C * b - S * a
            t1, t2 = -0.5 * inv * u - D * np.conj(sh) * w, D * sh * u - 0.5 * inv * w
            com = (np.conj(la) * t1 + np.conj(lb) * t2).real
            X, Y = np.conj(la) * w, np.conj(lb) * u
            gre, gim = r.real * com - inv * (X + Y).imag, r.imag * com + inv * (X - Y).real
            la, lb = C * la + np.conj(S) * lb, z * (C * lb - S * la)
            a, b = u, z * w
        else:
            phi = np.sqrt(np.abs(r) ** 2 + o ** 2)
            inv, D = _half_sinc(phi)
            al, be, bh, ka = np.cos(phi / 2) - 1j * o * inv, -1j * r * inv, -1j * r, -0.5 * inv - 1j * o * D
            u, v = np.conj(al) * a + np.conj(be) * b, al * b - be * a
            t1, t2 = ka * u - D * np.conj(bh) * v, D * bh * u + np.conj(ka) * v
            com = (np.conj(la) * t1 + np.conj(lb) * t2).real
            X, Y = np.conj(la) * v, np.conj(lb) * u
            gre, gim = r.real * com + inv * (X + Y).imag, r.imag * com + inv * (Y - X).real
            la, lb = np.conj(al) * la + np.conj(be) * lb, al * lb - be * la
            a, b = u, v
        grad[m] = gre.sum() + 1j * gim.sum()
    return grad


def vjp_scaled(rf, g, x, cot, scales, y=None, hard_pulse=False):
    """The adjoint of the scale sweep: cot = (ca, cb), each (S, ...); scale s contributes s times the gradient with respect to s rf"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    grad = np.zeros(len(rf), dtype=np.complex128)
    for k, s in enumerate(scales):
        grad += s * vjp(rf * s, g, x, cot[0][k], cot[1][k], y, hard_pulse)
    return grad
