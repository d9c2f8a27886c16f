"""NumPy restatement of the adjoint of the Cayley-Klein simulators with respect to rf and to the gradient waveform (helper of
tests/test_simgradg_cpu.py and tests/test_simgradg_gpu.py; not collected), vectorised over the points.  The forward model, the
reverse sweep and the rf pair are those of tests/simgrad_ref.py, loaded by path, in its arithmetic: the rf part of vjp_rfg equals
simgrad_ref.vjp to the bit.

Per point and sample of the reverse sweep, with u, v (mode 1: w = exp(-i om) v) the state before the sample and la, lb the
multipliers after it, the contribution dom = dL / d om of the precession angle is
    mode 0   dal = -om inv / 2 - i (inv + om^2 D),  dbe = -i r D om
             dom = Re( conj(la) (dal u - conj(dbe) v) + conj(lb) (dbe u + conj(dal) v) )
    mode 1   dom = Re( conj(la) (i conj(S) w) + conj(lb) (-i C w) )        (only exp(-i om) depends on om)
and om = x g (1D) or x Re g + y Im g (2D) gives dL/dg_m = sum_i x_i dom (1D, real) or sum x dom + i sum y dom (2D, complex: torch's
convention for a complex input).  A scale multiplies rf, not g: the g-gradients of a scale sweep add without a factor."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("simgrad_ref",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "simgrad_ref.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
forward = base.forward


def vjp_rfg(rf, g, x, ca, cb, y=None, hard_pulse=False):
    """(gbar_rf (n,) complex, gbar_g (n,): real in 1D, complex dL/dgx + i dL/dgy in 2D) for the cotangents ca, cb in forward's
    shapes; g None: differentiated at the default 2 pi / n (along x)"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    om = base._angles(len(rf), g, x, y)
    a, b = forward(rf, g, x, y, hard_pulse)
    la = np.asarray(ca, dtype=np.complex128).reshape(a.shape)
    lb = np.asarray(cb, dtype=np.complex128).reshape(a.shape)
    grad = np.zeros(len(rf), dtype=np.complex128)
    x = np.asarray(x, dtype=np.float64)
    if y is None:
        X2, Y2 = x, None
        gg = np.zeros(len(rf))
    else:
        X2, Y2 = np.meshgrid(x, np.asarray(y, dtype=np.float64), indexing="ij")
        gg = np.zeros(len(rf), dtype=np.complex128)
    for m in range(len(rf) - 1, -1, -1):
        r, o = rf[m], om[m]
        if hard_pulse:                                           # the rf lines are simgrad_ref.vjp's, token for token
            th = np.abs(r)
            inv, D = base._half_sinc(th)
            C, S, sh, z = np.cos(th / 2), 1j * r * inv, 1j * r, np.exp(1j * o)
            u, w = C * a + np.conj(S) * b, C * b - S * a
            t1, t2 = -0.5 * inv * u - D * np.conj(sh) * w, D * sh * u - 0.5 * inv * w
            com = (np.conj(la) * t1 + np.conj(lb) * t2).real
            X, Y = np.conj(la) * w, np.conj(lb) * u
            gre, gim = r.real * com - inv * (X + Y).imag, r.imag * com + inv * (X - Y).real
            dom = (np.conj(la) * (1j * np.conj(S) * w) + np.conj(lb) * (-1j * C * w)).real
            la, lb = C * la + np.conj(S) * lb, z * (C * lb - S * la)
            a, b = u, z * w
        else:
            phi = np.sqrt(np.abs(r) ** 2 + o ** 2)
            inv, D = base._half_sinc(phi)
            al, be, bh, ka = np.cos(phi / 2) - 1j * o * inv, -1j * r * inv, -1j * r, -0.5 * inv - 1j * o * D
            u, v = np.conj(al) * a + np.conj(be) * b, al * b - be * a
            t1, t2 = ka * u - D * np.conj(bh) * v, D * bh * u + np.conj(ka) * v
            com = (np.conj(la) * t1 + np.conj(lb) * t2).real
            X, Y = np.conj(la) * v, np.conj(lb) * u
            gre, gim = r.real * com + inv * (X + Y).imag, r.imag * com + inv * (Y - X).real
            dal, dbe = -0.5 * o * inv - 1j * (inv + o * o * D), -1j * r * D * o
            dom = (np.conj(la) * (dal * u - np.conj(dbe) * v) + np.conj(lb) * (dbe * u + np.conj(dal) * v)).real
            la, lb = np.conj(al) * la + np.conj(be) * lb, al * lb - be * la
            a, b = u, v
        grad[m] = gre.sum() + 1j * gim.sum()
        gg[m] = (X2 * dom).sum() if Y2 is None else (X2 * dom).sum() + 1j * (Y2 * dom).sum()
    return grad, gg


def vjp_rfg_scaled(rf, g, x, cot, scales, y=None, hard_pulse=False):
    """The adjoint of the scale sweep: cot = (ca, cb), each (S, ...); scale s contributes s times the rf gradient with respect to
    s rf, and its g gradient as it is"""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    grad = np.zeros(len(rf), dtype=np.complex128)
    gg = np.zeros(len(rf), dtype=np.float64 if y is None else np.complex128)
    for k, s in enumerate(scales):
        gr, g1 = vjp_rfg(rf * s, g, x, cot[0][k], cot[1][k], y, hard_pulse)
        grad += s * gr
        gg += g1
    return grad, gg
