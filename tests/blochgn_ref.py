"""NumPy restatement of the least-squares products of the Bloch simulator with relaxation (helper of tests/test_blochgn_cpu.py and
tests/test_blochgn_gpu.py; not collected), vectorised over the (frequency, position) points and the directions, in float64 or
np.longdouble.  The model, the forward sweep (forward), the adjoint (vjp) and the tangent (jvp) are those of tests/blochgrad_ref.py
and tests/blochjvp_ref.py, loaded by path.

With the end point m = (mx, my, mz) of the forward sweep at scale s, weights w = (wx, wy, wz) >= 0 and targets t = (tx, ty, tz) per
(scale, frequency, position) point:
    L   = 1/2 sum over the scales and points of sum_c w_c (m_c - t_c)^2
    g   = sum_s s J_s' W_s (m_s - t_s) = dL/dRe b1 + i dL/dIm b1                  (lsq)
    H v = sum_s s J_s' W_s J_s (s v),  J_s = d m / d (s b1)                       (gn)
Both are one forward sweep that keeps the trajectory (gn: blochjvp_ref.jvp beside it for the tangent dm), the pointwise seed
lambda_n = w (m - t) or w dm, and the reverse recursion of blochgrad_ref.vjp written once more with a leading axis for the K
directions (_reverse) and without vjp's rounding of the seed to float64, so that the long-double reference is long double
throughout.  tests/test_blochgn_cpu.py pins lsq and gn to blochgrad_ref.vjp of the residual and to jvp -> weights -> vjp.

Bounds of the device comparison.  They compose the two existing ones through the seed, as DESIGN 8m composes its own: the reverse
sweep with an exact seed lambda_n is within bound_b1 = 1e-12 max|s| gamma dt_t sum|lambda_n| (blochgrad_ref.bound_b1: a rotation's
derivative and the decay have norm at most 1), and it is linear in the seed with the same norm, so an error e of the seed adds at
most max|s| gamma dt_t sum|e|.
    g, per b1 entry t:  the forward tolerance of the Bloch tests is 1e-12 per component, so |e_c| <= 1e-12 w_c:
                        1e-12 max|s| gamma dt_t (N + sum (wx + wy + wz)),  N = sum|lambda_n| of the reference's seed
    H v:                |e_c| <= w_c bound_jvp (blochjvp_ref.bound_jvp = 1e-12 B_k, B_k = max|s| gamma sum_t dt_t |v_t|):
                        1e-12 max|s| gamma dt_t (N + B_k sum (wx + wy + wz)),  N of the seed w dm of direction k
    L:                  d(1/2 w r^2) = w r dr with |dr| <= 1e-12, plus the order of the sum over the points:
                        1e-12 sum w_c |m_c - t_c| + 1e-13 sum w_c (m_c - t_c)^2
All sums run over the pulse's points and scales."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("blochjvp_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "blochjvp_ref.py"))
jref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(jref)
_grad = jref._grad
forward, vjp, jvp, gamma_of, intervals = jref.forward, jref.vjp, jref.jvp, jref.gamma_of, jref.intervals
batch, directions, bound_jvp = jref.batch, jref.directions, jref.bound_jvp
SCALES, TOL, GAMMA_H1, _grid = jref.SCALES, jref.TOL, jref.GAMMA_H1, jref._grid


def planes(tri, S, nf, npos, dtype=np.float64):
    """A triple of weights or targets, each entry (S, nf, npos), (nf, npos) or a scalar -> (3, S, nf, npos)"""
    return np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (S, nf, npos)) for v in tri]).astype(dtype)


def _reverse(Q, traj, lam):
    """blochgrad_ref.vjp's reverse recursion from the seed lam = three arrays (..., nf, npos) in Q's dtype: the gradient (..., n),
    the factor s of the chain rule through s b1 included"""
    dtype = Q.dtype
    lead = lam[0].shape[:-2]
    g = np.zeros(lead + (Q.n,), dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
    for t in range(Q.n - 1, -1, -1):
        (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
        dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
        mp = traj[t]
        gxy = []
        for p, eb, ec in ((nx, 0, -1), (ny, 1, 0)):
            dsp = D * p
            dR = _grad._drot(ar, ai, br, bi, -sp * p / 2, -nz * dsp, ny * dsp + eb * sp, -nx * dsp + ec * sp)
            w = _grad._mat_vec(dR, mp)
            gxy.append((dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]).sum((-2, -1)))
        f = dtype(Q.s) * dtype(Q.gamma) * dtype(Q.dt[t])
        g[..., t] = -f * gxy[0] + 1j * (f * gxy[1])
        lam = _grad._mat_vec(_grad._rot(ar, ai, br, bi), dl, transpose=True)
    return g


def lsq(pulse, df, pos, targets, weights, scales, m0=None, dtype=np.float64, parts=False):
    """(L, g (n,)) of pulse = (b1, gr, tp, t1, t2, nucleus); with parts also dict(N = sum|seed|, W = sum w, A = sum w |m - t|,
    Q = sum w (m - t)^2) for the bounds"""
    b1, gr, tp, t1, t2, nucleus = pulse
    L, g, info = dtype(0), 0, dict(N=0.0, W=0.0, A=0.0, Q=0.0)
    w = tg = None
    for k, s in enumerate(scales):
        m, traj, Q = forward(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, dtype, keep=True)
        if w is None:
            w, tg = planes(weights, len(scales), Q.nf, Q.npos, dtype), planes(targets, len(scales), Q.nf, Q.npos, dtype)
        r = [m[c] - tg[c, k] for c in range(3)]
        lam = [w[c, k] * r[c] for c in range(3)]
        L = L + sum((w[c, k] * r[c] * r[c]).sum() for c in range(3)) / 2
        g = g + _reverse(Q, traj, lam)
        info["N"] += float(sum(np.abs(l).sum() for l in lam))
        info["A"] += float(sum(np.abs(l).sum() for l in lam))
        info["Q"] += float(sum((w[c, k] * r[c] * r[c]).sum() for c in range(3)))
    info["W"] = float(w.sum())
    return (L, g, info) if parts else (L, g)


def gn(pulse, df, pos, v, weights, scales, m0=None, dtype=np.float64, parts=False):
    """H v (K, n) for the directions v (K, n) (or (n,) -> (n,)); with parts also dict(N = sum|seed| per direction (K,), W = sum w,
    E = sum w dm^2 per direction (K,): Re <v, H v>)"""
    b1, gr, tp, t1, t2, nucleus = pulse
    v = np.asarray(v, dtype=np.complex128)
    one = v.ndim == 1
    v = v.reshape(-1, len(np.ravel(b1)))
    h, w = 0, None
    N, E = np.zeros(len(v)), np.zeros(len(v), dtype=dtype)
    for k, s in enumerate(scales):
        _, traj, Q = forward(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, dtype, keep=True)
        _, dm = jvp(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, v, None, dtype)
        if w is None:
            w = planes(weights, len(scales), Q.nf, Q.npos, dtype)
        lam = [w[c, k] * dm[c] for c in range(3)]                          # (K, nf, npos)
        h = h + _reverse(Q, traj, lam)
        N += np.array(sum(np.abs(l).sum((-2, -1)) for l in lam), dtype=np.float64)
        E = E + sum((w[c, k] * dm[c] * dm[c]).sum((-2, -1)) for c in range(3))
    h = h[0] if one else h
    return (h, dict(N=N, W=float(w.sum()), E=E)) if parts else h


def bound_g(pulse, info, scales):
    """Per b1 entry (n,)"""
    return TOL * max(abs(s) for s in scales) * gamma_of(pulse[5]) * intervals(pulse) * (info["N"] + info["W"])


def bound_h(pulse, v, info, scales):
    """Per entry of direction k (K, n)"""
    v = np.asarray(v).reshape(-1, len(pulse[0]))
    B = bound_jvp(pulse, v, None, scales)[:, 0, 0] / TOL                   # (K,)
    return TOL * max(abs(s) for s in scales) * gamma_of(pulse[5]) * intervals(pulse)[None, :] * (info["N"] + B * info["W"])[:, None]


def bound_L(info):
    return TOL * info["A"] + 1e-13 * info["Q"]


def cases(shared, K):
    """blochgrad_ref.batch(shared) -- eight pulses of 1, 7, 8, 9, 255, 256, 257 and 600 samples on grids of 1 x 1, 3 x 5, 1 x 257 and
    3 x 200 points or the shared 3 x 5 grid, random m0 with |m0| <= 1, a zero b1 sample at df = 0 and position 0, the 26 ms pulse at
    T2 = 1 ms -- with, per pulse, weights uniform in [0, 1] of which a third (of the 3 S nf npos entries) is set to zero, targets
    uniform in [-1, 1], each a triple of (S, nf, npos) arrays, and K directions as blochjvp_ref.directions draws them:
    (pulses, dfs, dps, m0s, targets, weights, vs)"""
    pulses, dfs, dps, m0s, _ = batch(shared)
    vs, _ = directions(pulses, dfs, dps, K)
    tgs, wts = [], []
    for q, (df, dp) in enumerate(zip(dfs, dps)):
        rng = np.random.default_rng([31, q])
        shape = (3, len(SCALES), len(df), np.shape(dp)[0])
        w = rng.uniform(0, 1, shape)
        flat = w.reshape(-1)
        flat[rng.permutation(flat.size)[:(flat.size + 2) // 3]] = 0.0
        wts.append(tuple(w))
        tgs.append(tuple(rng.uniform(-1, 1, shape)))
    return pulses, dfs, dps, m0s, tgs, wts, vs
