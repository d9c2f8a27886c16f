"""NumPy restatement of the tangent of the Bloch simulator with relaxation with respect to b1 and the initial magnetisation (helper
of tests/test_blochjvp_cpu.py and tests/test_blochjvp_gpu.py; not collected), vectorised over the (frequency, position) points and
the directions, in float64 or np.longdouble.  The model, its per-sample quantities (Setup), the rotation (_rot) and its derivative
(_drot) are those of tests/blochgrad_ref.py, loaded by path.

Per point and sample t the forward step is m_t = D_t R_t m_{t-1} + c_t.  Along a b1 direction v and an m0 direction dm_0:
    dm_t = D_t (R_t dm_{t-1} + dR_t[dn_t] m_{t-1}),   dn_t = (dnx, dny, 0),
    dnx = ((-(Re v_t s)) gamma) dt_t,  dny = ((Im v_t s) gamma) dt_t          (as rotx / roty are formed from b1)
and, with n.dn = nx dnx + ny dny, sp = sin(phi/2)/phi and D = (d sp / d phi) / phi, dR is _drot along
    d ar = -(sp/2)(n.dn),  d ai = -nz D (n.dn),  d br = ny D (n.dn) + sp dny,  d bi = -nx D (n.dn) - sp dnx
c_t has no tangent.  The primal is stepped with blochgrad_ref.forward's operations, so it has that function's bits."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("blochgrad_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "blochgrad_ref.py"))
_grad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_grad)
forward, vjp, vjp_scaled, gamma_of, intervals = _grad.forward, _grad.vjp, _grad.vjp_scaled, _grad.gamma_of, _grad.intervals
bound_b1, bound_m0, batch = _grad.bound_b1, _grad.bound_m0, _grad.batch
SCALES, TOL, GAMMA_H1, _grid = _grad.SCALES, _grad.TOL, _grad.GAMMA_H1, _grad._grid


def _dm0(dm0, K, nf, npos, dtype):
    if dm0 is None:
        return [np.zeros((K, nf, npos), dtype=dtype) for _ in range(3)]
    return [np.broadcast_to(np.asarray(d, dtype=np.float64), (K, nf, npos)).astype(dtype) for d in dm0]


def jvp(b1, gr, tp, t1, t2, df, pos, gamma, s, m0, v, dm0=None, dtype=np.float64):
    """((mx, my, mz) each (nf, npos), (dmx, dmy, dmz) each (K, nf, npos)) at scale s for the K directions v (K, n) of b1 and dm0 =
    (dmx0, dmy0, dmz0), each broadcastable to (K, nf, npos) (None: zero), of the initial magnetisation m0"""
    Q = _grad.Setup(b1, gr, tp, t1, t2, df, pos, gamma, s, dtype)
    v = np.asarray(v, dtype=np.complex128).reshape(-1, Q.n)
    K, T = v.shape[0], dtype
    dtl, gl, sl = Q.dt.astype(T), T(gamma), T(s)
    dnx = ((-(v.real.astype(T) * sl)) * gl) * dtl                        # (K, n)
    dny = ((v.imag.astype(T) * sl) * gl) * dtl
    m = _grad._m0(m0, Q.nf, Q.npos, dtype)
    dm = _dm0(dm0, K, Q.nf, Q.npos, dtype)
    for t in range(Q.n):
        (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
        dx, dy = dnx[:, t, None, None], dny[:, t, None, None]
        ndn = Q.rotx[t] * dx + Q.roty[t] * dy                            # (K, 1, 1): nx and ny are the same at every point
        # _drot is linear in the direction of (ar, ai, br, bi): its parts along n.dn, dnx and dny act on m once for all K
        zero = np.zeros_like(sp)
        U = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp / 2, -nz * D, ny * D, -nx * D), m)
        Vx = _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, zero, -sp), m)
        Vy = _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, sp, zero), m)
        R = _grad._rot(ar, ai, br, bi)
        a, b = _grad._mat_vec(R, dm), [ndn * U[i] + dx * Vx[i] + dy * Vy[i] for i in range(3)]
        dm = [Q.e2[t] * (a[0] + b[0]), Q.e2[t] * (a[1] + b[1]), Q.e1[t] * (a[2] + b[2])]
        o = _grad._mat_vec(R, m)
        m = [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + (1 - Q.e1[t])]
    return m, dm


def jvp_scaled(pulse, df, pos, v, scales, m0=None, dm0=None, dtype=np.float64):
    """The tangent of the scale sweep for pulse = (b1, gr, tp, t1, t2, nucleus): ((mx, my, mz) each (S, nf, npos), (dmx, dmy, dmz)
    each (K, S, nf, npos)); m0 and dm0 are the same at every scale"""
    b1, gr, tp, t1, t2, nucleus = pulse
    res = [jvp(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, v, dm0, dtype) for s in scales]
    return (tuple(np.stack([r[0][c] for r in res]) for c in range(3)),
            tuple(np.stack([r[1][c] for r in res], 1) for c in range(3)))


def directions(pulses, dfs, dps, K, seed=23):
    """Per pulse K directions v ~ (N(0,1) + i N(0,1)) max|b1| of shape (K, n) and dm0 ~ N(0,1), a triple of (K, nf, npos) arrays,
    drawn direction by direction: the first directions do not depend on K"""
    vs, dms = [], []
    for q, (p, df, dp) in enumerate(zip(pulses, dfs, dps)):
        rng = np.random.default_rng([seed, q])
        n, nf, npos = len(p[0]), len(df), np.shape(dp)[0]
        v, d = np.zeros((K, n), dtype=np.complex128), np.zeros((3, K, nf, npos))
        for k in range(K):
            v[k] = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(p[0]).max()
            d[:, k] = rng.standard_normal((3, nf, npos))
        vs.append(v)
        dms.append(tuple(d))
    return vs, dms


def cases(shared, K):
    """blochgrad_ref.batch(shared) plus K directions per pulse: (pulses, dfs, dps, m0s, cots, vs, dm0s)"""
    pulses, dfs, dps, m0s, cots = batch(shared)
    vs, dms = directions(pulses, dfs, dps, K)
    return pulses, dfs, dps, m0s, cots, vs, dms


def bound_jvp(pulse, v, dm0, scales):
    """Per entry of direction k, (K, nf, npos): 1e-12 (max|s| gamma sum_t dt_t |v_t| + (|dmx_0| + |dmy_0| + |dmz_0|) at that point).
    dR[dn] has norm at most |dn|, R and D have norm at most 1 and |m| <= 1 because |m0| <= 1, so the first term bounds the size of
    what the b1 direction contributes and the second what the m0 direction does; 1e-12 is the forward tolerance of the Bloch tests."""
    v = np.asarray(v).reshape(-1, len(pulse[0]))
    drive = max(abs(s) for s in scales) * gamma_of(pulse[5]) * (intervals(pulse) * np.abs(v)).sum(1)          # (K,)
    size = 0.0 if dm0 is None else np.abs(dm0[0]) + np.abs(dm0[1]) + np.abs(dm0[2])
    return TOL * (drive[:, None, None] + size)


def identity_tol(pulse, cot, v, dm0, scales):
    """The tolerance of sum cot . dm = Re sum conj(g) v + sum gm0 . dm_0 for one direction v (n,), dm0 a triple of (nf, npos) (or
    None), cot = (cmx, cmy, cmz) each (S, nf, npos): sum_t bound_b1_t |v_t| + bound_m0 sum|dm_0| + sum |cot| bound_jvp, the two
    sides' own bounds (the sums over the pulse's points and scales)"""
    S = len(scales)
    bj = bound_jvp(pulse, v, None if dm0 is None else tuple(np.asarray(d)[None] for d in dm0), scales)[0]
    left = float(sum((np.abs(c) * bj).sum() for c in cot))
    dsum = 0.0 if dm0 is None else S * float(sum(np.abs(d).sum() for d in dm0))
    return float((bound_b1(pulse, cot, scales) * np.abs(v)).sum()) + bound_m0(cot) * dsum + left
