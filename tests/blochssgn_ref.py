"""NumPy restatement of the least-squares products of the Bloch simulator's steady state (helper of tests/test_blochssgn_cpu.py and
tests/test_blochssgn_gpu.py; not collected), vectorised over the (frequency, position) points and the directions, in float64 or
np.longdouble.  The model, pass 0 and the inverse (_steady) and kappa are those of tests/blochss_ref.py, loaded by path.

With M_s = (I - A_s)^-1 B_s the steady state of the period at scale s, inv = (I - A_s)^-1, weights w = (wx, wy, wz) >= 0 and targets
t = (tx, ty, tz) per (scale, frequency, position) point:
    L   = 1/2 sum over the scales and points of sum_c w_c (M_c - t_c)^2
    g   = sum_s s J_s' W_s (M_s - t_s) = dL/dRe b1 + i dL/dIm b1                  (lsq)
          c = w (M - t), lambda = inv' c, then the transient adjoint from m0 = M with the end cotangent lambda
    H v = sum_s s J_s' W_s J_s (s v),  J_s = d M_s / d (s b1)                     (gn)
          d = the transient tangent from m0 = M with dm0 = 0 along v, dM = inv d, c = w dM, lambda = inv' c, the same reverse sweep
The sweeps are restated here (_forward, _reverse; products runs them) rather than called, so that nothing is rounded to float64 on the way
and the long-double reference is long double throughout.  tests/test_blochssgn_cpu.py pins lsq and gn to blochss_ref.ss_vjp_scaled
of the residual and to ss_jvp -> weights -> ss_vjp_scaled.

Bounds of the device comparison.  They compose DESIGN 8t's through the seed as blochgn_ref composes 8p's.  With k = kappa of the
pulse (the largest ||inv||_2 over its points and scales, floored at 1): the steady state's adjoint with an exact cotangent c is
within blochss_ref.bound_b1(pulse, c, scales, k) = 1e-12 k max|s| gamma dt_t sum|c|; it is linear in c, c -> lambda = inv' c has
norm at most k and the reverse sweep norm at most max|s| gamma dt_t per b1 entry, so an error e of the cotangent adds at most
k max|s| gamma dt_t sum|e|.
    g, per b1 entry t:  |e_c| <= w_c bound_m(k), bound_m = 1e-12 k^2 the bound of an entry of M:
                        bound_b1(pulse, c_ref, scales, k) + k max|s| gamma dt_t bound_m(k) sum (wx + wy + wz)
    H v:                |e_c| <= w_c bound_jvp (blochss_ref.bound_jvp = 1e-12 k^2 B_v, B_v = max|s| gamma sum_t dt_t |v_t|):
                        bound_b1(pulse, W dM_ref, scales, k) + k max|s| gamma dt_t bound_jvp(k) sum (wx + wy + wz)
    L:                  d(1/2 w r^2) = w r dr with |dr| <= bound_m(k), plus the order of the sum over the points:
                        bound_m(k) sum w_c |M_c - t_c| + 1e-13 sum w_c (M_c - t_c)^2
All sums run over the pulse's points and scales.  The powers of kappa are this derivation, not a measurement.

Worst shares of the float64 reference against its long-double twin over blochss_ref.batch's sixteen cases (both grid choices),
measured on the CPU before any device run: 6.8e-6 of the bound of L, 3.2e-7 of g's and 1.1e-6 of H v's, each on a kappa = 4.5 or
8.5 case.  The seed's term carries kappa^3 and dominates both gradient bounds at large kappa (at kappa = 5001 the shares are 2.6e-15
and 2.4e-16): against the first term alone, bound_b1 of the exact cotangent, the float64 reference reaches 5.1e-4 (g) and 5.6e-3
(H v).  The derivation needs every factor -- an error of M or dM of its full bound in every weighted entry goes through inv' (k) --
so the powers stay; tests/test_blochssgn_cpu.py holds the float64 reference within a hundredth of each on every case."""
import functools
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("blochss_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "blochss_ref.py"))
ssref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ssref)
_grad = ssref._grad
_setup, _steady, kappa, batch, directions = ssref._setup, ssref._steady, ssref.kappa, ssref.batch, ssref.directions
gamma_of, intervals, bound_m, bound_b1 = ssref.gamma_of, ssref.intervals, ssref.bound_m, ssref.bound_b1
SCALES, TOL, _grid = ssref.SCALES, ssref.TOL, ssref._grid


def planes(tri, S, nf, npos, dtype=np.float64):
    """A triple of weights or targets, each entry (S, nf, npos), (nf, npos) or a scalar -> (3, S, nf, npos)"""
    return np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (S, nf, npos)) for v in tri]).astype(dtype)


def _rot(Q, t):
    """The rotation of sample t, kept: the forward and the reverse sweep ask for the same one"""
    if t not in Q.rot:
        Q.rot[t] = _grad._rot(*Q.ck(t)[0])
    return Q.rot[t]


def _step(Q, t, m):
    o = _grad._mat_vec(_rot(Q, t), m)
    return [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + (1 - Q.e1[t])]


def _uvw(Q, t, m):
    """(U, Vx, Vy) of sample t at the state m before it: dR[dn] m = (n . dn) U + dnx Vx + dny Vy (sim_dev.h BlochJvpShared)"""
    (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
    zero = np.zeros_like(sp)
    return (_grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp / 2, -nz * D, ny * D, -nx * D), m),
            _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, zero, -sp), m),
            _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, sp, zero), m))


def _forward(Q, s, v, M):
    """(trajectory, (U, Vx, Vy) per sample, d (3 x (K, nf, npos)) or None): blochss_ref.ss_jvp's sweep from M with dm0 = 0 along the
    K directions v (K, n); v None: the trajectory and the derivative vectors alone"""
    T = Q.dtype
    dm = None
    if v is not None:
        dtl, gl, sl = Q.dt.astype(T), T(Q.gamma), T(s)
        dnx = ((-(v.real.astype(T) * sl)) * gl) * dtl
        dny = ((v.imag.astype(T) * sl) * gl) * dtl
        dm = [np.zeros((v.shape[0], Q.nf, Q.npos), dtype=T) for _ in range(3)]
    m, traj, uvw = M, [], []
    for t in range(Q.n):
        traj.append(m)
        U, Vx, Vy = _uvw(Q, t, m)
        uvw.append((U, Vx, Vy))
        if v is not None:
            dx, dy = dnx[:, t, None, None], dny[:, t, None, None]
            ndn = Q.rotx[t] * dx + Q.roty[t] * dy
            a, b = _grad._mat_vec(_rot(Q, t), dm), [ndn * U[i] + dx * Vx[i] + dy * Vy[i] for i in range(3)]
            dm = [Q.e2[t] * (a[0] + b[0]), Q.e2[t] * (a[1] + b[1]), Q.e1[t] * (a[2] + b[2])]
        m = _step(Q, t, m)
    return traj, uvw, dm


def _reverse(Q, s, uvw, lam):
    """The reverse recursion of blochss_ref.ss_vjp from the end cotangent lam = three arrays (..., nf, npos) in Q's dtype: the
    gradient (..., n), the factor s of the chain rule through s b1 included.  d m_t / d rotx = nx U + Vx and d m_t / d roty = ny U +
    Vy with the forward sweep's (U, Vx, Vy) at the state before the sample: ss_vjp's dR m, by linearity of dR in its direction."""
    dtype = Q.dtype
    g = np.zeros(lam[0].shape[:-2] + (Q.n,), dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
    for t in range(Q.n - 1, -1, -1):
        nx, ny, _ = Q.ck(t)[3]
        U, Vx, Vy = uvw[t]
        dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
        gxy = []
        for p, V in ((nx, Vx), (ny, Vy)):
            w = [p * U[i] + V[i] for i in range(3)]
            gxy.append((dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]).sum((-2, -1)))
        f = dtype(s) * dtype(Q.gamma) * dtype(Q.dt[t])
        g[..., t] = -f * gxy[0] + 1j * (f * gxy[1])
        lam = _grad._mat_vec(_rot(Q, t), dl, transpose=True)
    return g


def _period(pulse, df, pos, s, dtype):
    """(Q, inv, M) of the period at scale s; Q.ck keeps what it has computed: pass 0 and the two sweeps ask for the same samples"""
    Q = _setup(pulse, df, pos, s, dtype)
    Q.ck, Q.rot = functools.lru_cache(maxsize=None)(Q.ck), {}
    inv, M = _steady(Q)
    return Q, inv, M


def products(pulse, df, pos, targets, weights, v, scales, dtype=np.float64):
    """lsq and gn in one pass over each scale's period (they share pass 0, the trajectory and the reverse sweep, whose seeds are
    stacked): (L, g, info of lsq, h, info of gn); targets None: no lsq (L, g, info None); v None: no gn.  Both infos also hold
    kappa = the largest ||inv||_2 met, floored at 1 (blochss_ref.kappa when dtype is np.longdouble).  A scale s = 0 is not
    swept: every entry of its gradient carries the factor s gamma dt_t = 0; its loss and its share of the bounds' sums count."""
    n = len(np.ravel(pulse[0]))
    if v is not None:
        v = np.asarray(v, dtype=np.complex128).reshape(-1, n)
    K = 0 if v is None else len(v)
    L, g, h, w, tg, Ms, kap = dtype(0), 0, 0, None, None, [], 1.0
    li, hi = dict(N=0.0, W=0.0, A=0.0, Q=0.0), dict(N=np.zeros(K), W=0.0, E=np.zeros(K, dtype=dtype))
    for k, s in enumerate(scales):
        Q, inv, M = _period(pulse, df, pos, s, dtype)
        if w is None:
            w = planes(weights, len(scales), Q.nf, Q.npos, dtype)
            tg = None if targets is None else planes(targets, len(scales), Q.nf, Q.npos, dtype)
        seeds, swept = [], s != 0
        norm = np.stack([np.stack([inv[i][j] for j in range(3)], -1) for i in range(3)], -2).astype(np.float64)      # (nf, npos, 3, 3)
        kap = max(kap, float(np.linalg.norm(norm, 2, axis=(-2, -1)).max()))
        if tg is not None:
            r = [M[c] - tg[c, k] for c in range(3)]
            cot = [w[c, k] * r[c] for c in range(3)]
            L = L + sum((w[c, k] * r[c] * r[c]).sum() for c in range(3)) / 2
            li["N"] += float(sum(np.abs(c).sum() for c in cot))
            li["Q"] += float(sum((w[c, k] * r[c] * r[c]).sum() for c in range(3)))
            seeds.append([c[None] for c in cot])
        if not swept and K:                                                # dM = 0 along every direction: s v = 0
            zero = np.zeros((K, Q.nf, Q.npos), dtype=dtype)
            uvw, d = None, [zero, zero, zero]
        else:
            _, uvw, d = _forward(Q, s, v if K else None, M)
        if K:
            dM = _grad._mat_vec(inv, d)
            cot = [w[c, k] * dM[c] for c in range(3)]                      # (K, nf, npos)
            hi["N"] += np.array(sum(np.abs(c).sum((-2, -1)) for c in cot), dtype=np.float64)
            hi["E"] = hi["E"] + sum((w[c, k] * dM[c] * dM[c]).sum((-2, -1)) for c in range(3))
            seeds.append(cot)
        cot = [np.concatenate([sd[c] for sd in seeds]) for c in range(3)]
        if swept:
            out = _reverse(Q, s, uvw, _grad._mat_vec(inv, cot, transpose=True))
        else:
            out = np.zeros((len(cot[0]), Q.n), dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
        if tg is not None:
            g, out = g + out[0], out[1:]
        if K:
            h = h + out
        Ms.append(M)
    li["A"], li["W"], hi["W"] = li["N"], float(w.sum()), float(w.sum())
    li["kappa"] = hi["kappa"] = kap                                        # blochss_ref.kappa when dtype is np.longdouble
    li["M"] = tuple(np.stack([m[c] for m in Ms]) for c in range(3))
    if targets is None:
        return None, None, None, h, hi
    return L, g, li, (h if K else None), (hi if K else None)


def lsq(pulse, df, pos, targets, weights, scales, dtype=np.float64, parts=False):
    """(L, g (n,)) of the period pulse = (b1, gr, tp, t1, t2, nucleus); with parts also dict(N = sum|c| of the cotangent c = w (M -
    t), W = sum w, A = sum w |M - t|, Q = sum w (M - t)^2, M = (mx, my, mz) each (S, nf, npos)) for the bounds"""
    L, g, info, _, _ = products(pulse, df, pos, targets, weights, None, scales, dtype)
    return (L, g, info) if parts else (L, g)


def gn(pulse, df, pos, v, weights, scales, dtype=np.float64, parts=False):
    """H v (K, n) for the directions v (K, n) (or (n,) -> (n,)); with parts also dict(N = sum|c| of the cotangent c = w dM per
    direction (K,), W = sum w, E = sum w dM^2 per direction (K,): Re <v, H v>)"""
    _, _, _, h, info = products(pulse, df, pos, None, weights, v, scales, dtype)
    h = h[0] if np.ndim(v) == 1 else h
    return (h, info) if parts else h


def _drive(pulse, scales):
    """max|s| gamma dt_t per b1 entry (n,)"""
    return max(abs(s) for s in scales) * gamma_of(pulse[5]) * intervals(pulse)


def bound_g(pulse, info, scales, k):
    """Per b1 entry (n,)"""
    return _drive(pulse, scales) * k * (TOL * info["N"] + bound_m(k) * info["W"])


def bound_h(pulse, v, info, scales, k):
    """Per entry of direction j (K, n)"""
    v = np.asarray(v).reshape(-1, len(pulse[0]))
    bj = ssref.bound_jvp(pulse, v, scales, k)[:, 0, 0]                     # (K,)
    return _drive(pulse, scales)[None, :] * k * (TOL * info["N"] + bj * info["W"])[:, None]


def bound_L(info, k):
    return bound_m(k) * info["A"] + 1e-13 * info["Q"]


def cases(shared, K):
    """blochss_ref.batch(shared) -- eight periods of 1, 7, 8, 9, 255, 256, 257 and 600 samples on grids of 1 x 1, 3 x 5, 1 x 257 and
    3 x 200 points or the shared 3 x 5 grid, kappa from 4.5 to 5001 -- with, per pulse, weights uniform in [0, 1] of which a third
    (of the 3 S nf npos entries) is set to zero, targets uniform in [-1, 1], each a triple of (S, nf, npos) arrays, and K directions
    as blochjvp_ref.directions draws them: (pulses, dfs, dps, targets, weights, vs)"""
    pulses, dfs, dps, _ = batch(shared)
    vs, _ = directions(pulses, dfs, dps, K)
    tgs, wts = [], []
    for q, (df, dp) in enumerate(zip(dfs, dps)):
        rng = np.random.default_rng([37, q])
        shape = (3, len(SCALES), len(df), np.shape(dp)[0])
        w = rng.uniform(0, 1, shape)
        flat = w.reshape(-1)
        flat[rng.permutation(flat.size)[:(flat.size + 2) // 3]] = 0.0
        wts.append(tuple(w))
        tgs.append(tuple(rng.uniform(-1, 1, shape)))
    return pulses, dfs, dps, tgs, wts, vs
