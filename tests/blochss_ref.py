"""NumPy restatement of the steady state of the Bloch simulator with relaxation (k_bloch_batch, mode 1) and of its adjoint and
tangent with respect to b1 (helper of tests/test_blochss_cpu.py and tests/test_blochss_gpu.py; not collected), vectorised over the
(frequency, position) points, in float64 or np.longdouble.  The model, its per-sample quantities (Setup), the rotation (_rot) and
its derivative (_drot) are those of tests/blochgrad_ref.py, the directions those of tests/blochjvp_ref.py, both loaded by path.

One period is F(m) = A m + B with A = prod D_t R_t; pass 0 propagates (A, B) in the kernel's order (A <- D R A column by column,
B <- D R B + c) and M = (I - A)^-1 B by the adjugate (the reference's invmat).  F(M) = M, so dM = (I - A)^-1 dF at m0 = M:
    adjoint: lambda = (I - A)^-T c, then the transient adjoint of blochgrad_ref from m0 = M with the end cotangent lambda;
    tangent: d = the transient tangent of blochjvp_ref from m0 = M with dm0 = 0, then dM = (I - A)^-1 d.
The sweeps are restated here rather than called: blochgrad_ref.vjp and blochjvp_ref.jvp take m0 and the cotangents as float64, which
would round the long-double M and lambda.

Bounds.  kappa = the largest ||(I - A)^-1||_2 over the pulse's points and scales, from the long-double run, floored at 1 (about
T1 / TR).  The b1 gradient: blochgrad_ref.bound_b1 times kappa.  M: 1e-12 kappa^2 per entry; a tangent entry: 1e-12 kappa^2 max|s|
gamma sum_t dt_t |v_t| (blochjvp_ref.bound_jvp times kappa^2).  1e-12 is the forward tolerance of the Bloch tests and kappa the
amplification of (I - A)^-1.  The second power for M and the tangent is the worst case of the perturbation argument (an error
of relative size e in I - A moves (I - A)^-1 by kappa e times itself): with the first power the float64 reference is within a
hundredth of its long-double twin on every case but the 600-sample period, where it reaches 1.8e-2 of the bound for M and 1.1e-1
for the tangent at kappa = 2001 (the rounding of A over 600 products, not kappa, sets the constant).  The gradient keeps the first
power: 1.9e-3 at most.  tests/test_blochss_cpu.py holds the float64 reference within a hundredth of each on every case."""
import functools
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_jvp = _load("blochjvp_ref")
_grad = _jvp._grad
gamma_of, intervals, forward, _grid, directions = _grad.gamma_of, _grad.intervals, _grad.forward, _grad._grid, _jvp.directions
GAMMA_H1, GAMMA_C13, TOL = _grad.GAMMA_H1, _grad.GAMMA_C13, _grad.TOL
SCALES = [1.0, 0.0, 0.9]
LENGTHS = [1, 7, 8, 9, 255, 256, 257, 600]          # around the group of 8 samples and the 256-sample tile
POINTS = [(1, 1), (3, 5), (1, 257), (3, 200)]       # one point, a partial chunk, more than one chunk
KAPPA_CAP = 1e4


def _setup(pulse, df, pos, s, dtype):
    b1, gr, tp, t1, t2, nucleus = pulse
    return _grad.Setup(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, dtype)


def pass0(Q):
    """(A, B) of the period over the points: A[i][j] and B[i], each (nf, npos), in the kernel's order"""
    one, zero = np.ones((Q.nf, Q.npos), dtype=Q.dtype), np.zeros((Q.nf, Q.npos), dtype=Q.dtype)
    A = [[one if i == j else zero for j in range(3)] for i in range(3)]
    B = [zero, zero, zero]
    for t in range(Q.n):
        R = _grad._rot(*Q.ck(t)[0])
        e1, e2 = Q.e1[t], Q.e2[t]
        cols = []
        for j in range(3):
            o = _grad._mat_vec(R, [A[0][j], A[1][j], A[2][j]])
            cols.append([e2 * o[0], e2 * o[1], e1 * o[2]])
        A = [[cols[j][i] for j in range(3)] for i in range(3)]
        o = _grad._mat_vec(R, B)
        B = [e2 * o[0], e2 * o[1], e1 * o[2] + (1 - e1)]
    return A, B


def inverse(A):
    """(I - A)^-1 by the adjugate, inv[i][j] over the points (the kernel's inv[i + 3 j])"""
    K = [[(1 if i == j else 0) - A[i][j] for j in range(3)] for i in range(3)]
    k = lambda e: K[e % 3][e // 3]                                       # the kernel's column-major K[e]
    c00, c01, c02 = k(4) * k(8) - k(7) * k(5), k(7) * k(2) - k(1) * k(8), k(1) * k(5) - k(4) * k(2)
    det = k(0) * c00 + k(3) * c01 + k(6) * c02
    flat = [c00 / det, c01 / det, c02 / det,
            (k(6) * k(5) - k(3) * k(8)) / det, (k(0) * k(8) - k(6) * k(2)) / det, (k(3) * k(2) - k(0) * k(5)) / det,
            (k(3) * k(7) - k(6) * k(4)) / det, (k(6) * k(1) - k(0) * k(7)) / det, (k(0) * k(4) - k(3) * k(1)) / det]
    return [[flat[i + 3 * j] for j in range(3)] for i in range(3)]


def _steady(Q):
    A, B = pass0(Q)
    inv = inverse(A)
    return inv, _grad._mat_vec(inv, B)


def ss(pulse, df, pos, s=1.0, dtype=np.float64):
    """The steady state (mx, my, mz) of the period at scale s, each (nf, npos)"""
    return _steady(_setup(pulse, df, pos, s, dtype))[1]


def ss_scaled(pulse, df, pos, scales, dtype=np.float64):
    res = [ss(pulse, df, pos, s, dtype) for s in scales]
    return tuple(np.stack([r[c] for r in res]) for c in range(3))


def ss_vjp(pulse, df, pos, s, cot, dtype=np.float64):
    """(dL/dRe b1 + i dL/dIm b1 (n,), M) at scale s for cot = (cmx, cmy, cmz), each (nf, npos); the factor s of the chain rule
    through s b1 is included"""
    Q = _setup(pulse, df, pos, s, dtype)
    inv, M = _steady(Q)
    c = [np.asarray(v).reshape(Q.nf, Q.npos).astype(dtype) for v in cot]
    lam = _grad._mat_vec(inv, c, transpose=True)
    m, traj = M, []
    for t in range(Q.n):
        traj.append(m)
        o = _grad._mat_vec(_grad._rot(*Q.ck(t)[0]), m)
        m = [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + (1 - Q.e1[t])]
    g = np.zeros(Q.n, dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
    for t in range(Q.n - 1, -1, -1):
        (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
        dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
        gxy = []
        for p, eb, ec in ((nx, 0, -1), (ny, 1, 0)):
            dsp = D * p
            w = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp * p / 2, -nz * dsp, ny * dsp + eb * sp, -nx * dsp + ec * sp), traj[t])
            gxy.append((dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]).sum())
        f = dtype(s) * dtype(Q.gamma) * dtype(Q.dt[t])
        g[t] = -f * gxy[0] + 1j * (f * gxy[1])
        lam = _grad._mat_vec(_grad._rot(ar, ai, br, bi), dl, transpose=True)
    return g, M


def ss_vjp_scaled(pulse, df, pos, cot, scales, dtype=np.float64):
    """The adjoint of the scale sweep, cot = (cmx, cmy, cmz), each (S, nf, npos): (grad_b1 (n,) summed over the scales, (mx, my, mz)
    each (S, nf, npos))"""
    grad, Ms = 0, []
    for k, s in enumerate(scales):
        g, M = ss_vjp(pulse, df, pos, s, [c[k] for c in cot], dtype)
        grad = grad + g
        Ms.append(M)
    return grad, tuple(np.stack([m[c] for m in Ms]) for c in range(3))


def ss_jvp(pulse, df, pos, v, scales, dtype=np.float64):
    """((mx, my, mz) each (S, nf, npos), (dmx, dmy, dmz) each (K, S, nf, npos)) for the K directions v (K, n) of b1"""
    Ms, dMs = [], []
    for s in scales:
        Q = _setup(pulse, df, pos, s, dtype)
        vv = np.asarray(v, dtype=np.complex128).reshape(-1, Q.n)
        T = dtype
        dtl, gl, sl = Q.dt.astype(T), T(Q.gamma), T(s)
        dnx = ((-(vv.real.astype(T) * sl)) * gl) * dtl
        dny = ((vv.imag.astype(T) * sl) * gl) * dtl
        inv, M = _steady(Q)
        m, dm = M, [np.zeros((vv.shape[0], Q.nf, Q.npos), dtype=dtype) for _ in range(3)]
        for t in range(Q.n):
            (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
            dx, dy = dnx[:, t, None, None], dny[:, t, None, None]
            ndn = Q.rotx[t] * dx + Q.roty[t] * dy
            zero = np.zeros_like(sp)
            U = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp / 2, -nz * D, ny * D, -nx * D), m)
            Vx = _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, zero, -sp), m)
            Vy = _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, sp, zero), m)
            R = _grad._rot(ar, ai, br, bi)
            a, b = _grad._mat_vec(R, dm), [ndn * U[i] + dx * Vx[i] + dy * Vy[i] for i in range(3)]
            dm = [Q.e2[t] * (a[0] + b[0]), Q.e2[t] * (a[1] + b[1]), Q.e1[t] * (a[2] + b[2])]
            o = _grad._mat_vec(R, m)
            m = [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + (1 - Q.e1[t])]
        Ms.append(M)
        dMs.append(_grad._mat_vec(inv, dm))
    return (tuple(np.stack([m[c] for m in Ms]) for c in range(3)), tuple(np.stack([d[c] for d in dMs], 1) for c in range(3)))


def _kappa(pulse, df, pos, scales):
    k = 1.0
    for s in scales:
        inv, _ = _steady(_setup(pulse, df, pos, s, np.longdouble))
        m = np.stack([np.stack([inv[i][j] for j in range(3)], -1) for i in range(3)], -2).astype(np.float64)      # (nf, npos, 3, 3)
        k = max(k, float(np.linalg.norm(m, 2, axis=(-2, -1)).max()))
    return k


_kappa_cache = {}


def kappa(pulse, df, pos, scales):
    """max over the pulse's points and scales of ||(I - A)^-1||_2, from the long-double run, floored at 1"""
    key = (id(pulse), id(df), id(pos), tuple(scales))
    if key not in _kappa_cache:
        _kappa_cache[key] = (_kappa(pulse, df, pos, scales), pulse, df, pos)       # the objects are kept: their ids stay theirs
    return _kappa_cache[key][0]


def bound_m(k):
    return TOL * k * k


def bound_b1(pulse, cot, scales, k):
    return _grad.bound_b1(pulse, cot, scales) * k


def bound_jvp(pulse, v, scales, k):
    """(K, 1, 1): per entry of direction k"""
    return _jvp.bound_jvp(pulse, v, None, scales) * (k * k)


# ---- the cases of tests/test_blochss_gpu.py's comparison with this reference (tests/test_blochss_cpu.py checks the reference itself
# on the same cases) --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(shared):
    """Eight periods: (pulses, dfs, dps, cots).  Pulse q has LENGTHS[q] samples, 1 + q % 3 gradient axes, its own gamma, T1 and T2,
    and for n >= 3 one b1 sample exactly zero.  q even: tp a scalar, the pulse fills the period; q odd: per-sample intervals, the
    last sample a zero-b1 dead time of four times the rest (600 samples: 2 ms of pulse in a period of 6 ms).  T1 / period runs from 4
    to 5000: pulse 3 (8 samples of 10 us and a dead time that fills a period of 6 ms, at T1 = 30 s and T2 = 2 s) is the
    hyperpolarised-like one.  Grids: one of 3 x 5 points shared by all, or
    POINTS[q % 4] per pulse with 1 + q % 3 position axes; df = 0 and position 0 are on every grid.  Cotangents standard normal, (3
    scales, nf, npos)."""
    rng = np.random.default_rng(17)
    t1_over_tr = (4.0, 30.0, 8.0, 5000.0, 300.0, 1000.0, 3000.0, 2000.0)
    pulses, dfs, dps, cots = [], [], [], []
    for q, n in enumerate(LENGTHS):
        nucleus = ("C-13", "H-1", 10000.0)[q % 3]
        gamma = gamma_of(nucleus)
        odd = q % 2 == 1
        nrf = n - 1 if odd else n                                          # samples that carry b1
        dur = 2e-3 if n == 600 else max(nrf, 4) * (4e-6 + 2e-6 * q)
        flip = (0.3, 1.0, np.pi / 2, 2.0, 0.02, np.pi, 1.5, 1.0)[q]
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (flip / (gamma * dur))
        if n >= 3:
            b1[n // 3] = 0.0
        ax = 1 + q % 3
        gr = rng.uniform(0.5, 1.5, (n, ax)) * 0.1 * (GAMMA_H1 / gamma)
        if odd:
            tp = (dur / nrf) * (1.0 + 0.2 * (-1.0) ** np.arange(n) + 0.05 * rng.uniform(-1, 1, n))
            b1[-1], gr[-1] = 0.0, 0.0
            tp[-1] = 2.0 * dur if n == 600 else 6e-3 - tp[:-1].sum() if n == 9 else 4.0 * tp[:-1].sum()
            tr = float(tp.sum())
        else:
            tp, tr = dur / n, dur
        t1 = 30.0 if n == 9 else t1_over_tr[q] * tr
        t2 = 2.0 if n == 9 else t1 / (2.0 + q)
        pulses.append((b1, gr, tp, t1, t2, nucleus))
        nf, npos = (3, 5) if shared else POINTS[q % 4]
        dfs.append(_grid(nf, 200.0))
        dps.append(np.stack([_grid(npos, 2.0) * (1.0 - 0.3 * a) for a in range(ax)], 1))
        cots.append(tuple(rng.standard_normal((3, len(SCALES), nf, npos))))
    if shared:
        dfs, dps = [dfs[0]] * 8, [np.stack([_grid(5, 2.0) * (1.0 - 0.3 * a) for a in range(3)], 1)] * 8
    return pulses, dfs, dps, cots
