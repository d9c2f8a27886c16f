"""NumPy restatement of the adjoint of the Bloch simulator's steady state (k_bloch_batch, mode 1) with respect to b1, the gradient
waveform gr and the off-resonance df (helper of tests/test_blochssg_cpu.py and tests/test_blochssg_gpu.py; not collected), in
float64 or np.longdouble.  Pass 0, the adjugate and the model are those of tests/blochss_ref.py, the positions and the transient
bounds those of tests/blochgradg_ref.py, both loaded by path.

F(m) = A m + B, M = F(M), so dM = (I - A)^-1 dF|_{m0 = M} for any parameter of the period.  For a cotangent c of M, lambda =
(I - A)^-T c, and with dz_t(f, p) = (D lambda_t)' (dR_t / d rotz) m_{t-1} on the sweep started from m0 = M with the end cotangent
lambda, the derivative of R taken through all four Cayley-Klein parameters as blochgradg_ref.vjp_gr takes it (not the device's
closed form),
    dL/dg_{t,a}  = -(gamma dt_t) sum_{f,p} pos_{p,a} dz_t(f, p)        (summed over the scales without a factor)
    dL/ddf(f, p) = -sum_t (TWOPI dt_t) dz_t(f, p)                      (per scale)
The sweeps are restated here rather than called, as blochss_ref restates them: blochgradg_ref.vjp_gr takes m0 and the cotangents as
float64, which would round the long-double M and lambda.

Bounds, with kappa = blochss_ref.kappa.  b1: blochss_ref.bound_b1; M: blochss_ref.bound_m; gr: blochgradg_ref.bound_gr times
kappa; df: blochgradg_ref.bound_df times kappa^2.  The powers follow blochss_ref's rule: the first power, raised to the second where
the float64 reference does not stay within a hundredth of the bound of its long-double twin.  Worst shares of the float64 reference
against its long-double twin on the eight periods of blochss_ref.batch (both grids) and the four of batch_sub(), scales (1, 0,
0.9), as tests/test_blochssg_cpu.py measures them: gr with the first power 5.1e-5 (n = 256, 3 x 5 points); df with the first power
2.6e-2 (n = 600, 3 x 200 points, kappa 2001), which breaks the hundredth, and with the second power 1.3e-5 there and 1.7e-5 at most
(n = 2, kappa 4.5); b1 1.9e-3 and M 6.4e-5, as in blochss_ref.  So gr keeps the first power and df takes the second.  Where a gr
bound is zero (the positions lack the axis, or the grid is position 0 alone) the result is
exactly zero in both dtypes."""
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ss = _load("blochss_ref")
gg = _load("blochgradg_ref")
_grad = ss._grad
SCALES, POINTS, TOL = ss.SCALES, ss.POINTS, ss.TOL
kappa, bound_m, bound_b1 = ss.kappa, ss.bound_m, ss.bound_b1


def ss_vjp_gr(pulse, df, pos, s, cot, dtype=np.float64):
    """(grad_b1 (n,), grad_gr (n, 3), grad_df (nf, npos), M as three (nf, npos) arrays) at scale s for cot = (cmx, cmy, cmz), each
    (nf, npos); grad_b1 carries the factor s, grad_gr does not"""
    Q = ss._setup(pulse, df, pos, s, dtype)
    inv, M = ss._steady(Q)
    c = [np.asarray(v).reshape(Q.nf, Q.npos).astype(dtype) for v in cot]
    lam = _grad._mat_vec(inv, c, transpose=True)
    m, traj = M, []
    for t in range(Q.n):
        traj.append(m)
        o = _grad._mat_vec(_grad._rot(*Q.ck(t)[0]), m)
        m = [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + (1 - Q.e1[t])]
    g = np.zeros(Q.n, dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
    g3 = np.zeros((Q.n, 3), dtype=dtype)
    gdf = np.zeros((Q.nf, Q.npos), dtype=dtype)
    p3 = gg.positions(pos).astype(dtype)
    for t in range(Q.n - 1, -1, -1):
        (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
        dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
        mp = traj[t]
        gxy = []
        for p, eb, ec in ((nx, 0, -1), (ny, 1, 0)):                   # as blochss_ref.ss_vjp
            dsp = D * p
            w = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp * p / 2, -nz * dsp, ny * dsp + eb * sp, -nx * dsp + ec * sp), mp)
            gxy.append((dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]).sum())
        f = dtype(s) * dtype(Q.gamma) * dtype(Q.dt[t])
        g[t] = -f * gxy[0] + 1j * (f * gxy[1])
        dsp = D * nz                                                  # as blochgradg_ref.vjp_gr
        w = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp * nz / 2, -nz * dsp - sp, ny * dsp, -nx * dsp), mp)
        dz = dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]               # (nf, npos)
        fg = dtype(Q.gamma) * dtype(Q.dt[t])
        for a in range(3):
            g3[t, a] = -fg * (dz * p3[None, :, a]).sum()
        gdf -= (dtype(_grad.TWOPI_REF) * dtype(Q.dt[t])) * dz
        lam = _grad._mat_vec(_grad._rot(ar, ai, br, bi), dl, transpose=True)
    return g, g3, gdf, M


def ss_vjp_gr_scaled(pulse, df, pos, cot, scales, dtype=np.float64):
    """The adjoint of the scale sweep, cot = (cmx, cmy, cmz), each (S, nf, npos): (grad_b1 (n,), grad_gr (n, 3), grad_df (S, nf,
    npos), (mx, my, mz) each (S, nf, npos)); b1 and gr summed over the scales"""
    grad, g3, gd, Ms = 0, 0, [], []
    for k, s in enumerate(scales):
        g, a, d, M = ss_vjp_gr(pulse, df, pos, s, [c[k] for c in cot], dtype)
        grad, g3 = grad + g, g3 + a
        gd.append(d)
        Ms.append(M)
    return grad, g3, np.stack(gd), tuple(np.stack([m[c] for m in Ms]) for c in range(3))


def bound_gr(pulse, pos, cot, k):
    """(n, 3): blochgradg_ref.bound_gr times kappa; zero where the positions lack the axis or the grid is position 0 alone"""
    return gg.bound_gr(pulse, pos, cot) * k


def bound_df(pulse, cot, k):
    """(S, nf, npos): blochgradg_ref.bound_df times kappa^2"""
    return gg.bound_df(pulse, cot) * (k * k)


# ---- further cases: the device walks a group of 8 samples in sub-groups of 3, so periods of 2 .. 5 samples make every remainder of
# a sub-group occur in a group that is not full ----------------------------------------------------------------------------------
SUB_LENGTHS = [2, 3, 4, 5]
_sub = []


def batch_sub():
    """Four periods of 2 .. 5 samples in blochss_ref.batch's manner: (pulses, dfs, dps, cots).  q even: tp a scalar, the pulse fills
    the period; q odd: per-sample intervals, the last sample a zero-b1 dead time of four times the rest.  T1 / period is 4, 30, 300
    and 1000; each has its own grid POINTS[(q + 1) % 4] with 3 - q % 3 position axes against 1 + q % 3 gradient axes."""
    if _sub:
        return _sub[0]
    rng = np.random.default_rng(23)
    pulses, dfs, dps, cots = [], [], [], []
    for q, n in enumerate(SUB_LENGTHS):
        nucleus = ("C-13", "H-1", 10000.0)[q % 3]
        gamma = ss.gamma_of(nucleus)
        odd = q % 2 == 1
        nrf = n - 1 if odd else n
        dur = max(nrf, 4) * (4e-6 + 2e-6 * q)
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * ((0.3, 1.0, np.pi / 2, 2.0)[q] / (gamma * dur))
        if n >= 4:
            b1[n // 3] = 0.0
        ax = 1 + q % 3
        gr = rng.uniform(0.5, 1.5, (n, ax)) * 0.1 * (ss.GAMMA_H1 / gamma)
        if odd:
            tp = (dur / nrf) * (1.0 + 0.2 * (-1.0) ** np.arange(n) + 0.05 * rng.uniform(-1, 1, n))
            b1[-1], gr[-1] = 0.0, 0.0
            tp[-1] = 4.0 * tp[:-1].sum()
            tr = float(tp.sum())
        else:
            tp, tr = dur / n, dur
        t1 = (4.0, 30.0, 300.0, 1000.0)[q] * tr
        pulses.append((b1, gr, tp, t1, t1 / (2.0 + q), nucleus))
        nf, npos = POINTS[(q + 1) % 4]
        dfs.append(ss._grid(nf, 200.0))
        dps.append(np.stack([ss._grid(npos, 2.0) * (1.0 - 0.3 * a) for a in range(3 - q % 3)], 1))
        cots.append(tuple(rng.standard_normal((3, len(SCALES), nf, npos))))
    _sub.append((pulses, dfs, dps, cots))
    return _sub[0]
