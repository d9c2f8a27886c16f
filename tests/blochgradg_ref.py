"""NumPy restatement of the adjoint of the Bloch simulator with relaxation with respect to b1, the initial magnetisation, the
gradient waveform gr and the off-resonance df (helper of tests/test_blochgradg_cpu.py and tests/test_blochgradg_gpu.py; not
collected), in float64 or np.longdouble.  The forward recursion, the stored trajectory and the b1 / m0 part are those of
tests/blochgrad_ref.py, loaded by path, with the same operations in the same order.

Per point and sample rotz_t = -((gx_t gamma dt_t) x + (gy_t gamma dt_t) y + (gz_t gamma dt_t) z + df (TWOPI dt_t)).  With
dz_t(f, p) = (D lambda_t)' (dR_t / d rotz) m_{t-1}, the derivative of R through all four Cayley-Klein parameters (d cos(phi/2) =
-(sp/2) nz, d sp = D nz, so d ai = -(nz D nz + sp), d br = ny D nz, d bi = -nx D nz),
    dL/dg_{t,a}  = -(gamma dt_t) sum_{f,p} pos_{p,a} dz_t(f, p)        (summed over the scales without a factor)
    dL/ddf(f, p) = -sum_t (TWOPI dt_t) dz_t(f, p)                      (per scale)"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("blochgrad_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "blochgrad_ref.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
TOL = base.TOL


def positions(pos):
    """pos as (npos, 3) float64, missing axes as zeros"""
    pos = np.asarray(pos, dtype=np.float64)
    pos = pos.reshape(-1, 1) if pos.ndim < 2 else pos
    return np.concatenate([pos, np.zeros((pos.shape[0], 3 - pos.shape[1]))], 1)


def vjp_gr(b1, gr, tp, t1, t2, df, pos, gamma, s, m0, cot, dtype=np.float64):
    """(grad_b1 (n,), grad_gr (n, 3), dL/dm0 as three (nf, npos) arrays, grad_df (nf, npos)) at scale s for cot = (cmx, cmy, cmz),
    each (nf, npos); grad_b1 carries the factor s, grad_gr does not"""
    _, traj, Q = base.forward(b1, gr, tp, t1, t2, df, pos, gamma, s, m0, dtype, keep=True)
    lam = [np.asarray(c, dtype=np.float64).reshape(Q.nf, Q.npos).astype(dtype) for c in cot]
    g = np.zeros(Q.n, dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
    gg = np.zeros((Q.n, 3), dtype=dtype)
    gdf = np.zeros((Q.nf, Q.npos), dtype=dtype)
    p3 = positions(pos).astype(dtype)
    for t in range(Q.n - 1, -1, -1):
        (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
        dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
        mp = traj[t]
        gxy = []
        for p, eb, ec in ((nx, 0, -1), (ny, 1, 0)):                   # as blochgrad_ref.vjp
            dsp = D * p
            dR = base._drot(ar, ai, br, bi, -sp * p / 2, -nz * dsp, ny * dsp + eb * sp, -nx * dsp + ec * sp)
            w = base._mat_vec(dR, mp)
            gxy.append((dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]).sum())
        f = dtype(s) * dtype(Q.gamma) * dtype(Q.dt[t])
        g[t] = -f * gxy[0] + 1j * (f * gxy[1])
        dsp = D * nz
        w = base._mat_vec(base._drot(ar, ai, br, bi, -sp * nz / 2, -nz * dsp - sp, ny * dsp, -nx * dsp), mp)
        dz = dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]               # (nf, npos)
        fg = dtype(Q.gamma) * dtype(Q.dt[t])
        for a in range(3):
            gg[t, a] = -fg * (dz * p3[None, :, a]).sum()
        gdf -= (dtype(base.TWOPI_REF) * dtype(Q.dt[t])) * dz
        lam = base._mat_vec(base._rot(ar, ai, br, bi), dl, transpose=True)
    return g, gg, lam, gdf


def vjp_gr_scaled(pulse, df, pos, cot, scales, m0=None, dtype=np.float64):
    """The adjoint of the scale sweep for pulse = (b1, gr, tp, t1, t2, nucleus), cot = (cmx, cmy, cmz), each (S, nf, npos):
    (grad_b1 (n,), grad_gr (n, 3), (gmx, gmy, gmz) each (S, nf, npos), grad_df (S, nf, npos)); b1 and gr summed over the scales"""
    b1, gr, tp, t1, t2, nucleus = pulse
    grad, gg, gm, gd = 0, 0, [], []
    for k, s in enumerate(scales):
        g, g3, l0, d = vjp_gr(b1, gr, tp, t1, t2, df, pos, base.gamma_of(nucleus), s, m0, [c[k] for c in cot], dtype)
        grad, gg = grad + g, gg + g3
        gm.append(l0)
        gd.append(d)
    return grad, gg, tuple(np.stack([l[c] for l in gm]) for c in range(3)), np.stack(gd)


def _weight(cot):
    return np.abs(cot[0]) + np.abs(cot[1]) + np.abs(cot[2])             # (S, nf, npos)


def bound_gr(pulse, pos, cot):
    """(n, 3): 1e-12 gamma dt_t sum_{s,f,p} |pos_{p,a}| (|cmx| + |cmy| + |cmz|): the forward tolerance of the Bloch tests carried
    through the coordinate weight; zero where the positions lack the axis or the grid is position 0 alone: there the result must be
    exactly zero"""
    w = (_weight(cot).sum((0, 1))[:, None] * np.abs(positions(pos))).sum(0)         # (3,)
    return TOL * base.gamma_of(pulse[5]) * base.intervals(pulse)[:, None] * w[None, :]


def bound_df(pulse, cot):
    """(S, nf, npos): 1e-12 TWOPI (sum_t dt_t) (|cmx| + |cmy| + |cmz|)"""
    return TOL * base.TWOPI_REF * float(base.intervals(pulse).sum()) * _weight(cot)


# ---- further cases of tests/test_blochgradg_gpu.py: the device walks a group of 8 samples in sub-groups of 3, so lengths 2 .. 5
# make every remainder of a sub-group occur in a group that is not full -----------------------------------------------------------
SUB_LENGTHS = [2, 3, 4, 5]


def batch_sub():
    """Four pulses of 2 .. 5 samples in blochgrad_ref.batch's manner: (pulses, dfs, dps, m0s, cots) on grids of their own"""
    rng = np.random.default_rng(12)
    pulses, dfs, dps, m0s, cots = [], [], [], [], []
    for q, n in enumerate(SUB_LENGTHS):
        nucleus = ("C-13", "H-1", 10000.0)[q % 3]
        gamma = base.gamma_of(nucleus)
        dur = n * (4e-6 + 2e-6 * q)
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * ((0.3, 1.0, np.pi / 2, 2.0)[q] / (gamma * dur))
        if n >= 3:
            b1[n // 3] = 0.0
        ax = 1 + q % 3
        gr = rng.uniform(0.5, 1.5, (n, ax)) * 0.1 * (base.GAMMA_H1 / gamma)
        tp = dur / n if q % 2 == 0 else (dur / n) * (1.0 + 0.2 * (-1.0) ** np.arange(n))
        pulses.append((b1, gr, tp, 0.5 + 0.1 * q, (2.0 + q) * dur, nucleus))
        nf, npos = base.POINTS[(q + 1) % 4]
        dfs.append(base._grid(nf, 200.0))
        dps.append(np.stack([base._grid(npos, 2.0) * (1.0 - 0.3 * a) for a in range(3 - q % 3)], 1))
        v = rng.standard_normal((3, nf, npos))
        v *= rng.uniform(0, 1, (nf, npos)) / np.sqrt((v * v).sum(0))
        m0s.append(tuple(v))
        cots.append(tuple(rng.standard_normal((3, len(base.SCALES), nf, npos))))
    return pulses, dfs, dps, m0s, cots
