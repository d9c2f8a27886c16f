"""NumPy restatement of the Bloch simulator with relaxation as the device steps it (k_bloch_batch, mode 0) and of its adjoint with
respect to b1 and the initial magnetisation (helper of tests/test_blochgrad_cpu.py and tests/test_blochgrad_gpu.py; not collected),
vectorised over the (frequency, position) points, in float64 or np.longdouble.

Forward, per point and sample t: m_t = D_t R_t m_{t-1} + c_t, D_t = diag(e2, e2, e1), c_t = (0, 0, 1 - e1), R_t the rotation by
|n| about n = (rotx, roty, rotz) in the reference's Cayley-Klein form (blochC.c calcrotmat), rotx = ((-(Re b1 s)) gamma) dt, roty =
((Im b1 s) gamma) dt, rotz = -((gx gamma dt) x + (gy gamma dt) y + (gz gamma dt) z + df (TWOPI dt)).  E1 and E2 are the float64
exponentials the host hands the device, in either dtype: they are inputs of the recursion, not part of it.
Adjoint: the trajectory is stored (nothing is inverted: the step is a contraction); with lambda_n = the cotangent of m_n, over the
samples in reverse  dL/drotx_t = sum over the points of (D lambda_t)' (dR_t/drotx) m_{t-1}  (and roty),  lambda_{t-1} = R_t' D_t
lambda_t;  lambda_0 = dL/dm0;  dL/dRe b1_t = -(s gamma dt_t) dL/drotx_t,  dL/dIm b1_t = +(s gamma dt_t) dL/droty_t."""
import numpy as np

GAMMA_C13 = 6726.1
GAMMA_H1 = 26754.0
TWOPI_REF = 6.283185


def gamma_of(nucleus):
    return GAMMA_C13 if nucleus == "C-13" else GAMMA_H1 if nucleus == "H-1" else float(nucleus)


def _rot(ar, ai, br, bi):
    """The nine entries R[i][j] of calcrotmat from the Cayley-Klein parameters"""
    return [[ar * ar - ai * ai - br * br + bi * bi, 2 * ar * ai - 2 * br * bi, 2 * ar * br + 2 * ai * bi],
            [-2 * ar * ai - 2 * br * bi, ar * ar - ai * ai + br * br - bi * bi, 2 * ar * bi - 2 * ai * br],
            [-2 * ar * br + 2 * ai * bi, -2 * ai * br - 2 * ar * bi, ar * ar + ai * ai - br * br - bi * bi]]


def _drot(ar, ai, br, bi, dar, dai, dbr, dbi):
    """The derivative of _rot along (dar, dai, dbr, dbi)"""
    return [[2 * (ar * dar - ai * dai - br * dbr + bi * dbi), 2 * (dar * ai + ar * dai) - 2 * (dbr * bi + br * dbi),
             2 * (dar * br + ar * dbr) + 2 * (dai * bi + ai * dbi)],
            [-2 * (dar * ai + ar * dai) - 2 * (dbr * bi + br * dbi), 2 * (ar * dar - ai * dai + br * dbr - bi * dbi),
             2 * (dar * bi + ar * dbi) - 2 * (dai * br + ai * dbr)],
            [-2 * (dar * br + ar * dbr) + 2 * (dai * bi + ai * dbi), -2 * (dai * br + ai * dbr) - 2 * (dar * bi + ar * dbi),
             2 * (ar * dar + ai * dai - br * dbr - bi * dbi)]]


def _half_sinc(phi):
    """sin(phi/2)/phi and (its derivative)/phi, with the limits 1/2 and -1/24 + phi^2/960 below 1e-4 (tests/simgrad_ref.py)"""
    small = phi < 1e-4
    safe = np.where(small, 1, phi)
    pos = np.where(phi > 0, phi, 1)
    sp = np.where(phi > 0, np.sin(phi / 2) / pos, phi.dtype.type(0.5))
    D = np.where(small, -phi.dtype.type(1) / 24 + phi * phi / 960, (np.cos(safe / 2) / 2 - np.sin(safe / 2) / safe) / (safe * safe))
    return sp, D


def _mat_vec(R, v, transpose=False):
    if transpose:
        return [R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2] for i in range(3)]
    return [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]


class Setup:
    """The per-sample quantities of one pulse at scale s on its grid, in dtype: rotx, roty (n,), rotz (n, nf, npos), e1, e2, dt."""

    def __init__(self, b1, gr, tp, t1, t2, df, pos, gamma, s, dtype):
        b1 = np.asarray(b1, dtype=np.complex128).ravel()
        n = len(b1)
        gr = np.zeros((n, 3)) if gr is None else np.asarray(gr, dtype=np.float64).reshape(n, -1)
        gr = np.concatenate([gr, np.zeros((n, 3 - gr.shape[1]))], 1)
        pos = np.asarray(pos, dtype=np.float64)
        pos = pos.reshape(-1, 1) if pos.ndim < 2 else pos
        pos = np.concatenate([pos, np.zeros((pos.shape[0], 3 - pos.shape[1]))], 1)
        df = np.asarray(df, dtype=np.float64).ravel()
        dt = np.broadcast_to(np.asarray(tp, dtype=np.float64).ravel(), (n,))
        self.n, self.nf, self.npos, self.dtype = n, len(df), pos.shape[0], dtype
        self.dt, self.gamma, self.s = dt, gamma, s
        self.e1, self.e2 = np.exp(-dt / t1).astype(dtype), np.exp(-dt / t2).astype(dtype)
        T = dtype
        dtl, gl, sl = dt.astype(T), T(gamma), T(s)
        self.rotx = ((-(b1.real.astype(T) * sl)) * gl) * dtl
        self.roty = ((b1.imag.astype(T) * sl) * gl) * dtl
        g3 = gr.astype(T) * gl * dtl[:, None]                               # (n, 3)
        p3 = pos.astype(T)
        gp = g3[:, 0, None] * p3[None, :, 0] + g3[:, 1, None] * p3[None, :, 1] + g3[:, 2, None] * p3[None, :, 2]      # (n, npos)
        self.rotz = -(gp[:, None, :] + df.astype(T)[None, :, None] * (T(TWOPI_REF) * dtl)[:, None, None])

    def ck(self, t):
        """(ar, ai, br, bi), sp, D and the axis of sample t over the points"""
        nz = self.rotz[t]
        nx, ny = np.full_like(nz, self.rotx[t]), np.full_like(nz, self.roty[t])
        phi = np.sqrt(nx * nx + ny * ny + nz * nz)
        sp, D = _half_sinc(phi)
        return (np.cos(phi / 2), -nz * sp, ny * sp, -nx * sp), sp, D, (nx, ny, nz)


def _m0(m0, nf, npos, dtype):
    if m0 is None:
        return [np.zeros((nf, npos), dtype=dtype), np.zeros((nf, npos), dtype=dtype), np.ones((nf, npos), dtype=dtype)]
    return [np.broadcast_to(np.asarray(v, dtype=np.float64), (nf, npos)).astype(dtype) for v in m0]


def forward(b1, gr, tp, t1, t2, df, pos, gamma, s=1.0, m0=None, dtype=np.float64, keep=False):
    """(mx, my, mz) over the grid, each (nf, npos); with keep also the list of the n states before each sample"""
    Q = Setup(b1, gr, tp, t1, t2, df, pos, gamma, s, dtype)
    m = _m0(m0, Q.nf, Q.npos, dtype)
    traj = []
    for t in range(Q.n):
        if keep:
            traj.append(m)
        o = _mat_vec(_rot(*Q.ck(t)[0]), m)
        m = [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + (1 - Q.e1[t])]
    return (m, traj, Q) if keep else m


def vjp(b1, gr, tp, t1, t2, df, pos, gamma, s, m0, cot, dtype=np.float64):
    """(dL/dRe b1 + i dL/dIm b1 (n,), dL/dm0 as three (nf, npos) arrays) at scale s for cot = (cmx, cmy, cmz), each (nf, npos);
    the factor s of the chain rule through s b1 is included"""
    _, traj, Q = forward(b1, gr, tp, t1, t2, df, pos, gamma, s, m0, dtype, keep=True)
    lam = [np.asarray(c, dtype=np.float64).reshape(Q.nf, Q.npos).astype(dtype) for c in cot]
    g = np.zeros(Q.n, dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
    for t in range(Q.n - 1, -1, -1):
        (ar, ai, br, bi), sp, D, (nx, ny, nz) = Q.ck(t)
        dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
        mp = traj[t]
        gxy = []
        for p, eb, ec in ((nx, 0, -1), (ny, 1, 0)):                   # d cos(phi/2)/dp = -(sp/2) p, d sp/dp = D p
            dsp = D * p
            dR = _drot(ar, ai, br, bi, -sp * p / 2, -nz * dsp, ny * dsp + eb * sp, -nx * dsp + ec * sp)
            w = _mat_vec(dR, mp)
            gxy.append((dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]).sum())
        f = dtype(s) * dtype(Q.gamma) * dtype(Q.dt[t])
        g[t] = -f * gxy[0] + 1j * (f * gxy[1])
        lam = _mat_vec(_rot(ar, ai, br, bi), dl, transpose=True)
    return g, lam


def vjp_scaled(pulse, df, pos, cot, scales, m0=None, dtype=np.float64):
    """The adjoint of the scale sweep for pulse = (b1, gr, tp, t1, t2, nucleus), cot = (cmx, cmy, cmz), each (S, nf, npos):
    (grad_b1 (n,), (gmx, gmy, gmz) each (S, nf, npos)), the gradient summed over the scales, dL/dm0 per scale"""
    b1, gr, tp, t1, t2, nucleus = pulse
    grad, gm = 0, []
    for k, s in enumerate(scales):
        g, l0 = vjp(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, [c[k] for c in cot], dtype)
        grad = grad + g
        gm.append(l0)
    return grad, tuple(np.stack([l[c] for l in gm]) for c in range(3))


# ---- the cases of tests/test_blochgrad_gpu.py's comparison with this reference (tests/test_blochgrad_cpu.py checks the reference
# itself on the same cases) ----------------------------------------------------------------------------------------------------
SCALES = [1.0, 0.0, 0.9]
LENGTHS = [1, 7, 8, 9, 255, 256, 257, 600]          # around the group of 8 samples and the 256-sample tile
POINTS = [(1, 1), (3, 5), (1, 257), (3, 200)]       # one point, a partial chunk, more than one chunk
TOL = 1e-12


def _grid(k, span):
    """k points over +-span with 0 among them"""
    x = np.linspace(-span, span, k) if k > 1 else np.zeros(1)
    x[k // 2] = 0.0
    return x


def batch(shared):
    """Eight pulses: (pulses, dfs, dps, m0s, cots).  Pulse q has LENGTHS[q] samples, 1 + q % 3 gradient axes, tp a scalar (q even)
    or per-sample intervals (q odd), its own T1, T2 and gamma, and for n >= 3 one b1 sample exactly zero; the last one lasts 26 ms
    at T2 = 1 ms.  Grids: one of 3 x 5 points shared by all, or POINTS[q % 4] per pulse with 1 + q % 3 position axes; df = 0 and
    position 0 are on every grid.  m0 random with |m0| <= 1; cotangents standard normal, (3 scales, nf, npos)."""
    rng = np.random.default_rng(11)
    pulses, dfs, dps, m0s, cots = [], [], [], [], []
    for q, n in enumerate(LENGTHS):
        nucleus = ("C-13", "H-1", 10000.0)[q % 3]
        gamma = gamma_of(nucleus)
        dur = 26e-3 if n == 600 else n * (4e-6 + 2e-6 * q)
        flip = (0.3, 1.0, np.pi / 2, 2.0, 0.02, np.pi, 1.5, 3.0)[q]
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (flip / (gamma * dur))
        if n >= 3:
            b1[n // 3] = 0.0
        ax = 1 + q % 3
        gr = rng.uniform(0.5, 1.5, (n, ax)) * 0.1 * (GAMMA_H1 / gamma)
        tp = dur / n if q % 2 == 0 else (dur / n) * (1.0 + 0.2 * (-1.0) ** np.arange(n) + 0.05 * rng.uniform(-1, 1, n))
        t1 = 0.5 + 0.1 * q
        t2 = 1e-3 if n == 600 else (2.0 + q) * dur
        pulses.append((b1, gr, tp, t1, t2, nucleus))
        nf, npos = (3, 5) if shared else POINTS[q % 4]
        dfs.append(_grid(nf, 200.0))
        dps.append(np.stack([_grid(npos, 2.0) * (1.0 - 0.3 * a) for a in range(ax)], 1))
        v = rng.standard_normal((3, nf, npos))
        v *= rng.uniform(0, 1, (nf, npos)) / np.sqrt((v * v).sum(0))
        m0s.append(tuple(v))
        cots.append(tuple(rng.standard_normal((3, len(SCALES), nf, npos))))
    if shared:
        dfs, dps = [dfs[0]] * 8, [np.stack([_grid(5, 2.0) * (1.0 - 0.3 * a) for a in range(3)], 1)] * 8
    return pulses, dfs, dps, m0s, cots


def intervals(pulse):
    """The per-sample intervals of a pulse (n,)"""
    return np.broadcast_to(np.asarray(pulse[2], dtype=np.float64).ravel(), (len(pulse[0]),))


def bound_b1(pulse, cot, scales):
    """1e-12 N max|s| gamma dt_t per b1 entry, N = the sum of |cmx| + |cmy| + |cmz| over the pulse's points and scales: a rotation's
    derivative and the decay have norm at most 1, and 1e-12 is the forward tolerance of the Bloch tests"""
    N = float(sum(np.abs(c).sum() for c in cot))
    return TOL * N * max(abs(s) for s in scales) * gamma_of(pulse[5]) * intervals(pulse)


def bound_m0(cot):
    """1e-12 max over the pulse's points of |cmx| + |cmy| + |cmz|"""
    return TOL * float((np.abs(cot[0]) + np.abs(cot[1]) + np.abs(cot[2])).max())
