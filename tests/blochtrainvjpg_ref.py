"""NumPy restatement of the adjoint of a pulse train with respect to the period's b1, the initial magnetisation, the period's gradient
waveform gr and the off-resonance df (helper of tests/test_blochtrainvjpg_cpu.py and tests/test_blochtrainvjpg_gpu.py; not
collected), vectorised over the (frequency, position) points, in float64 or np.longdouble, on tests/blochtrainvjp_ref.py (the train's
adjoint in b1 and m0, whose operations the b1 and m0 parts repeat in the same order) and tests/blochgradg_ref.py (the sample's
derivative in rotz), both loaded by path.

gr and df enter a period only through a sample's rotz_t = -((gx_t gamma dt_t) x + (gy_t gamma dt_t) y + (gz_t gamma dt_t) z + df (TWOPI
dt_t)); neither the RF phase Z(phi_k) nor the gain of a repetition touches them.  With dz_t = (D lambda_t)' (dR_t / d rotz) m_{t-1}
(blochgradg_ref.vjp_gr's _drot(ar, ai, br, bi, -sp nz / 2, -nz D nz - sp, ny D nz, -nx D nz)) two routes to the same gradients:
    tiled_vjp_gr: blochtrainvjp_ref.tiled_vjp's reversed recursion over the tiled waveform; the rows of the tiled gr gradient are
                  summed over the repetitions, dL/ddf over all tiled samples.
    train_vjp_gr: the structured route in the device's order: blochtrainvjp_ref.train_vjp's walk of the repetitions as it
                  is, then the four columns of [A | B] swept backwards per distinct amplitude c with
                      dL/dg_{t,a}   = -(gamma dt_t) sum_c sum_{f,p} pos_{p,a} sum_col dz_t          no factor scale x gain
                      dL/ddf(f, p) = -sum_t (TWOPI dt_t) sum_c sum_col dz_t                         per scale
                  The echo cotangent column joins where the reverse walk reaches the state after `echo` samples; with echo = 0 the
                  echo map is the identity, depends on neither gr nor df, and its cotangents are ignored, as for b1.
In long double the two agree to 4.8e-18 of the largest entry in gr and 1.4e-17 in df over cases() (tests/test_blochtrainvjpg_cpu.py
asserts 1e-15).

Bounds (bound_gr, bound_df): blochgradg_ref's with blochtrainvjp_ref's factor ntr,
    bound_gr[t, a]    = TOL ntr gamma dt_t sum_p |pos_{p,a}| sum_{s,f} mu(f, p) W(s, f, p)
    bound_df[s, f, p] = TOL ntr TWOPI (sum_t dt_t) mu(f, p) W(s, f, p)
W the 1-norm of all of the point's cotangents (every echo and the final state), mu = blochtrain_ref.mu_of = max(|m0|inf, |meq|, 1),
TOL = blochgrad_ref.TOL = 1e-12.  A cotangent never grows on the way back (every step is the transpose of a contraction), the state
of a column is at most sqrt(3) mu, and each of the ntr repetitions adds its share of dz_t.  Where a gr bound is zero (no position
has the axis) the result must be exactly zero.  b1 and m0 keep blochtrainvjp_ref.bound_b1 / bound_m0.  Measured here: over cases()
the float64 twin of train_vjp_gr differs from its long-double twin by at most 8.8e-5 of the gr bound (the 257-sample period of
"batch") and 1.3e-3 of the df bound ("h1_long"), within the hundredth that tests/test_blochtrainvjpg_cpu.py asserts: TOL stands as
it started.

Central differences of the long-double blochtrain_ref.train on small(), entry by entry (FD_GR = 1e-6 G/cm, FD_DF = 1e-3 Hz): worst
4.2e-10 of max|grad_gr| and 1.3e-9 of max|grad_df| (summed over scale and position); FD_TOL = 1e-7 of the largest entry.

Directional derivative on the device (fd_problem, tests/test_blochtrainvjpg_gpu.py): L = sum_k (w . echo_k)^2 / 2 on the float64
train.  The float64 reference's own central difference against its own adjoint, relative, over h in HS_GR (G/cm, along a random
unit direction of gr) and HS_DF (Hz, a common shift of df), as fd_sweep() gives it:
    gr   h 1e-3: 3.4e-5   1e-4: 3.4e-7   1e-5: 3.5e-9   1e-6: 3.7e-10   1e-7: 4.9e-9   1e-8: 9.9e-9
    df   h 1e-1: 6.2e-5   1e-2: 6.2e-7   1e-3: 6.6e-9   1e-4: 2.3e-9    1e-5: 1.2e-7   1e-6: 7.3e-7
The minima are FD_DIR_GR_MIN = 3.71e-10 at FD_DIR_GR = 1e-6 G/cm and FD_DIR_DF_MIN = 2.25e-9 at FD_DIR_DF = 1e-4 Hz.  The device test
takes these steps and holds each difference to ten times its minimum, 3.7e-9 and 2.3e-8 relative."""
import functools
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_here, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vjp = _load("blochtrainvjp_ref")
gradg = _load("blochgradg_ref")
tr = vjp.tr
_grad = tr._grad

TOL = _grad.TOL
FD_GR = 1e-6
FD_DF = 1e-3
FD_TOL = 1e-7
HS_GR = (1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)
HS_DF = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)
FD_DIR_GR, FD_DIR_GR_MIN = 1e-6, 3.71e-10
FD_DIR_DF, FD_DIR_DF_MIN = 1e-4, 2.25e-9


def _bwd_z(Q, t, nx, ny, mp, lam):
    """blochtrainvjp_ref._bwd (the same operations in the same order for the rf pair and the multiplier) plus dz, the sample's
    dL / d rotz per point"""
    nz = Q.rotz[t]
    phi = np.sqrt(nx * nx + ny * ny + nz * nz)
    sp, D = _grad._half_sinc(phi)
    ar, ai, br, bi = np.cos(phi / 2), -nz * sp, ny * sp, -nx * sp
    dl = [Q.e2[t] * lam[0], Q.e2[t] * lam[1], Q.e1[t] * lam[2]]
    g = []
    for p, eb, ec in ((nx, 0, -1), (ny, 1, 0)):
        dsp = D * p
        w = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp * p / 2, -nz * dsp, ny * dsp + eb * sp, -nx * dsp + ec * sp), mp)
        g.append(dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2])
    dsp = D * nz
    w = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp * nz / 2, -nz * dsp - sp, ny * dsp, -nx * dsp), mp)
    dz = dl[0] * w[0] + dl[1] * w[1] + dl[2] * w[2]
    return g[0], g[1], dz, _grad._mat_vec(_grad._rot(ar, ai, br, bi), dl, transpose=True)


def _gr_rows(Q, t, dz, p3, dtype):
    """(-(gamma dt_t) sum_{f,p} pos_{p,a} dz for a = x, y, z; (TWOPI dt_t) dz): dz (nf, npos)"""
    f = dtype(Q.gamma) * dtype(Q.dt[t])
    return np.array([-(f * (dz * p3[None, :, a]).sum()) for a in range(3)], dtype=dtype), (dtype(_grad.TWOPI_REF) * dtype(Q.dt[t])) * dz


def tiled_vjp_gr(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(G (ntime,), grad_gr (ntime, 3), dL/dm0 as three (nf, npos) arrays, grad_df (nf, npos)) at one scale by the reversed recursion
    over the tiled waveform: blochtrainvjp_ref.tiled_vjp with the gr rows summed over the repetitions"""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Qs = {a: tr._setup(pulse, df, pos, a, dtype) for a in set(amps.tolist())}
    Q0 = next(iter(Qs.values()))
    n, mq = Q0.n, dtype(meq)
    p3 = gradg.positions(pos).astype(dtype)
    m, traj = tr._start(m0, Q0, dtype), []
    for k in range(ntr):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        for t in range(n):
            traj.append(m)
            nz = Q.rotz[t]
            m = vjp._fwd(Q, t, np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t]), m, mq)
    e, lam = vjp._cots(ce, cf, ntr, Q0, dtype)
    G = np.zeros(n, dtype=vjp._ctype(dtype))
    gg, gdf = np.zeros((n, 3), dtype=dtype), np.zeros((Q0.nf, Q0.npos), dtype=dtype)
    for k in range(ntr - 1, -1, -1):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        inj = None if e is None else (tr._zm(c, s, e[k]) if demod else e[k])
        for t in range(n - 1, -1, -1):
            if inj is not None and t + 1 == echo:
                lam = [a + b for a, b in zip(lam, inj)]
            nz = Q.rotz[t]
            gx, gy, dz, lam = _bwd_z(Q, t, np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]),
                                     np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t]), traj[k * n + t], lam)
            f = dtype(Q.gamma) * dtype(Q.dt[t])
            gw = -(f * gx.sum()) + 1j * (f * gy.sum())
            G[t] += dtype(amps[k]) * (c - 1j * s) * gw
            row, d = _gr_rows(Q, t, dz, p3, dtype)
            gg[t] += row
            gdf -= d
        if inj is not None and echo == 0:
            lam = [a + b for a, b in zip(lam, inj)]
    return G, gg, lam, gdf


def train_vjp_gr(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(G (ntime,), grad_gr (ntime, 3), dL/dm0 as three (nf, npos) arrays, grad_df (nf, npos)) at one scale by the structured route:
    blochtrainvjp_ref.train_vjp for the repetitions (G and dL/dm0 are its bits), then its sweep of the four columns with dz"""
    G0, lam, planes = vjp.train_vjp(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale, m0, meq, demod, dtype)
    Q0 = tr._setup(pulse, df, pos, 1.0, dtype)
    n = Q0.n
    p3 = gradg.positions(pos).astype(dtype)
    zero = np.zeros((Q0.nf, Q0.npos), dtype=dtype)
    rec = np.array([0, 0, 0, 1], dtype=dtype)[:, None, None]
    G = np.zeros(n, dtype=vjp._ctype(dtype))
    gg, gdf = np.zeros((n, 3), dtype=dtype), np.zeros((Q0.nf, Q0.npos), dtype=dtype)
    for key in sorted(planes):
        Q = tr._setup(pulse, df, pos, key, dtype)
        Ab, Bb, Aeb, Beb = planes[key]
        X = [np.stack([np.full_like(zero, 1.0 if i == j else 0.0) for j in range(3)] + [zero]) for i in range(3)]
        traj = []
        for t in range(n):
            traj.append(X)
            X = vjp._fwd(Q, t, np.full_like(zero, Q.rotx[t]), np.full_like(zero, Q.roty[t]), X, rec)
        col = lambda M, v: [np.stack([M[i][0], M[i][1], M[i][2], v[i]]) for i in range(3)]
        lx, le = col(Ab, Bb), col(Aeb, Beb)
        for t in range(n - 1, -1, -1):
            if t + 1 == echo:
                lx = [a + b for a, b in zip(lx, le)]
            gx, gy, dz, lx = _bwd_z(Q, t, np.full_like(zero, Q.rotx[t]), np.full_like(zero, Q.roty[t]), traj[t], lx)
            f = dtype(Q.gamma) * dtype(Q.dt[t])
            G[t] += dtype(key) * (-(f * gx.sum()) + 1j * (f * gy.sum()))
            row, d = _gr_rows(Q, t, dz.sum(0), p3, dtype)
            gg[t] += row
            gdf -= d
    assert np.array_equal(G, G0)
    return G, gg, lam, gdf


def vjp_gr_scaled(route, pulse, df, pos, ntr, phases, gains, echo, ce, cf, scales, m0, meq, demod, dtype):
    """The adjoint of the scale sweep by route: (G (ntime,), grad_gr (ntime, 3), (gmx, gmy, gmz) each (S, nf, npos), grad_df (S, nf,
    npos)); b1 and gr summed over the scales; ce: None or three (S, ntr, nf, npos), cf: None or three (S, nf, npos)"""
    G, gg, gm, gd = 0, 0, [], []
    for k, s in enumerate(scales):
        r = route(pulse, df, pos, ntr, phases, gains, echo, None if ce is None else [c[k] for c in ce],
                  None if cf is None else [c[k] for c in cf], s, m0, meq, demod, dtype)
        G, gg = G + r[0], gg + r[1]
        gm.append(r[2])
        gd.append(r[3])
    return G, gg, tuple(np.stack([l[c] for l in gm]) for c in range(3)), np.stack(gd)


SUB_LENGTHS = (2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def cases():
    """blochtrainvjp_ref.cases() plus "sub": four short periods of 2, 3, 4 and 5 samples, so that every remainder of a sub-group of 3
    occurs in a group of 8 that is not full, with 3, 2, 1 and 3 position axes (and as many gradient axes), trains of 3, 9, 8 and 5
    repetitions at three distinct gains, echo 1, 3, 0 and 2, scales (1, 0, 0.9), 15 to 70 points, cotangents on the echoes and on the
    final state, meq = 0.5, demodulated echoes"""
    rng = np.random.default_rng(37)
    out = dict(vjp.cases())
    axes, ntr, echo, points = (3, 2, 1, 3), (3, 9, 8, 5), (1, 3, 0, 2), ((3, 5), (2, 9), (5, 14), (1, 21))
    ramp = lambda n: np.minimum(1.0, 0.5 + 0.25 * np.arange(n))
    c = dict(pulses=[], dfs=[], dps=[], ntr=list(ntr), phases=[], gains=[], echo=list(echo), m0=[], scales=(1.0, 0.0, 0.9),
             cot="both", demod=True, meq=0.5, ce=[], cf=[])
    for q, n in enumerate(SUB_LENGTHS):
        nucleus, t1, t2 = tr.H1 if q % 2 else tr.C13
        gamma = tr.gamma_of(nucleus)
        tp = np.append(np.full(n - 1, 2.5e-4), 2e-3 + 1e-3 * q if q else 2e-4)          # never increasing: intervals, not end times
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * ((0.5, 0.9, 0.7, 1.2)[q] / (gamma * tp[:n - 1].sum()))
        b1[-1] = 0.0
        gr = rng.uniform(0.5, 1.5, (n, axes[q])) * 0.02 * (tr.GAMMA_H1 / gamma)
        gr[-1] = 0.0
        nf, npos = points[q]
        c["pulses"].append((b1, gr, tp, t1, t2, nucleus))
        c["dfs"].append(tr._grid(nf, 60.0))
        c["dps"].append(np.stack([tr._grid(npos, 2.0) * (1.0 - 0.3 * a) for a in range(axes[q])], 1))
        c["phases"].append(rng.uniform(-np.pi, np.pi, ntr[q]))
        c["gains"].append(ramp(ntr[q]))
        c["m0"].append(tr._m0(rng, nf, npos))
        c["ce"].append(tuple(rng.standard_normal((3, 3, ntr[q], nf, npos))))
        c["cf"].append(tuple(rng.standard_normal((3, 3, nf, npos))))
    out["sub"] = c
    return out


def small():
    return vjp.small()


def run(route, c, q, dtype):
    """route on pulse q of the case c over its scales"""
    return vjp_gr_scaled(route, c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q],
                         c["ce"][q], c["cf"][q], c["scales"], c["m0"][q], c["meq"], c["demod"], dtype)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64):
    """The structured route of a case in dtype: per pulse (G, grad_gr, (gmx, gmy, gmz), grad_df), computed once"""
    c = cases()[name]
    return [run(train_vjp_gr, c, q, dtype) for q in range(len(c["pulses"]))]


def weight(c, q):
    """mu(f, p) W(s, f, p), (S, nf, npos): W the 1-norm of all of the point's cotangents"""
    w = 0
    if c["ce"][q] is not None:
        w = w + sum(np.abs(v).sum(1) for v in c["ce"][q])
    if c["cf"][q] is not None:
        w = w + sum(np.abs(v) for v in c["cf"][q])
    nf, npos = len(c["dfs"][q]), len(c["dps"][q])
    return tr.mu_of(c["m0"][q], c["meq"], nf, npos)[None] * w


def bound_gr(c, q):
    """(ntime, 3); zero where no position has the axis: there the result must be exactly zero"""
    p = c["pulses"][q]
    w = (weight(c, q).sum((0, 1))[:, None] * np.abs(gradg.positions(c["dps"][q]))).sum(0)          # (3,)
    return TOL * c["ntr"][q] * tr.gamma_of(p[5]) * tr.intervals(p)[:, None] * w[None, :]


def bound_df(c, q):
    """(S, nf, npos)"""
    p = c["pulses"][q]
    return TOL * c["ntr"][q] * _grad.TWOPI_REF * float(tr.intervals(p).sum()) * weight(c, q)


bound_b1, bound_m0 = vjp.bound_b1, vjp.bound_m0


def loss_of_train(c, q, gr, df, dtype=np.longdouble):
    """L = sum_k <ce_k, echo_k> + <cf, m_N> of pulse q by blochtrain_ref.train with the period's gr and the grid's df replaced"""
    p = c["pulses"][q]
    pulse = (p[0], gr) + tuple(p[2:])
    L = dtype(0)
    for k, s in enumerate(c["scales"]):
        E, F = tr.train(pulse, df, c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], s, c["m0"][q], c["meq"],
                        c["demod"], dtype)
        if c["ce"][q] is not None:
            L = L + sum((np.asarray(ck[k]).astype(dtype) * E[:, i]).sum() for i, ck in enumerate(c["ce"][q]))
        if c["cf"][q] is not None:
            L = L + sum((np.asarray(ck[k]).astype(dtype) * F[i]).sum() for i, ck in enumerate(c["cf"][q]))
    return L


# ---- the directional derivative of a quadratic loss (tests/test_blochtrainvjpg_gpu.py) -------------------------------------------
@functools.lru_cache(maxsize=None)
def fd_problem():
    """9 samples (8 of 0.25 ms with b1 and a gradient, a dead time), 5 repetitions at three gains, 3 x 85 points, scales 0.9 / 1.0 /
    1.1, meq = 0, echo after 4 samples: (pulse, df, dp, kw of the train, w (3, 3, 5, 3, 85), unit direction of gr (9,))"""
    rng = np.random.default_rng(41)
    pulse = tr._period(rng, 9, *tr.H1, 0.9, 2e-3, True)
    df, dp = tr._grid(3, 60.0), tr._grid(85, 3.0)
    kw = dict(phases=np.pi * np.arange(5), gains=np.array([0.5, 0.75, 1.0, 1.0, 1.0]), echo=4, scales=(0.9, 1.0, 1.1), meq=0.0,
              m0=tr._m0(rng, 3, 85))
    d = rng.standard_normal(9)
    d[-1] = 0.0
    return pulse, df, dp, kw, rng.standard_normal((3, 3, 5, 3, 85)), d / np.linalg.norm(d)


def fd_loss(E, w):
    """L = sum (w . echo)^2 / 2 and its cotangents; E: three (S, ntr, nf, npos)"""
    r = w[0] * E[0] + w[1] * E[1] + w[2] * E[2]
    return 0.5 * float((r * r).sum()), tuple(w[c] * r for c in range(3))


def fd_echoes(pulse, gr, df, dp, kw, dtype=np.float64):
    """The echoes of the reference's train as mbfir.bloch_train_batch returns them: three (S, ntr, nf, npos)"""
    p = (pulse[0], gr) + tuple(pulse[2:])
    E = np.stack([tr.train(p, df, dp, len(kw["phases"]), kw["phases"], kw["gains"], kw["echo"], s, kw["m0"], kw["meq"], False, dtype)[0]
                  for s in kw["scales"]])                                 # (S, ntr, 3, nf, npos)
    return tuple(np.asarray(E[:, :, c], dtype=np.float64) for c in range(3))


def fd_sweep():
    """The float64 reference's central differences of fd_loss against <grad_gr, d> and sum(grad_df) of its own adjoint:
    ({h: relative error} for gr, the same for df)"""
    pulse, df, dp, kw, w, d = fd_problem()
    gr = np.asarray(pulse[1], dtype=np.float64).reshape(-1)
    L = lambda g, f: fd_loss(fd_echoes(pulse, g.reshape(-1, 1), f, dp, kw), w)[0]
    _, cot = fd_loss(fd_echoes(pulse, pulse[1], df, dp, kw), w)
    _, gg, _, gd = vjp_gr_scaled(train_vjp_gr, pulse, df, dp, 5, kw["phases"], kw["gains"], kw["echo"], cot, None, kw["scales"], kw["m0"],
                                 kw["meq"], False, np.float64)
    dd, ds = float((gg[:, 0] * d).sum()), float(gd.sum())
    eg = {h: abs((L(gr + h * d, df) - L(gr - h * d, df)) / (2 * h) - dd) / abs(dd) for h in HS_GR}
    ed = {h: abs((L(gr, df + h) - L(gr, df - h)) / (2 * h) - ds) / abs(ds) for h in HS_DF}
    return eg, ed
