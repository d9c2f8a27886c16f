"""NumPy restatement of the adjoint of a pulse train with respect to the period's b1 and to the initial magnetisation (helper of
tests/test_blochtrainvjp_cpu.py and tests/test_blochtrainvjp_gpu.py; not collected), vectorised over the (frequency, position)
points, in float64 or np.longdouble, on tests/blochtrain_ref.py (the train) and tests/blochgrad_ref.py (the sample's derivative).

The loss is L = sum_k <ce_k, echo_k> + <cf, m_N> for cotangents ce_k of the echoes (with demod: of the demodulated echoes) and cf of
the final state.  Two routes to the same gradient G = dL/dRe b1 + i dL/dIm b1 and to dL/dm0:
    tiled_vjp: the sample-by-sample recursion over the tiled waveform reversed, the echo cotangents injected at the echo samples
               (demod: turned back by Z(-phi_k) first).  Sample t of repetition k yields the gradient of the tiled sample
               w = gains[k] e^{i phi_k} b1_t, and w = c z gives G_z = conj(c) G_w, so G_b1[t] = sum_k gains[k] e^{-i phi_k} G_w[k, t].
    train_vjp: the structured route in the device's order: lambda through the repetitions in reverse, which accumulates
               the cotangents of the 24 propagator entries per distinct amplitude; then the four columns of [A | B], each of which
               obeys the sample recursion, swept forwards and backwards with those cotangents.  It returns the cotangent planes too.
Both take the amplitude of a repetition as blochtrain_ref does (the float64 product scale x gain), and the derivative of a sample's
rotation from blochgrad_ref._drot, which is not how the device's step (bloch_vjp_step, sim_dev.h) forms it.

Bounds (bound_b1, bound_m0), with N the 1-norm of all cotangents of the pulse:
    per b1 entry   TOL ntr N max|scale gain| gamma dt_t
    per m0 entry   TOL ntr (max over the point's cotangents ce_k, cf of the 1-norm)
Every step of the reverse recursion is the transpose of a contraction, so a cotangent never grows; a sample's gradient is at most
|lambda| |m| gamma dt amp, |m| <= sqrt(3) max(|m0|, |meq|, 1), and each of the ntr repetitions adds its own share: hence the
factor ntr on top of blochgrad_ref's bound.  TOL = blochgrad_ref.TOL = 1e-12 was measured, not assumed: over cases() the float64
twin of train_vjp differs from its long-double twin by at most 3.1e-4 of the b1 bound and 2.5e-3 of the m0 bound (both on the
257-sample pulse of case "shared"), within the hundredth that tests/test_blochtrainvjp_cpu.py asserts, so the constant stands as
it started and there is no "before and after".  The device's
shares are printed by tests/test_blochtrainvjp_gpu.py and quoted in DESIGN section 8z.

Central differences (FD_ANGLE, FD_TOL).  A b1 entry is moved by h = FD_ANGLE / (gamma dt_t amax), so that the sample turns by
FD_ANGLE = 1e-5 rad more or less.  In units of the bound's scale ntr N amax gamma dt_t the central difference is off by its
truncation, about (ntr FD_ANGLE)^2 / 6 = 1.5e-10 at ntr = 3, plus the rounding of the two losses over 2 h: a float64 train is
held to 200 u ntr (ntime + 4) = 8.7e-13 per entry at ntr = 3 and ntime = 9 (blochtrain_ref), so the quotient is off by at most
8.7e-13 N / FD_ANGLE = 8.7e-8 N, 2.9e-8 of the scale.  FD_TOL = 1e-7 covers the float64 device call with a factor 3 to spare and
the long-double reference with many orders.  L is affine in m0: its central difference has no truncation at any step, FD_M0 = 0.5
keeps the rounding at 8.7e-13 N, and the same FD_TOL applies to the m0 scale ntr max|c|_1 per point."""
import functools
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("blochtrain_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "blochtrain_ref.py"))
tr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tr)
_grad = tr._grad

TOL = _grad.TOL
FD_ANGLE = 1e-5
FD_M0 = 0.5
FD_TOL = 1e-7


def _ctype(dtype):
    return np.complex128 if dtype == np.float64 else np.clongdouble


def _fwd(Q, t, nx, ny, m, rec):
    """One sample forwards about the axis (nx, ny, rotz_t); rec scales the recovery term"""
    o = _grad._mat_vec(tr._rot_of(nx, ny, Q.rotz[t]), m)
    return [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + rec * (1 - Q.e1[t])]


def _bwd(Q, t, nx, ny, mp, lam):
    """One sample backwards: (dL/dnx, dL/dny) per point and the multiplier before the sample, from the state mp before it and the
    multiplier lam after it (blochgrad_ref.vjp's arithmetic, per point)"""
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
    return g[0], g[1], _grad._mat_vec(_grad._rot(ar, ai, br, bi), dl, transpose=True)


def _cots(ce, cf, ntr, Q, dtype):
    """The cotangents as lists of arrays in dtype: ce[k] (three (nf, npos)) or None, cf (three) or zeros"""
    shape = (Q.nf, Q.npos)
    e = None if ce is None else [[np.asarray(c[k], dtype=np.float64).reshape(shape).astype(dtype) for c in ce] for k in range(ntr)]
    f = [np.zeros(shape, dtype=dtype)] * 3 if cf is None else [np.asarray(c, dtype=np.float64).reshape(shape).astype(dtype) for c in cf]
    return e, f


def tiled_vjp(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64, sense=1):
    """(G (ntime,), dL/dm0 as three (nf, npos) arrays) at one scale by the reversed recursion over the tiled waveform.  ce: None or
    (cx, cy, cz), each (ntr, nf, npos); cf: None or (cx, cy, cz), each (nf, npos).  sense = -1 applies the chain rule through
    gains[k] e^{i phi_k} with the opposite sense of the phase, which is wrong (the CPU test holds it far off)."""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Qs = {a: tr._setup(pulse, df, pos, a, dtype) for a in set(amps.tolist())}
    Q0 = next(iter(Qs.values()))
    n, mq = Q0.n, dtype(meq)
    m, traj = tr._start(m0, Q0, dtype), []
    for k in range(ntr):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        for t in range(n):
            traj.append(m)
            nz = Q.rotz[t]
            m = _fwd(Q, t, np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t]), m, mq)
    e, lam = _cots(ce, cf, ntr, Q0, dtype)
    G = np.zeros(n, dtype=_ctype(dtype))
    for k in range(ntr - 1, -1, -1):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        inj = None if e is None else (tr._zm(c, s, e[k]) if demod else e[k])          # echo' = Z(+phi) echo: its transpose
        for t in range(n - 1, -1, -1):
            if inj is not None and t + 1 == echo:
                lam = [a + b for a, b in zip(lam, inj)]
            nz = Q.rotz[t]
            gx, gy, lam = _bwd(Q, t, np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t]),
                               traj[k * n + t], lam)
            f = dtype(Q.gamma) * dtype(Q.dt[t])
            gw = -(f * gx.sum()) + 1j * (f * gy.sum())                  # per unit of amplitude, with respect to e^{i phi_k} b1_t
            G[t] += dtype(amps[k]) * (c - sense * 1j * s) * gw
        if inj is not None and echo == 0:
            lam = [a + b for a, b in zip(lam, inj)]
    return G, lam


def train_vjp(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(G (ntime,), dL/dm0 as three (nf, npos) arrays, planes) at one scale by the structured route.  planes: amplitude -> the
    cotangents (Abar[i][j], Bbar[i], Aebar[i][j], Bebar[i]) of that amplitude's propagators, each entry (nf, npos)."""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Ps = {a: tr.prop(pulse, df, pos, a, echo, dtype) for a in set(amps.tolist())}
    Q0 = tr._setup(pulse, df, pos, 1.0, dtype)
    n, mq = Q0.n, dtype(meq)
    m, us = tr._start(m0, Q0, dtype), []
    for k in range(ntr):
        A, B, _, _ = Ps[float(amps[k])]
        u = tr._zp(cs[k], sn[k], m)
        us.append(u)
        m = tr._zm(cs[k], sn[k], [a + mq * b for a, b in zip(_grad._mat_vec(A, u), B)])
    e, lam = _cots(ce, cf, ntr, Q0, dtype)
    zero = np.zeros((Q0.nf, Q0.npos), dtype=dtype)
    planes = {a: ([[zero] * 3 for _ in range(3)], [zero] * 3, [[zero] * 3 for _ in range(3)], [zero] * 3) for a in Ps}
    for k in range(ntr - 1, -1, -1):
        key, c, s, u = float(amps[k]), cs[k], sn[k], us[k]
        A, _, Ae, _ = Ps[key]
        Ab, Bb, Aeb, Beb = planes[key]
        a = tr._zp(c, s, lam)
        Ab = [[Ab[i][j] + a[i] * u[j] for j in range(3)] for i in range(3)]
        Bb = [Bb[i] + mq * a[i] for i in range(3)]
        lam = _grad._mat_vec(A, a, transpose=True)
        if e is not None:
            ae = e[k] if demod else tr._zp(c, s, e[k])
            Aeb = [[Aeb[i][j] + ae[i] * u[j] for j in range(3)] for i in range(3)]
            Beb = [Beb[i] + mq * ae[i] for i in range(3)]
            lam = [x + y for x, y in zip(lam, _grad._mat_vec(Ae, ae, transpose=True))]
        planes[key] = (Ab, Bb, Aeb, Beb)
        lam = tr._zm(c, s, lam)
    # through the period: the four columns of [A | B] as one leading axis, the recovery term on the fourth alone
    rec = np.array([0, 0, 0, 1], dtype=dtype)[:, None, None]
    G = np.zeros(n, dtype=_ctype(dtype))
    for key in sorted(Ps):
        Q = tr._setup(pulse, df, pos, key, dtype)
        Ab, Bb, Aeb, Beb = planes[key]
        X = [np.stack([np.full_like(zero, 1.0 if i == j else 0.0) for j in range(3)] + [zero]) for i in range(3)]
        traj = []
        for t in range(n):
            traj.append(X)
            X = _fwd(Q, t, np.full_like(zero, Q.rotx[t]), np.full_like(zero, Q.roty[t]), X, rec)
        col = lambda M, v: [np.stack([M[i][0], M[i][1], M[i][2], v[i]]) for i in range(3)]
        lx, le = col(Ab, Bb), col(Aeb, Beb)
        for t in range(n - 1, -1, -1):
            if t + 1 == echo:
                lx = [a + b for a, b in zip(lx, le)]
            gx, gy, lx = _bwd(Q, t, np.full_like(zero, Q.rotx[t]), np.full_like(zero, Q.roty[t]), traj[t], lx)
            f = dtype(Q.gamma) * dtype(Q.dt[t])
            G[t] += dtype(key) * (-(f * gx.sum()) + 1j * (f * gy.sum()))
    return G, lam, planes


def vjp_scaled(route, pulse, df, pos, ntr, phases, gains, echo, ce, cf, scales, m0, meq, demod, dtype, **kw):
    """The adjoint of the scale sweep by route (tiled_vjp or train_vjp): (G (ntime,), (gmx, gmy, gmz) each (S, nf, npos)); ce: None or
    three (S, ntr, nf, npos), cf: None or three (S, nf, npos)"""
    G, gm = 0, []
    for k, s in enumerate(scales):
        r = route(pulse, df, pos, ntr, phases, gains, echo, None if ce is None else [c[k] for c in ce],
                  None if cf is None else [c[k] for c in cf], s, m0, meq, demod, dtype, **kw)
        G = G + r[0]
        gm.append(r[1])
    return G, tuple(np.stack([l[c] for l in gm]) for c in range(3))


# ---- the cases that tests/test_blochtrainvjp_cpu.py and tests/test_blochtrainvjp_gpu.py share ---------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """name -> blochtrain_ref's case dict plus cot ('echo', 'final' or 'both'), demod, meq, ce and cf (per pulse three arrays of shape
    (S, ntr, nf, npos) and (S, nf, npos), standard normal; None where the case has none).  blochtrain_ref.cases() (periods of 1, 9
    and 257 samples, trains of 1, 2 and 257 repetitions, every echo edge, 1 and 3 gains, 1 and 3 scales, 6 to 300 points) and the
    edges of the adjoint's kernels: trains of 7, 8 and 9 repetitions (around the group of 8), 65 points (two chunks of 64, one point
    in the last), a train of 5 repetitions at 5 distinct gains."""
    rng = np.random.default_rng(29)
    base = tr.cases()
    f3, p2 = tr._grid(3, 60.0), np.array([[-1.0], [0.7]])
    out = {k: dict(v) for k, v in base.items()}
    per = tr._period(rng, 9, *tr.C13, 0.6, 4e-3, True)
    out["groups"] = dict(pulses=[per] * 3, dfs=[f3] * 3, dps=[p2] * 3, ntr=[7, 8, 9], phases=[np.pi * np.arange(n) for n in (7, 8, 9)],
                         gains=[np.minimum(1.0, 0.5 + 0.25 * np.arange(n)) for n in (7, 8, 9)], echo=[4, 9, 0],
                         m0=[tr._m0(rng, 3, 2)] * 3, scales=(1.0,))
    out["p65"] = dict(pulses=[tr._period(rng, 9, *tr.H1, 0.9, 2e-3, True)], dfs=[tr._grid(5, 40.0)], dps=[tr._grid(13, 1.5)[:, None]],
                      ntr=[3], phases=[np.array([0.0, 2.0, -1.0])], gains=[np.ones(3)], echo=[5], m0=[tr._m0(rng, 5, 13)], scales=(1.0,))
    out["allgains"] = dict(pulses=[tr._period(rng, 9, *tr.C13, 0.5, 4e-3, True)], dfs=[f3], dps=[p2], ntr=[5],
                           phases=[0.5 * np.deg2rad(117.0) * np.arange(5) * (np.arange(5) + 1)], gains=[np.linspace(0.5, 1.0, 5)],
                           echo=[4], m0=[tr._m0(rng, 3, 2)], scales=(0.9, 1.1))
    mode = dict(c13_ramp=("both", True, 0.0), h1_long=("final", False, 1.0), one=("echo", False, 1.0), batch=("both", False, 1.0),
                shared=("echo", True, 0.0), groups=("both", False, 0.0), p65=("both", True, 1.0), allgains=("echo", False, 1.0))
    for name, c in out.items():
        c["cot"], c["demod"], c["meq"] = mode[name]
        S, ce, cf = len(c["scales"]), [], []
        for q in range(len(c["pulses"])):
            nf, npos = len(c["dfs"][q]), len(c["dps"][q])
            ce.append(tuple(rng.standard_normal((3, S, c["ntr"][q], nf, npos))) if c["cot"] != "final" else None)
            cf.append(tuple(rng.standard_normal((3, S, nf, npos))) if c["cot"] != "echo" else None)
        c["ce"], c["cf"] = ce, cf
    return out


@functools.lru_cache(maxsize=None)
def small():
    """The case of the central differences: 9 samples with a gradient, 3 repetitions at three gains and arbitrary phases, 3 x 2
    points, cotangents on the echoes and on the final state, meq = 1"""
    rng = np.random.default_rng(31)
    c = dict(pulses=[tr._period(rng, 9, *tr.C13, 0.6, 4e-3, True)], dfs=[tr._grid(3, 60.0)], dps=[np.array([[-1.0], [0.7]])], ntr=[3],
             phases=[np.array([0.4, -1.3, 2.2])], gains=[np.array([0.5, 0.75, 1.0])], echo=[4], m0=[tr._m0(rng, 3, 2)], scales=(1.0,),
             cot="both", demod=False, meq=1.0)
    c["ce"], c["cf"] = [tuple(rng.standard_normal((3, 1, 3, 3, 2)))], [tuple(rng.standard_normal((3, 1, 3, 2)))]
    return c


def run(route, c, q, dtype, meq=None, m0="case", **kw):
    """route on pulse q of the case c over its scales"""
    return vjp_scaled(route, c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q],
                      c["ce"][q], c["cf"][q], c["scales"], c["m0"][q] if isinstance(m0, str) else m0, c["meq"] if meq is None else meq,
                      c["demod"], dtype, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The long-double structured route of a case: per pulse (G, (gmx, gmy, gmz)), computed once"""
    c = cases()[name]
    return [run(lambda *a, **k: train_vjp(*a, **k)[:2], c, q, np.longdouble) for q in range(len(c["pulses"]))]


def amax_of(c, q):
    return max(abs(s) for s in c["scales"]) * float(np.abs(c["gains"][q]).max())


def norm1(c, q):
    """N: the 1-norm of all cotangents of pulse q"""
    return float(sum(np.abs(v).sum() for tri in (c["ce"][q], c["cf"][q]) if tri is not None for v in tri))


def scale_b1(c, q):
    """ntr N max|scale gain| gamma dt_t per b1 entry: the bound without its constant"""
    p = c["pulses"][q]
    return c["ntr"][q] * norm1(c, q) * amax_of(c, q) * tr.gamma_of(p[5]) * tr.intervals(p)


def scale_m0(c, q):
    """ntr times the largest 1-norm among the point's cotangents, (S, nf, npos)"""
    n1 = []
    if c["ce"][q] is not None:
        n1.append(sum(np.abs(v) for v in c["ce"][q]).max(1))
    if c["cf"][q] is not None:
        n1.append(sum(np.abs(v) for v in c["cf"][q]))
    return c["ntr"][q] * np.maximum.reduce(n1)


def bound_b1(c, q):
    return TOL * scale_b1(c, q)


def bound_m0(c, q):
    return TOL * scale_m0(c, q)


def loss(c, q, E, F):
    """L of pulse q from the echoes E (three (S, ntr, nf, npos)) and the final state F (three (S, nf, npos)), per point (nf, npos)"""
    L = 0
    if c["ce"][q] is not None:
        L = L + sum((np.asarray(ck) * e).sum((0, 1)) for ck, e in zip(c["ce"][q], E))
    if c["cf"][q] is not None:
        L = L + sum((np.asarray(ck) * f).sum(0) for ck, f in zip(c["cf"][q], F))
    return L
