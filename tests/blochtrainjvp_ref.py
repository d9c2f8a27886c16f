"""NumPy restatement of the tangent of a pulse train with respect to the period's b1 and to the initial magnetisation (helper of
tests/test_blochtrainjvp_cpu.py and tests/test_blochtrainjvp_gpu.py; not collected), vectorised over the (frequency, position)
points and the directions, in float64 or np.longdouble, on tests/blochtrain_ref.py (the train), tests/blochtrainvjp_ref.py (the
cases and the adjoint) and tests/blochjvp_ref.py (the directions; the sample's tangent is its arithmetic about a turned axis).

Along K directions v (K, n) of b1 and dm0 of m0, two routes to the tangent echoes dE and the tangent final state dF:
    tiled_jvp: the tangent of the sample-by-sample recursion over the tiled waveform, whose direction is tiled in the same sense as
               the waveform itself, w[k, t] = gains[k] e^{+i phi_k} v_t: the axis of a sample and its direction (dnx, dny) are both
               turned by Z(-phi_k).  The echo tangent is read after sample `echo` of repetition k and turned by Z(+phi_k) for demod.
               sense = -1 tiles the direction with e^{-i phi_k}, which is wrong (the CPU test holds it far off).
    train_jvp: the structured route in the device's order: the four columns of X = [A | B] and their tangents swept
               once per distinct amplitude (prop_jvp; dX_0 = 0, the recovery term has no tangent), then per repetition
               decho_k = Z(-phi_k) (A_e du_k + dA_e u_k + meq dB_e),  dm_{k+1} = Z(-phi_k) (A du_k + dA u_k + meq dB).
Both take the amplitude of a repetition as blochtrain_ref does (the float64 product scale x gain) and form (dnx, dny) from v as
rotx / roty are formed from b1.

Bound (bound_jvp), per entry of direction k at a point, the same at every scale:
    TOL ntr ( ntr max|scale gain| gamma sum_t dt_t |v_t| mu + |dm0|_1 at the point ),   mu = max(|m0|inf, |meq|, 1)
Every repetition adds at most amp gamma sum dt |v| |m| to the tangent and every step is a contraction, so the bracket is the size of
the tangent; the leading ntr is the repetitions' own roundings, as in blochtrainvjp_ref.  TOL = blochgrad_ref.TOL = 1e-12 was
measured, not assumed: over cases() the float64 twin of train_jvp differs from its long-double twin by at most 1.1e-3 of the bound
(the 257-sample pulse of case "shared"; tests/test_blochtrainjvp_cpu.py prints every share), within the hundredth that the CPU
test asserts, so the constant stands as it started: before 1e-12, after 1e-12.  The device's shares are printed by
tests/test_blochtrainjvp_gpu.py and quoted in DESIGN section 8aa.

Central differences (FD_ANGLE, FD_M0, FD_TOL of blochtrainvjp_ref).  b1 is moved by +-h v with h = FD_ANGLE / D1, D1 = max|scale
gain| gamma sum_t dt_t |v_t| the angle by which a unit of v turns one repetition, so that a repetition turns by FD_ANGLE = 1e-5 rad
more or less.  In units of scale_fd = ntr D1 mu, the size of the tangent, the central difference is off by its truncation,
(ntr FD_ANGLE)^2 / 6 = 1.5e-10 at ntr = 3, plus the rounding of the two trains over 2 h: a float64 train is held to
200 u ntr (ntime + 4) mu = 8.7e-13 mu per entry at ntr = 3 and ntime = 9 (blochtrain_ref), so the quotient is off by at most
8.7e-13 mu / h = 8.7e-8 mu D1, 2.9e-8 of the scale.  FD_TOL = 1e-7 covers the float64 device call with a factor 3 to spare and
the long-double reference with many orders.  The train is affine in m0: its central difference along dm0 is exact at any step, and
with FD_M0 = 0.5 the quotient is off by 2 x 8.7e-13 max(|m0 +- dm0 / 2|inf, 1) <= 2.6e-12 max(|dm0|_1, 1), far within
FD_TOL max(|dm0|_1, 1), the m0 scale of the test."""
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
jv = _load("blochjvp_ref")
tr = vjp.tr
_grad = tr._grad

TOL = _grad.TOL
FD_ANGLE, FD_M0, FD_TOL = vjp.FD_ANGLE, vjp.FD_M0, vjp.FD_TOL


def _step(Q, t, nx, ny, m, dm, dx, dy, rec):
    """One sample about the axis (nx, ny, rotz_t) for the state m and its K tangents dm along (dx, dy, 0) (blochjvp_ref.jvp's
    arithmetic); rec scales the recovery term, which has no tangent.  m: three arrays (..., nf, npos); dm: three (K, ..., nf, npos);
    dx, dy: (K, 1, ...)."""
    nz = Q.rotz[t]
    phi = np.sqrt(nx * nx + ny * ny + nz * nz)
    sp, D = _grad._half_sinc(phi)
    ar, ai, br, bi = np.cos(phi / 2), -nz * sp, ny * sp, -nx * sp
    zero = np.zeros_like(sp)
    ndn = nx * dx + ny * dy
    U = _grad._mat_vec(_grad._drot(ar, ai, br, bi, -sp / 2, -nz * D, ny * D, -nx * D), m)
    Vx = _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, zero, -sp), m)
    Vy = _grad._mat_vec(_grad._drot(ar, ai, br, bi, zero, zero, sp, zero), m)
    R = _grad._rot(ar, ai, br, bi)
    a, b = _grad._mat_vec(R, dm), [ndn * U[i] + dx * Vx[i] + dy * Vy[i] for i in range(3)]
    e1, e2 = Q.e1[t], Q.e2[t]
    dm = [e2 * (a[0] + b[0]), e2 * (a[1] + b[1]), e1 * (a[2] + b[2])]
    o = _grad._mat_vec(R, m)
    return [e2 * o[0], e2 * o[1], e1 * o[2] + rec * (1 - e1)], dm


def _dn(Q, v, amp, dtype):
    """(dnx, dny), each (K, n), of the directions v at the amplitude amp, as rotx / roty are formed"""
    T = dtype
    dtl, gl, sl = Q.dt.astype(T), T(Q.gamma), T(amp)
    return ((-(v.real.astype(T) * sl)) * gl) * dtl, ((v.imag.astype(T) * sl) * gl) * dtl


def _dirs(v, dm0, Q, dtype):
    v = np.asarray(v, dtype=np.complex128).reshape(-1, Q.n)
    return v, jv._dm0(dm0, v.shape[0], Q.nf, Q.npos, dtype)


def tiled_jvp(pulse, df, pos, ntr, phases, gains, echo, v, dm0=None, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64,
              sense=1):
    """(dE (K, ntr, 3, nf, npos), dF (K, 3, nf, npos)) at one scale by the tangent of the recursion over the tiled waveform"""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Qs = {a: tr._setup(pulse, df, pos, a, dtype) for a in set(amps.tolist())}
    Q0 = next(iter(Qs.values()))
    v, dm = _dirs(v, dm0, Q0, dtype)
    dns = {a: _dn(Q, v, a, dtype) for a, Q in Qs.items()}
    m, mq, dE = tr._start(m0, Q0, dtype), dtype(meq), []
    for k in range(ntr):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        dnx, dny = dns[float(amps[k])]
        if echo == 0:
            dE.append(tr._zp(c, s, dm) if demod else dm)
        for t in range(Q.n):
            nz = Q.rotz[t]
            nx, ny = np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t])
            dx = (c * dnx[:, t] + sense * s * dny[:, t])[:, None, None]
            dy = (c * dny[:, t] - sense * s * dnx[:, t])[:, None, None]
            m, dm = _step(Q, t, nx, ny, m, dm, dx, dy, mq)
            if t + 1 == echo:
                dE.append(tr._zp(c, s, dm) if demod else dm)
    return np.stack([np.stack(e, 1) for e in dE], 1), np.stack(dm, 1)


def prop_jvp(pulse, df, pos, amp, echo, v, dtype=np.float64):
    """((A, B, Ae, Be), (dA, dB, dAe, dBe)) of the period at RF amplitude amp and phase 0: the primal as blochtrain_ref.prop lays it
    out (A[i][j] and B[i] over the points), the tangents alike with a leading K axis on every entry"""
    Q = tr._setup(pulse, df, pos, amp, dtype)
    v = np.asarray(v, dtype=np.complex128).reshape(-1, Q.n)
    K = v.shape[0]
    dnx, dny = _dn(Q, v, amp, dtype)
    one, zero = np.ones((Q.nf, Q.npos), dtype=dtype), np.zeros((Q.nf, Q.npos), dtype=dtype)
    X = [np.stack([one if i == j else zero for j in range(3)] + [zero]) for i in range(3)]          # (4, nf, npos): columns of [A | B]
    dX = [np.zeros((K, 4, Q.nf, Q.npos), dtype=dtype) for _ in range(3)]
    rec = np.array([0, 0, 0, 1], dtype=dtype)[:, None, None]
    Xe, dXe = X, dX
    for t in range(Q.n):
        X, dX = _step(Q, t, np.full_like(zero, Q.rotx[t]), np.full_like(zero, Q.roty[t]), X, dX, dnx[:, t, None, None, None],
                      dny[:, t, None, None, None], rec)
        if t + 1 == echo:
            Xe, dXe = X, dX
    mat = lambda Y, d: [[Y[i][:, j] if d else Y[i][j] for j in range(3)] for i in range(3)]
    vec = lambda Y, d: [Y[i][:, 3] if d else Y[i][3] for i in range(3)]
    return (mat(X, 0), vec(X, 0), mat(Xe, 0), vec(Xe, 0)), (mat(dX, 1), vec(dX, 1), mat(dXe, 1), vec(dXe, 1))


def train_jvp(pulse, df, pos, ntr, phases, gains, echo, v, dm0=None, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(dE (K, ntr, 3, nf, npos), dF (K, 3, nf, npos)) at one scale by the structured route"""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Ps = {a: prop_jvp(pulse, df, pos, a, echo, v, dtype) for a in set(amps.tolist())}
    Q0 = tr._setup(pulse, df, pos, 1.0, dtype)
    v, dm = _dirs(v, dm0, Q0, dtype)
    m, mq, dE = tr._start(m0, Q0, dtype), dtype(meq), []
    mv = _grad._mat_vec
    for k in range(ntr):
        (A, B, Ae, _), (dA, dB, dAe, dBe) = Ps[float(amps[k])]
        c, s = cs[k], sn[k]
        u, du = tr._zp(c, s, m), tr._zp(c, s, dm)
        de = [x + y + mq * z for x, y, z in zip(mv(Ae, du), mv(dAe, u), dBe)]
        dn = [x + y + mq * z for x, y, z in zip(mv(A, du), mv(dA, u), dB)]
        dE.append(de if demod else tr._zm(c, s, de))
        dm = tr._zm(c, s, dn)
        m = tr._zm(c, s, [a + mq * b for a, b in zip(mv(A, u), B)])
    return np.stack([np.stack(e, 1) for e in dE], 1), np.stack(dm, 1)


def jvp_scaled(route, pulse, df, pos, ntr, phases, gains, echo, v, dm0, scales, m0, meq, demod, dtype, **kw):
    """The tangent of the scale sweep by route (tiled_jvp or train_jvp): ((dex, dey, dez) each (K, S, ntr, nf, npos), (dfx, dfy, dfz)
    each (K, S, nf, npos)); m0 and dm0 are the same at every scale"""
    r = [route(pulse, df, pos, ntr, phases, gains, echo, v, dm0, s, m0, meq, demod, dtype, **kw) for s in scales]
    return (tuple(np.stack([e[:, :, i] for e, _ in r], 1) for i in range(3)),
            tuple(np.stack([f[:, i] for _, f in r], 1) for i in range(3)))


# ---- the cases that tests/test_blochtrainjvp_cpu.py and tests/test_blochtrainjvp_gpu.py share ---------------------------------
cases = vjp.cases


@functools.lru_cache(maxsize=None)
def directions(name, K):
    """Per pulse of the case (or of small() for name 'small') K directions v (K, n) ~ (N(0,1) + i N(0,1)) max|b1| and dm0, a triple
    of (K, nf, npos) ~ N(0,1), drawn direction by direction: the first directions do not depend on K"""
    c = small() if name == "small" else cases()[name]
    return jv.directions(c["pulses"], c["dfs"], c["dps"], K)


small = vjp.small


def run(route, c, q, v, dm0, dtype, **kw):
    """route on pulse q of the case c over its scales"""
    return jvp_scaled(route, c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], v, dm0,
                      c["scales"], c["m0"][q], c["meq"], c["demod"], dtype, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, K):
    """The long-double structured route of a case along directions(name, K): per pulse (dE, dF), computed once.  A prefix of the
    directions has the prefix of the result."""
    c = cases()[name]
    vs, dms = directions(name, K)
    return [run(train_jvp, c, q, vs[q], dms[q], np.longdouble) for q in range(len(c["pulses"]))]


def drive(c, q, v):
    """D1 (K,): max|scale gain| gamma sum_t dt_t |v_t|, the angle by which a unit of v turns one repetition"""
    p = c["pulses"][q]
    v = np.asarray(v).reshape(-1, len(p[0]))
    return vjp.amax_of(c, q) * tr.gamma_of(p[5]) * (tr.intervals(p) * np.abs(v)).sum(1)


def mu_of(c, q, meq=None):
    return tr.mu_of(c["m0"][q], c["meq"] if meq is None else meq, len(c["dfs"][q]), len(c["dps"][q]))


def size_jvp(c, q, v, dm0):
    """ntr D1 mu + |dm0|_1 per entry of direction k, (K, nf, npos): the size of the tangent"""
    size = 0.0 if dm0 is None else np.abs(dm0[0]) + np.abs(dm0[1]) + np.abs(dm0[2])
    return c["ntr"][q] * drive(c, q, v)[:, None, None] * mu_of(c, q) + size


def bound_jvp(c, q, v, dm0):
    """(K, nf, npos), the same at every scale and repetition"""
    return TOL * c["ntr"][q] * size_jvp(c, q, v, dm0)


def identity_tol(c, q, v, dm0):
    """The tolerance of sum ce . decho + sum cf . dm_N = Re sum conj(G) v + sum gm0 . dm_0 for one direction v (n,), dm0 a triple of
    (nf, npos) (or None): sum_t bound_b1_t |v_t| + sum bound_m0 |dm_0| + sum |cot| bound_jvp, the two sides' own bounds"""
    bj = bound_jvp(c, q, v, None if dm0 is None else tuple(np.asarray(d)[None] for d in dm0))[0]           # (nf, npos)
    left = 0.0
    for tri in (c["ce"][q], c["cf"][q]):
        if tri is not None:
            left += float(sum((np.abs(ck) * bj).sum() for ck in tri))
    right = float((vjp.bound_b1(c, q) * np.abs(v)).sum())
    if dm0 is not None:
        right += float(sum((vjp.bound_m0(c, q) * np.abs(d)).sum() for d in dm0))
    return left + right


def pairing(c, q, dE, dF):
    """sum ce . decho + sum cf . dm_N of pulse q for one direction: dE three (S, ntr, nf, npos), dF three (S, nf, npos)"""
    L = 0.0
    if c["ce"][q] is not None:
        L = L + sum(float((np.asarray(ck) * e).sum()) for ck, e in zip(c["ce"][q], dE))
    if c["cf"][q] is not None:
        L = L + sum(float((np.asarray(ck) * f).sum()) for ck, f in zip(c["cf"][q], dF))
    return L
