"""NumPy restatement of the tangent of a pulse train in its schedule, the gain and the RF phase of every repetition, and in the
initial magnetisation (helper of tests/test_blochtrainschedjvp_cpu.py and tests/test_blochtrainschedjvp_gpu.py; not collected),
vectorised over the (frequency, position) points, in float64 or np.longdouble, on tests/blochtrainsched_ref.py (the cases, prop_dgain,
the adjoint it is paired with) and tests/blochtrain_ref.py.

Repetition k plays scale gains[k] e^{i phases[k]} b1.  A direction is (dg (ntr,), dp (ntr,), dm0); dp is per radian.  Two routes to
the same (dE, dF), the tangents of the echoes and of the final state:
    sched_jvp:  the structured route in the device's order.  With the period's planes (A, B, A_e, B_e) at the amplitude
                scale x gain and their tangent (dA, dB, dA_e, dB_e) along the period's own b1 at the amplitude `scale` alone
                (blochtrainsched_ref.prop_dgain; nothing is divided by a gain), J v = (-v_y, v_x, 0):
                    u_k  = Z(+phi_k) m_k                 du_k  = Z(+phi_k) dm_k + dp_k J u_k
                    n_k  = A u_k + meq B                 dn_k  = A du_k   + dg_k (dA u_k   + meq dB)
                    ne_k = A_e u_k + meq B_e             dne_k = A_e du_k + dg_k (dA_e u_k + meq dB_e)
                    m_{k+1} = Z(-phi_k) n_k              dm_{k+1} = Z(-phi_k) (dn_k  - dp_k J n_k)
                    echo_k  = Z(-phi_k) ne_k             decho_k  = Z(-phi_k) (dne_k - dp_k J ne_k)      (demod: decho_k = dne_k)
    tiled_jvp:  an independent route: the tangent of the sample-by-sample recursion over the tiled waveform
                (blochtrainjvp_ref._step, as blochtrainjvp_ref.tiled_jvp walks it), the direction of the tiled sample (k, t) being
                    dw = (dg_k + i dp_k gains[k]) scale e^{i phi_k} b1_t
                (d/dgains[k] of w = scale gains[k] e^{i phi_k} b1_t is scale e^{i phi_k} b1_t, d/dphases[k] is i w).  The demodulated
                echo Z(+phi_k) echo^lab_k depends on phi_k explicitly as well, d Z(phi) e / d phi = J Z(phi) e: demod adds dp_k J echo_k.

Directions (directions(name, K)), per pulse, direction j of kind j mod 3, each drawn from its own seeded generator so that a
direction does not depend on K:
    0: the unit gains direction on the last repetition;  1: the unit phases direction on the first repetition;
    2: dense, dg, dp and dm0 all ~ N(0, 1).

Bound per entry at a point, the same at every scale, repetition and component (bound_jvp):
    TOL ntr size,   size = mu (sum_k |dg_k| max|scale| Theta + 2 sum_k |dp_k|) + |dm0|_1 at the point,
mu = max(|m0|inf, |meq|, 1), Theta = gamma sum_t |b1_t| dt_t the angle by which a unit gain turns a repetition.  size is the size of
the tangent: a repetition's maps are contractions, so what a repetition injects is never amplified; repetition k injects dg_k (dA u +
meq dB), at most |dg_k| scale Theta mu (every sample's tangent adds at most its own angle times the state), and dp_k (A J u - J n), at
most 2 |dp_k| mu; dm0 passes through contractions.  The roundings of u_k, du_k and the planes are blochtrainjvp_ref's, each of the ntr
repetitions adding its own share: hence the factor ntr, as there.  TOL = blochgrad_ref.TOL = 1e-12 was measured, not assumed: over
cases() and the three kinds of direction the float64 twin of sched_jvp differs from its long-double twin by at most 2.0e-3 of this
bound (the second pulse of the case "batch", ntr = 1; tests/test_blochtrainschedjvp_cpu.py prints every share), within the hundredth
that the CPU test asserts, so the constant stands as it started: before 1e-12, after 1e-12.  The tangent itself reaches 0.88 of size
(the unit directions of the case "hard").
The device's shares are printed by tests/test_blochtrainschedjvp_gpu.py and quoted in DESIGN section 8ae.

Central differences (FD_ANGLE, FD_TOL of blochtrainvjp_ref) along one direction (dg, dp, dm0).  The step is h = FD_ANGLE / max_k a_k,
a_k = |dg_k| max|scale| Theta + |dp_k|, so that no repetition turns, and no repetition's axis swings, by more than FD_ANGLE = 1e-5
rad; m0 moves by h dm0, in which the train is affine.  In units of ntr size the central difference is off by its truncation, at most
(h sum_k a_k)^2 / 6 <= (ntr FD_ANGLE)^2 / 6 = 2.7e-10 of the tangent's size at ntr = 4 (the third derivative along the direction is
at most (sum_k a_k)^3 mu), plus the rounding of the two trains over 2 h: a float64 train is held to 200 u ntr (ntime + 4) mu per
entry (blochtrain_ref), 1.2e-12 mu at ntr = 4 and ntime = 9, so the quotient is off by at most 1.2e-12 mu max_k a_k / FD_ANGLE =
1.2e-7 mu max_k a_k <= 1.2e-7 size, which is 4e-8 of ntr size at ntr = 3.  FD_TOL = 1e-7 in units of ntr size covers the float64
device call with a factor 2 to spare on a worst-case rounding bound, and the long-double reference with many orders."""
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


sched = _load("blochtrainsched_ref")
jvp = sched.jvp
vjp = sched.vjp
tr = sched.tr
_grad = tr._grad

TOL = _grad.TOL
FD_ANGLE, FD_TOL = vjp.FD_ANGLE, vjp.FD_TOL
cases, case, small = sched.cases, sched.case, sched.small
FD_CASES = sched.FD_CASES
_J = sched._J


def _dirs(dg, dp, dm0, ntr, Q, dtype):
    """dg / dp: None (zero), (ntr,) or (K, ntr) -> (K, ntr) in dtype; dm0 -> three (K, nf, npos)"""
    given = [np.asarray(d, dtype=np.float64).reshape(-1, ntr) for d in (dg, dp) if d is not None]
    K = given[0].shape[0] if given else np.broadcast(*[np.asarray(d) for d in dm0]).shape[0]
    dg, dp = [np.zeros((K, ntr), dtype=dtype) if d is None else np.asarray(d, dtype=np.float64).reshape(K, ntr).astype(dtype)
              for d in (dg, dp)]
    return dg, dp, jvp.jv._dm0(dm0, K, Q.nf, Q.npos, dtype)


def sched_jvp(pulse, df, pos, ntr, phases, gains, echo, dg, dp, dm0=None, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(dE (K, ntr, 3, nf, npos), dF (K, 3, nf, npos)) at one scale by the structured route, in the device's order"""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Ps = {a: sched.prop_dgain(pulse, df, pos, a, np.float64(scale), echo, dtype) for a in set(amps.tolist())}
    Q0 = tr._setup(pulse, df, pos, 1.0, dtype)
    dg, dp, dm = _dirs(dg, dp, dm0, ntr, Q0, dtype)
    m, mq, mv, dE = tr._start(m0, Q0, dtype), dtype(meq), _grad._mat_vec, []
    for k in range(ntr):
        (A, B, Ae, Be), (dA, dB, dAe, dBe) = Ps[float(amps[k])]
        c, s = cs[k], sn[k]
        g, p = dg[:, k, None, None], dp[:, k, None, None]
        u = tr._zp(c, s, m)
        du = [a + p * b for a, b in zip(tr._zp(c, s, dm), _J(u))]
        e = [a + mq * b for a, b in zip(mv(Ae, u), Be)]
        ge = [a + mq * b for a, b in zip(mv(dAe, u), dBe)]
        de = [a + g * b for a, b in zip(mv(Ae, du), ge)]
        if not demod:
            de = tr._zm(c, s, [a - p * b for a, b in zip(de, _J(e))])
        dE.append(de)
        n = [a + mq * b for a, b in zip(mv(A, u), B)]
        gn = [a + mq * b for a, b in zip(mv(dA, u), dB)]
        dn = [a + g * b for a, b in zip(mv(A, du), gn)]
        dm = tr._zm(c, s, [a - p * b for a, b in zip(dn, _J(n))])
        m = tr._zm(c, s, n)
    return np.stack([np.stack(e, 1) for e in dE], 1), np.stack(dm, 1)


def tiled_jvp(pulse, df, pos, ntr, phases, gains, echo, dg, dp, dm0=None, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(dE, dF) at one scale by the tangent of the recursion over the tiled waveform, the direction formed per repetition"""
    T = dtype
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Qs = {a: tr._setup(pulse, df, pos, a, dtype) for a in set(amps.tolist())}
    Q0 = next(iter(Qs.values()))
    dg, dp, dm = _dirs(dg, dp, dm0, ntr, Q0, dtype)
    b1 = np.asarray(pulse[0], dtype=np.complex128)
    br, bi = b1.real.astype(T)[None], b1.imag.astype(T)[None]
    dtl, gl, sl = Q0.dt.astype(T), T(Q0.gamma), T(np.float64(scale))
    m, mq, dE = tr._start(m0, Q0, dtype), dtype(meq), []

    def echo_of(k, c, s, m, dm):
        if not demod:
            return dm
        return [a + dp[:, k, None, None] * b for a, b in zip(tr._zp(c, s, dm), _J(tr._zp(c, s, m)))]
    for k in range(ntr):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        gk = T(np.float64(np.asarray(gains, dtype=np.float64)[k]))
        a, b = dg[:, k, None], dp[:, k, None] * gk                      # dw / (scale e^{i phi_k}) = (a + i b) b1_t
        dnx = ((-((a * br - b * bi) * sl)) * gl) * dtl                  # (K, n), as rotx / roty are formed
        dny = (((a * bi + b * br) * sl) * gl) * dtl
        if echo == 0:
            dE.append(echo_of(k, c, s, m, dm))
        for t in range(Q.n):
            nz = Q.rotz[t]
            nx, ny = np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t])
            dx = (c * dnx[:, t] + s * dny[:, t])[:, None, None]
            dy = (c * dny[:, t] - s * dnx[:, t])[:, None, None]
            m, dm = jvp._step(Q, t, nx, ny, m, dm, dx, dy, mq)
            if t + 1 == echo:
                dE.append(echo_of(k, c, s, m, dm))
    return np.stack([np.stack(e, 1) for e in dE], 1), np.stack(dm, 1)


def jvp_scaled(route, pulse, df, pos, ntr, phases, gains, echo, dg, dp, dm0, scales, m0, meq, demod, dtype):
    """The tangent of the scale sweep by route: ((dex, dey, dez) each (K, S, ntr, nf, npos), (dfx, dfy, dfz) each (K, S, nf, npos));
    m0 and the direction are the same at every scale"""
    r = [route(pulse, df, pos, ntr, phases, gains, echo, dg, dp, dm0, s, m0, meq, demod, dtype) for s in scales]
    return (tuple(np.stack([e[:, :, i] for e, _ in r], 1) for i in range(3)),
            tuple(np.stack([f[:, i] for _, f in r], 1) for i in range(3)))


# ---- what tests/test_blochtrainschedjvp_cpu.py and tests/test_blochtrainschedjvp_gpu.py share ----------------------------------
@functools.lru_cache(maxsize=None)
def directions(name, K):
    """Per pulse of the case (dg (K, ntr), dp (K, ntr), dm0: a triple of (K, nf, npos)), the three kinds of the module docstring
    cycled; direction j of pulse q comes from its own generator"""
    c = case(name)
    out = []
    for q in range(len(c["pulses"])):
        n, nf, npos = c["ntr"][q], len(c["dfs"][q]), np.shape(c["dps"][q])[0]
        dg, dp, d = np.zeros((K, n)), np.zeros((K, n)), np.zeros((3, K, nf, npos))
        for j in range(K):
            if j % 3 == 0:
                dg[j, n - 1] = 1.0
            elif j % 3 == 1:
                dp[j, 0] = 1.0
            else:
                rng = np.random.default_rng([41, q, j])
                dg[j], dp[j], d[:, j] = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal((3, nf, npos))
        out.append((dg, dp, tuple(d)))
    return out


def run(route, c, q, dg, dp, dm0, dtype):
    """route on pulse q of the case c over its scales"""
    return jvp_scaled(route, c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], dg, dp,
                      dm0, c["scales"], c["m0"][q], c["meq"], c["demod"], dtype)


@functools.lru_cache(maxsize=None)
def reference(name, K):
    """The long-double structured route of a case along directions(name, K): per pulse (dE, dF), computed once"""
    c = case(name)
    return [run(sched_jvp, c, q, *directions(name, K)[q], np.longdouble) for q in range(len(c["pulses"]))]


def unit_directions(ntr):
    """The 2 ntr unit directions, gains first then phases: (dg, dp), each (2 ntr, ntr)"""
    eye, zero = np.eye(ntr), np.zeros((ntr, ntr))
    return np.concatenate([eye, zero]), np.concatenate([zero, eye])


@functools.lru_cache(maxsize=None)
def jacobian(name):
    """The long-double structured route along the 2 ntr unit directions, per pulse (dE, dF)"""
    c = case(name)
    return [run(sched_jvp, c, q, *unit_directions(c["ntr"][q]), None, np.longdouble) for q in range(len(c["pulses"]))]


def mu_of(c, q):
    return tr.mu_of(c["m0"][q], c["meq"], len(c["dfs"][q]), len(c["dps"][q]))


def angles(c, q, dg, dp):
    """a_k = |dg_k| max|scale| Theta + |dp_k|, (K, ntr): by how much a unit of the direction turns repetition k or swings its axis"""
    ntr = c["ntr"][q]
    dg = np.zeros((1, ntr)) if dg is None else np.abs(np.asarray(dg, dtype=np.float64).reshape(-1, ntr))
    dp = np.zeros((1, ntr)) if dp is None else np.abs(np.asarray(dp, dtype=np.float64).reshape(-1, ntr))
    return dg * (sched.smax_of(c) * sched.theta_of(c, q)) + dp


def size_jvp(c, q, dg, dp, dm0):
    """mu (sum_k |dg_k| max|scale| Theta + 2 sum_k |dp_k|) + |dm0|_1 per entry of direction k, (K, nf, npos)"""
    a = angles(c, q, dg, None).sum(1) + 2.0 * angles(c, q, None, dp).sum(1)
    size = 0.0 if dm0 is None else np.abs(dm0[0]) + np.abs(dm0[1]) + np.abs(dm0[2])
    return np.reshape(a, (-1, 1, 1)) * mu_of(c, q) + size


def bound_jvp(c, q, dg, dp, dm0):
    """(K, nf, npos), the same at every scale, repetition and component"""
    return TOL * c["ntr"][q] * size_jvp(c, q, dg, dp, dm0)


def worst(got, want, scale):
    """The largest |got - want| / scale over the planes of (dE three (K, S, ntr, nf, npos), dF three (K, S, nf, npos)); scale: (K, nf,
    npos).  Either of dE / dF may be None on both sides."""
    w = 0.0
    if got[0] is not None:
        for g, r in zip(got[0], want[0]):
            w = max(w, float((np.abs(g - r) / scale[:, None, None]).max()))
    if got[1] is not None:
        for g, r in zip(got[1], want[1]):
            w = max(w, float((np.abs(g - r) / scale[:, None]).max()))
    return w


def pairing(c, q, dE, dF):
    """sum ce . decho + sum cf . dm_N of pulse q for one direction: dE three (S, ntr, nf, npos), dF three (S, nf, npos)"""
    return jvp.pairing(c, q, dE, dF)


def cot_norms(c, q):
    """(sum |ce| over everything but the points, sum |cf| likewise), each (nf, npos) (0.0 where the case has none)"""
    ce, cf = c["ce"][q], c["cf"][q]
    a = 0.0 if ce is None else sum(np.abs(np.asarray(v)).sum((0, 1)) for v in ce)
    b = 0.0 if cf is None else sum(np.abs(np.asarray(v)).sum(0) for v in cf)
    return a, b


def fd_step(c, q, dg, dp):
    """h of the central difference along one direction (dg (ntr,), dp (ntr,))"""
    return FD_ANGLE / float(angles(c, q, dg, dp).max())


def hard_closed():
    """(dE (2 ntr, ntr, 3), dF (2 ntr, 3)) of the case 'hard' along the 2 ntr unit directions from its closed forms: with Th_k the
    angle of m_k (blochtrainsched_ref.hard_closed), d m_k' / d gains_j = theta (0, cos Th_k', -sin Th_k') for j < k' and d m_k' / d
    phases_k = (sin Th_{k+1} - sin Th_k, 0, 0) for k < k'; echo_k = m_{k+1}"""
    c = cases()["hard"]
    g, N, th = c["gains"][0], c["ntr"][0], sched.HARD_THETA
    Th = th * np.concatenate([[0.0], np.cumsum(g)])
    dM = np.zeros((2 * N, N + 1, 3))                                     # the tangent of m_k', k' = 0 .. N
    for kp in range(N + 1):
        for j in range(min(kp, N)):
            dM[j, kp] = th * np.array([0.0, np.cos(Th[kp]), -np.sin(Th[kp])])
            dM[N + j, kp] = np.array([np.sin(Th[j + 1]) - np.sin(Th[j]), 0.0, 0.0])
    return dM[:, 1:], dM[:, N]
