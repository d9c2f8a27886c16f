"""NumPy restatement of the adjoint of a pulse train with respect to its schedule, the gain and the RF phase of every repetition
(helper of tests/test_blochtrainsched_cpu.py and tests/test_blochtrainsched_gpu.py; not collected), vectorised over the (frequency,
position) points, in float64 or np.longdouble, on tests/blochtrainvjp_ref.py (the cases, the cotangents, the tiled adjoint's sample
steps) and tests/blochtrainjvp_ref.py (the period's tangent, _step and _dn).

The loss is blochtrainvjp_ref's, L = sum_k <ce_k, echo_k> + <cf, m_N>; repetition k plays scale gains[k] e^{i phases[k]} b1.  Two
routes to the same (gg, gp, dL/dm0), gg[k] = dL/dgains[k] and gp[k] = dL/dphases[k], one entry per repetition, summed over the points:
    sched_vjp:   the structured route in the device's order.  The period's planes (A, B, A_e, B_e) at the amplitude scale
                 x gain and their tangent along the period's own b1 at the amplitude `scale` alone (d amplitude / d gain = scale;
                 nothing is divided by a gain, so a gain of 0 is an ordinary case); then lambda through the repetitions in reverse with
                     u_k = Z(+phi_k) m_k,  a_k = Z(+phi_k) lambda_{k+1},  ae_k = Z(+phi_k) ce_k (demod: ce_k),  J v = (-v_y, v_x, 0)
                     gg[k] = a_k . (dA u_k + meq dB) + ae_k . (dA_e u_k + meq dB_e)
                     gp[k] = a_k . A (J u_k) - lambda_{k+1} . J m_{k+1} + ae_k . A_e (J u_k) - (demod ? 0 : ce_k . J echo_k)
                 written with m_{k+1} and echo_k themselves (the device forms the same two terms as a_k . J n_k and ae_k . J ne_k).
    tiled_sched: an independent route: the reversed recursion over the tiled waveform (blochtrainvjp_ref.tiled_vjp's steps) with the
                 gradient G_w[k, t] = dL/dRe w + i dL/dIm w of every tiled sample w[k, t] = scale gains[k] e^{i phi_k} b1_t kept per
                 repetition, contracted with dw/dgains[k] = scale e^{i phi_k} b1_t and dw/dphases[k] = i w:
                     gg[k] = sum_t Re(conj(G_w) scale e^{i phi_k} b1_t),   gp[k] = sum_t Re(conj(G_w) i w) + (demod: ce_k . J echo_k)
                 the last term because the demodulated echo Z(+phi_k) echo^lab_k depends on phi_k explicitly, d Z(phi) e / d phi =
                 J Z(phi) e.  The signs were fixed against the central differences of blochtrain_ref.train
                 (tests/test_blochtrainsched_cpu.py holds both routes to them).

Cases: blochtrainvjp_ref.cases() and three more.
    repeat:   gains (0.5, 0.5, 1.0, 0.5): one gain value on three repetitions, each with its own entry of gg.
    zerogain: gains (1.0, 0.0, 0.7), two scales, demodulated echoes.
    hard:     one on-resonance sample, real b1, T1 = T2 = 1e12, meq = 0, m0 = z, phases 0, echo = 1.  Nothing decays (T2 = 1e12), so
              the flips add up: with theta = gamma b1 dt and Th_k = theta (gains_0 + .. + gains_{k-1}), m_k = (0, sin Th_k, cos Th_k)
              and echo_k = m_{k+1}, whence
                  gg[j] = theta (sum_{k >= j} (cey_k cos Th_{k+1} - cez_k sin Th_{k+1}) + cfy cos Th_N - cfz sin Th_N)
                  gp[k] = (sin Th_{k+1} - sin Th_k) (sum_{k' >= k} cex_k' + cfx)
              (a phase turns the axis of one repetition in the plane: d m_{k+1} / d phi_k = (R J - J R) m_k, along x, which the later
              on-resonance rotations about x leave alone).  The product form m_z = prod cos(gains_k theta), echo_k = sin(gains_k theta)
              prod_{j<k} cos(gains_j theta) is the perfectly spoiled train's, T2 << TR; at T2 = 1e12 this case has the sums above.
              1 - E1 = 2.5e-16 here: the closed form's own error is far below the bounds.

Bounds (bound_gains, bound_phases), with N = (1-norm of all cotangents of the pulse) x sqrt(3) max(|m0|inf, |meq|, 1), the second
factor being blochtrain_ref's bound of |m_k|_2, and Theta = gamma sum_t |b1_t| dt_t the angle by which a unit gain turns a repetition:
    per gains entry    TOL ntr N max|scale| Theta
    per phases entry   TOL ntr N
A multiplier never grows (every reverse step is the transpose of a contraction), so |a_k|_1 and |ae_k|_1 summed over the points and
scales stay below the cotangents' 1-norm; |dA u + meq dB| <= scale Theta |m|_2 bound (every sample's tangent adds at most its own
angle times the state) and |A J u - J n| <= 2 |m|_2 bound: N max|scale| Theta and N are the sizes of an entry.  The roundings of u_k,
a_k and the planes are blochtrainvjp_ref's, each of the ntr repetitions adding its own share: hence the factor ntr, as there.
TOL = blochgrad_ref.TOL = 1e-12 was measured, not assumed: over cases() the float64 twin of sched_vjp differs from its long-double
twin by at most 6.3e-5 of the gains bound and 3.6e-5 of the phases bound (the 257-sample pulses of the cases "shared" and "batch";
tests/test_blochtrainsched_cpu.py prints every share), within the hundredth that the CPU test asserts, so the constant stands as it started: before 1e-12, after 1e-12.  dL/dm0 has
blochtrainvjp_ref.bound_m0.  The device's shares are printed by tests/test_blochtrainsched_gpu.py and quoted in DESIGN section 8ad.

Central differences (FD_ANGLE, FD_TOL of blochtrainvjp_ref), one repetition moved at a time.  gains[k] is moved by h = FD_ANGLE /
(max|scale| Theta), so that the repetition turns by FD_ANGLE = 1e-5 rad more or less; phases[k] by h = FD_ANGLE itself.  In units of
the entry's size (N max|scale| Theta, or N) the central difference is off by its truncation, FD_ANGLE^2 / 6 = 1.7e-11 (the third
derivative in one repetition's angle is at most the size), plus the rounding of the two losses over 2 h: a float64 train is held to
200 u ntr (ntime + 4) mu per entry (blochtrain_ref), 1.2e-12 mu at ntr = 4 and ntime = 9, so the quotient is off by at most 1.2e-12
mu |c|_1 / FD_ANGLE = 1.2e-7 mu |c|_1 = 6.7e-8 N.  FD_TOL = 1e-7 in units of ntr N max|scale| Theta (ntr N for a phase), ntr >= 3 in
the three cases, covers the float64 device call and the float64 reference with a factor 4 to spare and the long-double reference
with many orders."""
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


jvp = _load("blochtrainjvp_ref")
vjp = jvp.vjp
tr = vjp.tr
_grad = tr._grad

TOL = _grad.TOL
FD_ANGLE, FD_TOL = vjp.FD_ANGLE, vjp.FD_TOL


def _J(v):
    return [-v[1], v[0], np.zeros_like(v[2])]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def prop_dgain(pulse, df, pos, amp, scale, echo, dtype=np.float64):
    """((A, B, Ae, Be), (dA, dB, dAe, dBe)) of the period at RF amplitude amp and phase 0, the tangent along the period's own b1 at
    the amplitude `scale` (d amp / d gain): blochtrainjvp_ref.prop_jvp with the direction's amplitude apart from the primal's"""
    Q = tr._setup(pulse, df, pos, amp, dtype)
    v = np.asarray(pulse[0], dtype=np.complex128).reshape(1, Q.n)
    dnx, dny = jvp._dn(Q, v, scale, dtype)
    one, zero = np.ones((Q.nf, Q.npos), dtype=dtype), np.zeros((Q.nf, Q.npos), dtype=dtype)
    X = [np.stack([one if i == j else zero for j in range(3)] + [zero]) for i in range(3)]
    dX = [np.zeros((1, 4, Q.nf, Q.npos), dtype=dtype) for _ in range(3)]
    rec = np.array([0, 0, 0, 1], dtype=dtype)[:, None, None]
    Xe, dXe = X, dX
    for t in range(Q.n):
        X, dX = jvp._step(Q, t, np.full_like(zero, Q.rotx[t]), np.full_like(zero, Q.roty[t]), X, dX, dnx[:, t, None, None, None],
                          dny[:, t, None, None, None], rec)
        if t + 1 == echo:
            Xe, dXe = X, dX
    mat = lambda Y, d: [[Y[i][0, j] if d else Y[i][j] for j in range(3)] for i in range(3)]
    vec = lambda Y, d: [Y[i][0, 3] if d else Y[i][3] for i in range(3)]
    return (mat(X, 0), vec(X, 0), mat(Xe, 0), vec(Xe, 0)), (mat(dX, 1), vec(dX, 1), mat(dXe, 1), vec(dXe, 1))


def sched_vjp(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(gg (ntr,), gp (ntr,), dL/dm0 as three (nf, npos) arrays) at one scale by the structured route"""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Ps = {a: prop_dgain(pulse, df, pos, a, np.float64(scale), echo, dtype) for a in set(amps.tolist())}
    Q0 = tr._setup(pulse, df, pos, 1.0, dtype)
    mq, mv = dtype(meq), _grad._mat_vec
    m, us, ms, es = tr._start(m0, Q0, dtype), [], [], []
    for k in range(ntr):
        (A, B, Ae, Be), _ = Ps[float(amps[k])]
        u = tr._zp(cs[k], sn[k], m)
        us.append(u)
        e = [x + mq * y for x, y in zip(mv(Ae, u), Be)]
        es.append(e if demod else tr._zm(cs[k], sn[k], e))
        m = tr._zm(cs[k], sn[k], [x + mq * y for x, y in zip(mv(A, u), B)])
        ms.append(m)                                                    # m_{k+1}
    e, lam = vjp._cots(ce, cf, ntr, Q0, dtype)
    gg, gp = np.zeros(ntr, dtype=dtype), np.zeros(ntr, dtype=dtype)
    for k in range(ntr - 1, -1, -1):
        (A, B, Ae, Be), (dA, dB, dAe, dBe) = Ps[float(amps[k])]
        c, s, u = cs[k], sn[k], us[k]
        a = tr._zp(c, s, lam)
        g = _dot(a, [x + mq * y for x, y in zip(mv(dA, u), dB)])
        p = _dot(a, mv(A, _J(u))) - _dot(lam, _J(ms[k]))
        lam = mv(A, a, transpose=True)
        if e is not None:
            ae = e[k] if demod else tr._zp(c, s, e[k])
            g = g + _dot(ae, [x + mq * y for x, y in zip(mv(dAe, u), dBe)])
            p = p + _dot(ae, mv(Ae, _J(u)))
            if not demod:
                p = p - _dot(e[k], _J(es[k]))
            lam = [x + y for x, y in zip(lam, mv(Ae, ae, transpose=True))]
        lam = tr._zm(c, s, lam)
        gg[k], gp[k] = g.sum(), p.sum()
    return gg, gp, lam


def tiled_sched(pulse, df, pos, ntr, phases, gains, echo, ce, cf, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(gg (ntr,), gp (ntr,), dL/dm0) at one scale from the gradient of every sample of the tiled waveform, kept per repetition"""
    cs, sn = tr._table(phases, dtype)
    amps = tr._amps(scale, gains)
    Qs = {a: tr._setup(pulse, df, pos, a, dtype) for a in set(amps.tolist())}
    Q0 = next(iter(Qs.values()))
    n, mq = Q0.n, dtype(meq)
    b1 = np.asarray(pulse[0], dtype=np.complex128).astype(vjp._ctype(dtype))
    m, traj, E = tr._start(m0, Q0, dtype), [], []
    for k in range(ntr):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        if echo == 0:
            E.append(m)
        for t in range(n):
            traj.append(m)
            nz = Q.rotz[t]
            m = vjp._fwd(Q, t, np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t]), m, mq)
            if t + 1 == echo:
                E.append(m)
    e, lam = vjp._cots(ce, cf, ntr, Q0, dtype)
    gg, gp = np.zeros(ntr, dtype=dtype), np.zeros(ntr, dtype=dtype)
    for k in range(ntr - 1, -1, -1):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        inj = None if e is None else (tr._zm(c, s, e[k]) if demod else e[k])
        rot = c + 1j * s                                                # e^{i phi_k}
        for t in range(n - 1, -1, -1):
            if inj is not None and t + 1 == echo:
                lam = [a + b for a, b in zip(lam, inj)]
            nz = Q.rotz[t]
            gx, gy, lam = vjp._bwd(Q, t, np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t]), np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t]),
                                   traj[k * n + t], lam)
            f = dtype(Q.gamma) * dtype(Q.dt[t])
            gw = -(f * gx.sum()) + 1j * (f * gy.sum())                  # dL/dRe w + i dL/dIm w of the tiled sample
            dwg = dtype(scale) * rot * b1[t]
            w = dtype(amps[k]) * rot * b1[t]
            gg[k] += (np.conj(gw) * dwg).real
            gp[k] += (np.conj(gw) * (1j * w)).real
        if inj is not None and echo == 0:
            lam = [a + b for a, b in zip(lam, inj)]
        if demod and e is not None:                                     # the demodulated echo's own dependence on phi_k
            gp[k] += _dot(e[k], _J(tr._zp(c, s, E[k]))).sum()
    return gg, gp, lam


def sched_scaled(route, pulse, df, pos, ntr, phases, gains, echo, ce, cf, scales, m0, meq, demod, dtype):
    """The adjoint of the scale sweep by route: (gg (ntr,), gp (ntr,), (gmx, gmy, gmz) each (S, nf, npos))"""
    gg, gp, gm = 0, 0, []
    for k, s in enumerate(scales):
        r = route(pulse, df, pos, ntr, phases, gains, echo, None if ce is None else [c[k] for c in ce],
                  None if cf is None else [c[k] for c in cf], s, m0, meq, demod, dtype)
        gg, gp = gg + r[0], gp + r[1]
        gm.append(r[2])
    return gg, gp, tuple(np.stack([l[c] for l in gm]) for c in range(3))


# ---- the cases that tests/test_blochtrainsched_cpu.py and tests/test_blochtrainsched_gpu.py share ------------------------------
HARD_THETA = 0.4


@functools.lru_cache(maxsize=None)
def cases():
    """blochtrainvjp_ref.cases() plus 'repeat', 'zerogain' and 'hard' (module docstring), in blochtrainvjp_ref's format"""
    rng = np.random.default_rng(37)
    out = {k: v for k, v in vjp.cases().items()}
    f3, p2 = tr._grid(3, 60.0), np.array([[-1.0], [0.7]])

    def cots(c):
        S, ce, cf = len(c["scales"]), [], []
        for q in range(len(c["pulses"])):
            nf, npos = len(c["dfs"][q]), len(c["dps"][q])
            ce.append(tuple(rng.standard_normal((3, S, c["ntr"][q], nf, npos))) if c["cot"] != "final" else None)
            cf.append(tuple(rng.standard_normal((3, S, nf, npos))) if c["cot"] != "echo" else None)
        c["ce"], c["cf"] = ce, cf
        return c

    out["repeat"] = cots(dict(pulses=[tr._period(rng, 9, *tr.C13, 0.6, 4e-3, True)], dfs=[f3], dps=[p2], ntr=[4],
                              phases=[np.array([0.4, -1.3, 2.2, 0.9])], gains=[np.array([0.5, 0.5, 1.0, 0.5])], echo=[4],
                              m0=[tr._m0(rng, 3, 2)], scales=(1.0,), cot="both", demod=False, meq=1.0))
    out["zerogain"] = cots(dict(pulses=[tr._period(rng, 9, *tr.H1, 0.9, 2e-3, True)], dfs=[f3], dps=[p2], ntr=[3],
                                phases=[np.array([0.0, 2.0, -1.0])], gains=[np.array([1.0, 0.0, 0.7])], echo=[9],
                                m0=[tr._m0(rng, 3, 2)], scales=(0.9, 1.1), cot="both", demod=True, meq=1.0))
    dt = 1e-3
    b1 = np.array([HARD_THETA / (tr.gamma_of("H-1") * dt)], dtype=np.complex128)
    z = (np.zeros((1, 1)), np.zeros((1, 1)), np.ones((1, 1)))
    out["hard"] = cots(dict(pulses=[(b1, None, np.array([dt]), 1e12, 1e12, "H-1")], dfs=[np.zeros(1)], dps=[np.zeros((1, 1))], ntr=[4],
                            phases=[np.zeros(4)], gains=[np.array([0.3, 0.8, 0.5, 1.1])], echo=[1], m0=[z], scales=(1.0,), cot="both",
                            demod=False, meq=0.0))
    return out


small = vjp.small
FD_CASES = ("small", "repeat", "zerogain")


def case(name):
    return small() if name == "small" else cases()[name]


def hard_closed():
    """(gg, gp) of the case 'hard' from its closed forms (module docstring)"""
    c = cases()["hard"]
    g, N = c["gains"][0], c["ntr"][0]
    ce = [np.asarray(v, dtype=np.float64).reshape(N) for v in c["ce"][0]]
    cf = [float(np.asarray(v).reshape(())) for v in c["cf"][0]]
    Th = HARD_THETA * np.concatenate([[0.0], np.cumsum(g)])             # Th[k]: the angle of m_k
    along = ce[1] * np.cos(Th[1:]) - ce[2] * np.sin(Th[1:])            # d <ce_k, echo_k> / d Th_{k+1}
    fin = cf[1] * np.cos(Th[N]) - cf[2] * np.sin(Th[N])
    gg = HARD_THETA * (np.cumsum(along[::-1])[::-1] + fin)
    gp = (np.sin(Th[1:]) - np.sin(Th[:-1])) * (np.cumsum(ce[0][::-1])[::-1] + cf[0])
    return gg, gp


def run(route, c, q, dtype):
    """route on pulse q of the case c over its scales"""
    return sched_scaled(route, c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q],
                        c["ce"][q], c["cf"][q], c["scales"], c["m0"][q], c["meq"], c["demod"], dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The long-double structured route of a case: per pulse (gg, gp, (gmx, gmy, gmz)), computed once"""
    c = case(name)
    return [run(sched_vjp, c, q, np.longdouble) for q in range(len(c["pulses"]))]


def smax_of(c):
    return max(abs(s) for s in c["scales"])


def theta_of(c, q):
    """Theta = gamma sum_t |b1_t| dt_t"""
    p = c["pulses"][q]
    return float(tr.gamma_of(p[5]) * (np.abs(np.asarray(p[0])) * tr.intervals(p)).sum())


def norm_of(c, q):
    """N: the 1-norm of all cotangents of pulse q times sqrt(3) max(|m0|inf, |meq|, 1)"""
    mu = tr.mu_of(c["m0"][q], c["meq"], len(c["dfs"][q]), len(c["dps"][q])).max()
    return vjp.norm1(c, q) * np.sqrt(3.0) * float(mu)


def scale_gains(c, q):
    return c["ntr"][q] * norm_of(c, q) * smax_of(c) * theta_of(c, q)


def scale_phases(c, q):
    return c["ntr"][q] * norm_of(c, q)


def bound_gains(c, q):
    return TOL * scale_gains(c, q)


def bound_phases(c, q):
    return TOL * scale_phases(c, q)


bound_m0 = vjp.bound_m0
loss = vjp.loss


def fd_steps(c, q):
    """(h of a gain, h of a phase)"""
    return FD_ANGLE / (smax_of(c) * theta_of(c, q)), FD_ANGLE


def fd_schedules(c, q, which=None):
    """The perturbed schedules of the central differences of pulse q, in order: for every repetition k in `which` (None: all) the four
    (gains, phases) pairs (g + h e_k, p), (g - h e_k, p), (g, p + h e_k), (g, p - h e_k)"""
    g, p = np.asarray(c["gains"][q], dtype=np.float64), np.asarray(c["phases"][q], dtype=np.float64)
    hg, hp = fd_steps(c, q)
    out = []
    for k in (range(c["ntr"][q]) if which is None else which):
        e = np.zeros(len(g))
        e[k] = 1.0
        out += [(g + hg * e, p), (g - hg * e, p), (g, p + hp * e), (g, p - hp * e)]
    return out


def fd_quotients(c, q, losses):
    """(dL/dgains[k], dL/dphases[k]) per perturbed repetition from the total losses of fd_schedules' trains, in its order"""
    hg, hp = fd_steps(c, q)
    L = np.asarray(losses, dtype=np.longdouble).reshape(-1, 4)
    return (L[:, 0] - L[:, 1]) / (2 * hg), (L[:, 2] - L[:, 3]) / (2 * hp)
