"""NumPy restatement of the fused least-squares and Gauss-Newton products of a pulse train in its schedule, the gain and the RF phase
of every repetition (helper of tests/test_blochtrainschedgn_cpu.py and tests/test_blochtrainschedgn_gpu.py; not collected), in
float64 or np.longdouble, on tests/blochtrainsched_ref.py (the cases, the planes' tangent in the gain, the adjoint),
tests/blochtrainschedjvp_ref.py (the tangent and the directions) and tests/blochtraingn_ref.py (the dressing of a case with weights
and targets, the loss, the residuals' cotangents and the loss's and dL/dm0's bounds).  Those are imported, not edited, and no TOL of
theirs changes.

Per pulse, with echo_k and m_N what the train returns under the case's demod and the schedule (gains, phases) as the variable,
    L = 1/2 sum_s sum_k rw_k sum w_c (echo_kc - t_c)^2 + 1/2 sum_s sum wf_c (m_Nc - tf_c)^2
    gg[k] = dL/dgains[k], gp[k] = dL/dphases[k] (per radian): 8ad's contraction at ce_k = rw_k w (echo_k - t), cf = wf (m_N - tf);
            dL/dm0 is its lambda_0
    H v for v = (dg, dp): 8ae's recursion along v from dm_0 = 0 gives decho_k and dm_N; 8ad's contraction at ce_k = rw_k w decho_k,
            cf = wf dm_N, taken at the primal u_k.  (Hg, Hp) are its two halves.
Two routes, each in both precisions:
    structured (lsq, gn):           one walk per scale in the device's order.  Forwards, with (A, B, A_e, B_e) the planes
                                    at scale x gain and (dA, ..) their tangent in the gain, J v = (-v_y, v_x, 0):
                                        u_k = Z(+phi_k) m_k                    du_k = Z(+phi_k) dm_k + dp_k J u_k
                                        ne_k = A_e u_k + meq B_e               dne_k = A_e du_k + dg_k (dA_e u_k + meq dB_e)
                                        n_k = A u_k + meq B                    dn_k = A du_k + dg_k (dA u_k + meq dB)
                                        echo_k = Z(-phi_k) ne_k (demod: ne_k)  decho_k = Z(-phi_k) (dne_k - dp_k J ne_k) (demod: dne_k)
                                        m_{k+1} = Z(-phi_k) n_k                dm_{k+1} = Z(-phi_k) (dn_k - dp_k J n_k)
                                    then backwards from lambda_N = cf with a_k = Z(+phi_k) lambda_{k+1}, ae_k = Z(+phi_k) ce_k (demod: ce_k):
                                        gg[k] = a_k . (dA u_k + meq dB) + ae_k . (dA_e u_k + meq dB_e)
                                        gp[k] = a_k . A (J u_k) - lambda_{k+1} . J m_{k+1} + ae_k . A_e (J u_k) - (demod ? 0 : ce_k . J echo_k)
                                        lambda_k = Z(-phi_k) (A' a_k + A_e' ae_k)
    composed (lsq_composed, gn_composed): blochtraingn_ref's residual cotangents, or blochtrainschedjvp_ref.sched_jvp times the
                                    weights, handed to blochtrainsched_ref.sched_vjp.  The imported adjoint takes its cotangents
                                    through float64, a relative 2^-53 of the seed, so the two long-double routes agree to that
                                    and not to the last bit.  Every bound has the term TOL x (the size of what the seed can do), so
                                    the cast costs at most 2^-53 / TOL = 1.1e-4 of a bound; next to it stands the 1e-5 of the bounds
                                    that tests/test_blochtrainsched_cpu.py allows two long-double routes: ROUTE_TOL = 1e-5 + 2^-53 /
                                    TOL.  (The first comparison was made at 1e-5 alone and showed the cast: dL/dm0 of the case
                                    "one", ntr = 1, differed by 1.8e-5 of its bound.)

Cases: blochtrainsched_ref.cases() and small(), every one, dressed by blochtraingn_ref._dress (weights uniform in [0, 1] with every
third entry zero, targets uniform in [-1, 1], rep_weights with the first two zero where ntr > 2 and None for the call on NO_RW, a
final term where the case's cot has one; the broadcast form on BCAST, which are demodulated).

Bounds, composed through the seed as blochtraingn_ref composes its own.  Write bt = blochtrain_ref.bound_train(ntr, ntime, mu), the
bound of one echo or final entry at a point, bj = blochtrainschedjvp_ref.bound_jvp, the bound of one tangent entry, mu = max(|m0|inf,
|meq|, 1) at the point and Theta = gamma sum_t |b1_t| dt_t.  The weights are exact inputs, so the device's cotangent differs from the
reference's by at most rw_k w bt per entry (rw_k w bj for the products), wf bt for the final one.  The contraction is linear in the
cotangent.  A perturbation of the cotangent of 1-norm e at a point reaches a_k and ae_k through transposes of contractions, so with
no more than e; gg[k] pairs it with dA u + meq dB, at most max|scale| Theta mu (every sample's tangent adds at most its own angle
times the state), and gp[k] with A J u - J n, at most 2 mu.  So a gains entry moves by at most e max|scale| Theta mu and a phases entry
by at most 2 e mu, e summed over the points with each point's own mu (seed_reach).  Hence
    gg:   blochtrainsched_ref.bound_gains  at the reference cotangent + max|scale| Theta sum_points mu (sum rw w bt + sum wf bt)
    gp:   blochtrainsched_ref.bound_phases at the reference cotangent + 2             sum_points mu (sum rw w bt + sum wf bt)
    Hg, Hp: the same with bj in place of bt and the cotangent of the products
    dL/dm0 and L: blochtraingn_ref.bound_gm and bound_l themselves: the loss, its cotangent and the path to lambda_0 are the same
The constants are those of the imported references (TOL = 1e-12, C_BOUND = 200, L_QUAD = 1e-13); none was changed after a run.  A
point whose weights are all zero adds nothing to a bound, and a pulse whose weights are all zero has bounds of zero and differences
of exact zero (share() holds that).  tests/test_blochtrainschedgn_cpu.py prints the float64 twin's share of every bound and asserts
a hundredth.

Central differences (FD_ANGLE, FD_TOL of blochtrainvjp_ref; blochtrainsched_ref.fd_steps), one schedule coordinate of FD_CASES at a
time, of the long-double L.  In units of the entry's scale (ntr N max|scale| Theta for a gain, ntr N for a phase, N the 1-norm of the
reference cotangent times sqrt(3) mu, blochtrainsched_ref.scale_gains / scale_phases) the truncation is FD_ANGLE^2 / 6 = 1.7e-11 from
the linear loss's term r e''' as in 8ad, plus the quadratic loss's own 3 w e' e'' / 6, FD_ANGLE^2 / 2 times sum rw w mu^2 / N: the
weights are at most 1 and the residuals of order 1, so sum rw w mu^2 / N is of order 1 (8ab measured 0.66 on small()) and the
truncation stays below 1e-10 of the scale; the rounding of two long-double losses is many orders below.  FD_TOL = 1e-7 stands.

The dense H of FD_CASES from the 2 ntr unit directions in long double: H_TOL = blochtraingn_ref.H_TOL = 1e-15 for the asymmetry
max|H - H'| / max|H|, the smallest eigenvalue over max|H| (float64 eigvalsh of the symmetrised matrix) and v'H v against sum W |J v|^2.
For float64 results (the twin, the device) the tolerance of u'H v = v'H u is the two sides' bounds (pair_tol)."""
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


sj = _load("blochtrainschedjvp_ref")
gnr = _load("blochtraingn_ref")
sched, tr, vjp = sj.sched, sj.tr, sj.vjp
_grad = tr._grad

TOL = _grad.TOL
FD_ANGLE, FD_TOL = vjp.FD_ANGLE, vjp.FD_TOL
H_TOL, L_QUAD = gnr.H_TOL, gnr.L_QUAD
ROUTE_TOL = 1e-5 + 2.0 ** -53 / TOL
FD_CASES = sched.FD_CASES
share, full, rw_of = gnr.share, gnr.full, gnr.rw_of
_J, _dot = sched._J, sched._dot


@functools.lru_cache(maxsize=None)
def cases():
    """blochtrainsched_ref.cases(), every one, dressed with w / t, wf / tf, rw and bcast as blochtraingn_ref.cases() dresses its own"""
    rng = np.random.default_rng(43)
    return {name: gnr._dress(c, name, rng) for name, c in sched.cases().items()}


@functools.lru_cache(maxsize=None)
def small():
    return gnr._dress(sched.small(), "small", np.random.default_rng(47))


def case_of(name):
    return small() if name == "small" else cases()[name]


def directions(name, K):
    """Per pulse (dg (K, ntr), dp (K, ntr)) of blochtrainschedjvp_ref.directions, without its m0 part: m0 is not a variable of gn"""
    return [(dg, dp) for dg, dp, _ in sj.directions(name, K)]


# ---- the structured route ------------------------------------------------------------------------------------------------------
def _walk(c, q, si, dtype, dg=None, dp=None):
    """One scale, forwards.  Returns the planes per repetition, (cs, sn), us, the echoes es, the states ms (m_{k+1}), m_N and, along
    the K directions (dg, dp) (None: no tangent), the tangent echoes des (per repetition three (K, nf, npos)) and dm_N"""
    s, ntr, demod = c["scales"][si], c["ntr"][q], c["demod"]
    p = c["pulses"][q]
    cs, sn = tr._table(c["phases"][q], dtype)
    amps = tr._amps(s, c["gains"][q])
    Ps = {a: sched.prop_dgain(p, c["dfs"][q], c["dps"][q], a, np.float64(s), c["echo"][q], dtype) for a in set(amps.tolist())}
    Q0 = tr._setup(p, c["dfs"][q], c["dps"][q], 1.0, dtype)
    mq, mv = dtype(c["meq"]), _grad._mat_vec
    m = tr._start(c["m0"][q], Q0, dtype)
    tang = dg is not None
    if tang:
        K = dg.shape[0]
        dm = [np.zeros((K, Q0.nf, Q0.npos), dtype=dtype) for _ in range(3)]
    planes, us, es, ms, des = [], [], [], [], []
    for k in range(ntr):
        (A, B, Ae, Be), (dA, dB, dAe, dBe) = P = Ps[float(amps[k])]
        planes.append(P)
        ck, sk = cs[k], sn[k]
        u = tr._zp(ck, sk, m)
        us.append(u)
        ne = [x + mq * y for x, y in zip(mv(Ae, u), Be)]
        n = [x + mq * y for x, y in zip(mv(A, u), B)]
        es.append(ne if demod else tr._zm(ck, sk, ne))
        if tang:
            g, ph = dg[:, k, None, None], dp[:, k, None, None]
            du = [a + ph * b for a, b in zip(tr._zp(ck, sk, dm), _J(u))]
            ge = [x + mq * y for x, y in zip(mv(dAe, u), dBe)]
            de = [a + g * b for a, b in zip(mv(Ae, du), ge)]
            if not demod:
                de = tr._zm(ck, sk, [a - ph * b for a, b in zip(de, _J(ne))])
            des.append(de)
            gv = [x + mq * y for x, y in zip(mv(dA, u), dB)]
            dn = [a + g * b for a, b in zip(mv(A, du), gv)]
            dm = tr._zm(ck, sk, [a - ph * b for a, b in zip(dn, _J(n))])
        m = tr._zm(ck, sk, n)
        ms.append(m)
    return planes, (cs, sn), us, es, ms, m, des, (dm if tang else None), mq


def _contract(c, q, planes, table, us, es, ms, ce, lam, mq):
    """One scale, backwards: (gg, gp, lambda_0).  ce: None or per repetition three arrays; lam: three arrays; either with leading
    direction axes, over which nothing is summed"""
    cs, sn = table
    ntr, demod, mv = c["ntr"][q], c["demod"], _grad._mat_vec
    gg, gp = [None] * ntr, [None] * ntr
    for k in range(ntr - 1, -1, -1):
        (A, B, Ae, Be), (dA, dB, dAe, dBe) = planes[k]
        ck, sk, u = cs[k], sn[k], us[k]
        a = tr._zp(ck, sk, lam)
        g = _dot(a, [x + mq * y for x, y in zip(mv(dA, u), dB)])
        p = _dot(a, mv(A, _J(u))) - _dot(lam, _J(ms[k]))
        lam = mv(A, a, transpose=True)
        if ce is not None:
            ae = ce[k] if demod else tr._zp(ck, sk, ce[k])
            g = g + _dot(ae, [x + mq * y for x, y in zip(mv(dAe, u), dBe)])
            p = p + _dot(ae, mv(Ae, _J(u)))
            if not demod:
                p = p - _dot(ce[k], _J(es[k]))
            lam = [x + y for x, y in zip(lam, mv(Ae, ae, transpose=True))]
        lam = tr._zm(ck, sk, lam)
        gg[k], gp[k] = g.sum((-2, -1)), p.sum((-2, -1))
    return np.stack(gg, -1), np.stack(gp, -1), lam


def _planes(c, q, dtype):
    """(W, T, wf, tf) as lists of three arrays in dtype (None where the case has none; W, T repeated over the repetitions) and rw (ntr,)"""
    cast = lambda tri: None if tri is None else [np.asarray(v).astype(dtype) for v in tri]
    return cast(full(c, q, c["w"][q])), cast(full(c, q, c["t"][q])), cast(c["wf"][q]), cast(c["tf"][q]), rw_of(c, q).astype(dtype)


def lsq(c, q, dtype=np.longdouble):
    """(L, gg (ntr,), gp (ntr,), (gmx, gmy, gmz) each (S, nf, npos)) by the structured route"""
    W, T, wf, tf, rw = _planes(c, q, dtype)
    L, gg, gp, gm = dtype(0), 0, 0, []
    for si in range(len(c["scales"])):
        planes, table, us, es, ms, mN, _, _, mq = _walk(c, q, si, dtype)
        ce = None
        if W is not None:
            ce = []
            for k in range(c["ntr"][q]):
                r = [es[k][i] - T[i][si][k] for i in range(3)]
                ce.append([rw[k] * W[i][si][k] * r[i] for i in range(3)])
                L = L + sum((rw[k] * W[i][si][k] * r[i] * r[i]).sum() for i in range(3)) / 2
        lam = [np.zeros_like(mN[0])] * 3
        if wf is not None:
            rf = [mN[i] - tf[i][si] for i in range(3)]
            lam = [wf[i][si] * rf[i] for i in range(3)]
            L = L + sum((wf[i][si] * rf[i] * rf[i]).sum() for i in range(3)) / 2
        g, p, l0 = _contract(c, q, planes, table, us, es, ms, ce, lam, mq)
        gg, gp = gg + g, gp + p
        gm.append(l0)
    return L, gg, gp, tuple(np.stack([l[i] for l in gm]) for i in range(3))


def _dirs(c, q, dg, dp, dtype):
    n = c["ntr"][q]
    given = [np.asarray(d, dtype=np.float64).reshape(-1, n) for d in (dg, dp) if d is not None]
    K = given[0].shape[0]
    return [np.zeros((K, n), dtype=dtype) if d is None else np.asarray(d, dtype=np.float64).reshape(K, n).astype(dtype) for d in (dg, dp)]


def gn(c, q, dg, dp, dtype=np.longdouble):
    """(Hg (K, ntr), Hp (K, ntr)) along the directions dg / dp ((ntr,) or (K, ntr); either None: zeros) by the structured route"""
    W, _, wf, _, rw = _planes(c, q, dtype)
    dg, dp = _dirs(c, q, dg, dp, dtype)
    hg, hp = 0, 0
    for si in range(len(c["scales"])):
        planes, table, us, es, ms, _, des, dmN, mq = _walk(c, q, si, dtype, dg, dp)
        ce = None if W is None else [[rw[k] * W[i][si][k] * des[k][i] for i in range(3)] for k in range(c["ntr"][q])]
        lam = [np.zeros_like(dmN[0])] * 3 if wf is None else [wf[i][si] * dmN[i] for i in range(3)]
        g, p, _ = _contract(c, q, planes, table, us, es, ms, ce, lam, mq)
        hg, hp = hg + g, hp + p
    return hg, hp


def weighted_square(c, q, dg, dp, dtype=np.longdouble):
    """sum W |J v|^2 per direction (K,)"""
    W, _, wf, _, rw = _planes(c, q, dtype)
    dg, dp = _dirs(c, q, dg, dp, dtype)
    tot = 0
    for si in range(len(c["scales"])):
        _, _, _, _, _, _, des, dmN, _ = _walk(c, q, si, dtype, dg, dp)
        if W is not None:
            tot = tot + sum((rw[k] * W[i][si][k] * des[k][i] ** 2).sum((-2, -1)) for k in range(c["ntr"][q]) for i in range(3))
        if wf is not None:
            tot = tot + sum((wf[i][si] * dmN[i] ** 2).sum((-2, -1)) for i in range(3))
    return tot


# ---- the composed route --------------------------------------------------------------------------------------------------------
def _adj(c, q, ce, cf, dtype):
    return sched.sched_scaled(sched.sched_vjp, c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q],
                              c["echo"][q], ce, cf, c["scales"], c["m0"][q], c["meq"], c["demod"], dtype)


def lsq_composed(c, q, dtype=np.longdouble):
    """blochtraingn_ref's loss and residual cotangents -> blochtrainsched_ref.sched_vjp"""
    ce, cf = gnr.cotangents(c, q, dtype)
    return (gnr.loss(c, q, dtype),) + tuple(_adj(c, q, ce, cf, dtype))


def gn_cotangents(c, q, dg, dp, dtype=np.longdouble):
    """Per direction (ce, cf) of the products: blochtrainschedjvp_ref.sched_jvp times the weights"""
    W, _, wf, _, rw = _planes(c, q, dtype)
    dE, dF = sj.run(sj.sched_jvp, c, q, dg, dp, None, dtype)             # three (K, S, ntr, nf, npos), three (K, S, nf, npos)
    r = rw[:, None, None]
    out = []
    for d in range(dE[0].shape[0]):
        ce = None if W is None else tuple(r * W[i] * dE[i][d] for i in range(3))
        cf = None if wf is None else tuple(wf[i] * dF[i][d] for i in range(3))
        out.append((ce, cf))
    return out


def gn_composed(c, q, dg, dp, dtype=np.longdouble):
    res = [_adj(c, q, ce, cf, dtype) for ce, cf in gn_cotangents(c, q, dg, dp, dtype)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The long-double (L, gg, gp, gm) per pulse of a case, computed once"""
    c = case_of(name)
    return [lsq(c, q) for q in range(len(c["pulses"]))]


@functools.lru_cache(maxsize=None)
def reference_gn(name, K):
    """The long-double (Hg, Hp) along directions(name, K) per pulse, computed once"""
    c = case_of(name)
    return [gn(c, q, *directions(name, K)[q]) for q in range(len(c["pulses"]))]


def unit_directions(ntr):
    return sj.unit_directions(ntr)


def dense(c, q, dtype=np.longdouble, route=gn):
    """H (2 ntr, 2 ntr) of pulse q from the 2 ntr unit directions, gains first: row j = (Hg, Hp) of direction j"""
    hg, hp = route(c, q, *unit_directions(c["ntr"][q]), dtype)
    return np.concatenate([hg, hp], 1)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def _mu(c, q):
    return tr.mu_of(c["m0"][q], c["meq"], len(c["dfs"][q]), len(c["dps"][q]))           # (nf, npos)


def seed_reach(c, q, be):
    """sum over the points and scales of mu (sum_k rw_k sum_c w_c be + sum_c wf_c be): the 1-norm of the cotangent's error, each
    point's share times the bound mu of its state; be (nf, npos)"""
    return float((gnr._seed_sum(c, q, be) * _mu(c, q)).sum())


def _at(c, q, ce, cf):
    return gnr._with_cot(c, q, ce, cf)


def bound_g(c, q):
    """(bound of a gg entry, bound of a gp entry)"""
    ce, cf = gnr.cotangents(c, q)
    d, e = _at(c, q, ce, cf), seed_reach(c, q, gnr._bt(c, q))
    return sched.bound_gains(d, q) + sched.smax_of(c) * sched.theta_of(c, q) * e, sched.bound_phases(d, q) + 2.0 * e


bound_gm, bound_l = gnr.bound_gm, gnr.bound_l


def bound_h(c, q, dg, dp):
    """(bounds of the Hg entries (K,), of the Hp entries (K,)), one per direction"""
    bj = sj.bound_jvp(c, q, dg, dp, None)                                               # (K, nf, npos)
    bg, bp = [], []
    for d, (ce, cf) in enumerate(gn_cotangents(c, q, dg, dp)):
        at, e = _at(c, q, ce, cf), seed_reach(c, q, bj[d])
        bg.append(sched.bound_gains(at, q) + sched.smax_of(c) * sched.theta_of(c, q) * e)
        bp.append(sched.bound_phases(at, q) + 2.0 * e)
    return np.array(bg), np.array(bp)


def scale_fd(c, q):
    """(the scale of a gains entry, of a phases entry) at the reference cotangent: the units of the central differences"""
    ce, cf = gnr.cotangents(c, q)
    d = _at(c, q, ce, cf)
    return sched.scale_gains(d, q), sched.scale_phases(d, q)


def moved(c, q, gains, phases):
    """the case with the schedule of pulse q replaced"""
    d = dict(c)
    d["gains"], d["phases"] = list(c["gains"]), list(c["phases"])
    d["gains"][q], d["phases"][q] = np.asarray(gains, dtype=np.float64), np.asarray(phases, dtype=np.float64)
    return d


def pair(u, hv):
    """u' H v from the halves: u = (ug, up), hv = (Hg, Hp), one direction each"""
    return (np.asarray(u[0]) * hv[0]).sum() + (np.asarray(u[1]) * hv[1]).sum()


def pair_tol(c, q, u, v):
    """the tolerance of u'H v = v'H u for float64 products: the two sides' bounds"""
    bu, bv = bound_h(c, q, u[0], u[1]), bound_h(c, q, v[0], v[1])
    return float(bv[0][0] * np.abs(u[0]).sum() + bv[1][0] * np.abs(u[1]).sum() + bu[0][0] * np.abs(v[0]).sum()
                 + bu[1][0] * np.abs(v[1]).sum())


# ---- the closed forms of the case 'hard' -----------------------------------------------------------------------------------------
def hard_closed():
    """(L, gg, gp in long double, H (2 ntr, 2 ntr) in float64) of the dressed case 'hard' from blochtrainsched_ref's and blochtrainschedjvp_ref's closed forms:
    m_k = (0, sin Th_k, cos Th_k), echo_k = m_{k+1}, Th_k = theta (gains_0 + .. + gains_{k-1}); the gradient is
    blochtrainsched_ref.hard_closed's at ce_k = rw_k w (echo_k - t), cf = wf (m_N - tf), and H = sum_k rw_k sum_c w_c dE dE' + sum_c
    wf_c dF dF' on blochtrainschedjvp_ref.hard_closed's Jacobian"""
    c = cases()["hard"]
    LD = np.longdouble
    g, N, th = np.asarray(c["gains"][0]).astype(LD), c["ntr"][0], LD(sched.HARD_THETA)
    Th = th * np.concatenate([np.zeros(1, dtype=LD), np.cumsum(g)])
    E = np.stack([np.zeros(N, dtype=LD), np.sin(Th[1:]), np.cos(Th[1:])])                 # (3, N)
    W, T = [np.stack([np.asarray(v).reshape(N) for v in full(c, 0, tri)]).astype(LD) for tri in (c["w"][0], c["t"][0])]
    wf, tf = [np.array([float(np.asarray(v).reshape(())) for v in tri]).astype(LD) for tri in (c["wf"][0], c["tf"][0])]
    rw = rw_of(c, 0).astype(LD)
    r, rf = E - T, E[:, -1] - tf
    ce, cf = rw * W * r, wf * rf
    L = (rw * W * r * r).sum() / 2 + (wf * rf * rf).sum() / 2
    along = ce[1] * np.cos(Th[1:]) - ce[2] * np.sin(Th[1:])
    fin = cf[1] * np.cos(Th[N]) - cf[2] * np.sin(Th[N])
    gg = th * (np.cumsum(along[::-1])[::-1] + fin)
    gp = (np.sin(Th[1:]) - np.sin(Th[:-1])) * (np.cumsum(ce[0][::-1])[::-1] + cf[0])
    rw, W, wf = [np.asarray(v, dtype=np.float64) for v in (rw, W, wf)]
    dE, dF = sj.hard_closed()                                                            # (2N, N, 3), (2N, 3)
    H = np.einsum("k,ck,ikc,jkc->ij", rw, W, dE, dE) + np.einsum("c,ic,jc->ij", wf, dF, dF)
    return L, gg, gp, H
