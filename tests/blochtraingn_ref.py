"""NumPy restatement of the fused least-squares and Gauss-Newton products of a pulse train (helper of
tests/test_blochtraingn_cpu.py and tests/test_blochtraingn_gpu.py; not collected), in float64 or np.longdouble, on
tests/blochtrain_ref.py (the train), tests/blochtrainvjp_ref.py (the cases and the adjoint) and tests/blochtrainjvp_ref.py (the
tangent and the directions).  Those are imported, not edited.

Per pulse, with echo_k and m_N what the train returns under the case's demod,
    L = 1/2 sum_s sum_k rw_k sum w_c (echo_kc - t_c)^2 + 1/2 sum_s sum wf_c (m_Nc - tf_c)^2
    g   = train_vjp at the cotangents ce_k = rw_k w (echo_k - t), cf = wf (m_N - tf);  dL/dm0 is its lambda_0
    H v = train_vjp at the cotangents ce_k = rw_k w decho_k[v], cf = wf dm_N[v]        (train_jvp along v, m0 not moved)

Bounds, composed through the seed.  Write bt = blochtrain_ref.bound_train(ntr, ntime, mu), the bound of one echo or final entry
at a point, and bj = blochtrainjvp_ref.bound_jvp, the bound of one tangent entry.  The device's cotangent differs from the
reference's by at most dc = rw_k w bt (rw_k w bj for the products) per entry, because the weights are exact inputs.  The adjoint is
linear in the cotangent, and blochtrainvjp_ref's bound says what a cotangent of 1-norm N can do to a b1 entry: at most
ntr N max|scale gain| gamma dt_t (every step back is the transpose of a contraction).  So
    g:     bound_b1 at the reference cotangent  +  ntr max|scale gain| gamma dt_t (sum rw w bt + sum wf bt)
    H v:   the same with bj in place of bt and the cotangent of the products
    dL/dm0 per point: bound_m0 at the reference cotangent (TOL ntr times the largest 1-norm of the point's cotangents)
           + sum_k rw_k sum_c w_c bt + sum_c wf_c bt at the point (a perturbed cotangent reaches lambda_0 through contractions)
    L:     sum rw w |r| bt + sum wf |rf| bt  (the first order of 1/2 w r^2 in the echo's error)
           + 1e-13 (sum rw w r^2 + sum wf rf^2)  (the second order, the products and the sum of the loss itself)
The constants are those of the imported references (TOL = 1e-12, C_BOUND = 200) and L_QUAD = 1e-13, about 450 u for the loss's own
products and sums; none was changed after a run.
Measured on the CPU before any device run (tests/test_blochtraingn_cpu.py prints every share): the float64 twin differs from its
long-double twin by at most 5.1e-5 of the gradient bound (shared), 9.0e-5 of the product bound (shared), 4.4e-4 of the dL/dm0 bound
(p65) and 3.6e-4 of the loss bound (one), within the hundredth that the CPU test asserts: the constants stand as they started.
The long-double twin passes its cotangents through float64 (blochtrainvjp_ref.train_vjp takes them so), a relative 1.1e-16 of the
seed, many orders below every bound.  A point whose weights are all zero has a bound of zero and a difference of exact zero
(share() holds that).

Central differences (FD_ANGLE, FD_TOL of blochtrainvjp_ref).  A b1 entry of small() is moved by h = FD_ANGLE / (gamma dt_t amax), so
that the sample turns by FD_ANGLE = 1e-5 rad.  In units of scale_t = ntr N amax gamma dt_t, N the 1-norm of the reference
cotangent, the central difference of L is off by its truncation h^2 L''' / 6.  With e' <= ntr FD_ANGLE mu per step, L''' has the
linear loss's term r e''' (8z: (ntr FD_ANGLE)^2 / 6 of the scale = 1.5e-10 at ntr = 3) and the quadratic loss's own 3 w e' e'',
which is (ntr FD_ANGLE)^2 / 2 times sum rw w mu^2 / N of the scale: on small() sum rw w mu^2 / N = 0.66, so the truncation stays
below 4.5e-10 of the scale.  The rounding of two float64 losses over 2 h is, as in 8z, at most 8.7e-13 N / FD_ANGLE = 2.9e-8 of
the scale.  FD_TOL = 1e-7 covers the float64 device call with a factor 3 to spare; the long-double reference reaches 5.9e-12 of
the scale (printed by the CPU test, which asserts FD_TOL / 10: more than the factor of ten of 8u).

The dense H of small() (n = 9, 2 n = 18 real directions) in long double, its seeds through float64 as said above: the asymmetry
max|H - H'| / max|H| reaches 2.4e-17, the smallest eigenvalue (float64 eigvalsh of the symmetrised matrix) is +3.5e-14 max|H|, and
Re<v, H v> differs from sum W |J v|^2 by 5.0e-17 of it.  H_TOL = 1e-15 is more than ten times each, and 18 u of eigvalsh's own
rounding besides.  For float64 results (the twin, the device) the tolerance of Re<u, H v> = Re<H u, v> is the two sides' bounds,
sum_t bound_h(v)_t |u_t| + sum_t bound_h(u)_t |v_t| (pair_tol), and Re<v, H v> >= -pair_tol(v, v) / 2."""
import functools
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("blochtrainjvp_ref", os.path.join(_here, "blochtrainjvp_ref.py"))
jvp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(jvp)
vjp, tr = jvp.vjp, jvp.tr

FD_ANGLE, FD_TOL = vjp.FD_ANGLE, vjp.FD_TOL
L_QUAD = 1e-13
H_TOL = 1e-15
BCAST = ("c13_ramp", "shared", "p65")           # the demod=True cases take the broadcast form
NO_RW = ("one", "allgains")                     # rep_weights=None


def _weights(rng, shape):
    """uniform in [0, 1], every third entry zero"""
    w = rng.uniform(0.0, 1.0, shape)
    w.reshape(-1)[::3] = 0.0
    return w


def _dress(c, name, rng):
    """adds w, t (per pulse a triple, or None), rw (per pulse, or None for the call), wf, tf, bcast to a copy of the case"""
    c = dict(c)
    S = len(c["scales"])
    c["bcast"] = name in BCAST
    assert not c["bcast"] or c["demod"]
    c["w"], c["t"], c["wf"], c["tf"], rw = [], [], [], [], []
    for q in range(len(c["pulses"])):
        nf, npos, ntr = len(c["dfs"][q]), len(c["dps"][q]), c["ntr"][q]
        es = (3, S, nf, npos) if c["bcast"] else (3, S, ntr, nf, npos)
        echo, final = c["cot"] != "final", c["cot"] != "echo"
        c["w"].append(tuple(_weights(rng, es)) if echo else None)
        c["t"].append(tuple(rng.uniform(-1.0, 1.0, es)) if echo else None)
        c["wf"].append(tuple(_weights(rng, (3, S, nf, npos))) if final else None)
        c["tf"].append(tuple(rng.uniform(-1.0, 1.0, (3, S, nf, npos))) if final else None)
        r = rng.uniform(0.5, 1.5, ntr)
        if ntr > 2:
            r[:2] = 0.0
        rw.append(r)
    c["rw"] = None if name in NO_RW else rw
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """blochtrainvjp_ref.cases() (periods of 1, 9 and 257 samples, trains of 1, 2, 5, 7, 8, 9 and 257 repetitions, 6, 65 and 300
    points, 1 to 5 gains, 1 to 3 scales) plus, per pulse: w / t, the echo weights and targets (a triple of (S, ntr, nf, npos), or of
    (S, nf, npos) on the broadcast cases; None where the case's cot is 'final'), wf / tf (None where it is 'echo'), and rw, the
    repetitions' factors (the first two zero where ntr > 2; None for the whole call on NO_RW)."""
    rng = np.random.default_rng(37)
    return {name: _dress(c, name, rng) for name, c in vjp.cases().items()}


@functools.lru_cache(maxsize=None)
def small():
    return _dress(vjp.small(), "small", np.random.default_rng(41))


def case_of(name):
    return small() if name == "small" else cases()[name]


@functools.lru_cache(maxsize=None)
def directions(name, K):
    return jvp.directions(name, K)[0]


def rw_of(c, q):
    return np.ones(c["ntr"][q]) if c["rw"] is None else np.asarray(c["rw"][q])


def full(c, q, tri):
    """an echo triple of the case as three (S, ntr, nf, npos) arrays: a broadcast plane repeated ntr times"""
    if tri is None:
        return None
    n = c["ntr"][q]
    return tuple(np.repeat(np.asarray(v)[:, None], n, 1) if np.ndim(v) == 3 else np.asarray(v) for v in tri)


def _train(c, q, s, dtype, b1=None):
    p = c["pulses"][q]
    if b1 is not None:
        p = (b1,) + tuple(p[1:])
    return tr.train(p, c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], s, c["m0"][q], c["meq"],
                    c["demod"], dtype)


def _adj(c, q, s, ce, cf, dtype):
    return vjp.train_vjp(c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], ce, cf, s,
                         c["m0"][q], c["meq"], c["demod"], dtype)[:2]


def _planes(c, q, dtype):
    W, T = full(c, q, c["w"][q]), full(c, q, c["t"][q])
    cast = lambda tri: None if tri is None else [np.asarray(v).astype(dtype) for v in tri]
    return cast(W), cast(T), cast(c["wf"][q]), cast(c["tf"][q]), rw_of(c, q).astype(dtype)[:, None, None]


def residuals(c, q, dtype=np.longdouble, b1=None, rw=None):
    """Per scale (r (3, ntr, nf, npos) or None, rf (3, nf, npos) or None) of pulse q"""
    W, T, wf, tf, _ = _planes(c, q, dtype)
    out = []
    for k, s in enumerate(c["scales"]):
        E, F = _train(c, q, s, dtype, b1)
        r = None if W is None else np.stack([E[:, i] - T[i][k] for i in range(3)])
        rf = None if wf is None else np.stack([F[i] - tf[i][k] for i in range(3)])
        out.append((r, rf))
    return out


def loss(c, q, dtype=np.longdouble, b1=None):
    W, _, wf, _, rw = _planes(c, q, dtype)
    L = dtype(0)
    for k, (r, rf) in enumerate(residuals(c, q, dtype, b1)):
        if r is not None:
            L = L + sum((rw * W[i][k] * r[i] * r[i]).sum() for i in range(3)) / 2
        if rf is not None:
            L = L + sum((wf[i][k] * rf[i] * rf[i]).sum() for i in range(3)) / 2
    return L


def cotangents(c, q, dtype=np.longdouble):
    """(ce, cf) of the loss as blochtrainvjp_ref's cases hold them: three (S, ntr, nf, npos) or None, three (S, nf, npos) or None"""
    W, _, wf, _, rw = _planes(c, q, dtype)
    res = residuals(c, q, dtype)
    ce = None if W is None else tuple(np.stack([rw * W[i][k] * r[i] for k, (r, _) in enumerate(res)]) for i in range(3))
    cf = None if wf is None else tuple(np.stack([wf[i][k] * rf[i] for k, (_, rf) in enumerate(res)]) for i in range(3))
    return ce, cf


def _sweep(c, q, ce, cf, dtype):
    """train_vjp over the scales: (G, (gmx, gmy, gmz) each (S, nf, npos))"""
    G, gm = 0, []
    for k, s in enumerate(c["scales"]):
        g, l = _adj(c, q, s, None if ce is None else [v[k] for v in ce], None if cf is None else [v[k] for v in cf], dtype)
        G = G + g
        gm.append(l)
    return G, tuple(np.stack([l[i] for l in gm]) for i in range(3))


def lsq(c, q, dtype=np.longdouble):
    """(L, g (ntime,), (gmx, gmy, gmz))"""
    ce, cf = cotangents(c, q, dtype)
    return (loss(c, q, dtype),) + _sweep(c, q, ce, cf, dtype)


def tangent(c, q, v, dtype=np.longdouble):
    """Per scale (dE (K, ntr, 3, nf, npos), dF (K, 3, nf, npos)) along the directions v of b1"""
    return [jvp.train_jvp(c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], v, None, s,
                          c["m0"][q], c["meq"], c["demod"], dtype) for s in c["scales"]]


def gn_cotangents(c, q, v, dtype=np.longdouble):
    """Per direction (ce, cf) of the products"""
    W, _, wf, _, rw = _planes(c, q, dtype)
    tan = tangent(c, q, v, dtype)
    out = []
    for d in range(tan[0][0].shape[0]):
        ce = None if W is None else tuple(np.stack([rw * W[i][k] * dE[d][:, i] for k, (dE, _) in enumerate(tan)]) for i in range(3))
        cf = None if wf is None else tuple(np.stack([wf[i][k] * dF[d][i] for k, (_, dF) in enumerate(tan)]) for i in range(3))
        out.append((ce, cf))
    return out


def gn(c, q, v, dtype=np.longdouble):
    """H v (K, ntime) along v (K, ntime)"""
    v = np.asarray(v).reshape(-1, len(c["pulses"][q][0]))
    return np.stack([_sweep(c, q, ce, cf, dtype)[0] for ce, cf in gn_cotangents(c, q, v, dtype)])


def weighted_square(c, q, v, dtype=np.longdouble):
    """sum W |J v|^2 per direction (K,)"""
    W, _, wf, _, rw = _planes(c, q, dtype)
    tan = tangent(c, q, np.asarray(v).reshape(-1, len(c["pulses"][q][0])), dtype)
    out = []
    for d in range(tan[0][0].shape[0]):
        tot = dtype(0)
        for k, (dE, dF) in enumerate(tan):
            if W is not None:
                tot = tot + sum((rw * W[i][k] * dE[d][:, i] ** 2).sum() for i in range(3))
            if wf is not None:
                tot = tot + sum((wf[i][k] * dF[d][i] ** 2).sum() for i in range(3))
        out.append(tot)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The long-double (L, g, gm) per pulse of a case, computed once"""
    c = case_of(name)
    return [lsq(c, q) for q in range(len(c["pulses"]))]


@functools.lru_cache(maxsize=None)
def reference_gn(name, K):
    """The long-double H v along directions(name, K) per pulse, computed once"""
    c = case_of(name)
    return [gn(c, q, directions(name, K)[q]) for q in range(len(c["pulses"]))]


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
def _bt(c, q):
    p = c["pulses"][q]
    mu = tr.mu_of(c["m0"][q], c["meq"], len(c["dfs"][q]), len(c["dps"][q]))
    return tr.bound_train(c["ntr"][q], len(p[0]), mu)                                   # (nf, npos)


def _with_cot(c, q, ce, cf):
    d = dict(c)
    d["ce"], d["cf"] = list(c["ce"]), list(c["cf"])
    d["ce"][q] = None if ce is None else tuple(np.asarray(v, dtype=np.float64) for v in ce)
    d["cf"][q] = None if cf is None else tuple(np.asarray(v, dtype=np.float64) for v in cf)
    return d


def _seed_sum(c, q, be):
    """per point (S, nf, npos): sum_k rw_k sum_c w_c be + sum_c wf_c be, be (nf, npos) the bound of one echo / final entry"""
    W, rw = full(c, q, c["w"][q]), rw_of(c, q)[:, None, None]
    tot = 0.0
    if W is not None:
        tot = tot + sum((rw * w).sum(1) for w in W) * be
    if c["wf"][q] is not None:
        tot = tot + sum(np.asarray(w) for w in c["wf"][q]) * be
    return tot


def _reach(c, q):
    """ntr max|scale gain| gamma dt_t: what a unit of cotangent can do to a b1 entry"""
    p = c["pulses"][q]
    return c["ntr"][q] * vjp.amax_of(c, q) * tr.gamma_of(p[5]) * tr.intervals(p)


def bound_g(c, q):
    """per b1 entry (ntime,)"""
    ce, cf = cotangents(c, q)
    return vjp.bound_b1(_with_cot(c, q, ce, cf), q) + _reach(c, q) * float(_seed_sum(c, q, _bt(c, q)).sum())


def bound_gm(c, q):
    """per dL/dm0 entry (S, nf, npos)"""
    ce, cf = cotangents(c, q)
    return vjp.bound_m0(_with_cot(c, q, ce, cf), q) + _seed_sum(c, q, _bt(c, q))


def bound_h(c, q, v):
    """per entry of H v, (K, ntime)"""
    v = np.asarray(v).reshape(-1, len(c["pulses"][q][0]))
    bj = jvp.bound_jvp(c, q, v, None)                                                   # (K, nf, npos)
    out = []
    for d, (ce, cf) in enumerate(gn_cotangents(c, q, v)):
        out.append(vjp.bound_b1(_with_cot(c, q, ce, cf), q) + _reach(c, q) * float(_seed_sum(c, q, bj[d]).sum()))
    return np.stack(out)


def bound_l(c, q):
    W, _, wf, _, rw = _planes(c, q, np.float64)
    bt, lin, quad = _bt(c, q), 0.0, 0.0
    for k, (r, rf) in enumerate(residuals(c, q)):
        if r is not None:
            r = r.astype(np.float64)
            lin += sum(float((rw * W[i][k] * np.abs(r[i]) * bt).sum()) for i in range(3))
            quad += sum(float((rw * W[i][k] * r[i] ** 2).sum()) for i in range(3))
        if rf is not None:
            rf = rf.astype(np.float64)
            lin += sum(float((wf[i][k] * np.abs(rf[i]) * bt).sum()) for i in range(3))
            quad += sum(float((wf[i][k] * rf[i] ** 2).sum()) for i in range(3))
    return lin + L_QUAD * quad


def scale_fd(c, q):
    """ntr N amax gamma dt_t with N the 1-norm of the reference cotangent: the scale of the central differences"""
    ce, cf = cotangents(c, q)
    return vjp.scale_b1(_with_cot(c, q, ce, cf), q)


def fd_steps(c, q):
    p = c["pulses"][q]
    return FD_ANGLE / (tr.gamma_of(p[5]) * tr.intervals(p) * vjp.amax_of(c, q))


def share(diff, bound):
    """max |diff| / bound; where the bound is zero the difference must be: inf otherwise"""
    diff = np.abs(np.asarray(diff)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(diff))
    if np.any((bound == 0) & (diff != 0)):
        return float("inf")
    ok = bound > 0
    return float((diff[ok] / bound[ok]).max()) if ok.any() else 0.0


def redot(u, v):
    return (np.conj(u) * v).real.sum()


def pair_tol(c, q, u, v):
    """the tolerance of Re<u, H v> = Re<H u, v> for float64 products: the two sides' bounds"""
    return float((bound_h(c, q, v)[0] * np.abs(u)).sum() + (bound_h(c, q, u)[0] * np.abs(v)).sum())
