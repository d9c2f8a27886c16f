"""NumPy restatement of the magnitude fits of the pulse train (helper of tests/test_blochtrainmag_cpu.py and
tests/test_blochtrainmag_gpu.py; not collected): the fits of (|Mxy|, mz) of every echo and of the final state of DESIGN 8ai, in the
period's b1 (chain "b1": tests/blochtraingn_ref.py) and in the schedule (chain "sched": tests/blochtrainschedgn_ref.py), in float64
or np.longdouble.  The two references and tests/blochmag_ref.py are loaded by path and used as they are: their trains, tangents,
adjoints, cases, bounds and constants.  Only the seed between the forward and the reverse walk is new.

With e echo k of a point as the train returns it under the case's demod, or the final state m_N, weights (w_xy, w_z) >= 0 and
targets (t_xy, t_z):
    rho = sqrt(ex ex + ey ey),   u = (ex, ey) / rho, and (0, 0) where rho = 0
    L   = 1/2 sum_s sum_k rw_k sum [w_xy (rho_k - t_xy)^2 + w_z (e_kz - t_z)^2] + 1/2 sum_s sum [wf_xy (rho_N - tf_xy)^2 + wf_z (m_Nz - tf_z)^2]
    lsq seed  ce_k = rw_k (w_xy (rho_k - t_xy) u_x, w_xy (rho_k - t_xy) u_y, w_z (e_kz - t_z)),  cf likewise with wf, tf
    gn  seed  ce_k = rw_k (w_xy (u . de_xy) u_x,    w_xy (u . de_xy) u_y,    w_z de_z),           cf likewise with dm_N
The seeds go to the imported adjoints (blochtrainvjp_ref.train_vjp through blochtraingn_ref._sweep; blochtrainsched_ref.sched_vjp
through blochtrainschedgn_ref._adj), the tangents come from the imported blochtrainjvp_ref.train_jvp and
blochtrainschedjvp_ref.sched_jvp: H v is jvp -> U' W U -> vjp of the component references by construction.  For the schedule a second
route (lsq_walk, gn_walk) puts the same seeds into blochtrainschedgn_ref's own structured walk (_walk, _contract).

Cases: blochtraingn_ref.cases() / small() and blochtrainschedgn_ref.cases() / small(), every one, with the triples replaced by pairs
from a fixed seed (weights uniform in [0, 1] with every third entry zero, t_xy uniform in [-0.2, 1], t_z uniform in [-1, 1]); the
shapes, the broadcast form, rep_weights and which terms a case has are the dressed case's.  "z0" is small() of the schedule with
m0 = (0, 0, 1) at every point, for the phase invariance: adding one constant to every phase turns the whole train about z, which the
magnitude loss does not see, so sum_k dL/dphases[k] = 0.

Bounds, composed through the seed as blochmag_ref's docstring composes them, with bt = blochtrain_ref.bound_train in the place of eps
and bj = bound_jvp of the chain's tangent.  Per echo entry of a point, with r = rho - t_xy and D = |de_x| + |de_y|:
    lsq:  the seed errs by at most rw w_xy (2 + 4 |r| / rho) bt + rw w_z bt                                          (S_lsq bt per point)
    gn:   by at most bj rw (2 w_xy + w_z) + C_GN bt rw w_xy D / rho,  C_GN = 2 sqrt 2 + 4                          (W2 bj + C_GN G bt)
and likewise for the final entry with wf.  These sums take the place of blochtraingn_ref._seed_sum in the bounds of both chains:
    b1:     g: vjp.bound_b1 at the reference seed + reach (sum over points);  dL/dm0: vjp.bound_m0 + the point's own sum
    sched:  gg: bound_gains + max|scale| Theta sum_points mu (.),  gp: bound_phases + 2 sum_points mu (.)
    L:      bt (sqrt 2 sum rw w_xy |r| + sum rw w_z |e_z - t_z|) + L_QUAD sum rw w (.)^2, final term likewise
The constants are the imported ones (TOL, C_BOUND, L_QUAD, C_GN); none is tuned after a device run.  The factor 1 / rho makes the
bounds vacuous where rho is tiny, so the bounded comparisons run on bounded(chain, name): the case with w_xy set to 0 wherever the
long-double rho of an echo or final state is below RHO_MIN = 1e-3 (mask_small_rho; a point-sized weight of the broadcast form goes
where any repetition's rho is).  On every case here the mask removes nothing (small_rho: the smallest rho is 5.2e-3, on h1_long's
echoes), which tests/test_blochtrainmag_cpu.py asserts, so bounded() returns the case's own arrays; the exact properties (rho = 0
itself among them) are tested on case_of(), without the mask."""
import functools
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sgr = _load("blochtrainschedgn_ref")
mag = _load("blochmag_ref")
gnr, sj, sched, tr, vjp = sgr.gnr, sgr.sj, sgr.sched, sgr.tr, sgr.vjp
jvp = gnr.jvp
RHO_MIN, C_GN = mag.RHO_MIN, mag.C_GN
TOL, L_QUAD, H_TOL, ROUTE_TOL = sgr.TOL, sgr.L_QUAD, sgr.H_TOL, sgr.ROUTE_TOL
FD_ANGLE, FD_TOL = gnr.FD_ANGLE, gnr.FD_TOL
share, full, rw_of, mag_dir = gnr.share, gnr.full, gnr.rw_of, mag.mag_dir
CHAINS = ("b1", "sched")
_SRC = dict(b1=gnr, sched=sgr)


def _dress(c, rng):
    """the dressed case with its triples replaced by pairs (xy, z) of the same shapes"""
    c = dict(c)
    for key, lo in (("w", None), ("t", -0.2), ("wf", None), ("tf", -0.2)):
        out = []
        for tri in c[key]:
            if tri is None:
                out.append(None)
                continue
            shape = np.shape(tri[0])
            out.append(tuple(gnr._weights(rng, (2,) + shape)) if lo is None
                       else (rng.uniform(lo, 1.0, shape), rng.uniform(-1.0, 1.0, shape)))
        c[key] = out
    return c


@functools.lru_cache(maxsize=None)
def cases(chain):
    rng = np.random.default_rng(dict(b1=53, sched=59)[chain])
    return {name: _dress(c, rng) for name, c in _SRC[chain].cases().items()}


@functools.lru_cache(maxsize=None)
def small(chain):
    return _dress(_SRC[chain].small(), np.random.default_rng(dict(b1=61, sched=67)[chain]))


@functools.lru_cache(maxsize=None)
def z0():
    """small() of the schedule with m0 = (0, 0, 1) at every point"""
    c = dict(small("sched"))
    c["m0"] = [None]
    return c


def case_of(chain, name):
    return z0() if name == "z0" else small(chain) if name == "small" else cases(chain)[name]


def mask_small_rho(c):
    """(the case with w_xy = 0 wherever the long-double rho of an echo or of the final state is below RHO_MIN, entries masked)"""
    d, n = dict(c, w=list(c["w"]), wf=list(c["wf"])), 0
    for q in range(len(c["pulses"])):
        E, F = primal(c, q)
        for key, e in (("w", E), ("wf", F)):
            if c[key][q] is None:
                continue
            low = np.asarray(mag_dir(e[0], e[1])[0] < RHO_MIN)
            n += int(low.sum())
            wxy = np.asarray(c[key][q][0])
            if key == "w" and wxy.ndim == 3:                                     # the broadcast form: one weight for every repetition
                low = low.any(1)
            if low.any():
                d[key][q] = (np.where(low, 0.0, wxy), c[key][q][1])
    return d, n


@functools.lru_cache(maxsize=None)
def bounded(chain, name):
    """the case of the bounded comparisons: case_of(chain, name) under mask_small_rho"""
    return mask_small_rho(case_of(chain, name))[0]


def directions(chain, name, K):
    return _SRC[chain].directions("small" if name == "z0" else name, K)


# ---- the seeds ------------------------------------------------------------------------------------------------------------------
def primal(c, q, dtype=np.longdouble, b1=None):
    """(E, F): the echoes, three (S, ntr, nf, npos), and the final state, three (S, nf, npos)"""
    runs = [gnr._train(c, q, s, dtype, b1) for s in c["scales"]]
    return [np.stack([E[:, i] for E, _ in runs]) for i in range(3)], [np.stack([F[i] for _, F in runs]) for i in range(3)]


def _pairs(c, q, dtype):
    cast = lambda v: None if v is None else [np.asarray(x).astype(dtype) for x in v]
    rw = rw_of(c, q).astype(dtype)[None, :, None, None]
    return cast(full(c, q, c["w"][q])), cast(full(c, q, c["t"][q])), cast(c["wf"][q]), cast(c["tf"][q]), rw


def _inv(w, rho):
    """1 / rho where the entry is weighted, 0 elsewhere"""
    on = np.asarray(w > 0)
    return np.where(on, 1 / np.where(on & (rho > 0), rho, 1), 0).astype(np.float64)


def lsq_seed(c, q, dtype=np.longdouble, b1=None):
    """(ce, cf, L, info): the seeds as the imported adjoints take them (three (S, ntr, nf, npos) or None, three (S, nf, npos) or
    None), the loss, and per point (S, nf, npos) the sums of the bounds: S (the seed's error per unit of bt), A and Q (the loss's)"""
    W, T, wf, tf, rw = _pairs(c, q, dtype)
    E, F = primal(c, q, dtype, b1)
    ce = cf = None
    L, info = dtype(0), dict(S=0.0, A=0.0, Q=0.0)
    for e, w, t, r_, ax in ((E, W, T, rw, 1), (F, wf, tf, dtype(1), None)):
        if w is None:
            continue
        rho, ux, uy = mag_dir(e[0], e[1])
        r, rz = rho - t[0], e[2] - t[1]
        cot = (r_ * w[0] * r * ux, r_ * w[0] * r * uy, r_ * w[1] * rz)
        L = L + ((r_ * w[0] * r * r).sum() + (r_ * w[1] * rz * rz).sum()) / 2
        red = (lambda v: np.asarray(v, dtype=np.float64).sum(ax)) if ax is not None else (lambda v: np.asarray(v, dtype=np.float64))
        info["S"] = info["S"] + red(r_ * (w[0] * (2 + 4 * np.abs(r) * _inv(w[0], rho)) + w[1]))
        info["A"] = info["A"] + red(r_ * (np.sqrt(2.0) * w[0] * np.abs(r) + w[1] * np.abs(rz)))
        info["Q"] = info["Q"] + red(r_ * (w[0] * r * r + w[1] * rz * rz))
        if ax is not None:
            ce = cot
        else:
            cf = cot
    return ce, cf, L, info


def tangents(chain, c, q, v, dtype=np.longdouble):
    """(dE, dF): three (K, S, ntr, nf, npos), three (K, S, nf, npos) along the directions v (b1: (K, ntime); sched: (dg, dp))"""
    if chain == "sched":
        return sj.run(sj.sched_jvp, c, q, v[0], v[1], None, dtype)
    tan = gnr.tangent(c, q, np.asarray(v).reshape(-1, len(c["pulses"][q][0])), dtype)
    return ([np.stack([dE[:, :, i] for dE, _ in tan], 1) for i in range(3)], [np.stack([dF[:, i] for _, dF in tan], 1) for i in range(3)])


def gn_seed(chain, c, q, v, dtype=np.longdouble):
    """(per direction (ce, cf), info): info holds per direction and point (K, S, nf, npos) W2 (per unit of bj) and G (per unit of
    C_GN bt), and E (K,), sum W (U J v)^2"""
    W, _, wf, _, rw = _pairs(c, q, dtype)
    E, F = primal(c, q, dtype)
    dE, dF = tangents(chain, c, q, v, dtype)
    K = dE[0].shape[0]
    ces, cfs = [None] * K, [None] * K
    info = dict(W2=0.0, G=0.0, E=np.zeros(K, dtype=dtype))
    for e, de, w, r_, ax in ((E, dE, W, rw, 2), (F, dF, wf, dtype(1), None)):
        if w is None:
            continue
        rho, ux, uy = mag_dir(e[0], e[1])
        a = ux * de[0] + uy * de[1]                                                          # (K, ...)
        cot = (r_ * w[0] * a * ux, r_ * w[0] * a * uy, r_ * w[1] * de[2])
        red = (lambda x: np.asarray(x, dtype=np.float64).sum(ax)) if ax is not None else (lambda x: np.asarray(x, dtype=np.float64))
        info["W2"] = info["W2"] + red(np.broadcast_to(r_ * (2 * w[0] + w[1]), a.shape))
        info["G"] = info["G"] + red(r_ * w[0] * (np.abs(de[0]) + np.abs(de[1])) * _inv(w[0], rho))
        info["E"] = info["E"] + (r_ * (w[0] * a * a + w[1] * de[2] * de[2])).reshape(K, -1).sum(1)
        for d in range(K):
            if ax is not None:
                ces[d] = tuple(x[d] for x in cot)
            else:
                cfs[d] = tuple(x[d] for x in cot)
    return list(zip(ces, cfs)), info


# ---- the fits ---------------------------------------------------------------------------------------------------------------------
def lsq(chain, c, q, dtype=np.longdouble):
    """b1: (L, g (ntime,), (gmx, gmy, gmz));  sched: (L, gg (ntr,), gp (ntr,), (gmx, gmy, gmz))"""
    ce, cf, L, _ = lsq_seed(c, q, dtype)
    return (L,) + tuple(gnr._sweep(c, q, ce, cf, dtype) if chain == "b1" else sgr._adj(c, q, ce, cf, dtype))


def loss(c, q, dtype=np.longdouble, b1=None):
    return lsq_seed(c, q, dtype, b1)[2]


def gn(chain, c, q, v, dtype=np.longdouble):
    """b1: H v (K, ntime);  sched: (Hg (K, ntr), Hp (K, ntr))"""
    seeds, _ = gn_seed(chain, c, q, v, dtype)
    if chain == "b1":
        return np.stack([gnr._sweep(c, q, ce, cf, dtype)[0] for ce, cf in seeds])
    res = [sgr._adj(c, q, ce, cf, dtype) for ce, cf in seeds]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def weighted_square(chain, c, q, v, dtype=np.longdouble):
    return gn_seed(chain, c, q, v, dtype)[1]["E"]


def _mag_cot(e, w, t, de, r_, dtype):
    """the seed of one repetition or of the final state on lists of three arrays: lsq (de None) or gn"""
    rho, ux, uy = mag_dir(e[0], e[1])
    if de is None:
        r, rz = rho - t[0], e[2] - t[1]
        return [r_ * w[0] * r * ux, r_ * w[0] * r * uy, r_ * w[1] * rz], (r_ * w[0] * r * r).sum() / 2 + (r_ * w[1] * rz * rz).sum() / 2
    a = ux * de[0] + uy * de[1]
    return [r_ * w[0] * a * ux, r_ * w[0] * a * uy, r_ * w[1] * de[2]], dtype(0)


def _walks(c, q, dtype, dg=None, dp=None):
    """The schedule's second route: blochtrainschedgn_ref's structured walk with the magnitude seed.  (L, gg, gp, gm), or (Hg, Hp)"""
    W, T, wf, tf, _ = sgr._planes(c, q, dtype)[:4] + (None,)
    rw = rw_of(c, q).astype(dtype)
    L, gg, gp, gm = dtype(0), 0, 0, []
    for si in range(len(c["scales"])):
        planes, table, us, es, ms, mN, des, dmN, mq = sgr._walk(c, q, si, dtype, dg, dp)
        ce = None
        if W is not None:
            ce = []
            for k in range(c["ntr"][q]):
                cot, Lk = _mag_cot(es[k], [W[i][si][k] for i in range(2)], None if T is None else [T[i][si][k] for i in range(2)],
                                   None if dg is None else des[k], rw[k], dtype)
                ce.append(cot)
                L = L + Lk
        lam = [np.zeros_like(mN[0] if dg is None else dmN[0])] * 3
        if wf is not None:
            lam, Lk = _mag_cot(mN, [wf[i][si] for i in range(2)], None if tf is None else [tf[i][si] for i in range(2)],
                               None if dg is None else dmN, dtype(1), dtype)
            L = L + Lk
        g, p, l0 = sgr._contract(c, q, planes, table, us, es, ms, ce, lam, mq)
        gg, gp = gg + g, gp + p
        gm.append(l0)
    if dg is not None:
        return gg, gp
    return L, gg, gp, tuple(np.stack([l[i] for l in gm]) for i in range(3))


def lsq_walk(c, q, dtype=np.longdouble):
    return _walks(c, q, dtype)


def gn_walk(c, q, dg, dp, dtype=np.longdouble):
    return _walks(c, q, dtype, *sgr._dirs(c, q, dg, dp, dtype))


@functools.lru_cache(maxsize=None)
def reference(chain, name):
    """The long-double lsq() per pulse of a bounded case, computed once"""
    c = bounded(chain, name)
    return [lsq(chain, c, q) for q in range(len(c["pulses"]))]


@functools.lru_cache(maxsize=None)
def reference_gn(chain, name, K):
    """The long-double gn() along directions(chain, name, K) per pulse of a bounded case, computed once"""
    c = bounded(chain, name)
    return [gn(chain, c, q, directions(chain, name, K)[q]) for q in range(len(c["pulses"]))]


def projected(c, q, E=None, F=None):
    """The component case whose L and g are the magnitude fit's: targets (t_xy u_x, t_xy u_y, t_z) at the direction u of (E, F)
    (None: the long-double train's), weights (w_xy, w_xy, w_z), full echo form, as float64"""
    if E is None:
        E, F = primal(c, q)
    d = dict(c, bcast=False)
    for key in ("w", "t", "wf", "tf"):
        d[key] = list(c[key])
    W, T, wf, tf, _ = _pairs(c, q, np.float64)
    for e, w, t, kw, kt in ((E, W, T, "w", "t"), (F, wf, tf, "wf", "tf")):
        if w is None:
            continue
        _, ux, uy = mag_dir(*[np.asarray(x) for x in e[:2]])
        d[kw][q] = (w[0], w[0], w[1])
        d[kt][q] = tuple(np.asarray(x, dtype=np.float64) for x in (t[0] * ux, t[0] * uy, t[1]))
    return d


def small_rho(c, q):
    """(the number of echo and final entries whose long-double rho is below RHO_MIN, the smallest rho)"""
    E, F = primal(c, q)
    rho = np.concatenate([mag_dir(e[0], e[1])[0].ravel() for e in (E, F)])
    return int((rho < RHO_MIN).sum()), float(rho.min())


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
def _with(c, q, ce, cf):
    return gnr._with_cot(c, q, ce, cf)


def bound_g(chain, c, q):
    """b1: per b1 entry (ntime,);  sched: (bound of a gg entry, bound of a gp entry)"""
    ce, cf, _, info = lsq_seed(c, q)
    at, e = _with(c, q, ce, cf), info["S"] * gnr._bt(c, q)                                  # e: (S, nf, npos)
    if chain == "b1":
        return vjp.bound_b1(at, q) + gnr._reach(c, q) * float(e.sum())
    e = float((e * sgr._mu(c, q)).sum())
    return sched.bound_gains(at, q) + sched.smax_of(c) * sched.theta_of(c, q) * e, sched.bound_phases(at, q) + 2.0 * e


def bound_gm(c, q):
    """per dL/dm0 entry (S, nf, npos), either chain"""
    ce, cf, _, info = lsq_seed(c, q)
    return vjp.bound_m0(_with(c, q, ce, cf), q) + info["S"] * gnr._bt(c, q)


def bound_l(c, q):
    info = lsq_seed(c, q)[3]
    return float((info["A"] * gnr._bt(c, q)).sum() + L_QUAD * np.sum(info["Q"]))


def bound_h(chain, c, q, v):
    """b1: per entry of H v (K, ntime);  sched: (bounds of the Hg entries (K,), of the Hp entries (K,))"""
    seeds, info = gn_seed(chain, c, q, v)
    if chain == "b1":
        bj = jvp.bound_jvp(c, q, np.asarray(v).reshape(-1, len(c["pulses"][q][0])), None)  # (K, nf, npos)
    else:
        bj = sj.bound_jvp(c, q, v[0], v[1], None)
    e = info["W2"] * bj[:, None] + C_GN * info["G"] * gnr._bt(c, q)                        # (K, S, nf, npos)
    if chain == "b1":
        return np.stack([vjp.bound_b1(_with(c, q, ce, cf), q) + gnr._reach(c, q) * float(e[d].sum()) for d, (ce, cf) in enumerate(seeds)])
    bg, bp = [], []
    for d, (ce, cf) in enumerate(seeds):
        at, ed = _with(c, q, ce, cf), float((e[d] * sgr._mu(c, q)).sum())
        bg.append(sched.bound_gains(at, q) + sched.smax_of(c) * sched.theta_of(c, q) * ed)
        bp.append(sched.bound_phases(at, q) + 2.0 * ed)
    return np.array(bg), np.array(bp)


def scale_fd(chain, c, q):
    """the units of the central differences at the reference seed: b1 (ntime,); sched (gains, phases)"""
    ce, cf, _, _ = lsq_seed(c, q)
    at = _with(c, q, ce, cf)
    return vjp.scale_b1(at, q) if chain == "b1" else (sched.scale_gains(at, q), sched.scale_phases(at, q))


def pair_tol(chain, c, q, u, v):
    """the tolerance of <u, H v> = <H u, v> for float64 products: the two sides' bounds"""
    if chain == "b1":
        return float((bound_h(chain, c, q, v)[0] * np.abs(u)).sum() + (bound_h(chain, c, q, u)[0] * np.abs(v)).sum())
    bu, bv = bound_h(chain, c, q, u), bound_h(chain, c, q, v)
    return float(bv[0][0] * np.abs(u[0]).sum() + bv[1][0] * np.abs(u[1]).sum() + bu[0][0] * np.abs(v[0]).sum()
                 + bu[1][0] * np.abs(v[1]).sum())
