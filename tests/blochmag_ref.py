"""NumPy restatement of the magnitude least-squares products of the Bloch simulator (helper of tests/test_blochmag_cpu.py and
tests/test_blochmag_gpu.py; not collected): the fits of (|Mxy|, mz) of DESIGN 8ah, for the end point of the transient (mode 0) and
for the steady state of the period (mode 1), in float64 or np.longdouble.  tests/blochgn_ref.py and tests/blochssgn_ref.py are loaded
by path; their forward sweeps, tangents, reverse recursions, cases and the steady state's pass 0 are used as they are.  Only the
seed between the forward and the reverse sweep is new.

With m = (mx, my, mz) the end point or the steady state at scale s, weights (w_xy, w_z) >= 0 and targets (t_xy, t_z) per (scale,
frequency, position) point:
    rho = sqrt(mx mx + my my),   u = (mx, my) / rho, and (0, 0) where rho = 0
    L   = 1/2 sum w_xy (rho - t_xy)^2 + w_z (mz - t_z)^2
    lsq seed  c = (w_xy (rho - t_xy) u_x, w_xy (rho - t_xy) u_y, w_z (mz - t_z))            g = J' c
    gn  seed  c = (w_xy (u . dm_xy) u_x,  w_xy (u . dm_xy) u_y,  w_z dm_z),  dm = J v        H v = J' U' W U J v
In the steady state lambda = inv' c follows, as in blochssgn_ref.

Bounds of the device comparison.  They compose the component bounds through the seed as blochgn_ref and blochssgn_ref do: the sweep
after the seed is linear in it, so an error e of the seed adds (gain) sum|e| to an entry of g or H v, gain = max|s| gamma dt_t in the
transient and kappa times that in the steady state.  Let eps be the bound of a component of m (1e-12 in the transient, bound_m(kappa)
in the steady state) and bj that of a component of dm (bound_jvp), and write r = rho - t_xy, a = u . dm_xy.
    rho:  d rho = u . dm_xy-error, |u| <= 1, so |d rho| <= |(ex, ey)|_2 <= sqrt(2) eps
    u:    d u = (I - u u') (ex, ey) / rho to first order, a projection: |d u|_2 <= sqrt(2) eps / rho; a component is taken as
          <= 2 eps / rho, which also covers the second order for rho >= 1e-3 (it is smaller by eps / rho <= 1e-9)
    lsq:  c_x = w_xy r u_x:  |e_x| + |e_y| <= w_xy (|d rho| (|u_x| + |u_y|) + |r| (|d u_x| + |d u_y|)) <= w_xy eps (2 + 4 |r| / rho),
          |e_z| <= w_z eps.                                   sum|e| <= eps sum (w_xy (2 + 4 |r| / rho) + w_z)                  =: eps S
    gn:   |d a| <= (|d u_x| |dm_x| + |d u_y| |dm_y|) + |u . (dm-error)| <= 2 eps D / rho + sqrt(2) bj,  D = |dm_x| + |dm_y|, |a| <= D
          |e_x| + |e_y| <= w_xy (|d a| (|u_x| + |u_y|) + |a| (|d u_x| + |d u_y|)) <= w_xy (2 bj + (2 sqrt(2) + 4) eps D / rho)
          |e_z| <= w_z bj.                     sum|e| <= bj sum (2 w_xy + w_z) + (2 sqrt(2) + 4) eps sum w_xy D / rho        =: bj W2 + C eps G
    g:    gain (tol N + eps S),  N = sum|c| of the reference's seed, tol = 1e-12 the reverse sweep's own term
    H v:  gain (tol N + bj W2 + C eps G)
    L:    d(1/2 w r^2) = w r dr:  eps (sqrt(2) sum w_xy |r| + sum w_z |mz - t_z|) + 1e-13 sum w (.)^2 for the order of the sum
All sums run over the pulse's points and scales.  The factor 1 / rho makes them vacuous where rho is tiny, so the bounded
comparisons run with w_xy = 0 wherever the long-double reference has rho < RHO_MIN = 1e-3 (mask_small_rho); the exact properties
(rho = 0 itself among them) are tested without the mask."""
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gnref = _load("blochgn_ref")
ssg = _load("blochssgn_ref")
_grad = gnref._grad
SCALES, TOL, GAMMA_H1, _grid = gnref.SCALES, gnref.TOL, gnref.GAMMA_H1, gnref._grid
gamma_of, intervals = gnref.gamma_of, gnref.intervals
RHO_MIN = 1e-3
C_GN = 2 * np.sqrt(2.0) + 4


def planes(pair, S, nf, npos, dtype=np.float64):
    """A pair of weights or targets, each entry (S, nf, npos), (nf, npos) or a scalar -> (2, S, nf, npos)"""
    return np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (S, nf, npos)) for v in pair]).astype(dtype)


def mag_dir(mx, my):
    """(rho, ux, uy); u = 0 where rho = 0"""
    rho = np.sqrt(mx * mx + my * my)
    safe = np.where(rho > 0, rho, 1)
    return rho, np.where(rho > 0, mx / safe, 0), np.where(rho > 0, my / safe, 0)


def _lsq_seed(m, w, tg, k, info):
    """The lsq seed of scale k and its loss, the sums of the bounds added to info"""
    rho, ux, uy = mag_dir(m[0], m[1])
    r, rz = rho - tg[0, k], m[2] - tg[1, k]
    lam = [w[0, k] * r * ux, w[0, k] * r * uy, w[1, k] * rz]
    q = float((w[0, k] * r * r).sum() + (w[1, k] * rz * rz).sum())
    on = np.asarray(w[0, k] > 0)
    rel = np.where(on, np.abs(r) / np.where(on & (rho > 0), rho, 1), 0)                      # |r| / rho where it is weighted
    info["N"] += float(sum(np.abs(l).sum() for l in lam))
    info["S"] += float((w[0, k] * (2 + 4 * rel)).sum() + w[1, k].sum())
    info["A"] += float(np.sqrt(2.0) * (w[0, k] * np.abs(r)).sum() + (w[1, k] * np.abs(rz)).sum())
    info["Q"] += q
    return lam, ((w[0, k] * r * r).sum() + (w[1, k] * rz * rz).sum()) / 2


def _gn_seed(m, dm, w, k, info):
    """The gn seed of scale k for the K directions dm (3 x (K, nf, npos)), the sums of the bounds added to info"""
    rho, ux, uy = mag_dir(m[0], m[1])
    a = ux * dm[0] + uy * dm[1]
    lam = [w[0, k] * a * ux, w[0, k] * a * uy, w[1, k] * dm[2]]
    on = np.asarray(w[0, k] > 0)
    inv_rho = np.where(on, 1 / np.where(on & (rho > 0), rho, 1), 0)
    info["N"] += np.array(sum(np.abs(l).sum((-2, -1)) for l in lam), dtype=np.float64)
    info["G"] += np.array((w[0, k] * (np.abs(dm[0]) + np.abs(dm[1])) * inv_rho).sum((-2, -1)), dtype=np.float64)
    info["E"] = info["E"] + (w[0, k] * a * a + w[1, k] * dm[2] * dm[2]).sum((-2, -1))
    return lam


def _w2(w):
    return float(2 * w[0].sum() + w[1].sum())


# ---- the transient's end point (mode 0) -----------------------------------------------------------------------------------------
def rho_of(pulse, df, pos, scales, m0=None, dtype=np.longdouble):
    """rho (S, nf, npos) of the end point"""
    b1, gr, tp, t1, t2, nucleus = pulse
    out = []
    for s in scales:
        m = gnref.forward(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, dtype)
        out.append(mag_dir(m[0], m[1])[0])
    return np.stack(out)


def lsq(pulse, df, pos, targets, weights, scales, m0=None, dtype=np.float64, parts=False):
    """(L, g (n,)) of pulse = (b1, gr, tp, t1, t2, nucleus) for pairs of targets and weights; with parts also the sums of the bounds"""
    b1, gr, tp, t1, t2, nucleus = pulse
    L, g, info = dtype(0), 0, dict(N=0.0, S=0.0, A=0.0, Q=0.0)
    w = tg = None
    for k, s in enumerate(scales):
        m, traj, Q = gnref.forward(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, dtype, keep=True)
        if w is None:
            w, tg = planes(weights, len(scales), Q.nf, Q.npos, dtype), planes(targets, len(scales), Q.nf, Q.npos, dtype)
        lam, Lk = _lsq_seed(m, w, tg, k, info)
        L = L + Lk
        g = g + gnref._reverse(Q, traj, lam)
    return (L, g, info) if parts else (L, g)


def gn(pulse, df, pos, v, weights, scales, m0=None, dtype=np.float64, parts=False):
    """H v (K, n) for the directions v (K, n) (or (n,) -> (n,)); with parts also the sums of the bounds, per direction"""
    b1, gr, tp, t1, t2, nucleus = pulse
    v = np.asarray(v, dtype=np.complex128)
    one = v.ndim == 1
    v = v.reshape(-1, len(np.ravel(b1)))
    h, w = 0, None
    info = dict(N=np.zeros(len(v)), G=np.zeros(len(v)), E=np.zeros(len(v), dtype=dtype))
    for k, s in enumerate(scales):
        m, traj, Q = gnref.forward(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, dtype, keep=True)
        _, dm = gnref.jvp(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), s, m0, v, None, dtype)
        if w is None:
            w = planes(weights, len(scales), Q.nf, Q.npos, dtype)
        h = h + gnref._reverse(Q, traj, _gn_seed(m, dm, w, k, info))
    info["W2"] = _w2(w)
    h = h[0] if one else h
    return (h, info) if parts else h


def _drive(pulse, scales):
    return max(abs(s) for s in scales) * gamma_of(pulse[5]) * intervals(pulse)


def bound_g(pulse, info, scales):
    """Per b1 entry (n,)"""
    return _drive(pulse, scales) * TOL * (info["N"] + info["S"])


def bound_h(pulse, v, info, scales):
    """Per entry of direction k (K, n)"""
    v = np.asarray(v).reshape(-1, len(pulse[0]))
    bj = gnref.bound_jvp(pulse, v, None, scales)[:, 0, 0]                  # (K,)
    return _drive(pulse, scales)[None, :] * (TOL * info["N"] + bj * info["W2"] + C_GN * TOL * info["G"])[:, None]


def bound_L(info):
    return TOL * info["A"] + 1e-13 * info["Q"]


def to_pairs(tgs, wts):
    """The triples of blochgn_ref.cases / blochssgn_ref.cases -> pairs: w_xy = wx, w_z = wz, t_xy = |tx| (in [0, 1]), t_z = tz"""
    return [(np.abs(t[0]), t[2]) for t in tgs], [(w[0], w[2]) for w in wts]


def mask_small_rho(w, rho):
    """(the pair with w_xy = 0 where rho < RHO_MIN, the share of the points that removes)"""
    small = np.asarray(rho < RHO_MIN)
    return (np.where(small, 0.0, w[0]), w[1]), float(small.mean())


def cases(shared, K):
    """blochgn_ref.cases(shared, K) with pairs for triples and w_xy = 0 where the long-double rho is below RHO_MIN:
    (pulses, dfs, dps, m0s, targets, weights, vs, the share of the points each pulse loses)"""
    pulses, dfs, dps, m0s, tgs, wts, vs = gnref.cases(shared, K)
    tgs, wts = to_pairs(tgs, wts)
    lost = []
    for q, (p, df, dp, m0) in enumerate(zip(pulses, dfs, dps, m0s)):
        wts[q], share = mask_small_rho(wts[q], rho_of(p, df, dp, SCALES, m0))
        lost.append(share)
    return pulses, dfs, dps, m0s, tgs, wts, vs, lost


# ---- the steady state of the period (mode 1) ------------------------------------------------------------------------------------
def ss_rho_of(pulse, df, pos, scales, dtype=np.longdouble):
    """rho (S, nf, npos) of the steady state"""
    return np.stack([mag_dir(*ssg._period(pulse, df, pos, s, dtype)[2][:2])[0] for s in scales])


def ss_products(pulse, df, pos, targets, weights, v, scales, dtype=np.float64):
    """blochssgn_ref.products with the magnitude seeds: (L, g, info of lsq, h, info of gn); targets None: no lsq; v None: no gn.
    Both infos hold kappa, the largest ||inv||_2 met, floored at 1, and lsq's holds M."""
    n = len(np.ravel(pulse[0]))
    if v is not None:
        v = np.asarray(v, dtype=np.complex128).reshape(-1, n)
    K = 0 if v is None else len(v)
    L, g, h, w, tg, Ms, kap = dtype(0), 0, 0, None, None, [], 1.0
    li, hi = dict(N=0.0, S=0.0, A=0.0, Q=0.0), dict(N=np.zeros(K), G=np.zeros(K), E=np.zeros(K, dtype=dtype))
    for k, s in enumerate(scales):
        Q, inv, M = ssg._period(pulse, df, pos, s, dtype)
        if w is None:
            w = planes(weights, len(scales), Q.nf, Q.npos, dtype)
            tg = None if targets is None else planes(targets, len(scales), Q.nf, Q.npos, dtype)
        seeds, swept = [], s != 0
        norm = np.stack([np.stack([inv[i][j] for j in range(3)], -1) for i in range(3)], -2).astype(np.float64)
        kap = max(kap, float(np.linalg.norm(norm, 2, axis=(-2, -1)).max()))
        if tg is not None:
            cot, Lk = _lsq_seed(M, w, tg, k, li)
            L = L + Lk
            seeds.append([c[None] for c in cot])
        if not swept and K:
            zero = np.zeros((K, Q.nf, Q.npos), dtype=dtype)
            uvw, d = None, [zero, zero, zero]
        else:
            _, uvw, d = ssg._forward(Q, s, v if K else None, M)
        if K:
            seeds.append(_gn_seed(M, _grad._mat_vec(inv, d), w, k, hi))
        cot = [np.concatenate([sd[c] for sd in seeds]) for c in range(3)]
        if swept:
            out = ssg._reverse(Q, s, uvw, _grad._mat_vec(inv, cot, transpose=True))
        else:
            out = np.zeros((len(cot[0]), Q.n), dtype=np.complex128 if dtype == np.float64 else np.clongdouble)
        if tg is not None:
            g, out = g + out[0], out[1:]
        if K:
            h = h + out
        Ms.append(M)
    hi["W2"] = _w2(w)
    li["kappa"] = hi["kappa"] = kap
    li["M"] = tuple(np.stack([m[c] for m in Ms]) for c in range(3))
    if targets is None:
        return None, None, None, h, hi
    return L, g, li, (h if K else None), (hi if K else None)


def ss_lsq(pulse, df, pos, targets, weights, scales, dtype=np.float64, parts=False):
    L, g, info, _, _ = ss_products(pulse, df, pos, targets, weights, None, scales, dtype)
    return (L, g, info) if parts else (L, g)


def ss_gn(pulse, df, pos, v, weights, scales, dtype=np.float64, parts=False):
    _, _, _, h, info = ss_products(pulse, df, pos, None, weights, v, scales, dtype)
    h = h[0] if np.ndim(v) == 1 else h
    return (h, info) if parts else h


def ss_bound_g(pulse, info, scales, k):
    """Per b1 entry (n,)"""
    return _drive(pulse, scales) * k * (TOL * info["N"] + ssg.bound_m(k) * info["S"])


def ss_bound_h(pulse, v, info, scales, k):
    """Per entry of direction j (K, n)"""
    v = np.asarray(v).reshape(-1, len(pulse[0]))
    bj = ssg.ssref.bound_jvp(pulse, v, scales, k)[:, 0, 0]                  # (K,)
    return _drive(pulse, scales)[None, :] * k * (TOL * info["N"] + bj * info["W2"] + C_GN * ssg.bound_m(k) * info["G"])[:, None]


def ss_bound_L(info, k):
    return ssg.bound_m(k) * info["A"] + 1e-13 * info["Q"]


SS_DROPPED = ((True, 4),)


def ss_cases(shared, K):
    """blochssgn_ref.cases(shared, K) with pairs for triples and w_xy = 0 where the long-double rho is below RHO_MIN:
    (pulses, dfs, dps, targets, weights, vs, the share of the points each period loses, the periods kept for the bounded comparisons).
    At scale 0 the steady state is (0, 0, 1) exactly, so rho = 0 at every point of that scale by construction (the exact-zero tests
    cover it); the share counts the points of the other scales.  SS_DROPPED: (shared, period) whose share exceeds a tenth, the 255-sample
    period on the shared 3 x 5 grid (a third of its points), which stays out of the bounded comparisons and in every other test."""
    pulses, dfs, dps, tgs, wts, vs = ssg.cases(shared, K)
    tgs, wts = to_pairs(tgs, wts)
    lost = []
    on = np.array([s != 0 for s in SCALES])
    for q, (p, df, dp) in enumerate(zip(pulses, dfs, dps)):
        rho = ss_rho_of(p, df, dp, SCALES)
        wts[q], _ = mask_small_rho(wts[q], rho)
        lost.append(float(np.asarray(rho[on] < RHO_MIN).mean()))
    kept = [q for q in range(len(pulses)) if (shared, q) not in SS_DROPPED]
    return pulses, dfs, dps, tgs, wts, vs, lost, kept
