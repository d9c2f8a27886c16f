"""A high-precision reference of the cone algebra of one interior-point iteration (cone_dev.h and the kernels of solver.hip between
the KKT solves), for mbfir.test_unit_cone: tests/test_cone_gpu.py holds the device to it stage by stage, tests/test_cone_cpu.py
holds the float64 NumPy formulas of oracle/conic_ipm.py (`twin`) to the same bounds on the same inputs and checks the reference
against its own definitions.  Nothing here needs a GPU.

Arithmetic.  Second-order cones (the 3-row cones and the big cone) are worked in mpmath at 60 digits; the orthant rows, whose
formulas are a ratio, a product and a square root per row, and the long sums (h'z, c'x, ||v||^2) in numpy.longdouble (64-bit
mantissa: 2^-11 u per operation, pairwise sums: below 0.1 u of the envelope at 15 000 rows, which the "+ 2" of every K covers).

Hand-over.  Every stage takes the DEVICE's outputs of the stages before it as exact inputs (the NT scaling as (eta, w) per cone and
dl, wl per row, lam, the scaled affine direction, sigma, ...), so a wrong stage fails alone and its bound follows from its own
arithmetic.  `end_to_end` runs the whole chain in the reference from the inputs alone.

What a definition gives is taken from the definition, not from the kernel's closed form:
  NT scaling     W is formed from the device's (eta, w) as the matrix eta [w0 w1'; w1 I + w1 w1'/(1 + w0)] (dense where the cone
                 has at most DENSE rows; `Soc.mul` is the same matrix row by row), W^-1 is that matrix's exact inverse (block
                 elimination, valid for any w, not only w'Jw = 1), W^-2 its square.  Checked: (eta, w) against the textbook scaling
                 of (s, z) (`nt_ref`), w'Jw = 1, lam = W z, lam = W^-1 s, wbz2 = W^-2 bz2.
  step bound     per cone the largest alpha with lam + alpha d in K: a ratio on the orthant; on a second-order cone the first
                 root of (lam + alpha d)'J(lam + alpha d) = A alpha^2 + 2 B alpha + C: 1/alpha = (-B + sqrt(B^2 - A C))/C.
                 S_TMAX = max(0, these, -dtau/tau, -dkappa/kappa); alpha_a, sigma, alpha_0, alpha follow.
  dtau, dkappa   the scalar equation of the embedding with high-precision h'z, c'x, ||W z1||^2.
  lam \\ d        the arrow matrix Arw(lam) = [l0 l1'; l1 l0 I] solved by elimination (dense LU where the cone has <= DENSE rows).
  corrector      eigenvalues of the Jordan product from its arrow matrix (v0 +- ||v1||; `mp.eigsy` of the dense matrix on the
                 small cones in the CPU test), the projection as oracle/conic_ipm.py states it (CORR_*); 3-row cones: exact zeros.

Bounds.  u = 2^-53; every bound is K u times an envelope: the sum of the absolute values of the stage's own terms, pushed through
|W| / |W^-1| / |Arw^-1| where the stage applies them.  kd(m) = min(m, ceil(m / 1024) + 16) + 2 is the length of the longest
rounding chain of a dot product of m terms (a 3-row cone: serial; the big cone: ceil(m / 1024) strided terms per thread, a
6-step wave tree, 16 waves folded by one more tree; + 2 for the reference).  Conditioning: a cone vector v with relative boundary
gap g(v) = (v0 - ||v1||)/||v1|| loses 1/g in its Jordan residual v'Jv: ||v1|| carries kd/2 + 1 roundings, v0 - ||v1|| then has the
relative error (kd/2 + 1)/g + 1, the product with v0 + ||v1||, the square root and the division give
        r(v) = (kd/4 + 5)/min(1, g(v))                 [relative error of v / sqrt(v'Jv) in units of u]
and 2 r without the square root (soc3_div).  The float64 formulas of the oracle miss the 60-digit scaling by 0.5 - 0.8 u/g (measured:
684 u at g = 1e-3, 7e5 u at 1e-6); that loss is in the data and the bounds carry it as r, never as a constant.
  scaling    dl: 2; wl, lam (orthant): 3; wbz2 (orthant): 2.
             w_i: (|sb_i| r(s) + |zb_i| r(z))/(2 gamma) + |w_i| (E (r(s) + r(z) + kd) / 2 + 4),  E = sum |sb_i zb_i| / (1 + sb'zb),
             the cancellation in gamma^2 = (1 + sb'zb)/2;   eta: (r(s) + r(z))/2 + 3, relative.
             w'Jw - 1: 2 sum |w_i| bound_i.   lam = W z: (kd + 6) |W| |z|.
             lam = W^-1 s: that, + 4 (|dW| |z| + |dW^-1| |s|) + rel(eta) (|W| |z| + |W^-1| |s|) with |dW| the first-order change of W
             under the bound of w (W^-1 s = W z holds for the exact scaling only; the device's differs from it by that much).
             wbz2 (cones): ((kd + 8) u + 4 |w'Jw - 1|_bound) eta^-2 (2 |w_i| |w|'|v| + |v_i|).
  dtau       numerator K_R + K_N + 8 on its envelope, denominator K_R + 2 kd + 16 on kappa/tau + sum (|W| |z1|)^2, with
             K_R = 2 + 8 + ceil(blocks / 256) + 8 (product, block tree, fold and its tree), K_N = 2 + ceil(N / 256) + 8.
             dkappa (dtau handed over): 4.
  directions orthant ds: 6 (+ 1 for the division by wl), dz: 3 (+ 1); cones: (kd + 12) |W^-1| env(ds), (kd + 9) |W| env(dz).
  step       orthant: 2 |d / lam| (+ 2 where d is formed from ds, dz in the kernel: combined and corrected direction).
             cone: (2 r(lam) + 2 kd + 12 [+ kd + 6]) (||env(rho_1)|| + env(rho_0)), rho = T(lam) d as soc3_step forms it.
             S_TMAX: the largest cone bound (max is 1-Lipschitz), + 2 u on the scalar terms.  alpha: 2, sigma: 5, bx: 3.
  comb. rhs  lds orthant: 6; cones: (2 r(lam) + 2 kd + 16) |Arw^-1|-envelope of soc3_div on (sigma mu e + |lam| o |lam| + |a| o |b|).
             bz: 5 resp. kd + 10 on |rz| + |W| |lds|.   wbz: as wbz2.
  corrector  orthant: v = (lam + at ds/w)(lam + at w dz) carries 8 roundings of V = (|lam| + at |ds/w|)(|lam| + at |w dz|): three per
             factor, the product, the reference; the target t = clip - v carries the box edge's two (sigma mu, its multiple), the
             difference, the division by lam, the product with w and the reference: bz_k: (8 V + 6 |t|) w / lam.  Big cone: (6 kd + 60 + 3 r(lam)) |W| div_env(T), T_0 = V_0 + ||V_1||,
             T_i = T_0 (|v_i| + V_i)/||v_1||.  An orthant product inside the box gives t = 0 in the oracle; the kernel's
             min(max(v, lo), hi) - v contracts the subtraction with the product into one fma and returns the product's rounding error,
             at most u |v|: inside the bound, so no exact zero is asked there (it is on the 3-row cones and, inside the box, on the
             big cone, whose eigenvalues are sums).
  update     x, s, z: 4 on |v| + alpha |dv|; tau, kappa: 3.  The candidate sums of k_corr_add are single additions: bit-exact.
  shift      RB[0]: (kd/2 + 2)(||v1|| + |v0|); RB[1]: K_R sum v^2; shifted entries: 3 (|v| + 1 + |t|); the others bit-exact.
  end to end the end state against `end_to_end` (no hand-over): the stage bounds carried forward to first order, see there.
`twin` must stay inside these bounds on every input of the device tests (tests/test_cone_cpu.py); a device fraction above 1 where
the twin passes is a finding about the kernel, not about K.

Decisions (alpha = 1 at a zero bound, min(1, .), the cap on sigma, the corrector's projections and its floor, the pick, the shift
test) are taken by the reference; `margins` holds, per decision, the distance of the deciding quantity from its threshold
relative to the quantity's envelope, and the inputs are drawn so that it is at least MARGIN = 1e-6.  The device must reproduce
every decision exactly.
"""
import numpy as np
import mpmath as mp

import lattice_ref as L
from oracle import conic_ipm as O

mp.mp.dps = 60
U = 2.0 ** -53
LD = np.longdouble
STEP = 0.99
MARGIN = 1e-6
DENSE = 64
STAGES = ("scaling", "affine", "comb_rhs", "combined", "corr_rhs", "corrector", "update", "shift")


def kd(m):
    return min(m, -(-m // 1024) + 16) + 2


def k_rows(P):
    nb = max(1, -(-(P["l"] + P["nq3"]) // 256)) + (1 if P["big"] else 0)
    return 2 + 8 + -(-nb // 256) + 8


def k_cols(P):
    return 2 + -(-P["N"] // 256) + 8


# ---- small helpers --------------------------------------------------------------------------------------------------
def ld(a):
    a = np.asarray(a)
    return a if a.dtype == LD else a.astype(np.float64).astype(LD)


def M(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def m2ld(x):
    """mpmath -> longdouble without passing through one float64"""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def mpv(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).ravel()]


def mdot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def mnorm(a):
    return mp.sqrt(mp.fsum(x * x for x in a))


def jf(a, b):
    return a[0] * b[0] - mdot(a[1:], b[1:])


def tof(a):
    return np.array([float(x) for x in a], dtype=np.float64)


def merr(dev, ref):
    """|dev - ref| per entry: dev float64, ref mpf (the difference formed in mpmath)."""
    return np.array([float(abs(mp.mpf(float(d)) - r)) for d, r in zip(np.asarray(dev, dtype=np.float64).ravel(), ref)])


def socs(P):
    """(first row, rows, kind, index) of every second-order cone: the 3-row cones, then the big cone."""
    out = [(P["l"] + 3 * c, 3, "q3", c) for c in range(P["nq3"])]
    if P["big"]:
        out.append((P["l"] + 3 * P["nq3"], P["big"], "big", 0))
    return out


def gap(v):
    """relative boundary gap (v0 - ||v1||) / ||v1|| of a cone vector (float64 from mpmath)."""
    v = mpv(v)
    n1 = mnorm(v[1:])
    return float((v[0] - n1) / n1) if n1 > 0 else np.inf


def rcond(v, m):
    return (kd(m) / 4.0 + 5.0) / min(1.0, gap(v))


class Rec:
    """worst error / bound per (stage, output) and the exact checks that failed."""

    def __init__(self):
        self.frac, self.failed = {}, []

    def add(self, stage, name, err, bound):
        err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(err == 0, 0.0, err / bound)
        f = np.where(np.isfinite(f), f, np.inf)
        v = float(f.max()) if f.size else 0.0
        self.frac[(stage, name)] = max(self.frac.get((stage, name), 0.0), v)

    def exact(self, stage, name, ok):
        if not bool(ok):
            self.failed.append((stage, name))

    def worst(self):
        out = {}
        for (st, _), v in self.frac.items():
            out[st] = max(out.get(st, 0.0), v)
        return out

    def over(self):
        return sorted((k, v) for k, v in self.frac.items() if not v <= 1.0)


# ---- a second-order cone's scaling matrix from (eta, w) --------------------------------------------------------------------
class Soc:
    def __init__(self, eta, w):
        self.eta, self.w, self.m = mp.mpf(float(eta)), mpv(w), len(w)
        self.ef, self.wa = float(eta), np.abs(np.asarray(w, dtype=np.float64))

    def mul(self, u):
        w = self.w
        d = mdot(w[1:], u[1:])
        f = u[0] + d / (1 + w[0])
        return [self.eta * (w[0] * u[0] + d)] + [self.eta * (ui + f * wi) for ui, wi in zip(u[1:], w[1:])]

    def inv(self, u):
        """the exact inverse of the matrix `mul` applies (block elimination on [w0 w1'; w1 B], B = I + w1 w1'/(1 + w0))."""
        w = self.w
        beta = 1 / (1 + w[0])
        n = mdot(w[1:], w[1:])
        k = beta / (1 + beta * n)                           # B^-1 = I - k w1 w1'
        wu = mdot(w[1:], u[1:])
        x0 = (u[0] - (wu - k * n * wu)) / (w[0] - (n - k * n * n))
        c = x0 + k * (wu - n * x0)
        return [x0 / self.eta] + [(ui - c * wi) / self.eta for ui, wi in zip(u[1:], w[1:])]

    def inv2(self, u):
        return self.inv(self.inv(u))

    def dense(self):
        w, m = self.w, self.m
        M = mp.matrix(m, m)
        for i in range(m):
            for j in range(m):
                if i == 0 or j == 0:
                    M[i, j] = w[i + j]
                else:
                    M[i, j] = (1 if i == j else 0) + w[i] * w[j] / (1 + w[0])
        return M * self.eta

    def wjw(self):
        return jf(self.w, self.w)

    def _abs(self, ua):
        w = self.wa
        d = float(w[1:] @ ua[1:])
        f = ua[0] + d / (1 + w[0])
        return np.concatenate([[w[0] * ua[0] + d], ua[1:] + f * w[1:]])

    def abs_mul(self, ua):
        return self.ef * self._abs(np.asarray(ua, dtype=np.float64))

    def abs_inv(self, ua):
        return self._abs(np.asarray(ua, dtype=np.float64)) / self.ef

    def abs_inv2(self, va):
        va = np.asarray(va, dtype=np.float64)
        return (2 * self.wa * float(self.wa @ va) + va) / self.ef ** 2

    def dabs(self, b, ua):
        """|dW| |u| / eta to first order for |dw| <= b (the same expression serves W and W^-1: J w has the magnitudes of w)."""
        w, ua = self.wa, np.asarray(ua, dtype=np.float64)
        q = 1 + w[0]
        wu, bu = float(w[1:] @ ua[1:]), float(b[1:] @ ua[1:])
        row0 = float(b @ ua)
        rest = b[1:] * (ua[0] + wu / q) + w[1:] * (bu / q + wu * b[0] / q ** 2)
        return np.concatenate([[row0], rest])


def nt_ref(s, z):
    """the textbook NT scaling of a cone pair in mpmath: eta, w, sbar, zbar, gamma."""
    a, b = mp.sqrt(jf(s, s)), mp.sqrt(jf(z, z))
    sb, zb = [x / a for x in s], [x / b for x in z]
    gamma = mp.sqrt((1 + mdot(sb, zb)) / 2)
    w = [(sb[0] + zb[0]) / (2 * gamma)] + [(x - y) / (2 * gamma) for x, y in zip(sb[1:], zb[1:])]
    return mp.sqrt(a / b), w, sb, zb, gamma


def arw_solve(lam, d):
    """x with Arw(lam) x = d, Arw(lam) = [l0 l1'; l1 l0 I]: dense LU on the small cones, elimination of the arrow on the others."""
    m = len(lam)
    if m <= DENSE:
        A = mp.matrix(m, m)
        for i in range(m):
            A[i, i] = lam[0]
            if i:
                A[0, i] = A[i, 0] = lam[i]
        return list(mp.lu_solve(A, mp.matrix(d)))
    x0 = (d[0] - mdot(lam[1:], d[1:]) / lam[0]) / (lam[0] - mdot(lam[1:], lam[1:]) / lam[0])
    return [x0] + [(di - x0 * li) / lam[0] for di, li in zip(d[1:], lam[1:])]


def div_env(lamf, D, m):
    """the envelope of soc3_div / the big cone's division on |d| <= D, and its K (2 r(lam) + 2 kd + 16)."""
    lamf = np.asarray(lamf, dtype=np.float64)
    nl = float(np.linalg.norm(lamf[1:]))
    a = (lamf[0] - nl) * (lamf[0] + nl)
    e0 = (abs(lamf[0]) * D[0] + float(np.abs(lamf[1:]) @ D[1:])) / a
    return np.concatenate([[e0], (D[1:] + e0 * np.abs(lamf[1:])) / lamf[0]]), 2 * rcond(lamf, m) + 2 * kd(m) + 16


def jprod(u, v):
    return [mdot(u, v)] + [u[0] * y + v[0] * x for x, y in zip(u[1:], v[1:])]


def jprod_abs(ua, va):
    return np.concatenate([[float(ua @ va)], ua[0] * va[1:] + va[0] * ua[1:]])


def soc_t(lam, d):
    """1/alpha of the first root of (lam + alpha d)'J(lam + alpha d) (negative or zero: no bound)."""
    A, B, C = jf(d, d), jf(lam, d), jf(lam, lam)
    disc = B * B - A * C
    return (-B + mp.sqrt(disc if disc > 0 else 0)) / C


def soc_t_bound(lamf, D, m, extra=0):
    lamf, D = np.asarray(lamf, dtype=np.float64), np.asarray(D, dtype=np.float64)
    nl = float(np.linalg.norm(lamf[1:]))
    a = np.sqrt((lamf[0] - nl) * (lamf[0] + nl))
    lb = np.abs(lamf) / a
    dote = float(lb[1:] @ D[1:])
    rho0 = (lb[0] * D[0] + dote) / a
    re = (D[1:] + (D[0] + dote / (1 + lb[0])) * lb[1:]) / a
    return U * (2 * rcond(lamf, m) + 2 * kd(m) + 12 + extra) * (float(np.linalg.norm(re)) + rho0)


# ---- the device's (or the twin's) outputs by name -------------------------------------------------------------------------
def unpack(o, b, P):
    """lane b of mbfir.test_unit_cone's result as a dict of named outputs, cut to the lane's own rows."""
    import mbfir
    R, N = P["R"], P["N"]
    D = {k: o["out_r"][b, i, :R].copy() for i, k in enumerate(mbfir.UNIT_CONE_OUT_R)}
    D["wbb"] = o["out_r"][b, mbfir.UNIT_CONE_OUT_R.index("wbb"), :max(P["big"], 1)].copy()
    D.update({"x_" + k if k in ("x",) else k: o["out_x"][b, i, :N].copy() for i, k in enumerate(mbfir.UNIT_CONE_OUT_X)})
    D["w3"] = o["w3"][b, :max(P["nq3"], 1)].copy()
    D["sc"] = {sn: dict(zip(mbfir.UNIT_CONE_SC, o["sc"][b, i])) for i, sn in enumerate(mbfir.UNIT_CONE_SNAPS)}
    D["raw_r"], D["raw_x"] = o["out_r"][b].copy(), o["out_x"][b].copy()
    return D


def device_scaling(P, D):
    out = []
    for (r0, m, kind, c) in socs(P):
        out.append(Soc(D["w3"][c, 0], D["w3"][c, 1:4]) if kind == "q3" else Soc(D["sc"]["scaling"]["etab"], D["wbb"][:m]))
    return out


# ---- stage 1: NT scaling ----------------------------------------------------------------------------------------------------
def check_scaling(P, I, D, rec):
    l = P["l"]
    s, z = ld(I["s"][:l]), ld(I["z"][:l])
    st = "scaling"
    rec.add(st, "dl", np.abs(ld(D["dl"][:l]) - z / s), 2 * U * np.abs(z / s))
    rec.add(st, "wl", np.abs(ld(D["wl"][:l]) - np.sqrt(s / z)), 3 * U * np.sqrt(s / z))
    rec.add(st, "lam", np.abs(ld(D["lam"][:l]) - np.sqrt(s * z)), 3 * U * np.sqrt(s * z))
    for k in ("a", "b"):
        ref = ld(D["dl"][:l]) * ld(I["bz2" + k][:l])
        rec.add(st, "wbz2", np.abs(ld(D["wbz2" + k][:l]) - ref), 2 * U * np.abs(ref))
    Ws = device_scaling(P, D)
    for (r0, m, kind, c), W in zip(socs(P), Ws):
        sf, zf = I["s"][r0:r0 + m], I["z"][r0:r0 + m]
        sm, zm = mpv(sf), mpv(zf)
        eta, w, sb, zb, gamma = nt_ref(sm, zm)
        rs, rz = rcond(sf, m), rcond(zf, m)
        sba, zba, g = np.abs(tof(sb)), np.abs(tof(zb)), float(gamma)
        E = float(sba @ zba) / float(1 + mdot(sb, zb))
        bw = U * ((sba * rs + zba * rz) / (2 * g) + np.abs(tof(w)) * (E * (rs + rz + kd(m)) / 2 + 4))
        reta = U * ((rs + rz) / 2 + 3)
        rec.add(st, "w_" + kind, merr([float(x) for x in W.w], w), bw)
        rec.add(st, "eta_" + kind, abs(float(W.eta - eta)), reta * float(eta))
        bj = 2 * float(np.abs(tof(w)) @ bw)
        rec.add(st, "wJw_" + kind, abs(float(W.wjw() - 1)), bj)
        lam_d = D["lam"][r0:r0 + m]
        eW = W.abs_mul(np.abs(zf))
        b1 = U * (kd(m) + 6) * eW
        rec.add(st, "lam=Wz_" + kind, merr(lam_d, W.mul(zm)), b1)
        eWi = W.abs_inv(np.abs(sf))
        b2 = b1 + 4 * (W.ef * W.dabs(bw, np.abs(zf)) + W.dabs(bw, np.abs(sf)) / W.ef) + reta * (eW + eWi) + U * (kd(m) + 6) * eWi
        rec.add(st, "lam=Wis_" + kind, merr(lam_d, W.inv(sm)), b2)
        if kind == "q3":
            for k in ("a", "b"):
                v = I["bz2" + k][r0:r0 + m]
                rec.add(st, "wbz2_q3", merr(D["wbz2" + k][r0:r0 + m], W.inv2(mpv(v))), (U * (kd(m) + 8) + 4 * bj) * W.abs_inv2(np.abs(v)))
    return Ws


def winv2_check(P, Ws, D, vname, oname, st, rec):
    """out = W^-2 v on the orthant rows (dl handed over) and the 3-row cones."""
    l = P["l"]
    ref = ld(D["dl"][:l]) * ld(D[vname][:l])
    rec.add(st, oname, np.abs(ld(D[oname][:l]) - ref), 2 * U * np.abs(ref))
    for (r0, m, kind, c), W in zip(socs(P), Ws):
        if kind != "q3":
            continue
        v = D[vname][r0:r0 + m]
        bj = 4 * abs(float(W.wjw() - 1)) + 8 * U
        rec.add(st, oname + "_q3", merr(D[oname][r0:r0 + m], W.inv2(mpv(v))), (U * (kd(m) + 8) + bj) * W.abs_inv2(np.abs(v)))


# ---- dtau / dkappa and the directions ------------------------------------------------------------------------------------------
def lsum(a):
    return np.sum(ld(a)) if len(a) else LD(0)


def dtau_ref(P, I, Ws, sc, x2, z2, mode):
    """the scalar equation of the embedding: dtau and the bound of the kernels' value (mpmath scalars from longdouble / mpmath sums)."""
    l, N = P["l"], P["N"]
    h, c = P["h"], P["c"][:N]
    tau, kap, mu, rt = [M(sc[k]) for k in ("tau", "kappa", "mu", "rt")]
    z1 = I["z1"]

    def rows(a, b):
        t = mp.mpf(float(lsum(ld(a[:l]) * ld(b[:l])))) if l else mp.mpf(0)
        # (longdouble products are not exact: the orthant part is split, see the module docstring)
        return t + mdot(mpv(a[l:]), mpv(b[l:]))
    hz2, cx2 = rows(h, z2), mp.mpf(float(lsum(ld(c) * ld(x2[:N]))))
    wz = mp.mpf(float(lsum((ld(sc["wl_dev"][:l]) * ld(z1[:l])) ** 2))) if l else mp.mpf(0)
    wz_env = float(wz)
    for (r0, m, kind, cc), W in zip(socs(P), Ws):
        wz += mp.fsum(x * x for x in W.mul(mpv(z1[r0:r0 + m])))
        wz_env += float(np.sum(W.abs_mul(np.abs(z1[r0:r0 + m])) ** 2))
    den = kap / tau + wz
    if mode == 0:
        dkc, bt, sig = -kap * tau, -rt, mp.mpf(0)
        dkc_env = float(kap * tau)
    else:
        sig = M(sc["sigma"])
        dka, dta = M(sc["dkap_a"]), M(sc["dtau_a"])
        dkc, bt = sig * mu - kap * tau - dka * dta, -(1 - sig) * rt
        dkc_env = float(sig * mu + kap * tau + abs(dka * dta))
    num = dkc / tau - bt + cx2 + hz2
    env_num = dkc_env / float(tau) + float(abs(bt)) + float(np.abs(c) @ np.abs(x2[:N])) + float(np.abs(h) @ np.abs(z2))
    dt = num / den
    kmax = max([kd(m) for (_, m, _, _) in socs(P)] + [0])
    bound = U * ((k_rows(P) + k_cols(P) + 12) * env_num + (k_rows(P) + 2 * kmax + 16) * abs(float(dt)) * (float(kap / tau) + wz_env)) / float(den)
    return dt, bound, dkc, dkc_env


def check_dir(P, I, Ws, D, rec, st, mode, x2, z2, g2, dtau, dkap, sigma, outA, outB, scal):
    """dtau, dkappa and the direction's two vectors: mode 0 (W^-1 ds_a, W dz_a), else (ds, dz)."""
    l = P["l"]
    sc = dict(scal, wl_dev=D["wl"])
    dt, bdt, dkc, dkc_env = dtau_ref(P, I, Ws, sc, x2, z2, mode)
    keep = dict(bdt=bdt, dkc_env=dkc_env, den=abs(float(dkc / M(scal["tau"]) + M(scal["rt"]) * (1 - M(sigma))
                                                         + mp.mpf(float(lsum(ld(P["c"][:P["N"]]) * ld(x2[:P["N"]])))) + mp.mpf(float(np.asarray(P["h"]) @ np.asarray(z2)))) / abs(float(dt))) if dt != 0 else 1.0)
    rec.add(st, "dtau", abs(float(mp.mpf(float(dtau)) - dt)), bdt)
    tau, kap = mp.mpf(float(scal["tau"])), mp.mpf(float(scal["kappa"]))
    dtd = mp.mpf(float(dtau))
    rec.add(st, "dkappa", abs(float(mp.mpf(float(dkap)) - (dkc - kap * dtd) / tau)), 4 * U * (dkc_env + float(kap * abs(dtd))) / float(tau))
    oms = LD(1) if mode == 0 else LD(1) - LD(float(sigma))
    dtl = LD(float(dtau))
    h, z1, g1, rz = P["h"], I["z1"], I["g1"], I["rz"]
    ds = -oms * ld(rz) - ld(g2) - dtl * (ld(g1) - ld(h))
    dz = ld(z2) + dtl * ld(z1)
    ds_env = np.abs(float(oms) * rz) + np.abs(g2) + abs(float(dtau)) * (np.abs(g1) + np.abs(h))
    dz_env = np.abs(z2) + abs(float(dtau)) * np.abs(z1)
    wl = ld(D["wl"][:l])
    if mode == 0:
        rec.add(st, "dss", np.abs(ld(outA[:l]) - ds[:l] / wl), 7 * U * ds_env[:l] / D["wl"][:l])
        rec.add(st, "wdz", np.abs(ld(outB[:l]) - dz[:l] * wl), 4 * U * dz_env[:l] * D["wl"][:l])
    else:
        rec.add(st, "ds", np.abs(ld(outA[:l]) - ds[:l]), 6 * U * ds_env[:l])
        rec.add(st, "dz", np.abs(ld(outB[:l]) - dz[:l]), 3 * U * dz_env[:l])
    omm, dtm = mp.mpf(float(oms)), mp.mpf(float(dtau))
    for (r0, m, kind, c), W in zip(socs(P), Ws):
        sl = slice(r0, r0 + m)
        dsm = [-omm * a - b - dtm * (cc - d) for a, b, cc, d in zip(mpv(rz[sl]), mpv(g2[sl]), mpv(g1[sl]), mpv(h[sl]))]
        dzm = [a + dtm * b for a, b in zip(mpv(z2[sl]), mpv(z1[sl]))]
        if mode == 0:
            rec.add(st, "dss_" + kind, merr(outA[sl], W.inv(dsm)), U * (kd(m) + 12) * W.abs_inv(ds_env[sl]))
            rec.add(st, "wdz_" + kind, merr(outB[sl], W.mul(dzm)), U * (kd(m) + 9) * W.abs_mul(dz_env[sl]))
        else:
            rec.add(st, "ds_" + kind, merr(outA[sl], dsm), 6 * U * ds_env[sl])
            rec.add(st, "dz_" + kind, merr(outB[sl], dzm), 3 * U * dz_env[sl])
    keep.update(ds_env=ds_env, dz_env=dz_env)
    return keep


# ---- step bound ---------------------------------------------------------------------------------------------------------------
def step_ref(P, Ws, D, dA, dB, scaled, dtau, dkap, tau, kap):
    """S_TMAX of the direction by the definition of the step bound.  scaled: (dA, dB) are W^-1 ds and W dz (the affine direction's
    outputs); otherwise they are ds, dz and are scaled here in the reference.  Returns dict(t, bound, label, row, terms): terms
    holds every kind's largest 1/alpha (negative: no bound from that kind)."""
    l = P["l"]
    lam = D["lam"]
    terms, bounds = {}, [0.0]
    if l:
        wl, lm = ld(D["wl"][:l]), ld(lam[:l])
        a = ld(dA[:l]) if scaled else ld(dA[:l]) / wl
        b = ld(dB[:l]) if scaled else ld(dB[:l]) * wl
        t = np.maximum(-a / lm, -b / lm)
        i = int(np.argmax(t))
        terms["orth"] = (float(t[i]), i)
        bounds.append(float((2 if scaled else 4) * U * np.max(np.maximum(np.abs(a / lm), np.abs(b / lm)))))
    for (r0, m, kind, c), W in zip(socs(P), Ws):
        sl = slice(r0, r0 + m)
        lm = mpv(lam[sl])
        if scaled:
            a, b = mpv(dA[sl]), mpv(dB[sl])
            ea, eb, extra = np.abs(dA[sl]), np.abs(dB[sl]), 0
        else:
            a, b = W.inv(mpv(dA[sl])), W.mul(mpv(dB[sl]))
            ea, eb, extra = W.abs_inv(np.abs(dA[sl])), W.abs_mul(np.abs(dB[sl])), kd(m) + 6
        t = max(soc_t(lm, a), soc_t(lm, b))
        if kind not in terms or float(t) > terms[kind][0]:
            terms[kind] = (float(t), c)
        bounds.append(max(soc_t_bound(lam[sl], ea, m, extra), soc_t_bound(lam[sl], eb, m, extra)))
    terms["tau"] = (float(-mp.mpf(float(dtau)) / mp.mpf(float(tau))), 0)
    terms["kappa"] = (float(-mp.mpf(float(dkap)) / mp.mpf(float(kap))), 0)
    bounds.append(2 * U * max(abs(terms["tau"][0]), abs(terms["kappa"][0])))
    label = max(terms, key=lambda k: terms[k][0])
    t = terms[label][0]
    if t <= 0:
        label, t = "none", 0.0
    return dict(t=t, bound=max(bounds), label=label, row=terms.get(label, (0, 0))[1], terms=terms)


def alpha_of(t, frac):
    return 1.0 if t == 0.0 else min(1.0, frac / t)


def margin_step(S, frac):
    """margins of the decisions of a step length: bound 0 or not, and min(1, frac / t)."""
    out = {}
    top = max(v[0] for v in S["terms"].values())
    out["zero_bound"] = abs(top) / max(1.0, abs(top))
    if S["t"] > 0:
        out["min1"] = abs(S["t"] - frac) / max(S["t"], frac)
    return out


# ---- the whole check of one lane -------------------------------------------------------------------------------------------------
def check_lane(P, I, D, corrector, corr_big=True):
    """Every output of every stage of lane inputs I against the reference.  Returns (Rec, facts): facts holds the reference's
    decisions, their margins and what bound each step length."""
    rec, facts = Rec(), dict(margins={}, decisions={})
    l, N = P["l"], P["N"]
    sc_in = dict(zip(("tau", "kappa", "mu", "rt", "sigmax", "dres", "nrmc", "rnc"), I["sc"]))
    S = D["sc"]
    Ws = check_scaling(P, I, D, rec)
    # ---- affine direction ------------------------------------------------------------------------------------------------
    st = "affine"
    A = S["comb_rhs"]
    Ka = check_dir(P, I, Ws, D, rec, st, 0, I["x2"], I["z2"], I["g2"], A["dtau_a"], A["dkap_a"], 0.0, D["dssa"], D["wdza"], sc_in)
    T = step_ref(P, Ws, D, D["dssa"], D["wdza"], True, A["dtau_a"], A["dkap_a"], sc_in["tau"], sc_in["kappa"])
    rec.add(st, "tmax", abs(A["tmax"] - T["t"]), T["bound"])
    facts["affine"] = T
    facts["margins"].update({"affine_" + k: v for k, v in margin_step(T, 1.0).items()})
    rec.exact(st, "alpha_a==1 at a zero bound", (A["tmax"] == 0.0) == (T["t"] == 0.0))
    a_ref = alpha_of(A["tmax"], 1.0)
    rec.add(st, "alpha_a", abs(A["alpha_a"] - a_ref), 2 * U * a_ref)
    facts["decisions"]["affine_alpha1"] = alpha_of(T["t"], 1.0) == 1.0
    rec.exact(st, "alpha_a capped", (A["alpha_a"] == 1.0) == facts["decisions"]["affine_alpha1"])
    cube = (1.0 - A["alpha_a"]) ** 3
    capped = cube > sc_in["sigmax"]
    facts["decisions"]["sigma_capped"] = bool(capped)
    facts["margins"]["sigma_cap"] = abs(cube - sc_in["sigmax"]) / max(cube, sc_in["sigmax"])
    if capped:
        rec.exact(st, "sigma == cap", A["sigma"] == sc_in["sigmax"])
    else:
        rec.add(st, "sigma", abs(A["sigma"] - float((1 - mp.mpf(float(A["alpha_a"]))) ** 3)), 5 * U * cube)
    sig = A["sigma"]
    bx_ref = -(LD(1) - LD(sig)) * ld(I["rx"][:N])
    rec.add(st, "bxc", np.abs(ld(D["bxc"][:N]) - bx_ref), 3 * U * np.abs(bx_ref))
    # ---- combined right-hand side ------------------------------------------------------------------------------------------
    st = "comb_rhs"
    smu = LD(sig) * LD(sc_in["mu"])
    lam, a, b = ld(D["lam"][:l]), ld(D["dssa"][:l]), ld(D["wdza"][:l])
    q_ref = (smu - lam * lam - a * b) / lam
    rec.add(st, "lds", np.abs(ld(D["lds"][:l]) - q_ref), 6 * U * (float(smu) + np.abs(lam * lam) + np.abs(a * b)) / np.abs(lam))
    oms = LD(1) - LD(sig)
    bz_ref = -oms * ld(I["rz"][:l]) - ld(D["wl"][:l]) * ld(D["lds"][:l])
    rec.add(st, "bzc", np.abs(ld(D["bzc"][:l]) - bz_ref), 5 * U * (np.abs(float(oms) * I["rz"][:l]) + np.abs(D["wl"][:l] * D["lds"][:l])))
    smum, omm = mp.mpf(float(sig)) * mp.mpf(float(sc_in["mu"])), 1 - mp.mpf(float(sig))
    for (r0, m, kind, c), W in zip(socs(P), Ws):
        sl = slice(r0, r0 + m)
        lm, am, bm = mpv(D["lam"][sl]), mpv(D["dssa"][sl]), mpv(D["wdza"][sl])
        ll, ab = jprod(lm, lm), jprod(am, bm)
        dsc = [smum - ll[0] - ab[0]] + [-x - y for x, y in zip(ll[1:], ab[1:])]
        la, aa, ba = np.abs(D["lam"][sl]), np.abs(D["dssa"][sl]), np.abs(D["wdza"][sl])
        Denv = jprod_abs(la, la) + jprod_abs(aa, ba)
        Denv[0] += float(smum)
        env, K = div_env(D["lam"][sl], Denv, m)
        rec.add(st, "lds_" + kind, merr(D["lds"][sl], arw_solve(lm, dsc)), U * K * env)
        wq = W.mul(mpv(D["lds"][sl]))
        rec.add(st, "bzc_" + kind, merr(D["bzc"][sl], [-omm * r - y for r, y in zip(mpv(I["rz"][sl]), wq)]),
                U * (kd(m) + 10) * (np.abs(float(omm) * I["rz"][sl]) + W.abs_mul(np.abs(D["lds"][sl]))))
    winv2_check(P, Ws, D, "bzc", "wbzc", st, rec)
    # ---- combined direction ------------------------------------------------------------------------------------------------
    st = "combined"
    Cc = S["comb"]
    scal = dict(sc_in, sigma=sig, dtau_a=A["dtau_a"], dkap_a=A["dkap_a"])
    K1 = check_dir(P, I, Ws, D, rec, st, 1, I["xc"], I["zc"], I["gc"], Cc["dtau"], Cc["dkap"], sig, D["ds"], D["dz"], scal)
    T1 = step_ref(P, Ws, D, D["ds"], D["dz"], False, Cc["dtau"], Cc["dkap"], sc_in["tau"], sc_in["kappa"])
    facts["combined"] = T1
    facts["margins"].update({"combined_" + k: v for k, v in margin_step(T1, STEP).items()})
    E = S["update"]

    def step_checks(st, snap, Tr, key, name):
        rec.add(st, "tmax" + name, abs(snap["tmax"] - Tr["t"]), Tr["bound"])
        rec.exact(st, "alpha" + name + "==1 at a zero bound", (snap["tmax"] == 0.0) == (Tr["t"] == 0.0))
        ar = alpha_of(snap["tmax"], STEP)
        rec.add(st, "alpha" + name, abs(snap[key] - ar), 2 * U * ar)
        rec.exact(st, "alpha" + name + " capped", (snap[key] == 1.0) == (alpha_of(Tr["t"], STEP) == 1.0))

    def moved(st, alpha, dtau, dkap, x2, dsv, dzv):
        al = LD(float(alpha))
        xr = ld(I["x"][:N]) + al * (ld(x2[:N]) + LD(float(dtau)) * ld(I["x1"][:N]))
        rec.add(st, "x", np.abs(ld(D["x_x"][:N]) - xr), 4 * U * (np.abs(I["x"][:N]) + alpha * (np.abs(x2[:N]) + abs(dtau) * np.abs(I["x1"][:N]))))
        for nm, v, dv in (("s", I["s"], dsv), ("z", I["z"], dzv)):
            rec.add(st, nm, np.abs(ld(D[nm]) - (ld(v) + al * ld(dv))), 3 * U * (np.abs(v) + alpha * np.abs(dv)))
        for nm, v, dv in (("tau", sc_in["tau"], dtau), ("kappa", sc_in["kappa"], dkap)):
            rec.add(st, nm, abs(E[nm] - float(LD(v) + al * LD(float(dv)))), 3 * U * (abs(v) + alpha * abs(dv)))
        # strictly interior after the update, by definition
        ok = bool(np.all(D["s"][:l] > 0) and np.all(D["z"][:l] > 0))
        for (r0, m, kind, c) in socs(P):
            for v in (D["s"], D["z"]):
                vm = mpv(v[r0:r0 + m])
                ok = ok and vm[0] > 0 and jf(vm, vm) > 0
        rec.exact(st, "(s, z) strictly interior after the update", ok and E["tau"] > 0 and E["kappa"] > 0)

    def beyond(st, Tr, alpha, dsv, dzv, dtau, dkap):
        """at alpha / STEP (1 + 1e-6) the binding term is outside its cone (only where the step bound decided the step)."""
        if not (Tr["t"] > 0 and alpha < 1.0):
            return
        a2 = mp.mpf(float(alpha)) / mp.mpf(STEP) * (1 + mp.mpf(10) ** -6)
        out = (sc_in["tau"] + float(a2) * dtau < 0) or (sc_in["kappa"] + float(a2) * dkap < 0)
        if l:
            wl, lm = ld(D["wl"][:l]), ld(D["lam"][:l])
            out = out or bool(np.any(lm + LD(float(a2)) * ld(dsv[:l]) / wl < 0) or np.any(lm + LD(float(a2)) * ld(dzv[:l]) * wl < 0))
        for (r0, m, kind, c), W in zip(socs(P), Ws):
            sl = slice(r0, r0 + m)
            lm = mpv(D["lam"][sl])
            for d in (W.inv(mpv(dsv[sl])), W.mul(mpv(dzv[sl]))):
                p = [x + a2 * y for x, y in zip(lm, d)]
                out = out or p[0] < 0 or jf(p, p) < 0
        rec.exact(st, "outside the cone just past alpha / STEP", out)

    if not corrector:
        step_checks("update", E, T1, "alpha", "")
        moved("update", E["alpha"], Cc["dtau"], Cc["dkap"], I["xc"], D["ds"], D["dz"])
        beyond("update", T1, E["alpha"], D["ds"], D["dz"], Cc["dtau"], Cc["dkap"])
    else:
        # ---- corrector right-hand side -------------------------------------------------------------------------------------
        st = "corr_rhs"
        K0 = S["corr_rhs"]
        step_checks(st, K0, T1, "alpha0", "0")
        a0 = K0["alpha0"]
        at = min(1.0, a0 + O.CORR_DELTA)
        facts["margins"]["corr_at"] = abs(a0 + O.CORR_DELTA - 1.0)
        mut = LD(sig) * LD(sc_in["mu"])
        lo, hi = LD(O.CORR_BMIN) * mut, LD(O.CORR_BMAX) * mut
        wl, lam = ld(D["wl"][:l]), ld(D["lam"][:l])
        dss, wdz = ld(D["ds"][:l]) / wl, wl * ld(D["dz"][:l])
        v = (lam + LD(at) * dss) * (lam + LD(at) * wdz)
        V = (np.abs(lam) + at * np.abs(dss)) * (np.abs(lam) + at * np.abs(wdz))
        tt = np.maximum(np.minimum(np.maximum(v, lo), hi) - v, -hi)
        branch = np.where(v < lo, 0, np.where(v <= hi, 1, np.where(v <= 2 * hi, 2, 3)))
        facts["decisions"]["corr_branches"] = sorted(set(int(x) for x in branch))
        if l:
            thr = np.stack([lo + 0 * v, hi + 0 * v, 2 * hi + 0 * v])
            facts["margins"]["corr_box"] = float(np.min(np.abs(v[None, :] - thr) / np.maximum(V, float(hi))[None, :]))
        b_ref = -wl * (tt / lam)
        rec.add(st, "kbz", np.abs(ld(D["kbz"][:l]) - b_ref), U * (8 * V + 6 * np.abs(tt)) * D["wl"][:l] / D["lam"][:l])
        ref = ld(D["dl"][:l]) * ld(D["kbz"][:l])
        rec.add(st, "wbzk", np.abs(ld(D["wbzk"][:l]) - ref), 2 * U * np.abs(ref))
        for (r0, m, kind, c), W in zip(socs(P), Ws):
            sl = slice(r0, r0 + m)
            if kind == "q3":
                rec.exact(st, "kbz, wbzk == 0 on the 3-row cones", np.all(D["kbz"][sl] == 0.0) and np.all(D["wbzk"][sl] == 0.0))
                continue
            if not corr_big:
                rec.exact(st, "kbz == 0 on the big cone (CORR_BIG=0)", np.all(D["kbz"][sl] == 0.0))
                continue
            lm = mpv(D["lam"][sl])
            atm = mp.mpf(at)
            um = [x + atm * y for x, y in zip(lm, W.inv(mpv(D["ds"][sl])))]
            wm = [x + atm * y for x, y in zip(lm, W.mul(mpv(D["dz"][sl])))]
            vm = jprod(um, wm)
            nv = mnorm(vm[1:])
            mutm = mp.mpf(float(sig)) * mp.mpf(float(sc_in["mu"]))
            lom, him = mp.mpf(O.CORR_BMIN) * mutm, mp.mpf(O.CORR_BMAX) * mutm
            Ue = np.abs(D["lam"][sl]) + at * W.abs_inv(np.abs(D["ds"][sl]))
            We = np.abs(D["lam"][sl]) + at * W.abs_mul(np.abs(D["dz"][sl]))
            Ve = jprod_abs(Ue, We)
            T0 = Ve[0] + float(np.linalg.norm(Ve[1:]))
            ds_, br = [], []
            for e in (vm[0] + nv, vm[0] - nv):
                ds_.append(max(min(max(e, lom), him) - e, -him))
                br.append(0 if e < lom else 1 if e <= him else 2 if e <= 2 * him else 3)
                # (an eigenvalue v0 - ||v1|| of a nearly active cone is small against its envelope T0: the margin is relative to the
                #  eigenvalue and the box edge, and must ALSO be a hundred times the rounding error K u T0 of the eigenvalue)
                Kb = 6 * kd(m) + 60
                for t in (lom, him, 2 * him):
                    dist = float(abs(e - t))
                    mg = facts["margins"]
                    mg["corr_big_box"] = min(mg.get("corr_big_box", np.inf), dist / max(float(abs(e)), float(t), 1e-300))
                    mg["corr_big_box_100_bounds"] = min(mg.get("corr_big_box_100_bounds", np.inf), MARGIN * dist / max(100 * Kb * U * T0, 1e-300))
            facts["decisions"]["corr_big_branches"] = br
            tm = [(ds_[0] + ds_[1]) / 2] + [(ds_[0] - ds_[1]) / 2 / (nv if nv > 0 else 1) * x for x in vm[1:]]
            ref = [-x for x in W.mul(arw_solve(lm, tm))]
            if br == [1, 1]:
                rec.exact(st, "kbz == 0 on the big cone inside the box", np.all(D["kbz"][sl] == 0.0))
            Te = np.concatenate([[T0], T0 * (np.abs(tof(vm[1:])) + Ve[1:]) / float(nv)])
            env, _ = div_env(D["lam"][sl], Te, m)
            rec.add(st, "kbz_big", merr(D["kbz"][sl], ref), U * (6 * kd(m) + 60 + 3 * rcond(D["lam"][sl], m)) * W.abs_mul(env))
        # ---- corrector tail --------------------------------------------------------------------------------------------------
        st = "corrector"
        rec.exact(st, "xc + kx bit-exact", np.array_equal(D["kxsum"][:N], I["xc"][:N] + I["kx"][:N]))
        rec.exact(st, "zc + kz bit-exact", np.array_equal(D["kzsum"], I["zc"] + I["kz"]))
        rec.exact(st, "gc + kg bit-exact", np.array_equal(D["kgsum"], I["gc"] + I["kg"]))
        K3 = check_dir(P, I, Ws, D, rec, st, 3, D["kxsum"], D["kzsum"], D["kgsum"], E["dtau_c"], E["dkap_c"], sig, D["kds"], D["kdz"], scal)
        T3 = step_ref(P, Ws, D, D["kds"], D["kdz"], False, E["dtau_c"], E["dkap_c"], sc_in["tau"], sc_in["kappa"])
        facts["corrector"] = T3
        facts["margins"].update({"corrector_" + k: v for k, v in margin_step(T3, STEP).items()})
        rec.add(st, "tmax_c", abs(E["tmax"] - T3["t"]), T3["bound"])
        rec.exact(st, "alpha_c==1 at a zero bound", (E["tmax"] == 0.0) == (T3["t"] == 0.0))
        ac = alpha_of(E["tmax"], STEP)                       # (the device's own S_TMAX handed over: alpha_c is not stored unless picked)
        tolk = max(O.REFTOL * sc_in["nrmc"], O.CORR_ETA * sc_in["dres"] * sc_in["tau"] * sc_in["nrmc"])
        ac_ref = alpha_of(T3["t"], STEP)
        by_step, by_guard = ac_ref >= O.CORR_ACCEPT * a0, sc_in["rnc"] <= tolk
        pick = by_step and by_guard
        facts["decisions"].update(pick=pick, pick_by_step=by_step, pick_by_guard=by_guard)
        facts["margins"]["pick_step"] = abs(ac_ref - O.CORR_ACCEPT * a0) / max(ac_ref, O.CORR_ACCEPT * a0)
        facts["margins"]["pick_guard"] = abs(sc_in["rnc"] - tolk) / max(sc_in["rnc"], tolk)
        rec.exact(st, "S_PICK", E["pick"] == (1.0 if pick else 0.0))
        rec.exact(st, "S_NCORR, S_NPICK", E["ncorr"] == 1.0 and E["npick"] == (1.0 if pick else 0.0))
        a_fin = ac if pick else a0
        dt_fin, dk_fin = (E["dtau_c"], E["dkap_c"]) if pick else (Cc["dtau"], Cc["dkap"])
        rec.add(st, "alpha", abs(E["alpha"] - a_fin), 2 * U * a_fin)
        rec.exact(st, "S_DTAU, S_DKAP are the picked direction's", E["dtau"] == dt_fin and E["dkap"] == dk_fin)
        x2, dsv, dzv = (D["kxsum"], D["kds"], D["kdz"]) if pick else (I["xc"], D["ds"], D["dz"])
        moved("update", E["alpha"], dt_fin, dk_fin, x2, dsv, dzv)
        beyond("update", T3 if pick else T1, E["alpha"], dsv, dzv, dt_fin, dk_fin)
        # ... and not along the other direction (where the two differ by more than the bounds)
        ox, ods, odz = (I["xc"], D["ds"], D["dz"]) if pick else (D["kxsum"], D["kds"], D["kdz"])
        far = np.abs(E["alpha"] * (ods - dsv)) > 1e3 * U * (np.abs(I["s"]) + np.abs(dsv) + np.abs(ods))
        moved_s = D["s"] - I["s"]
        rec.exact("update", "s moved along the picked direction, not the other",
                  np.all(np.abs(moved_s[far] - E["alpha"] * dsv[far]) < np.abs(moved_s[far] - E["alpha"] * ods[far])))
        facts["decisions"]["directions_differ"] = bool(far.any())
    # ---- first-order bound of the END STATE against the chain without hand-over (end_to_end) ------------------------------------------
    tau_, kap_, mu_, rt_ = sc_in["tau"], sc_in["kappa"], sc_in["mu"], sc_in["rt"]
    ta = T["t"]
    d_aa = T["bound"] / ta ** 2 + 2 * U if ta > 1.0 else 0.0
    d_sig = 0.0 if capped else 3 * (1 - A["alpha_a"]) ** 2 * d_aa + 5 * U * abs(sig)
    d_dta = Ka["bdt"]
    d_dka = (kap_ * d_dta + 4 * U * (Ka["dkc_env"] + kap_ * abs(A["dtau_a"]))) / tau_
    d_dkc = mu_ * d_sig + abs(A["dkap_a"]) * d_dta + abs(A["dtau_a"]) * d_dka

    def e2e_dir(Kj, Tj, dtau_j, dkap_j, alpha_j):
        d_dt = Kj["bdt"] + (d_dkc / tau_ + abs(rt_) * d_sig) / Kj["den"]
        d_dk = (d_dkc + kap_ * d_dt + 4 * U * (Kj["dkc_env"] + kap_ * abs(dtau_j))) / tau_
        d_ds = 6 * U * Kj["ds_env"] + d_sig * np.abs(I["rz"]) + d_dt * (np.abs(I["g1"]) + np.abs(P["h"]))
        d_dz = 3 * U * Kj["dz_env"] + d_dt * np.abs(I["z1"])
        sens = [d_dt / tau_, d_dk / kap_]
        if l:
            sens.append(float(np.max((d_ds[:l] / D["wl"][:l] + d_dz[:l] * D["wl"][:l]) / D["lam"][:l])))
        for (r0, m, kind, c), W in zip(socs(P), Ws):
            sl = slice(r0, r0 + m)
            sens.append(2 * max(soc_t_bound(D["lam"][sl], W.abs_inv(d_ds[sl]), m), soc_t_bound(D["lam"][sl], W.abs_mul(d_dz[sl]), m))
                        / (U * (2 * rcond(D["lam"][sl], m) + 2 * kd(m) + 12)))
        d_t = Tj["bound"] + max(sens)
        d_al = alpha_j * (d_t / Tj["t"] + 2 * U) if (Tj["t"] > STEP) else 0.0
        return d_dt, d_dk, d_ds, d_dz, d_al

    def e2e_bounds(Kj, Tj, alpha, dtau_j, dkap_j, x2, dsv, dzv):
        d_dt, d_dk, d_ds, d_dz, d_al = e2e_dir(Kj, Tj, dtau_j, dkap_j, alpha)
        dx = np.abs(x2[:N]) + abs(dtau_j) * np.abs(I["x1"][:N])
        return {"x_x": 4 * U * (np.abs(I["x"][:N]) + alpha * dx) + d_al * dx + alpha * d_dt * np.abs(I["x1"][:N]),
                "s": 3 * U * (np.abs(I["s"]) + alpha * np.abs(dsv)) + d_al * np.abs(dsv) + alpha * d_ds,
                "z": 3 * U * (np.abs(I["z"]) + alpha * np.abs(dzv)) + d_al * np.abs(dzv) + alpha * d_dz,
                "tau": 3 * U * (tau_ + alpha * abs(dtau_j)) + d_al * abs(dtau_j) + alpha * d_dt,
                "kappa": 3 * U * (kap_ + alpha * abs(dkap_j)) + d_al * abs(dkap_j) + alpha * d_dk}
    if not corrector:
        facts["e2e_bound"] = e2e_bounds(K1, T1, E["alpha"], Cc["dtau"], Cc["dkap"], I["xc"], D["ds"], D["dz"])
    elif pick:
        facts["e2e_bound"] = e2e_bounds(K3, T3, E["alpha"], E["dtau_c"], E["dkap_c"], D["kxsum"], D["kds"], D["kdz"])
    else:
        facts["e2e_bound"] = e2e_bounds(K1, T1, E["alpha"], Cc["dtau"], Cc["dkap"], I["xc"], D["ds"], D["dz"])
    # ---- cone shift ---------------------------------------------------------------------------------------------------------------
    st = "shift"
    v = I["shift"]
    H = S["shift"]
    dist, bd = [-np.inf], [0.0]
    if l:
        dist.append(float(np.max(-v[:l])))
    heads = list(range(l))
    for (r0, m, kind, c) in socs(P):
        vm = mpv(v[r0:r0 + m])
        dist.append(float(mnorm(vm[1:]) - vm[0]))
        bd.append(U * (kd(m) / 2 + 2) * (float(np.linalg.norm(v[r0 + 1:r0 + m])) + abs(v[r0])))
        heads.append(r0)
    t_ref, n2 = max(dist), float(lsum(ld(v) ** 2))
    rec.add(st, "rb0", abs(H["rb0"] - t_ref), max(bd))
    rec.add(st, "rb1", abs(H["rb1"] - n2), U * (k_rows(P) + kd(max(P["big"], 1))) * n2)
    thr = -1e-8 * max(1.0, np.sqrt(n2))
    shifted = t_ref >= thr
    facts["decisions"]["shifted"] = bool(shifted)
    facts["margins"]["shift"] = abs(t_ref - thr) / max(abs(t_ref), abs(thr))
    facts["shift_t"] = t_ref
    ref = v.copy()
    other = np.ones(len(v), dtype=bool)
    if shifted:
        other[heads] = False
        want = ld(v[heads]) + (LD(1) + LD(H["rb0"]))
        rec.add(st, "shifted", np.abs(ld(D["shift"][heads]) - want), 3 * U * (np.abs(v[heads]) + 1 + abs(H["rb0"])))
    rec.exact(st, "untouched entries bit-exact", np.array_equal(D["shift"][other], ref[other]))
    return rec, facts


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
E2E_FACTOR = 2.0


def end_to_end(P, I, corrector):
    """The end state (x, s, z, tau, kappa) from the INPUTS alone, every stage in the reference's arithmetic (no device value is handed
    over): the textbook scaling, the scalar equations, the directions, the step bounds by their definition, the pick.  The bound of
    the end state (check_lane: facts["e2e_bound"]) carries the stage bounds forward to first order: the error of alpha_a
    (bound(S_TMAX) / t^2) into sigma (3 (1 - alpha_a)^2), sigma's and the affine dtau's, dkappa's into the combined right-hand side
    of the scalar equation, that and the stage's own bound into dtau, dtau and sigma into ds and dz, their change through
    |W^-1|, |W| and the step envelope (Lipschitz 2) into S_TMAX, into alpha = STEP / t, and all of it into x, s, z, tau, kappa;
    E2E_FACTOR = 2 covers the second-order terms."""
    l, N = P["l"], P["N"]
    tau, kap, mu, rt, sigmax, dres, nrmc, rnc = [M(v) for v in I["sc"]]
    s, z = ld(I["s"]), ld(I["z"])
    wl, laml = np.sqrt(s[:l] / z[:l]), np.sqrt(s[:l] * z[:l])
    Ws, lams = [], []
    for (r0, m, kind, c) in socs(P):
        eta, w, *_ = nt_ref(mpv(I["s"][r0:r0 + m]), mpv(I["z"][r0:r0 + m]))
        W = Soc(1.0, np.ones(m))
        W.eta, W.w, W.ef, W.wa = eta, w, float(eta), np.abs(tof(w))
        Ws.append(W)
        lams.append(W.mul(mpv(I["z"][r0:r0 + m])))
    sc = dict(tau=tau, kappa=kap, mu=mu, rt=rt, wl_dev=wl)
    h = P["h"]

    def direction(mode, x2, z2, g2, sigma):
        dt, _, dkc, _ = dtau_ref(P, I, Ws, sc, x2, z2, mode)
        dk = (dkc - kap * dt) / tau
        oms, dtl = m2ld(1 - sigma), m2ld(dt)
        ds = -oms * ld(I["rz"]) - ld(g2) - dtl * (ld(I["g1"]) - ld(h))
        dz = ld(z2) + dtl * ld(I["z1"])
        ts = [mp.mpf(0), -dt / tau, -dk / kap]
        if l:
            ts.append(M(np.max(np.maximum(-(ds[:l] / wl) / laml, -(dz[:l] * wl) / laml))))
        dsm, dzm = [], []
        for (r0, m, kind, c), W, lm in zip(socs(P), Ws, lams):
            sl = slice(r0, r0 + m)
            a = [-(1 - sigma) * r - g - dt * (g1 - hh) for r, g, g1, hh in zip(mpv(I["rz"][sl]), mpv(g2[sl]), mpv(I["g1"][sl]), mpv(h[sl]))]
            b = [p + dt * q for p, q in zip(mpv(z2[sl]), mpv(I["z1"][sl]))]
            dsm.append(a), dzm.append(b)
            ts += [soc_t(lm, W.inv(a)), soc_t(lm, W.mul(b))]
        for (r0, m, kind, c), a, b in zip(socs(P), dsm, dzm):
            ds[r0:r0 + m], dz[r0:r0 + m] = [m2ld(v) for v in a], [m2ld(v) for v in b]
        return dt, dk, ds, dz, max(ts)
    dta, dka, _, _, ta = direction(0, I["x2"], I["z2"], I["g2"], mp.mpf(0))
    aa = mp.mpf(1) if ta == 0 else min(mp.mpf(1), 1 / ta)
    sigma = min((1 - aa) ** 3, sigmax)
    sc.update(sigma=sigma, dtau_a=dta, dkap_a=dka)
    dt, dk, ds, dz, t1 = direction(1, I["xc"], I["zc"], I["gc"], sigma)
    step = lambda t: mp.mpf(1) if t == 0 else min(mp.mpf(1), mp.mpf(STEP) / t)
    alpha, x2 = step(t1), ld(I["xc"][:N])
    if corrector:
        x2k = ld(I["xc"][:N]) + ld(I["kx"][:N])
        dtc, dkc_, dsk, dzk, t3 = direction(3, I["xc"][:N] + I["kx"][:N], I["zc"] + I["kz"], I["gc"] + I["kg"], sigma)
        tolk = max(M(O.REFTOL) * nrmc, M(O.CORR_ETA) * dres * tau * nrmc)
        if step(t3) >= M(O.CORR_ACCEPT) * alpha and rnc <= tolk:
            alpha, dt, dk, ds, dz, x2 = step(t3), dtc, dkc_, dsk, dzk, x2k
    al = m2ld(alpha)
    return dict(x_x=ld(I["x"][:N]) + al * (x2 + m2ld(dt) * ld(I["x1"][:N])), s=s + al * ds, z=z + al * dz,
                tau=m2ld(tau + alpha * dt), kappa=m2ld(kap + alpha * dk))


def check_end_to_end(P, I, D, corrector, rec, facts, ref=None):
    """the end state against the chain without hand-over, within E2E_FACTOR = 2 times the first-order bound check_lane forms."""
    ref = ref or end_to_end(P, I, corrector)
    B = facts["e2e_bound"]
    for k in ("x_x", "s", "z"):
        rec.add("end_to_end", k, np.abs(ld(D[k]) - ref[k]).astype(np.float64), E2E_FACTOR * B[k])
    for k in ("tau", "kappa"):
        rec.add("end_to_end", k, float(abs(LD(D["sc"]["update"][k]) - ref[k])), E2E_FACTOR * B[k])
    return ref


# ---- the float64 twin: the formulas of oracle/conic_ipm.py --------------------------------------------------------------------------
def twin(P, I, corrector, corr_big=True):
    """Every output of the hook by the float64 NumPy functions of oracle/conic_ipm.py, in the layout of `unpack`."""
    l, N, R = P["l"], P["N"], P["R"]
    cone = O._Cone(P["l"], P["nq3"], P["big"])
    tau, kap, mu, rt, sigmax, dres, nrmc, rnc = I["sc"]
    h, c = P["h"], P["c"][:N]
    s, z, rz = I["s"], I["z"], I["rz"]
    Wm = O._Scaling(cone, s, z)
    lam = Wm.apply(z)
    D = dict(lam=lam, dl=np.zeros(R), wl=np.ones(R))
    D["dl"][:l], D["wl"][:l] = Wm.dl, Wm.wl
    wb = Wm.inv2(np.stack([I["bz2a"], I["bz2b"]], 1))
    D["wbz2a"], D["wbz2b"] = wb[:, 0], wb[:, 1]
    D["w3"] = np.concatenate([Wm.eta3[:, None], Wm.wb3], 1) if P["nq3"] else np.zeros((1, 4))
    D["wbb"] = Wm.wbb if P["big"] else np.zeros(1)
    snap = dict(etab=Wm.etab if P["big"] else 0.0)
    wz1 = Wm.apply(I["z1"])
    den = kap / tau + wz1 @ wz1

    def direction(sigma, dkc, x2, z2, g2):
        dtau = (dkc / tau + (1 - sigma) * rt + c @ x2[:N] + h @ z2) / den
        dz = z2 + dtau * I["z1"]
        ds = -(1 - sigma) * rz - g2 - dtau * (I["g1"] - h)
        return ds, dz, dtau, (dkc - kap * dtau) / tau, Wm.apply(ds, inverse=True), Wm.apply(dz)

    def tmax(dss, wdz, dtau, dkap):
        return max(0.0, O._max_step(cone, lam, dss), O._max_step(cone, lam, wdz), -dtau / tau, -dkap / kap)
    _, _, dta, dka, dssa, wdza = direction(0.0, -kap * tau, I["x2"], I["z2"], I["g2"])
    ta = tmax(dssa, wdza, dta, dka)
    aa = alpha_of(ta, 1.0)
    sigma = min((1 - aa) ** 3, sigmax)
    D.update(dssa=dssa, wdza=wdza, bxc=-(1 - sigma) * I["rx"][:N])
    dsc = sigma * mu * cone.e() - O._cone_prod(cone, lam, lam) - O._cone_prod(cone, dssa, wdza)
    D["lds"] = O._cone_div(cone, lam, dsc)
    D["bzc"] = -(1 - sigma) * rz - Wm.apply(D["lds"])
    D["wbzc"] = Wm.inv2(D["bzc"])
    dkc = sigma * mu - kap * tau - dka * dta
    ds, dz, dt, dk, dss, wdz = direction(sigma, dkc, I["xc"], I["zc"], I["gc"])
    D.update(ds=ds, dz=dz)
    t1 = tmax(dss, wdz, dt, dk)
    a1 = alpha_of(t1, STEP)
    A = dict(snap, dtau_a=dta, dkap_a=dka, tmax=ta, alpha_a=aa, sigma=sigma)
    Cc = dict(A, dtau=dt, dkap=dk)
    sc = dict(scaling=snap, comb_rhs=A, comb=Cc)
    x2 = I["xc"]
    if not corrector:
        alpha, E = a1, dict(Cc, tmax=t1, alpha=a1)
    else:
        sc["corr_rhs"] = dict(Cc, tmax=t1, alpha0=a1)
        at, mut = min(1.0, a1 + O.CORR_DELTA), sigma * mu
        v = (lam[:l] + at * dss[:l]) * (lam[:l] + at * wdz[:l])
        tt = np.maximum(np.minimum(np.maximum(v, O.CORR_BMIN * mut), O.CORR_BMAX * mut) - v, -O.CORR_BMAX * mut)
        kbz = np.zeros(R)
        kbz[:l] = -Wm.wl * (tt / lam[:l])
        if P["big"] and corr_big:
            ub, wbv = (lam + at * dss)[cone.ob:], (lam + at * wdz)[cone.ob:]
            tc = np.zeros(R)
            tc[cone.ob:] = O._soc_target(O._soc_prod(ub[None, :], wbv[None, :]), mut)[0]
            kbz[cone.ob:] = -Wm.apply(O._cone_div(cone, lam, tc))[cone.ob:]
        D["kbz"] = kbz
        D["wbzk"] = Wm.inv2(kbz)
        D["kxsum"], D["kzsum"], D["kgsum"] = I["xc"][:N] + I["kx"][:N], I["zc"] + I["kz"], I["gc"] + I["kg"]
        kds, kdz, dtc, dkc_, kdss, kwdz = direction(sigma, dkc, D["kxsum"], D["kzsum"], D["kgsum"])
        D.update(kds=kds, kdz=kdz)
        t3 = tmax(kdss, kwdz, dtc, dkc_)
        a3 = alpha_of(t3, STEP)
        tolk = max(O.REFTOL * nrmc, O.CORR_ETA * dres * tau * nrmc)
        pick = a3 >= O.CORR_ACCEPT * a1 and rnc <= tolk
        alpha = a3 if pick else a1
        if pick:
            dt, dk, x2, ds, dz = dtc, dkc_, D["kxsum"], kds, kdz
        E = dict(Cc, tmax=t3, alpha0=a1, alpha=alpha, dtau_c=dtc, dkap_c=dkc_, pick=float(pick), ncorr=1.0, npick=float(pick), dtau=dt, dkap=dk)
    E.update(tau=tau + alpha * dt, kappa=kap + alpha * dk)
    D["x_x"] = I["x"][:N] + alpha * (x2[:N] + dt * I["x1"][:N])
    D["s"], D["z"] = s + alpha * ds, z + alpha * dz
    sc["update"] = E
    v = I["shift"].copy()
    t, n2 = cone.min_residual(v), float(v @ v)
    if t >= -1e-8 * max(1.0, np.sqrt(n2)):
        v = v + (1 + t) * cone.e()
    D["shift"] = v
    sc["shift"] = dict(E, rb0=t, rb1=n2)
    D["sc"] = sc
    return D


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
IN_R = ("s", "z", "rz", "bz2a", "bz2b", "z1", "z2", "g1", "g2", "zc", "gc", "kz", "kg", "shift")
IN_X = ("x", "rx", "x1", "x2", "xc", "kx")


def late_sz(P, rng, gap_rel=1e-6, comp=1e-8):
    """A late-iteration pair: complementary and near the boundary.  Orthant: s z = comp with s over six decades; cones:
    s = a (1 + gap, u), z = b (1 + gap, -u), |u| = 1, so that both have the relative boundary gap `gap_rel` and s'z ~ comp."""
    R, l = P["R"], P["l"]
    s, z = np.ones(R), np.ones(R)
    e = 10.0 ** rng.uniform(-7, -1, l)
    s[:l], z[:l] = e, comp * rng.uniform(0.5, 2, l) / e
    for (r0, m, kind, c) in socs(P):
        u = rng.standard_normal(m - 1)
        u /= np.linalg.norm(u)
        a = 10.0 ** rng.uniform(-3, 0)
        b = comp / (2 * gap_rel * a) * rng.uniform(0.5, 2)        # s'z = a b ((1 + g)^2 - 1) ~ 2 g a b
        s[r0], s[r0 + 1:r0 + m] = a * (1 + gap_rel), a * u
        z[r0], z[r0 + 1:r0 + m] = b * (1 + gap_rel), -b * u
    return s, z


def draw_inputs(P, s, z, rng, bind=("orth", "orth", "orth"), pick="step", scale=0.2, T=3.0, shift="outside"):
    """Inputs of one lane at the iterate (s, z).  The "solutions" are drawn in the scaled space -- every cone's terms of the step
    bound stay below `scale` + 0.25 -- and mapped back with the float64 scaling; then the term named in bind = (affine, combined,
    corrector) is made the binding one with 1/alpha ~ T: 'orth' (a row of the last cone block), 'q3', 'big', 'tau', 'kappa', or
    'none' (no term positive; not reachable for the affine direction, whose -dkappa/kappa = 1 + dtau/tau).  pick: 'step' (the
    corrected direction's step decides), 'guard' (S_RNC above its tolerance), 'short' (the corrected step is not long enough)."""
    l, N, R = P["l"], P["N"], P["R"]
    cone = O._Cone(P["l"], P["nq3"], P["big"])
    Wm = O._Scaling(cone, s, z)
    lam = Wm.apply(z)
    h, c = P["h"], P["c"][:N]
    I = dict(s=s.copy(), z=z.copy())
    tau, kap = 0.9, 0.7
    mu = float(s @ z + tau * kap) / (cone.degree + 1)
    hs = max(float(np.abs(h).max()), 1e-300)

    def scaled(k):
        """a scaled-space vector whose step terms are at most k: rho lam + noise of k/2 of each cone's smallest eigenvalue"""
        d = lam * rng.uniform(-k / 2, k / 2, R)
        for (r0, m, kind, cc) in socs(P):
            lm = lam[r0:r0 + m]
            nl = np.linalg.norm(lm[1:])
            d[r0:r0 + m] = lm * rng.uniform(-k / 2, k / 2) + (lm[0] - nl) * k / 2 * rng.standard_normal(m) / np.sqrt(m)
        return d
    # z1, g1 - h: small, so that dtau (free through S_RT and c'x) moves (tau, kappa) without moving the cones much
    I["z1"] = Wm.apply(scaled(0.05), inverse=True)
    I["g1"] = h + Wm.apply(scaled(0.05))
    I["rz"] = Wm.apply(scaled(0.05))
    I["bz2a"], I["bz2b"] = rng.standard_normal(R) * np.abs(s), rng.standard_normal(R) * np.abs(s)
    I["x"], I["rx"], I["x1"] = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(N)
    wz1 = Wm.apply(I["z1"])
    den = kap / tau + wz1 @ wz1
    rt = 0.3
    sigmax = O.SIGMA_MAX

    def make(sig_oms, dkc, want):
        """one direction's (x2, z2, g2): scaled targets D_s, D_z with the binder set, dtau placed through c'x2"""
        Ds, Dz = scaled(scale), scaled(scale)
        # (-dtau/tau) + (-dkappa/kappa) = -dkc / (tau kappa) whatever dtau is (1 for the affine direction): split it evenly
        dtau = {"tau": -T * tau, "kappa": None}.get(want, 0.5 * dkc / kap)
        if want == "kappa":
            dtau = (dkc + T * kap * tau) / kap                  # -dkappa/kappa = -(dkc - kappa dtau)/(tau kappa) = T
        if want == "none":
            dtau = rng.uniform(0.1, 0.3) * tau
            Ds, Dz = lam * rng.uniform(0.05, scale, R), lam * rng.uniform(0.05, scale, R)
            for (r0, m, kind, cc) in socs(P):
                Ds[r0:r0 + m], Dz[r0:r0 + m] = lam[r0:r0 + m] * rng.uniform(0.05, scale), lam[r0:r0 + m] * rng.uniform(0.05, scale)
        if want == "orth":
            r = l - 1 - int(rng.integers(0, min(l, 40)))
            Dz[r] = -T * lam[r]
        if want in ("q3", "big"):
            r0, m = [(a, b) for (a, b, kind, cc) in socs(P) if kind == want][-1 if want == "big" else P["nq3"] // 2][:2]
            Ds[r0:r0 + m] = -T * lam[r0:r0 + m]
        ds, dz = Wm.apply(Ds), Wm.apply(Dz, inverse=True)
        z2 = dz - dtau * I["z1"]
        g2 = -sig_oms * I["rz"] - ds - dtau * (I["g1"] - h)
        x2 = rng.standard_normal(N)
        need = dtau * den - (dkc / tau + sig_oms * rt + h @ z2)      # = c'x2
        x2 += (need - c @ x2) * c / (c @ c)
        return x2, z2, g2, dtau, (dkc - kap * dtau) / tau, Ds, Dz
    # affine
    x2, z2, g2, dta, dka, Dsa, Dza = make(1.0, -kap * tau, bind[0])
    I.update(x2=x2, z2=z2, g2=g2)
    ta = max(0.0, O._max_step(cone, lam, Dsa), O._max_step(cone, lam, Dza), -dta / tau, -dka / kap)
    aa = alpha_of(ta, 1.0)
    sigma = min((1 - aa) ** 3, sigmax)
    if bind[1] == "none" or bind[2] == "none":
        mu = max(mu, 10 * (kap * tau + abs(dka * dta) + kap * tau) / max(sigma, 1e-3))
    dkc = sigma * mu - kap * tau - dka * dta
    xc, zc, gc, dt, dk, Ds, Dz = make(1 - sigma, dkc, bind[1])
    I.update(xc=xc, zc=zc, gc=gc)
    # corrector solution: the candidate is (xc + kx, ...): draw the candidate, subtract
    T_keep = T
    if pick != "short" and bind[2] != "none" and T > 1.0:
        T = T / 2.0            # a step twice as long ('short': as tight as the uncorrected direction's, alpha_c < 1.01 alpha_0)
    xk, zk, gk, _, _, _, _ = make(1 - sigma, dkc, bind[2])
    T = T_keep
    I.update(kx=xk - xc, kz=zk - zc, kg=gk - gc)
    nrmc = float(np.linalg.norm(c))
    dres = 1e-3
    tolk = max(O.REFTOL * nrmc, O.CORR_ETA * dres * tau * nrmc)
    I["sc"] = np.array([tau, kap, mu, rt, sigmax, dres, nrmc, tolk * (10.0 if pick == "guard" else 0.1)])
    # the vector of the cone shift
    v = rng.standard_normal(R)
    for (r0, m, kind, cc) in socs(P):
        v[r0] = np.linalg.norm(v[r0 + 1:r0 + m]) + {"outside": -0.5, "interior": 0.5, "barely": 0.5}[shift]
    if shift != "outside":
        v[:l] = np.abs(v[:l]) + 0.5
    if shift == "barely":                                      # inside by less than 1e-8 max(1, ||v||): one cone 0.3e-8 ||v|| from its boundary
        nv = max(1.0, float(np.linalg.norm(v)))
        if P["nq3"] or P["big"]:
            r0, m = socs(P)[len(socs(P)) // 2][:2]
            v[r0] = float(mnorm(mpv(v[r0 + 1:r0 + m]))) + 0.3e-8 * nv
        else:
            v[l // 2] = 0.3e-8 * nv
    I["shift"] = v
    return I


def pack(Is, R, N):
    """in_r, in_x, in_sc of mbfir.test_unit_cone from per-lane input dicts (zero-padded to the unit's R, N)."""
    in_r, in_x = np.zeros((len(Is), len(IN_R), R)), np.zeros((len(Is), len(IN_X), N))
    for b, I in enumerate(Is):
        for i, k in enumerate(IN_R):
            in_r[b, i, :len(I[k])] = I[k]
        for i, k in enumerate(IN_X):
            in_x[b, i, :len(I[k])] = I[k]
    return in_r, in_x, np.stack([I["sc"] for I in Is])


# ---- the designs and runs of the device tests (the CPU tests check what the device tests rely on) ---------------------------------------
def designs():
    """name -> dict(job, grid_m, ddkkt, dims): the smallest designs that have each edge (dims = (l, nq3, big) as mbfir_assemble gives
    them, asserted by the CPU test).  No designer yields all three cone kinds at once."""
    from conftest import CASES
    U_ = L.unit_cases()
    qphs = CASES["qphs21"][1]
    out = {k: dict(job=U_[k]["job"], grid_m=U_[k]["grid_m"], ddkkt=U_[k].get("ddkkt", 0)) for k in ("c8_dup12", "c3_lin64", "c6_qp25", "c4_qphs21")}
    out["c8_dup12"]["dims"], out["c3_lin64"]["dims"] = (900, 11, 0), (1928, 0, 0)
    out["c6_qp25"]["dims"], out["c4_qphs21"]["dims"] = (0, 281, 51), (12772, 0, 43)
    # the big cone longer than its 1024-thread workgroup: the second pass of every strided loop, big_dot's tails
    out["n600"] = dict(job=("fir_qprog_phs", (600,) + tuple(qphs[1:])), grid_m=700, ddkkt=0, dims=(14168, 0, 1201))
    return out


# (design, iterate, (affine, combined, corrector) binder, pick, T, shift vector, corrector runs)
RUNS = (
    ("c8_dup12", "centred", ("orth", "q3", "tau"), "step", 3.0, "outside", True),
    ("c8_dup12", "wide", ("q3", "tau", "orth"), "guard", 1.5, "interior", True),
    ("c8_dup12", "late", ("tau", "orth", "q3"), "short", 3.0, "barely", True),
    ("c8_dup12", "centred", ("kappa", "none", "none"), "step", 3.0, "interior", True),
    ("c8_dup12", "late", ("orth", "kappa", "kappa"), "step", 1.5, "outside", True),
    ("c8_dup12", "wide", ("q3", "none", "none"), "step", 3.0, "barely", False),
    ("c8_dup12", "centred", ("orth", "q3", "orth"), "step", 0.95, "outside", True),       # every bound below 1: alpha_a = 1, sigma = 0
    ("c3_lin64", "centred", ("orth", "tau", "kappa"), "step", 3.0, "outside", True),
    ("c3_lin64", "late", ("kappa", "orth", "none"), "guard", 1.5, "barely", True),
    ("c3_lin64", "wide", ("tau", "kappa", "orth"), "step", 3.0, "interior", False),
    ("c6_qp25", "centred", ("q3", "big", "none"), "step", 3.0, "outside", False),
    ("c6_qp25", "late", ("big", "q3", "none"), "step", 1.5, "barely", False),
    ("c6_qp25", "wide", ("tau", "kappa", "none"), "step", 3.0, "interior", False),
    ("c6_qp25", "late", ("kappa", "none", "none"), "step", 3.0, "outside", False),
    ("c4_qphs21", "centred", ("big", "orth", "big"), "step", 3.0, "outside", True),
    ("c4_qphs21", "late", ("orth", "big", "tau"), "short", 1.5, "barely", True),
    ("c4_qphs21", "wide", ("tau", "kappa", "none"), "guard", 3.0, "interior", True),
    ("n600", "centred", ("big", "orth", "big"), "step", 3.0, "outside", True),
    ("n600", "late", ("orth", "big", "tau"), "step", 1.5, "barely", True),
    ("n600", "wide", ("tau", "none", "none"), "step", 3.0, "interior", False),
)
_PROGRAMS = {}


def program_of(name):
    if name not in _PROGRAMS:
        d = designs()[name]
        _PROGRAMS[name] = L.program(*d["job"], grid_m=d["grid_m"])
    return _PROGRAMS[name]


def run_id(run):
    return "%s-%s-%s-%s-%s%s" % (run[0], run[1], "_".join(run[2]), run[3], run[5], "" if run[6] else "-nocorr")


def iterate(P, kind, rng):
    if kind == "late":
        return late_sz(P, rng)
    return L.draw_sz(P, rng, kind == "wide")


def run_inputs(run, seed=0):
    """the inputs of one run (deterministic: the CPU and the device tests draw the same)."""
    import zlib
    P = program_of(run[0])
    rng = np.random.default_rng(zlib.crc32(run_id(run).encode()) + seed)
    s, z = iterate(P, run[1], rng)
    return P, draw_inputs(P, s, z, rng, bind=run[2], pick=run[3], T=run[4], shift=run[5])


def make_opts_of(name, **kw):
    import mbfir
    d = designs()[name]
    return mbfir.make_opts(grid_m=d["grid_m"], ddkkt=d["ddkkt"], **kw) if d["ddkkt"] else mbfir.make_opts(grid_m=d["grid_m"], **kw)


def untouched(P, D, corrector, form):
    """names of the output blocks that do not hold the caller's sentinel (NaN) where no kernel writes: rows past the ones a stage owns,
    and every block of a stage that did not run."""
    l, R, N, o3 = P["l"], P["R"], P["N"], P["l"] + 3 * P["nq3"]
    import mbfir
    rows = {k: D["raw_r"][i] for i, k in enumerate(mbfir.UNIT_CONE_OUT_R)}
    bad = []
    for k, lo in (("dl", l), ("wl", l), ("wbz2a", o3), ("wbz2b", o3), ("wbzc", o3), ("wbb", max(P["big"], 1))):
        if not np.all(np.isnan(rows[k][lo:])):
            bad.append(k)
    if corrector:
        if not np.all(np.isnan(rows["wbzk"][o3:])):
            bad.append("wbzk")
    else:
        bad += [k for k in ("kbz", "wbzk", "kzsum", "kgsum", "kds", "kdz") if not np.all(np.isnan(rows[k]))]
        if not np.all(np.isnan(D["raw_x"][1])):
            bad.append("kxsum")
        if not all(np.isnan(v) for v in D["sc"]["corr_rhs"].values()):
            bad.append("snapshot corr_rhs")
    for k in rows:                                          # (the in-place blocks hold the caller's input there, its padding)
        if k not in ("wbb", "kzsum", "kgsum", "s", "z", "shift") and not np.all(np.isnan(rows[k][R:])):
            bad.append(k + " past R")
    return bad
