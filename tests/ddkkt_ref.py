"""The reference of the extended-precision KKT path (csrc/ddkkt.inc with dd_prepare / dd_prepare_lanes, build_H(ddk > 0) and
kkt_solve_dd) for mbfir.test_unit_ddkkt: tests/test_ddkkt_gpu.py holds the device to it stage by stage, tests/test_ddkkt_ref_cpu.py
checks the inputs, the bounds against a float64 twin and that the checker rejects planted errors, without a GPU.

Everything is numpy.longdouble on top of lattice_ref (program, G_ref, G_hat, K_G, K_GT, K_H), cone_ref (Rec, kd, k_rows) and kkt_ref
(k_n, vnorm, the summation orders); mpmath where a double-double quantity is checked; capkkt_ref's stage checks for the capacitance
form's matrices and vectors, unchanged.  Every stage takes the device's earlier outputs as exact, so one wrong kernel fails alone.
u = 2^-53.  A bound is K u times an envelope of the sum the kernel forms; K counts the roundings of the expression in the code and
carries the project's margin of 4; no K comes from a device result.  Decisions (the strong set, the slot maps, sX, dlc, every copy and
every fl(a + b)) must match exactly; what no launch of a lane writes must hold its sentinel.

  eig   lam_p = g e2, lam_m = e2 / g, g = (w0 + n1)^2, n1 = sqrt(w1^2 + w2^2), e2 = 1 / eta^2 from the device's w3: n1 2 roundings
        (the sum, the root; the squares enter at half weight), w0 + n1 one more, the square doubles them and adds one: 7; e2: 2; the
        product or quotient: 1.  K_LAM = 4 x 10 for lam_p and lam_m, 4 x 2 for lam_0; what = w / n1: K_WHAT = 4 x 3; ||what|| = 1
        within 4 x 4 u.  The big cone: its norm is a block-wide dot product, kd(big) of cone_ref: K = 4 (kd + 8), what 4 (kd / 2 + 2).
        n1 = 0 gives what = (1, 0, ...) exactly.
  cap   cap = theta exp(sum log / count): every log within 2 u |log|, the fold of the block partials (a tree of 256, then the
        rows) k_rows(P) of cone_ref, the quotient, exp and the product 3 more: relative 4 u (k_rows sum |log| / count + |mean| + 3).
  set   the set {(kind, index, direction): lam > cap} is the reference's own (longdouble eigenvalues of (s, z), its own cap) exactly;
        slots sorted by (kind, index, direction); slotl / slot3 / slotb the inverse map, -1 elsewhere; sX = fl(lam - cap) and
        dlc = min(d, cap) of the device's own lam and cap, bit for bit; the cap factor theta0 100^(attempts - 1), every earlier
        attempt's set larger than the form takes, the last one fitting.
  m3c   sum_k min(lam_k, cap) e_k e_k' from the device's e3 and cap: soc3_eig_apply spends 10 roundings on a term: K_M3 = 40, the
        envelope sum_k f_k |e_k| |e_k|'.
  U     e'G over the cone's rows, G = G_ref(P, round_arg=True): g_entry is one sincos per entry, lattice_ref's dense trig(X, 0) per
        entry of the amplitude envelope, + 16 for the products and the three-term sum: K_U.  Rows k .. kp-1 and columns N .. np-1
        exact zeros, rows past kp the sentinel.
  H     the kept H against G'W_w^-2 G, W_w^-2 in capped eigen form from the device's eigen data: K_H(P) of lattice_ref + K_M3 +
        4 (kd(big) + 8) on Ghat'|W_w^-2| Ghat.
  r1    G'dz by K_GT; r1 = fl(bx - G'dz) bit for bit; its norm by k_n(N) as kkt_ref's stage 4; the slots of later passes untouched.
  r2    bz - gdx + W^2 dz in eigen form (1 / lam_k): an orthant row 3 roundings (K = 12 on |bz| + |gdx| + |dz / d|), a 3-row cone
        K_M3 + 4 on the eigen envelope + 12 on the sum, the big cone 4 (kd + 8) on its envelope, in which (f_p - f_0) counts as
        |f_p| + |f_0|.  tS: an orthant row's r2 itself; e'r2 within 4 x 6 u |e|'|r2| (the big cone: 4 (kd + 4)).
  wbz   W_w^-2 (in - sub): an orthant row two roundings (K = 8), cones as r2 with f_k = min(lam_k, cap).
  gtw, gbh   G'wbz by K_GT, G Bh by K_G.
  solve capacitance form: capkkt_ref.stage_checks (M, Yt, Zt, S, Ms once; rhs_w, y, w, zeta, dx per pass) on the device's own H, U, sX,
        r1, G'wbz and tS.  Double-double form: k_dd_rhs against r1 + gtw + U'(X t) in mpmath within K_DD(k / 16 + 16) 2^-102 of the
        envelope (a double-double operation errs by at most 4 u^2 = 2^-104 of its operands; three per term; the margin of 4), k_dd_zeta
        against X (U (Bh + Bl) - t) within K_DD(N / 64 + 8) 2^-102 and one rounding; the triangular solves against oracle/ddlin.py's
        cho_solve with the device's own factor and right-hand side at test_kernels_gpu's tolerance 1e-24 max(1, X_max).
  acc   dz += dzw + spread(zeta): two roundings of the device's own operands (K.two_roundings) plus, on a cone, 4 x 6 u of the spread's
        terms; gdx += gd and dx += Bh bit for bit.
  end   with no hand-over: ||bx - G'dz|| and max |bz - G dx + W^2 dz| in longdouble against the float64 twin (oracle/conic_ipm.py's
        kkt_solve_dd restated with explicit factors): the device's may not exceed FACTOR max(twin's, floor), the floor being the
        rounding of evaluating the residual itself (K_GT u ||Ghat'|dz|||, resp. K_G u Ghat |dx| + 12 u of the terms).  The twin's own
        norms under two summation orders and both forms spread by SPREAD_MEASURED (tests/test_ddkkt_ref_cpu.py measures it and asserts
        that FACTOR = 4 x that covers it).

Inputs (strong_iterate): lattice_ref.draw_sz(P, rng, False); on the planned orthant rows z = s, then s /= sqrt F, z *= sqrt F with
F = 10^U(8, 14); on planned cones s = a (1 + g, u), z = b (1 + g, -u), |u| = 1 with (b / a, g) = (1, 1e-9): lam_p = 2e9 alone strong,
(1e8, 1e-3): lam_p = 2e11 and lam_0 = 1e8, (1e12, 1e-2): all three (lam_m = 5e9); then z of every untouched block times one factor that
makes the geometric mean of the typical weights 1, so that cap = theta.  (z = s first: with the draw's z / s in 0.25 .. 4 an orthant
weight F z / s would come within 0.4 decades of a cap.)  A run that raises the cap (x 100) holds rows that drop out at the second cap:
they sit at F = 1e7, one decade from both caps -- no other value is -- and the others in 1e10 .. 1e14.  margins() gives the distance in
decades of every eigenvalue from every cap a run meets; the tests assert >= 1 (to 1e-6: 1e7 against 1e6 is one decade to rounding).
"""
import numpy as np

import capkkt_ref as CK
import cone_ref as CR
import kkt_ref as K
import lattice_ref as L

LD = np.longdouble
U = 2.0 ** -53
THETA = 1e6
DD_KMAX, CAP_KMAX = 3072, 1024
RS2 = 0.70710678118654752440             # RSQRT2 of ddkkt.inc (a double)
K_LAM, K_LAM0, K_WHAT, K_M3 = 40.0, 8.0, 12.0, 40.0
K_PART = 48.0                            # a log (2) and the block's tree of 256 (6 levels in a wave, 4 waves: 10), the margin of 4
EPS_DD = 2.0 ** -102
# (test_ddkkt_ref_cpu.test_twin_spread_sets_the_factor prints the measured value.  It is 1 because every compared value is clamped to its
#  floor first and the floors -- evaluating a residual whose dz is of the order lam - cap -- dominate: the end check is in effect
#  4 x floor, a weak check that catches gross errors only; the stages above are the sharp ones.)
SPREAD_MEASURED = 1.0
FACTOR = 4.0
MODES = {"p": (1.0, 1e-9), "p0": (1e8, 1e-3), "p0m": (1e12, 1e-2)}
DIRS = {"p": (0,), "p0": (0, 1), "p0m": (0, 1, 2)}
# the bounds that count the one or two roundings of a short expression: float64 arithmetic attains them, the twin is held to the bound
# itself there and to a quarter of every other
COUNTED = {("acc", "dz"), ("wbz", "orth"), ("wbz", "second orth"), ("r2", "orth"), ("solve", "zeta")}

ld, f64 = K.ld, K.f64


def k_big(P):
    return 4.0 * (CR.kd(P["big"]) + 8) if P["big"] else 0.0


def k_u(P):
    return L._trig(L.grid_facts(P)["X"], 0) + 16.0


def k_dd(terms):
    return 3.0 * terms + 4.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def strong_iterate(P, seed, plan):
    """(s, z, planned): an interior pair whose strong set at cap = THETA is `planned`, a sorted list of (kind, index, direction).
    plan: dict(kl=orthant rows, drop=rows among them that fall out at the raised cap 100 THETA (a retry run), q3=((mode, count), ...),
    big=mode or None), modes being the keys of MODES."""
    rng = np.random.default_rng(seed)
    s, z = L.draw_sz(P, rng, False)
    l, nq3, big, o3 = P["l"], P["nq3"], P["big"], P["l"] + 3 * P["nq3"]
    kl, drop = plan.get("kl", 0), plan.get("drop", 0)
    planned, touched_rows = [], np.zeros(P["R"], dtype=bool)
    if kl:
        rows = np.sort(rng.choice(l, kl, replace=False))
        F = 10.0 ** (rng.uniform(10, 14, kl) if drop else rng.uniform(8, 14, kl))
        F[rng.choice(kl, drop, replace=False)] = 1e7
        z[rows] = s[rows]
        s[rows], z[rows] = s[rows] / np.sqrt(F), z[rows] * np.sqrt(F)
        touched_rows[rows] = True
        planned += [(0, int(r), 0) for r in rows]

    def cone_pair(m, mode):
        ba, g = MODES[mode]
        u = rng.standard_normal(m - 1)
        u /= np.linalg.norm(u)
        a = rng.uniform(0.5, 2)
        return a * np.concatenate([[1 + g], u]), a * ba * np.concatenate([[1 + g], -u])
    ncone = sum(c for _, c in plan.get("q3", ()))
    if ncone:
        cones = np.sort(rng.choice(nq3, ncone, replace=False))
        modes = [m for m, c in plan["q3"] for _ in range(c)]
        for c, m in zip(cones, [modes[i] for i in rng.permutation(ncone)]):
            r0 = l + 3 * c
            s[r0:r0 + 3], z[r0:r0 + 3] = cone_pair(3, m)
            touched_rows[r0:r0 + 3] = True
            planned += [(1, int(c), d) for d in DIRS[m]]
    if plan.get("big"):
        s[o3:], z[o3:] = cone_pair(big, plan["big"])
        touched_rows[o3:] = True
        planned += [(2, 0, d) for d in DIRS[plan["big"]] if d != 1]     # (lam_0 of the big cone is never capped)
    # one factor on z of every untouched block: the geometric mean of the typical weights becomes 1
    E = ref_eigs(P, s, z)
    typ = E["typ"]
    free = np.concatenate([~touched_rows[:l], ~touched_rows[l:o3:3], ~touched_rows[o3:o3 + 1] if big else np.zeros(0, dtype=bool)])
    assert free.sum() > 0
    c = float(np.exp(-np.log(typ).sum() / free.sum()))
    z[~touched_rows] *= c
    return s, z, sorted(planned)


def ref_eigs(P, s, z):
    """The eigenvalues of W^-2 at (s, z) in longdouble: d (l), q3 (nq3, 3: lam_p, lam_0, lam_m), big (3) and the typical weights."""
    l, nq3, big, o3 = P["l"], P["nq3"], P["big"], P["l"] + 3 * P["nq3"]
    s, z = ld(s), ld(z)

    def lam(eta, wb):
        n1 = np.sqrt((wb[..., 1:] ** 2).sum(-1))
        g, e2 = (wb[..., 0] + n1) ** 2, 1 / eta ** 2
        return np.stack([g * e2, e2, e2 / g], -1)
    out = dict(d=z[:l] / s[:l], q3=np.zeros((0, 3), dtype=LD), big=None)
    if nq3:
        out["q3"] = lam(*L._soc_nt(s[l:o3].reshape(-1, 3), z[l:o3].reshape(-1, 3)))
    if big:
        out["big"] = lam(*L._soc_nt(s[o3:], z[o3:]))
    out["typ"] = np.concatenate([out["d"], out["q3"][:, 1], out["big"][1:2] if big else np.zeros(0, dtype=LD)])
    return out


def ref_cap(E, theta):
    return LD(theta) * np.exp(np.log(E["typ"]).sum() / len(E["typ"]))


def ref_set(E, cap):
    out = [(0, int(i), 0) for i in np.nonzero(E["d"] > cap)[0]]
    out += [(1, int(c), int(d)) for c, d in zip(*np.nonzero(E["q3"] > cap))]
    if E["big"] is not None:
        out += [(2, 0, d) for d in (0, 2) if E["big"][d] > cap]
    return sorted(out)


def margins(E, caps):
    """the smallest distance, in decades, of an eigenvalue a decision is taken on from any of the caps"""
    lam = np.concatenate([E["d"], E["q3"].ravel(), E["big"][[0, 2]] if E["big"] is not None else np.zeros(0, dtype=LD)])
    return min(float(np.abs(np.log10(lam / c)).min()) for c in caps)


def attempts_of(E, theta0, fit):
    """the selections a lane runs: [(theta, set)], the cap raised x 100 while the set does not fit"""
    out, theta = [], theta0
    for _ in range(8):
        st = ref_set(E, ref_cap(E, theta))
        out.append((theta, st))
        if len(st) <= fit:
            return out
        theta *= 100.0
    raise AssertionError("the strong set never fits")


# ---- the runs of the device tests ----------------------------------------------------------------------------------------------------
# name -> design, plan, the strong count at the first cap, the forms that take the run, whether it solves.  k = 63 / 64 / 65: 57 / 58 /
# 59 rows and one cone of each kind (six cone directions); 1025 rows do not fit the capacitance form: one raise, 25 rows drop out; 1102
# (the sort's second strided trip, SZ = 2048) and the two runs at DD_KMAX take the double-double form, the last two without a solve
_Q6 = (("p", 1), ("p0", 1), ("p0m", 1))
RUNS = {
    "dup_k0": dict(design="c8_dup12", plan=dict(), k=0, forms=("cap", "dd"), solve=True),
    "dup_k1": dict(design="c8_dup12", plan=dict(kl=1), k=1, forms=("cap", "dd"), solve=True),
    "dup_k63": dict(design="c8_dup12", plan=dict(kl=57, q3=_Q6), k=63, forms=("cap", "dd"), solve=True),
    "dup_k64": dict(design="c8_dup12", plan=dict(kl=58, q3=_Q6), k=64, forms=("cap", "dd"), solve=True),
    "dup_k65": dict(design="c8_dup12", plan=dict(kl=59, q3=_Q6), k=65, forms=("cap", "dd"), solve=True),
    "dup_k315": dict(design="c8_dup12", plan=dict(kl=300, q3=(("p", 3), ("p0", 3), ("p0m", 2))), k=315, forms=("cap", "dd"), solve=True),
    "qp_p5": dict(design="c6_qp25", plan=dict(q3=(("p", 5),)), k=5, forms=("cap", "dd"), solve=True),
    "qp_k33": dict(design="c6_qp25", plan=dict(q3=(("p", 10), ("p0", 5), ("p0m", 4)), big="p"), k=33, forms=("cap", "dd"), solve=True),
    "qp_k22": dict(design="c6_qp25", plan=dict(q3=(("p", 4), ("p0", 5), ("p0m", 2)), big="p0m"), k=22, forms=("cap", "dd"), solve=True),
    "qp_big2": dict(design="c6_qp25", plan=dict(big="p0m"), k=2, forms=("cap", "dd"), solve=True),
    "lin_k1024": dict(design="c3_lin64", plan=dict(kl=1024), k=1024, forms=("cap", "dd"), solve=True),
    "lin_k1025": dict(design="c3_lin64", plan=dict(kl=1025, drop=25), k=1025, forms=("cap", "dd"), solve=True),
    "qphs_k1102": dict(design="c4_qphs21", plan=dict(kl=1100, big="p0m"), k=1102, forms=("dd",), solve=True),
    "qphs_k3072": dict(design="c4_qphs21", plan=dict(kl=3070, big="p0m"), k=3072, forms=("dd",), solve=False),
    "qphs_k3100": dict(design="c4_qphs21", plan=dict(kl=3098, drop=100, big="p0m"), k=3100, forms=("dd",), solve=False),
    "ap150_k70": dict(design="c2_ap150", plan=dict(kl=60, q3=(("p", 2), ("p0", 1), ("p0m", 2))), k=70, forms=("cap", "dd"), solve=True),
}
_IN = {}


def run_inputs(name, seed=0, nv=2, rhs="random"):
    """(P, s, z, planned, bx, bz) of a run (deterministic).  rhs: 'random' | 'zero' (an all-zero second column)."""
    import zlib
    key = (name, seed, nv, rhs)
    if key not in _IN:
        run = RUNS[name]
        P = K.program_of(run["design"])
        sd = zlib.crc32(name.encode()) + seed
        s, z, planned = strong_iterate(P, sd, run["plan"])
        rng = np.random.default_rng(sd + 7)
        scale = 10.0 ** rng.uniform(-2, 2, (nv, 1))
        bx, bz = rng.standard_normal((nv, P["N"])) * scale, rng.standard_normal((nv, P["R"])) * scale
        if rhs == "zero":
            bx[1:], bz[1:] = 0.0, 0.0
        _IN[key] = (P, s, z, planned, bx, bz)
    return _IN[key]


def fit_of(form):
    return CAP_KMAX if form == "cap" else DD_KMAX


_DESIGNS = {}


def design_of(name):
    if name not in _DESIGNS:
        _DESIGNS[name] = Design(K.program_of(name))
    return _DESIGNS[name]


# ---- the hook's result -----------------------------------------------------------------------------------------------------------
def unpack(o, b, P):
    """lane b of mbfir.test_unit_ddkkt's result as a dict of named blocks, cut to the lane's own dimensions."""
    import mbfir
    l, nq3, big, R, N = P["l"], P["nq3"], P["big"], P["R"], P["N"]
    nq = o["sel_q"].shape[1] // 18
    ldr = o["sel_r"].shape[2]
    D = dict(dl=o["sel_r"][b, 0, :l], dlc=o["sel_r"][b, 1, :l], wbb=o["sel_r"][b, 2, :big], whb=o["sel_r"][b, 3, :max(big - 1, 0)],
             w3=o["sel_q"][b, :4 * nq].reshape(nq, 4)[:nq3], e3=o["sel_q"][b, 4 * nq:12 * nq].reshape(nq, 8)[:nq3],
             m3c=o["sel_q"][b, 12 * nq:18 * nq].reshape(nq, 6)[:nq3], eb=o["sel_sc"][b, :8], etab=o["sel_sc"][b, 8], theta=o["sel_sc"][b, 9],
             slotl=o["sel_i"][b, :l], slot3=o["sel_i"][b, ldr:ldr + 3 * nq].reshape(nq, 3)[:nq3], slotb=o["sel_i"][b, ldr + 3 * nq:ldr + 3 * nq + 2],
             kcnt=int(o["sel_i"][b, ldr + 3 * nq + 2]), skind=o["strong_i"][b, 0], sidx=o["strong_i"][b, 1], sdir=o["strong_i"][b, 2],
             sX=o["strong_x"][b], mode=int(o["lane_rep"][b, 0]), k=int(o["lane_rep"][b, 1]), attempts=int(o["lane_rep"][b, 2]),
             part=o["sel_part"][b], nbp=int(o["lane_rep"][b, 3]),
             flag=int(o["flag"][b]), kp=o["report"]["kp"], cap_form=bool(o["report"]["cap_form"]), passes=o["report"]["passes"])
    npd = -(-N // 64) * 64
    for k in ("H", "M", "Hf"):
        D[k] = o[k][b, :npd, :npd]
    D["U"] = o["U"][b][:, :npd]
    for k in ("Yt", "Zt", "S", "Ms"):
        if k in o:
            D[k] = o[k][b]
    D["cap"] = float(D["eb"][4])
    D["pass"] = []
    for q in range(3):
        pq = {k: o["out_x"][b, q, i] for i, k in enumerate(mbfir.UNIT_DDKKT_OUT_X)}
        pq.update({k: o["out_r"][b, q, i] for i, k in enumerate(mbfir.UNIT_DDKKT_OUT_R)})
        pq.update({k: o["out_k"][b, q, i] for i, k in enumerate(mbfir.UNIT_DDKKT_OUT_K)})
        pq["sc"] = o["sc"][b, q]
        D["pass"].append(pq)
    D["sc_end"], D["dx_end"], D["dz_end"], D["gdx_end"] = o["sc"][b, 3], o["end_x"][b], o["end_r"][b, 0], o["end_r"][b, 1]
    return D


def is_sent(a, sentinel=np.nan):
    a = np.asarray(a)
    return bool(np.all(np.isnan(a) if np.isnan(sentinel) else a == sentinel))


# ---- the eigen form of the device's scaling ----------------------------------------------------------------------------------------
class Eig:
    """sum_k f_k e_k e_k' in longdouble from the device's eigen data (e3, eb, whb, dl, dlc, cap), and its envelopes."""

    def __init__(self, P, D):
        self.P, self.D = P, D
        l, nq3, big = P["l"], P["nq3"], P["big"]
        r2 = 1 / np.sqrt(LD(2))
        e3 = ld(D["e3"])
        w1, w2 = e3[:, 3], e3[:, 4]
        one, zero = np.ones(nq3, dtype=LD), np.zeros(nq3, dtype=LD)
        # (direction, cone, component): e_p, e_0, e_m of soc3_evec
        self.E3 = np.stack([np.stack([one * r2, -w1 * r2, -w2 * r2], 1), np.stack([zero, w2, -w1], 1), np.stack([one * r2, w1 * r2, w2 * r2], 1)])
        self.lam3 = e3[:, :3]
        cap = LD(D["cap"])
        self.f_inv2c = dict(orth=ld(D["dlc"]), q3=np.minimum(self.lam3, cap), big=None)
        self.f_w2 = dict(orth=1 / ld(D["dl"]), q3=1 / self.lam3, big=None)
        if big:
            wh = ld(D["whb"])
            self.eb = np.stack([np.concatenate([[r2], -wh * r2]), np.concatenate([[r2], wh * r2])])          # e_p, e_m
            lb = ld(D["eb"][:3])
            self.f_inv2c["big"] = np.array([min(lb[0], cap), lb[1], min(lb[2], cap)], dtype=LD)
            self.f_w2["big"] = 1 / lb

    def apply(self, V, f, env=False):
        """sum_k f_k e_k e_k' V for V (R, nc); env: with |f|, |e|, |V| and |f_p| + |f_0| for the big cone's differences (float64)."""
        P = self.P
        l, nq3, big, o3 = P["l"], P["nq3"], P["big"], P["l"] + 3 * P["nq3"]
        V = np.abs(f64(V)) if env else ld(V)
        a = (lambda x: np.abs(f64(x))) if env else (lambda x: x)
        out = np.zeros(V.shape, dtype=V.dtype)
        out[:l] = a(f["orth"])[:, None] * V[:l]
        if nq3:
            V3 = V[l:o3].reshape(nq3, 3, -1)
            acc = 0
            for d in range(3):
                e = a(self.E3[d])
                acc = acc + e[:, :, None] * (a(f["q3"][:, d])[:, None] * np.einsum("ca,cak->ck", e, V3))[:, None, :]
            out[l:o3] = acc.reshape(3 * nq3, -1)
        if big:
            fp, f0, fm = a(f["big"])
            ep, em = a(self.eb[0]), a(self.eb[1])
            dp, dm = (fp + f0, fm + f0) if env else (fp - f0, fm - f0)
            out[o3:] = f0 * V[o3:] + dp * ep[:, None] * (ep @ V[o3:])[None, :] + dm * em[:, None] * (em @ V[o3:])[None, :]
        return out

    def bound(self, V, f, k_orth, extra3=0.0):
        """the kernels' error applying sum f e e' to an exact V: k_orth u on the orthant rows, K_M3 (+ extra3) on a 3-row cone, k_big."""
        P = self.P
        env = self.apply(V, f, env=True)
        l, o3 = P["l"], P["l"] + 3 * P["nq3"]
        env[:l] *= k_orth * U
        env[l:o3] *= (K_M3 + extra3) * U
        env[o3:] *= k_big(P) * U
        return env


class Design:
    """G (longdouble), its envelope and the constants of one design."""

    def __init__(self, P, dense=False):
        self.P = P
        self.G, self.Gr, self.Gh = L.G_ref(P), L.G_ref(P, round_arg=True), L.G_hat(P)
        self.kg, self.kgt, self.kh, self.ku = L.K_G(P, dense), L.K_GT(P, dense), L.K_H(P, dense), k_u(P)

    def gv(self, v):
        return (self.G @ ld(v).T).T, self.kg * U * (self.Gh @ np.abs(f64(v)).T).T

    def gtv(self, u):
        return (self.G.T @ ld(u).T).T, self.kgt * U * (self.Gh.T @ np.abs(f64(u)).T).T


# ---- the selection ----------------------------------------------------------------------------------------------------------------
def check_selection(P, D, s, z, theta0=THETA, rec=None, sentinel=np.nan):
    """Eigen data, cap, strong set, slot maps, m3c of one live lane.  Returns (rec, facts)."""
    rec = rec or CR.Rec()
    l, nq3, big = P["l"], P["nq3"], P["big"]
    fit = CAP_KMAX if D["cap_form"] else DD_KMAX
    # eig
    if nq3:
        w = ld(D["w3"])
        eta, w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2], w[:, 3]
        n1 = np.sqrt(w1 * w1 + w2 * w2)
        g, e2 = (w0 + n1) ** 2, 1 / (eta * eta)
        e3 = D["e3"]
        for j, (ref, kk) in enumerate(((g * e2, K_LAM), (e2, K_LAM0), (e2 / g, K_LAM))):
            rec.add("eig", "lam%d" % j, np.abs(ld(e3[:, j]) - ref), kk * U * f64(ref))
        nz = f64(n1) > 0
        wh = np.stack([np.where(nz, w1 / np.where(nz, n1, 1), 1), np.where(nz, w2 / np.where(nz, n1, 1), 0)], 1)
        rec.add("eig", "what", np.abs(ld(e3[:, 3:5]) - wh), K_WHAT * U * np.abs(f64(wh)))
        rec.exact("eig", "n1 = 0 gives (1, 0)", np.array_equal(e3[~nz, 3:5], np.tile([1.0, 0.0], ((~nz).sum(), 1))))
        rec.add("eig", "|what| = 1", np.abs(np.sqrt((ld(e3[:, 3:5]) ** 2).sum(1)) - 1), 16 * U)
    if big:
        wb = ld(D["wbb"])
        nn = np.sqrt((wb[1:] ** 2).sum())
        g, e2 = (wb[0] + nn) ** 2, 1 / (LD(D["etab"]) ** 2)
        for j, ref in enumerate((g * e2, e2, e2 / g)):
            rec.add("eig", "big lam%d" % j, abs(LD(D["eb"][j]) - ref), (K_LAM0 if j == 1 else k_big(P)) * U * float(ref))
        wh = wb[1:] / nn if nn > 0 else np.concatenate([[LD(1)], np.zeros(big - 2, dtype=LD)])
        rec.add("eig", "whb", np.abs(ld(D["whb"]) - wh), 4 * (CR.kd(big) / 2 + 2) * U * np.abs(f64(wh)) + 1e-300)
        rec.add("eig", "|whb| = 1", abs(np.sqrt((ld(D["whb"]) ** 2).sum()) - 1), 4 * (CR.kd(big) + 4) * U)
    # the partial rows of (sum log, count): the big cone's first, then one per block of 256 orthant rows and 3-row cones
    if "part" in D:
        seq = np.concatenate([ld(D["dl"]), ld(D["e3"][:, 1]) if nq3 else np.zeros(0, dtype=LD)])
        lgs = np.log(seq)
        nbp, o0 = D["nbp"], 1 if big else 0
        rows, envs = np.zeros((nbp, 2), dtype=LD), np.zeros(nbp)
        if big:
            rows[0], envs[0] = (np.log(LD(D["eb"][1])), 1), abs(float(np.log(LD(D["eb"][1]))))
        for q in range(nbp - o0):
            blk = lgs[256 * q:256 * q + 256]
            rows[o0 + q], envs[o0 + q] = (blk.sum(), len(blk)), float(np.abs(blk).sum())
        rec.exact("eig", "partial rows: at least the lane's blocks", nbp >= max(1, -(-(l + nq3) // 256)) + o0)      # (a unit: its largest lane's)
        rec.add("eig", "partial sum log", np.abs(ld(D["part"][:nbp, 0]) - rows[:, 0]), K_PART * U * envs)
        rec.exact("eig", "partial counts", np.array_equal(D["part"][:nbp, 1], f64(rows[:, 1])))
        rec.exact("eig", "rows past the partials untouched", is_sent(D["part"][nbp:], sentinel))
    # cap: from the device's own weights
    typ = np.concatenate([ld(D["dl"]), ld(D["e3"][:, 1]) if nq3 else np.zeros(0, dtype=LD), ld(D["eb"][1:2]) if big else np.zeros(0, dtype=LD)])
    lg = np.log(typ)
    mean = lg.sum() / len(typ)
    cap_ref = LD(D["theta"]) * np.exp(mean)
    rel = 4 * U * (CR.k_rows(P) * float(np.abs(lg).sum()) / len(typ) + abs(float(mean)) + 3)
    rec.add("cap", "cap", abs(LD(D["cap"]) - cap_ref), rel * float(cap_ref))
    # the attempts and the set: the reference's own eigenvalues and caps
    E = ref_eigs(P, s, z)
    att = attempts_of(E, theta0, fit)
    rec.exact("set", "attempts", D["attempts"] >= len(att))        # (a unit runs as many selections as its slowest lane)
    rec.exact("set", "theta", D["theta"] == att[-1][0])
    want = att[-1][1]
    k = len(want)
    rec.exact("set", "kcnt", D["kcnt"] == k and D["k"] == k)
    got = list(zip(D["skind"][:k].tolist(), D["sidx"][:k].tolist(), D["sdir"][:k].tolist()))
    rec.exact("set", "the set is the reference's", sorted(got) == want)
    rec.exact("set", "sorted by (kind, index, direction)", got == sorted(got))
    rec.exact("set", "slots past the count untouched", bool(np.all(D["skind"][k:] == -9) and np.all(D["sidx"][k:] == -9) and np.all(D["sdir"][k:] == -9))
              and is_sent(D["sX"][k:], sentinel))
    sl, s3, sb = np.full(l, -1), np.full((nq3, 3), -1), np.full(2, -1)
    lam_dev = np.zeros(k)
    for slot, (kind, idx, d) in enumerate(got):
        if kind == 0 and 0 <= idx < l:
            sl[idx], lam_dev[slot] = slot, D["dl"][idx]
        elif kind == 1 and 0 <= idx < nq3 and 0 <= d < 3:
            s3[idx, d], lam_dev[slot] = slot, D["e3"][idx, d]
        elif kind == 2 and d in (0, 2):
            sb[d // 2], lam_dev[slot] = slot, D["eb"][d]
    rec.exact("set", "slotl", np.array_equal(D["slotl"], sl))
    rec.exact("set", "slot3", np.array_equal(D["slot3"], s3))
    rec.exact("set", "slotb", np.array_equal(D["slotb"], sb) if big else True)
    rec.exact("set", "sX = fl(lam - cap)", np.array_equal(D["sX"][:k], lam_dev - D["cap"]))
    rec.exact("set", "dlc = min(d, cap)", np.array_equal(D["dlc"], np.minimum(D["dl"], D["cap"])))
    # m3c
    if nq3:
        Eg = Eig(P, D)
        f = Eg.f_inv2c["q3"]
        ref = sum(f[:, d, None, None] * Eg.E3[d][:, :, None] * Eg.E3[d][:, None, :] for d in range(3))
        env = sum(f64(f[:, d, None, None]) * np.abs(f64(Eg.E3[d]))[:, :, None] * np.abs(f64(Eg.E3[d]))[:, None, :] for d in range(3))
        ij = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
        rec.add("m3c", "m3c", np.abs(ld(D["m3c"]) - ref[:, ij[0], ij[1]]), K_M3 * U * env[:, ij[0], ij[1]])
    return rec, dict(k=k, want=want, attempts=att, E=E)


# ---- the strong rows and the capped normal matrix -----------------------------------------------------------------------------------
def u_ref(P, Dn, D, k):
    """rows 0 .. k-1 of U in longdouble from the device's slots and eigen data, and the envelope."""
    l, nq3, o3 = P["l"], P["nq3"], P["l"] + 3 * P["nq3"]
    Eg = Eig(P, D)
    N = P["N"]
    ref, env = np.zeros((k, N), dtype=LD), np.zeros((k, N))
    Ga, Gh = Dn.Gr, Dn.Gh
    for slot in range(k):
        kind, idx, d = int(D["skind"][slot]), int(D["sidx"][slot]), int(D["sdir"][slot])
        if kind == 0:
            ref[slot], env[slot] = Ga[idx], Gh[idx]
        elif kind == 1:
            e, r0 = Eg.E3[d][idx], l + 3 * idx
            ref[slot], env[slot] = e @ Ga[r0:r0 + 3], np.abs(f64(e)) @ Gh[r0:r0 + 3]
        else:
            e = Eg.eb[0 if d == 0 else 1]
            ref[slot], env[slot] = e @ Ga[o3:], np.abs(f64(e)) @ Gh[o3:]
    return ref, env


def check_build(P, Dn, D, rec=None, sentinel=np.nan, rows_only=False, ref=None):
    """U, the kept H, and (capacitance form) M, Yt, Zt, S, Ms of a lane in the extended-precision mode.  ref: the float64 twin of the
    same inputs (twin(..., 'cap')), whose own H and S give the condition numbers M and Ms are held by -- nothing of the device's."""
    rec = rec or CR.Rec()
    N, k, kp = P["N"], D["k"], D["kp"]
    Um = D["U"]
    uref, env = u_ref(P, Dn, D, min(k, Um.shape[0]))
    kk = len(uref)
    rec.add("U", "rows", np.abs(ld(Um[:kk, :N]) - uref), Dn.ku * U * env)
    rec.exact("U", "columns past N exactly zero", bool(np.all(Um[:kk, N:] == 0.0)))
    rec.exact("U", "padding rows exactly zero", bool(np.all(Um[kk:kp] == 0.0)) and not np.any(np.signbit(Um[kk:kp])))
    rec.exact("U", "rows past kp untouched", is_sent(Um[max(kp, kk):], sentinel))
    if rows_only:
        return rec
    Eg = Eig(P, D)
    f = Eg.f_inv2c
    WG = Eg.apply(Dn.G, f)
    href = Dn.G.T @ WG
    henv = Dn.Gh.T @ Eg.apply(Dn.Gh, f, env=True)
    # (the lower triangle: what the factorisation reads)
    rec.add("H", "H_w", np.tril(np.abs(ld(D["H"][:N, :N]) - href)), (Dn.kh + K_M3 + k_big(P)) * U * henv)
    rec.exact("H", "pivots", D["flag"] == 0)
    if D["cap_form"] and "Yt" in D:
        p, out = cap_problem(P, D, 0), cap_out(P, D, 0)
        fold_report(rec, CK.stage_checks(p, kp, out, stages=("Yt", "Zt", "S")), "cap ")
        Hp = np.eye(len(out["M"]))
        Hp[:p["n"], :p["n"]] = p["H"]
        inverse_factor(rec, "cap M", Hp, out["M"], N, cond_of(ref["H"][:N, :N]))
        inverse_factor(rec, "cap Ms", np.tril(out["S"]) + np.tril(out["S"], -1).T, out["Ms"], k, cond_of(ref["S"][:k, :k]))
    return rec


def cond_of(A):
    ev = np.linalg.eigvalsh(A)
    return float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf


def check_plain_H(P, Dn, D, s, z, rec):
    """the kept H of a lane in the plain mode against G'W^-2 G at (s, z) in longdouble, lattice_ref's bound"""
    N = P["N"]
    S = L.Scaling(P, s, z)
    rec.add("H", "plain", np.tril(np.abs(ld(D["H"][:N, :N]) - L.H_ref(Dn.G, S))), Dn.kh * U * L.H_env(Dn.Gh, S))
    return rec


def inverse_factor(rec, stage, A, Minv, core, cond):
    """capkkt_ref._inverse_factor's two checks (|M L - I| with NumPy's factor L; |A x - c| / |c| for x = M'(M c)) and the exact zeros above
    the diagonal inside the diagonal tiles.  capkkt_ref holds them to 1e-11 and 1e-10, which it states for cond(A) <= 1e6; the
    iterates here give cond(S) up to 1e10 (the float64 twin misses the 1e-10 by a factor 26 at k = 65).  Both errors are first-order
    in the backward error of the factorisation, |dA| <= c q u |A| for a q x q Cholesky factorisation (Higham, Accuracy and Stability,
    Thm 10.3 / 10.4), carried through the inverse: q u cond, with the margin of 4.  cond is the caller's: that of the leading
    core x core block of the REFERENCE's matrix (the float64 twin's H_w resp. S, built from (s, z) alone) -- never of A, which the
    device produced; the padding (unit diagonal, zero coupling) factorises exactly and would only inflate it.  The tolerance is the
    larger of the two."""
    q = len(A)
    tiles = np.arange(q) // CK.TB
    same_tile_above = (tiles[None, :] == tiles[:, None]) & (np.arange(q)[None, :] > np.arange(q)[:, None])
    rec.exact(stage, "zero above the diagonal inside a diagonal tile", bool(np.all(Minv[same_tile_above] == 0.0)))
    rec.exact(stage, "finite lower triangle", bool(np.isfinite(Minv[np.tril_indices(q)]).all()))
    rec.exact(stage, "padding exact", np.array_equal(np.tril(Minv)[core:], np.eye(q)[core:]))
    M = np.tril(np.nan_to_num(Minv))
    tol = 4.0 * core * U * cond if np.isfinite(cond) else 0.0
    Lc = np.linalg.cholesky(A)
    c = np.random.default_rng(q).standard_normal(q)
    rec.add(stage, "M L - I", float(np.abs(M @ Lc - np.eye(q)).max()), max(CK.CHOL_INV_TOL, tol))
    rec.add(stage, "A x - c", float(np.linalg.norm(A @ (M.T @ (M @ c)) - c) / np.linalg.norm(c)), max(CK.CHOL_RESID_TOL, tol))


def cap_problem(P, D, q, nv=None):
    # (a lane of a unit of several orders: the vector kernels run over the unit's largest N, the lane's H being the identity past its
    #  own -- the problem is the padded one, whatever the caller left past the lane's N included)
    N, k = D.get("n_unit", P["N"]), D["k"]
    pq = D["pass"][q]
    nv = nv or 2
    Hl = np.tril(D["H"][:N, :N])
    return {"n": N, "k": k, "H": Hl + np.tril(Hl, -1).T, "U": D["U"][:k, :N], "X": D["sX"][:k], "a": np.nan_to_num(pq["r1"][:nv, :N]),
            "b": np.nan_to_num(pq["gtw"][:nv, :N]), "t": np.nan_to_num(pq["ts"][:nv, :k])}


def cap_out(P, D, q, nv=None):
    kp = D["kp"]
    pq = D["pass"][q]
    nv = nv or 2
    return {"M": D["M"], "Yt": D["Yt"][:kp], "Zt": D["Zt"][:kp], "S": D["S"][:kp, :kp], "Ms": D["Ms"][:kp, :kp], "rhs_w": pq["rhs_l"][:nv],
            "y": pq["y"][:nv], "w": pq["capw"][:nv, :kp], "zeta": pq["zeta"][:nv, :kp], "dx": pq["bh"][:nv]}


def fold_report(rec, rep, prefix):
    """capkkt_ref's report into a Rec: the fractions by stage, a failure as a failed exact check."""
    for st, v in rep.fractions.items():
        rec.frac[(prefix + st, st)] = max(rec.frac.get((prefix + st, st), 0.0), float(v))
    for st, what in rep.failures:
        rec.failed.append((prefix + st, what))


# ---- the passes of kkt_solve_dd -----------------------------------------------------------------------------------------------------
def spread_ref(P, D, Eg, zeta):
    """the strong multipliers (nv, slots) spread over their cone rows in longdouble, and the envelope of the terms."""
    l, nq3, o3, R = P["l"], P["nq3"], P["l"] + 3 * P["nq3"], P["R"]
    nv = zeta.shape[0]
    out, env = np.zeros((nv, R), dtype=LD), np.zeros((nv, R))
    for slot in range(D["k"]):
        kind, idx, d = int(D["skind"][slot]), int(D["sidx"][slot]), int(D["sdir"][slot])
        zt = ld(zeta[:, slot])
        if kind == 0:
            out[:, idx] += zt
        elif kind == 1:
            e, r0 = Eg.E3[d][idx], l + 3 * idx
            out[:, r0:r0 + 3] += zt[:, None] * e[None, :]
            env[:, r0:r0 + 3] += np.abs(f64(zt))[:, None] * np.abs(f64(e))[None, :]
        else:
            e = Eg.eb[0 if d == 0 else 1]
            out[:, o3:] += zt[:, None] * e[None, :]
            env[:, o3:] += np.abs(f64(zt))[:, None] * np.abs(f64(e))[None, :]
    return out, env


def t_ref(P, D, Eg, r2):
    """t = e'r2 per strong slot from the device's own r2 (nv, R): (ref, bound, exact mask)."""
    l, nq3, o3 = P["l"], P["nq3"], P["l"] + 3 * P["nq3"]
    k, nv = D["k"], r2.shape[0]
    ref, bnd, exact = np.zeros((nv, k), dtype=LD), np.zeros((nv, k)), np.zeros(k, dtype=bool)
    for slot in range(k):
        kind, idx, d = int(D["skind"][slot]), int(D["sidx"][slot]), int(D["sdir"][slot])
        if kind == 0:
            ref[:, slot], exact[slot] = ld(r2[:, idx]), True
        elif kind == 1:
            e, r0 = Eg.E3[d][idx], l + 3 * idx
            ref[:, slot] = ld(r2[:, r0:r0 + 3]) @ e
            bnd[:, slot] = 24 * U * (np.abs(r2[:, r0:r0 + 3]) @ np.abs(f64(e)))
        else:
            e = Eg.eb[0 if d == 0 else 1]
            ref[:, slot] = ld(r2[:, o3:]) @ e
            bnd[:, slot] = 4 * (CR.kd(P["big"]) + 4) * U * (np.abs(r2[:, o3:]) @ np.abs(f64(e)))
    return ref, bnd, exact


def mp_dd(P, D, pq, nv, cols=None, slots=None):
    """k_dd_rhs and k_dd_zeta in mpmath, at the columns `cols` and slots `slots` (default all): (rhs ref, rhs envelope, zeta ref, zeta
    envelope) as lists."""
    import mpmath as mp
    mp.mp.prec = 240
    N, k = P["N"], D["k"]
    Um, X = D["U"][:k, :N], D["sX"][:k]
    f = lambda a: [mp.mpf(float(x)) for x in a]
    out = []
    for v in range(nv):
        xt = [mp.mpf(float(X[r])) * mp.mpf(float(pq["ts"][v, r])) for r in range(k)]
        rhs, renv = [], []
        for j in (range(N) if cols is None else cols):
            col = f(Um[:, j])
            terms = [c * y for c, y in zip(col, xt) if c != 0]
            rhs.append(mp.mpf(float(pq["r1"][v, j])) + mp.mpf(float(pq["gtw"][v, j])) + mp.fsum(terms))
            renv.append(abs(float(pq["r1"][v, j])) + abs(float(pq["gtw"][v, j])) + float(mp.fsum(abs(t) for t in terms)))
        B = [mp.mpf(float(h)) + mp.mpf(float(lo)) for h, lo in zip(pq["bh"][v, :N], pq["bl"][v, :N])]
        zeta, zenv = [], []
        for r in (range(k) if slots is None else slots):
            terms = [mp.mpf(float(u)) * b for u, b in zip(Um[r], B) if u != 0]
            tt = mp.mpf(float(pq["ts"][v, r]))
            zeta.append((mp.fsum(terms) - tt) * mp.mpf(float(X[r])))
            zenv.append(float(X[r]) * (float(mp.fsum(abs(t) for t in terms)) + abs(float(tt))))
        out.append((rhs, renv, zeta, zenv))
    return out


def check_passes(P, Dn, D, bx, bz, nv, rec=None, sentinel=np.nan, slow=True):
    """The passes of kkt_solve_dd of one lane in the extended-precision mode, group by group.  Returns (rec, facts)."""
    rec = rec or CR.Rec()
    N, R, l, o3, k, kp = P["N"], P["R"], P["l"], P["l"] + 3 * P["nq3"], D["k"], D["kp"]
    bx, bz = np.asarray(bx, dtype=np.float64)[:nv, :N], np.asarray(bz, dtype=np.float64)[:nv, :R]
    Eg = Eig(P, D)
    kn = K.k_n(N)
    dz, gdx, dx = np.zeros((nv, R)), np.zeros((nv, R)), np.zeros((nv, N))
    norms = []
    cap = D["cap_form"]
    acc = dict(gt=np.zeros((nv, R)))
    for q in range(D["passes"]):
        pq = {key: (v[:nv] if key != "sc" else v) for key, v in D["pass"][q].items()}
        # r1
        ref, b = Dn.gtv(dz)
        rec.add("r1", "G'dz", np.abs(ld(pq["gtdz"][:, :N]) - ref), b)
        rec.exact("r1", "r1 = fl(bx - G'dz)", np.array_equal(pq["r1"][:, :N], bx - pq["gtdz"][:, :N]))
        rec.exact("r1", "past N untouched", is_sent(pq["gtdz"][:, N:], sentinel) and is_sent(pq["r1"][:, N:], sentinel))
        n = K.vnorm(pq["r1"][:, :N])
        rec.add("r1", "norm", abs(LD(pq["sc"][q]) - n), kn * U * float(n))
        rec.exact("r1", "later norm slots untouched", is_sent(pq["sc"][q + 1:], sentinel))
        rec.exact("r1", "earlier norm slots kept", np.array_equal(pq["sc"][:q], np.array(norms)))
        norms.append(float(pq["sc"][q]))
        # r2, t
        w2 = Eg.apply(dz.T, Eg.f_w2).T
        ref = ld(bz) - ld(gdx) + w2
        b = Eg.bound(dz.T, Eg.f_w2, 4.0, 4.0).T + 12 * U * (np.abs(bz) + np.abs(gdx) + np.abs(f64(w2)))
        rec.add("r2", "orth", np.abs(ld(pq["r2"][:, :l]) - ref[:, :l]), b[:, :l])
        rec.add("r2", "cones", np.abs(ld(pq["r2"][:, l:R]) - ref[:, l:]), b[:, l:])
        tr, tb, ex = t_ref(P, D, Eg, pq["r2"][:, :R])
        ts = pq["ts"]
        rec.exact("r2", "t of an orthant row is its r2", np.array_equal(ts[:, :k][:, ex], f64(tr)[:, ex]))
        rec.add("r2", "t", np.abs(ld(ts[:, :k]) - tr)[:, ~ex], tb[:, ~ex])
        rec.exact("r2", "t past the count untouched", is_sent(ts[:, k:], sentinel))
        # wbz = W_w^-2 r2
        ref = Eg.apply(pq["r2"][:, :R].T, Eg.f_inv2c).T
        b = Eg.bound(pq["r2"][:, :R].T, Eg.f_inv2c, 4.0).T
        rec.add("wbz", "orth", np.abs(ld(pq["wbz"][:, :l]) - ref[:, :l]), b[:, :l])
        rec.add("wbz", "cones", np.abs(ld(pq["wbz"][:, l:R]) - ref[:, l:]), b[:, l:])
        ref, b = Dn.gtv(pq["wbz"][:, :R])
        rec.add("gtw", "G'wbz", np.abs(ld(pq["gtw"][:, :N]) - ref), b)
        # the normal-equation solve
        if cap:
            rep = CK.stage_checks(cap_problem(P, D, q, nv), kp, cap_out(P, D, q, nv), stages=("rhs_w", "y", "w", "zeta", "dx"))
            fold_report(rec, rep, "cap ")
            rec.exact("solve", "dd blocks untouched", is_sent(pq["rhs_h"], sentinel) and is_sent(pq["bl"], sentinel))
            rec.exact("solve", "past kp untouched", is_sent(pq["capw"][:, kp:], sentinel) and is_sent(pq["zeta"][:, kp:], sentinel))
        else:
            rec.exact("solve", "capacitance blocks untouched", is_sent(pq["y"], sentinel) and is_sent(pq["capw"], sentinel))
            rec.exact("solve", "zeta past the count untouched", is_sent(pq["zeta"][:, k:], sentinel))
            rec.exact("solve", "past N exactly zero", bool(np.all(pq["rhs_h"][:, N:] == 0) and np.all(pq["rhs_l"][:, N:] == 0)))
            from oracle import ddlin
            Bh, Bl = np.array(pq["rhs_h"].T, order="C", copy=True), np.array(pq["rhs_l"].T, order="C", copy=True)     # (solved in place)
            ddlin.cho_solve(np.ascontiguousarray(D["Hf"]), np.ascontiguousarray(D["M"]), Bh, Bl)
            sref = (ld(Bh) + ld(Bl)).T[:, :N]
            got = ld(pq["bh"][:, :N]) + ld(pq["bl"][:, :N])
            rec.add("solve", "triangular solves", np.abs(got - sref).max(), 1e-24 * float(np.abs(sref).max()) * max(1.0, float(D["sX"][:k].max())))
            # (slow: every column and slot in mpmath; otherwise a sample of both -- every column workgroup of k_dd_rhs, every 29th slot)
            cols = list(range(N)) if slow else sorted(set(range(0, N, 5)) | {N - 1})
            slots = list(range(k)) if slow else sorted(set(range(0, k, 29)) | {k - 1})
            if True:
                import mpmath as mp
                for v, (rhs, renv, zeta, zenv) in enumerate(mp_dd(P, D, pq, nv, cols, slots)):
                    got = [mp.mpf(float(pq["rhs_h"][v, j])) + mp.mpf(float(pq["rhs_l"][v, j])) for j in cols]
                    rec.add("solve", "rhs", [float(abs(g - r)) for g, r in zip(got, rhs)], k_dd(-(-k // 16) + 16) * EPS_DD * np.array(renv))
                    rec.add("solve", "zeta", [float(abs(mp.mpf(float(g)) - r)) for g, r in zip(pq["zeta"][v, slots], zeta)],
                            k_dd(-(-N // 64) + 8) * EPS_DD * np.array(zenv) + U * np.array([abs(float(r)) for r in zeta]))
        bh = pq["bh"][:, :N]
        ref, b = Dn.gv(bh)
        rec.add("gbh", "G Bh", np.abs(ld(pq["gbh"][:, :R]) - ref), b)
        vin = ld(pq["gbh"][:, :R]) - ld(pq["r2"][:, :R])
        ref = Eg.apply(vin.T, Eg.f_inv2c).T
        b = Eg.bound(vin.T, Eg.f_inv2c, 8.0, 4.0).T + Eg.apply((U * (np.abs(pq["gbh"][:, :R]) + np.abs(pq["r2"][:, :R]))).T, Eg.f_inv2c, env=True).T * np.where(np.arange(R) < l, 0.0, 1.0)
        rec.add("wbz", "second orth", np.abs(ld(pq["wbz2"][:, :l]) - ref[:, :l]), b[:, :l])
        rec.add("wbz", "second cones", np.abs(ld(pq["wbz2"][:, l:R]) - ref[:, l:]), b[:, l:])
        # accumulation
        sp, senv = spread_ref(P, D, Eg, pq["zeta"])
        K.two_roundings(rec, "acc", "dz", pq["dz"][:, :R], dz, ld(pq["wbz2"][:, :R]) + sp, 24 * U * senv * (1 if o3 > l or P["big"] else 0) + U * np.abs(f64(sp)))
        rec.exact("acc", "gdx = fl(gdx + G Bh)", np.array_equal(pq["gdx"][:, :R], gdx + pq["gbh"][:, :R]))
        rec.exact("acc", "dx = fl(dx + Bh)", np.array_equal(pq["dx"][:, :N], dx + bh))
        acc["gt"] += np.abs(pq["wbz2"][:, :R]) + np.abs(f64(sp))
        dz, gdx, dx = pq["dz"][:, :R].copy(), pq["gdx"][:, :R].copy(), pq["dx"][:, :N].copy()
    for q in range(D["passes"], 3):
        rec.exact("end", "pass %d untouched" % q, all(is_sent(v, sentinel) for v in D["pass"][q].values()))
    if nv == 1:
        rec.exact("end", "vector 1 untouched", all(is_sent(v[1], sentinel) for pq in D["pass"] for key, v in pq.items() if key != "sc"))
    # the end: what the solve leaves and the two residuals with no hand-over
    rec.exact("end", "dx, dz, gdx as the last pass left them", np.array_equal(D["dx_end"][:nv, :N], dx) and np.array_equal(D["dz_end"][:nv, :R], dz)
              and np.array_equal(D["gdx_end"][:nv, :R], gdx))
    rec.exact("end", "norm slots", np.array_equal(D["sc_end"][:D["passes"]], np.array(norms)) and is_sent(D["sc_end"][D["passes"]:], sentinel))
    n1, n2, fl1, fl2 = residuals(P, Dn, Eg, bx, bz, dx, dz)
    return rec, dict(norms=norms, n1=n1, n2=n2, floor1=fl1, floor2=fl2)


def residuals(P, Dn, Eg, bx, bz, dx, dz):
    """||bx - G'dz|| (largest over the vectors) and max |bz - G dx + W^2 dz| in longdouble, and the floors: what evaluating them in
    float64 would cost by the bounds above."""
    g, gb = Dn.gv(dx)
    gt, gtb = Dn.gtv(dz)
    w2 = Eg.apply(np.asarray(dz).T, Eg.f_w2).T
    r1 = ld(bx) - gt
    r2 = ld(bz) - g + w2
    fl1 = float(np.sqrt((gtb ** 2).sum(1)).max()) + 2 * U * float(np.sqrt(((np.abs(bx) + np.abs(f64(gt))) ** 2).sum(1)).max())
    fl2 = float((gb + Eg.bound(np.asarray(dz).T, Eg.f_w2, 4.0, 4.0).T + 12 * U * (np.abs(bz) + np.abs(f64(g)) + np.abs(f64(w2)))).max())
    return float(np.sqrt((r1 ** 2).sum(1)).max()), float(np.abs(r2).max()), fl1, fl2


def refines(facts, tw):
    """the device's residuals against the twin's: the names of those that exceed FACTOR max(twin's, floor)."""
    return [(k, facts[k], tw[k]) for k, fl in (("n1", "floor1"), ("n2", "floor2")) if not facts[k] <= FACTOR * max(tw[k], facts[fl])]


# ---- the float64 twin: oracle/conic_ipm.py's factor_dd / kkt_solve_dd restated with explicit factors -------------------------------
def twin(P, Gm, s, z, bx, bz, form, theta=THETA, order="device", mutate=None):
    """Returns a dict shaped like unpack()'s (float64 throughout): the selection, U, H, the factors and every group of every pass,
    so that the checks above run on it.  form: 'cap' | 'dd'; order: 'device' (kkt_ref.dev_sum) | 'seq', the sums of the norms."""
    from scipy.linalg import cholesky, solve_triangular
    from oracle import ddlin
    l, nq3, big, R, N, o3 = P["l"], P["nq3"], P["big"], P["R"], P["N"], P["l"] + 3 * P["nq3"]
    npd = -(-N // 64) * 64
    nv = bx.shape[0]
    add = K.dev_sum if order == "device" else K.seq_sum
    Wm = K.oracle_scaling(P, s, z)
    D = dict(dl=Wm.dl.copy(), cap_form=form == "cap", flag=0, mode=1)
    D["w3"] = np.concatenate([Wm.eta3[:, None], Wm.wb3], 1) if nq3 else np.zeros((0, 4))
    e3 = np.zeros((nq3, 8))
    if nq3:
        w = D["w3"]
        n1 = np.sqrt(w[:, 2] * w[:, 2] + w[:, 3] * w[:, 3])
        g, e2 = (w[:, 1] + n1) * (w[:, 1] + n1), 1.0 / (w[:, 0] * w[:, 0])
        e3[:, 0], e3[:, 1], e3[:, 2] = g * e2, e2, e2 / g
        e3[:, 3], e3[:, 4] = np.where(n1 > 0, w[:, 2] / np.where(n1 > 0, n1, 1), 1.0), np.where(n1 > 0, w[:, 3] / np.where(n1 > 0, n1, 1), 0.0)
    D["e3"], D["eb"], D["wbb"], D["whb"], D["etab"] = e3, np.zeros(8), np.zeros(0), np.zeros(0), 0.0
    if big:
        wb = Wm.wbb
        nn = float(np.sqrt(wb[1:] @ wb[1:]))
        g, e2 = (wb[0] + nn) ** 2, 1.0 / (Wm.etab * Wm.etab)
        D["eb"][:3] = g * e2, e2, e2 / g
        D["wbb"], D["whb"], D["etab"] = wb.copy(), wb[1:] / nn, float(Wm.etab)
    typ = np.concatenate([D["dl"], e3[:, 1], D["eb"][1:2] if big else np.zeros(0)])
    fit = CAP_KMAX if form == "cap" else DD_KMAX
    th, att = theta, 0
    while True:
        att += 1
        capv = th * float(np.exp(np.log(typ).sum() / len(typ)))
        st = [(0, int(i), 0) for i in np.nonzero(D["dl"] > capv)[0]] + [(1, int(c), int(d)) for c, d in zip(*np.nonzero(e3[:, :3] > capv))]
        st += [(2, 0, d) for d in (0, 2) if big and D["eb"][d] > capv]
        if len(st) <= fit:
            break
        th *= 100.0
    st = sorted(st)
    k = len(st)
    kp = -(-k // 64) * 64 if form == "cap" else k
    D.update(theta=th, attempts=att, k=k, kcnt=k, kp=kp, passes=3 if form == "cap" else 2)
    D["eb"][4] = D["cap"] = capv
    D["dlc"] = np.minimum(D["dl"], capv)
    D["skind"], D["sidx"], D["sdir"] = [np.full(DD_KMAX, -9, dtype=np.int32) for _ in range(3)]
    D["sX"] = np.full(DD_KMAX, np.nan)
    D["slotl"], D["slot3"], D["slotb"] = np.full(l, -1, dtype=np.int32), np.full((nq3, 3), -1, dtype=np.int32), np.full(2, -1, dtype=np.int32)
    for slot, (kind, idx, d) in enumerate(st):
        D["skind"][slot], D["sidx"][slot], D["sdir"][slot] = kind, idx, d
        lam = D["dl"][idx] if kind == 0 else e3[idx, d] if kind == 1 else D["eb"][d]
        D["sX"][slot] = lam - capv
        if kind == 0:
            D["slotl"][idx] = slot
        elif kind == 1:
            D["slot3"][idx, d] = slot
        else:
            D["slotb"][d // 2] = slot
    # the eigen form in float64 (soc3_eig_apply's formulas are one of many orders: the twin uses dense blocks)
    E3 = np.zeros((3, nq3, 3))
    if nq3:
        w1, w2 = e3[:, 3], e3[:, 4]
        E3[0] = np.stack([np.full(nq3, RS2), -w1 * RS2, -w2 * RS2], 1)
        E3[1] = np.stack([np.zeros(nq3), w2, -w1], 1)
        E3[2] = np.stack([np.full(nq3, RS2), w1 * RS2, w2 * RS2], 1)
    ebv = np.stack([np.concatenate([[RS2], -D["whb"] * RS2]), np.concatenate([[RS2], D["whb"] * RS2])]) if big else None

    def eig_apply(V, fo, f3, fb):
        out = np.empty_like(V)
        out[:l] = fo[:, None] * V[:l]
        if nq3:
            V3 = V[l:o3].reshape(nq3, 3, -1)
            a = 0
            for d in range(3):
                a = a + E3[d][:, :, None] * (f3[:, d, None] * np.einsum("ca,cak->ck", E3[d], V3))[:, None, :]
            out[l:o3] = a.reshape(3 * nq3, -1)
        if big:
            out[o3:] = fb[1] * V[o3:] + (fb[0] - fb[1]) * ebv[0][:, None] * (ebv[0] @ V[o3:])[None, :] + (fb[2] - fb[1]) * ebv[1][:, None] * (ebv[1] @ V[o3:])[None, :]
        return out
    fbc = np.array([min(D["eb"][0], capv), D["eb"][1], min(D["eb"][2], capv)]) if big else None
    inv2c = lambda V: eig_apply(V, D["dlc"], np.minimum(e3[:, :3], capv), fbc)
    w2 = lambda V: eig_apply(V, 1.0 / D["dl"], 1.0 / e3[:, :3], 1.0 / D["eb"][:3] if big else None)
    m3 = sum(np.minimum(e3[:, d], capv)[:, None, None] * E3[d][:, :, None] * E3[d][:, None, :] for d in range(3))
    D["m3c"] = m3[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]] if nq3 else np.zeros((0, 6))
    Um = np.full((max(kp, 64), npd), np.nan)
    Um[:kp] = 0.0
    Gr =L.G_ref(P, round_arg=True).astype(np.float64)
    for slot, (kind, idx, d) in enumerate(st):
        Um[slot, :N] = Gr[idx] if kind == 0 else E3[d][idx] @ Gr[l + 3 * idx:l + 3 * idx + 3] if kind == 1 else ebv[d // 2] @ Gr[o3:]
    D["U"] = Um
    H = np.eye(npd)
    Hw = Gm.T @ inv2c(Gm)
    H[:N, :N] = 0.5 * (Hw + Hw.T)
    D["H"] = H.copy()
    X = D["sX"][:k]
    if mutate:
        mutate("build", D)
        Um, st = D["U"], list(zip(D["skind"][:k].tolist(), D["sidx"][:k].tolist(), D["sdir"][:k].tolist()))
    if k and form == "cap":
        Lc = cholesky(H, lower=True)
        Mw = solve_triangular(Lc, np.eye(npd), lower=True)
        Yt = Um[:kp] @ Mw.T
        S = Yt @ Yt.T + np.diag(np.concatenate([1.0 / X, np.ones(kp - k)]))
        Ms = solve_triangular(cholesky(S, lower=True), np.eye(kp), lower=True)
        D.update(M=Mw, Hf=H, Yt=Yt, Zt=Yt @ Mw, S=S, Ms=Ms)
    elif k:
        Hh, Hl = np.ascontiguousarray(H), np.zeros_like(H)
        ddlin.rank_k(np.ascontiguousarray(Um[:k]), np.ascontiguousarray(X), Hh, Hl)
        ddlin.chol(Hh, Hl, 1e-28, np.diag(Hh).copy())
        D.update(M=Hl, Hf=Hh)
    D["pass"] = []
    nan = lambda *sh: np.full(sh, np.nan)
    BX, BZ = np.zeros((npd, nv)), bz.T.copy()
    BX[:N] = bx.T
    DX, DZ, GDX = np.zeros((N, nv)), np.zeros((R, nv)), np.zeros((R, nv))
    norms = []

    def comp(V):
        out = np.zeros((k, nv))
        for slot, (kind, idx, d) in enumerate(st):
            out[slot] = V[idx] if kind == 0 else E3[d][idx] @ V[l + 3 * idx:l + 3 * idx + 3] if kind == 1 else ebv[d // 2] @ V[o3:]
        return out

    def spread(Z):
        out = np.zeros((R, nv))
        for slot, (kind, idx, d) in enumerate(st):
            if kind == 0:
                out[idx] += Z[slot]
            elif kind == 1:
                out[l + 3 * idx:l + 3 * idx + 3] += E3[d][idx][:, None] * Z[slot][None, :]
            else:
                out[o3:] += ebv[d // 2][:, None] * Z[slot][None, :]
        return out
    for q in range(D["passes"] if k else 0):
        pq = dict(rhs_h=nan(nv, npd), rhs_l=nan(nv, npd), y=nan(nv, npd), bl=nan(nv, npd), capw=nan(nv, DD_KMAX), zeta=nan(nv, DD_KMAX), ts=nan(nv, DD_KMAX))
        gtdz = Gm.T @ DZ
        r1 = BX[:N] - gtdz
        norms.append(float(np.sqrt(add(r1 * r1)).max()))
        sc = nan(9)
        sc[:q + 1] = norms
        r2 = BZ - GDX + w2(DZ)
        t = comp(r2)
        wbz = inv2c(r2)
        gtw = Gm.T @ wbz
        pad = lambda a: np.concatenate([a.T, nan(nv, npd - N)], 1)
        pq.update(gtdz=pad(gtdz), r1=pad(r1), sc=sc, r2=r2.T.copy(), wbz=wbz.T.copy(), gtw=pad(gtw))
        pq["ts"][:, :k] = t.T
        if form == "cap":
            rw = np.zeros((npd, nv))
            rw[:N] = r1 + gtw
            y = D["M"].T @ (D["M"] @ rw)
            w = np.zeros((kp, nv))
            w[:k] = Um[:k, :N] @ y[:N] - t
            zeta = D["Ms"].T @ (D["Ms"] @ w)
            dxh = np.zeros((npd, nv))
            dxh[:N] = y[:N] - D["Zt"][:k, :N].T @ zeta[:k]
            pq.update(rhs_l=rw.T.copy(), y=y.T.copy(), bh=dxh.T.copy())
            pq["capw"][:, :kp], pq["zeta"][:, :kp] = w.T, zeta.T
            zs = zeta[:k]
        else:
            rh, rl = np.zeros((npd, nv)), np.zeros((npd, nv))
            rh[:N] = r1 + gtw                                   # (two_sum, as k_dd_rhs has it: the oracle rounds this sum)
            bb = rh[:N] - r1
            rl[:N] = (r1 - (rh[:N] - bb)) + (gtw - bb)
            yh, yl = ddlin.vec_mul_d(np.ascontiguousarray(t.ravel()), np.zeros(t.size), np.repeat(X, nv))
            ddlin.cols_times_acc(np.ascontiguousarray(Um[:k]), yh.reshape(-1, nv), yl.reshape(-1, nv), rh, rl)
            pq.update(rhs_h=rh.T.copy(), rhs_l=rl.T.copy())
            ddlin.cho_solve(D["Hf"], D["M"], rh, rl)
            uh, ul = ddlin.rows_times(np.ascontiguousarray(Um[:k]), rh, rl)
            uh, ul = ddlin.vec_sub(uh.ravel(), ul.ravel(), np.ascontiguousarray(t.ravel()), np.zeros(t.size))
            zh, zl = ddlin.vec_mul_d(uh, ul, np.repeat(X, nv))
            zs = (zh + zl).reshape(-1, nv)
            pq.update(bh=rh.T.copy(), bl=rl.T.copy())
            pq["zeta"][:, :k] = zs.T
            dxh = rh
        gbh = Gm @ dxh[:N]
        wbz2 = inv2c(gbh - r2)
        DZ = DZ + (wbz2 + spread(zs))
        GDX, DX = GDX + gbh, DX + dxh[:N]
        pq.update(gbh=gbh.T.copy(), wbz2=wbz2.T.copy(), dz=DZ.T.copy(), gdx=GDX.T.copy(), dx=pad(DX))
        pq["dx"][:, N:] = 0.0
        if mutate:
            mutate("pass%d" % q, pq)
        if nv == 1:
            pq = {key: (np.concatenate([v, np.full_like(v, np.nan)]) if key != "sc" else v) for key, v in pq.items()}
        D["pass"].append(pq)
    while len(D["pass"]) < 3:
        D["pass"].append(dict(sc=nan(9), **{key: nan(2, npd) for key in ("gtdz", "r1", "gtw", "rhs_h", "rhs_l", "y", "bh", "bl", "dx")},
                              **{key: nan(2, R) for key in ("r2", "wbz", "gbh", "wbz2", "dz", "gdx")}, **{key: nan(2, DD_KMAX) for key in ("ts", "capw", "zeta")}))
    two = lambda a, n: np.concatenate([a.T, nan(2 - nv, n)], 0)
    D["dx_end"], D["dz_end"], D["gdx_end"] = two(np.concatenate([DX, np.zeros((npd - N, nv))]), npd), two(DZ, R), two(GDX, R)
    D["sc_end"] = nan(9)
    D["sc_end"][:len(norms)] = norms
    return D
