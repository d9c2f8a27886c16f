"""References of the capacitance form of the extended-precision KKT solve (capkkt.hip and the chol.hip kernels that consume its
output), for mbfir.test_capsolve: tests/test_capkkt_gpu.py holds the device to them, tests/test_capkkt_cpu.py shows that they
reject what they should.  Everything here is NumPy (float64 and numpy.longdouble, 64-bit mantissa here), SciPy's triangular solves
and oracle/ddlin.c; nothing needs a GPU.

One problem is  (H_w + U' X U) dx = (a + b) + U' X t,  H_w n x n SPD, U k x n, X = diag of k weights, solved by block elimination
on H_w:  M = chol(H_w)^-1,  Yt = U M',  Zt = Yt M,  S = Yt Yt' + X^-1,  Ms = chol(S)^-1,  rhs_w = a + b,  y = M'(M rhs_w),
w = U y - t,  zeta = Ms'(Ms w),  dx = y - Zt' zeta.  The device pads n to np (multiple of 64: identity rows of H_w, zero columns
of U) and k to kp (zero rows of U / Yt / Zt, unit diagonal of S).

(a) Stage checks (`stage_checks`), numpy.longdouble.  Every stage takes the DEVICE's output of the stages before it as exact
input, so a failure names one kernel and the bound follows from that kernel's summation alone.  u = 2^-53, gamma(K) = K u / (1 - K u),
all bounds componentwise:
    Yt     | U M'                 | gamma(np + 8) |U| |M|'                        | rows >= k exactly 0
    Zt     | Yt M                 | gamma(np + 8) |Yt| |M|                        | rows >= k exactly 0
    S      | Yt Yt' + diag(1 / X) | gamma(np + 8) |Yt| |Yt|' + 2 u diag(1 / X)    | lower tiles; padding: diagonal exactly 1, rest exactly 0
    rhs_w  | a + b                | u |a + b|                                     | entries n .. np-1 exactly 0
    y      | M'(M rhs_w)          | 3 gamma(np + 40) |M|'(|M| |rhs_w|)            |
    w      | U y - t              | gamma(n + 8) (|U| |y| + |t|)                  | rows k .. kp-1 exactly 0
    zeta   | Ms'(Ms w)            | 3 gamma(kp + 40) |Ms|'(|Ms| |w|)              |
    dx     | y - Zt' zeta         | gamma(k + 40) (|Zt|' |zeta| + |y|)            | entries n .. np-1 exactly 0
M and Ms are read through their lower triangle only (the products mask the diagonal tile, the solves rely on exact zeros there, which
the "M" / "Ms" stages assert).  Where the constants come from: a sum of K terms accumulated by fused multiply-adds in any order has
an error of at most gamma(K) times the sum of the terms' magnitudes.  The products are sums of at most np terms (a tile's K range
in four contiguous parts on the matrix cores, the masked entries exact zeros), + 8 covers the fold of the four parts (k_cap_fold: four
additions to 0.0), the diagonal term of S and its reciprocal.  The vector kernels sum n resp. k terms in 64 (k_cap_uy: one wave, a
6-step wave tree) resp. 32 (k_cap_dx: DXG groups folded serially) interleaved partial sums and subtract once; M'(M b) is two
dependent sums of at most np terms each -- the inner one a wave tree, the outer one spread over 4 waves (LDS, 3 additions) and
HS_PARTS = 32 partial vectors (32 additions) -- so the inner sum's error enters the outer one: (1 + g)^2 - 1 + g < 3 g with
g = gamma(np + 40); + 40 >= 6 + 3 + 32 covers the wave, LDS and 32-partial trees (the GEMV pair has the wave trees only).
M and Ms themselves are held to the bounds test_cholesky_and_inverse states for this factorisation: |M L - I| <= 1e-11 with
NumPy's factor L, exact zeros above the diagonal in the diagonal tiles, and |H x - c| <= 1e-10 |c| for x = M'(M c).

(b) End to end (`dd_solution`, `restate_solve`): dx against the double-double solution of the UN-eliminated system by oracle/ddlin.c
(rank_k, chol, cho_solve), the right-hand side formed in long double and split into (hi, lo).  The tolerance of a case is 16 x the
error of `restate_solve` -- the same block elimination in float64 NumPy / SciPy, with triangular substitutions where the device
multiplies by explicit inverses -- against that solution.

Inputs (`family`): H_w = B'B with B (n + 30) x n standard normal, U standard normal with INDEPENDENT rows, X = 10^uniform(8, 16),
t = 0 or N(0, 1) / X.  The tests assert what the reference itself needs of them: the restatement's S positive definite with
cond(S) <= 1e6 and the restatement within 1e-12 of the double-double solution.  (Nearly dependent rows of U make S indefinite in
float64 from k ~ 130 on, t of order 1e-3 leaves the answer to the refinement passes of the solver, which the hook does not run.)
"""
import numpy as np
import scipy.linalg as sla

U_ROUND = 2.0 ** -53
LD = np.longdouble
TB = 64
STAGES = ("M", "Yt", "Zt", "S", "Ms", "rhs_w", "y", "w", "zeta", "dx")
# the tolerances of tests/test_kernels_gpu.py test_cholesky_and_inverse
CHOL_INV_TOL, CHOL_RESID_TOL = 1e-11, 1e-10
E2E_FACTOR = 16.0
COND_S_MAX, RESTATE_TOL = 1e6, 1e-12


def gamma(K):
    return K * U_ROUND / (1.0 - K * U_ROUND)


def pad64(n):
    return -(-n // TB) * TB


def family(n, k, nrhs, t_mode, seed=None):
    """One problem of the input family.  t_mode: "zero" or "scaled" (N(0, 1) / X)."""
    rng = np.random.default_rng(1000 * n + k if seed is None else seed)
    B = rng.standard_normal((n + 30, n))
    H = B.T @ B
    H = 0.5 * (H + H.T)
    U = rng.standard_normal((k, n))
    X = 10.0 ** rng.uniform(8, 16, k)
    a, b = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
    tn = rng.standard_normal((nrhs, k))
    t = np.zeros((nrhs, k)) if t_mode == "zero" else tn / X
    return {"n": n, "k": k, "H": H, "U": U, "X": X, "a": a, "b": b, "t": t}


def pack(problems, kp):
    """The problems (same n and nrhs) as the padded arrays mbfir.test_capsolve takes: (H, U, X, a, b, t, k)."""
    n, nv = problems[0]["n"], problems[0]["a"].shape[0]
    nl = len(problems)
    H, U, X = np.zeros((nl, n, n)), np.zeros((nl, kp, n)), np.ones((nl, kp))
    a, b, t = np.zeros((nl, nv, n)), np.zeros((nl, nv, n)), np.zeros((nl, nv, kp))
    for q, p in enumerate(problems):
        k = p["k"]
        H[q], a[q], b[q] = p["H"], p["a"], p["b"]
        U[q, :k], X[q, :k], t[q, :, :k] = p["U"], p["X"], p["t"]
    return H, U, X, a, b, t, [p["k"] for p in problems]


def lane(out, q):
    """Lane q of what mbfir.test_capsolve returned."""
    return {name: v[q] for name, v in out.items()}


def _pad_inputs(p, kp):
    n, k = p["n"], p["k"]
    npad, nv = pad64(n), p["a"].shape[0]
    Hp = np.eye(npad)
    Hp[:n, :n] = p["H"]
    Up = np.zeros((kp, npad))
    Up[:k, :n] = p["U"]
    ap, bp, tp = np.zeros((nv, npad)), np.zeros((nv, npad)), np.zeros((nv, kp))
    ap[:, :n], bp[:, :n], tp[:, :k] = p["a"], p["b"], p["t"]
    return Hp, Up, ap, bp, tp


def restate(p, kp, mutate=None):
    """The device's algorithm in float64 NumPy with explicit inverses, in the padded layout mbfir.test_capsolve returns (one lane;
    the tiles above the diagonal of M, S, Ms hold NaN as the hook leaves them).  mutate(stage, out, inputs), if given, is called
    after every stage and may alter what that stage left in `out`: the later stages go on from the altered values, as the
    device's would (tests/test_capkkt_cpu.py); inputs: the padded (H, U, a, b, t)."""
    n, k = p["n"], p["k"]
    inputs = _pad_inputs(p, kp)
    Hp, Up, ap, bp, tp = inputs
    out = {}

    def stage(name, value):
        out[name] = value
        if mutate is not None:
            mutate(name, out, inputs)
        return out[name]

    stage("M", np.tril(sla.solve_triangular(np.linalg.cholesky(Hp), np.eye(len(Hp)), lower=True)))
    M = np.tril(out["M"])                                      # (the products mask the diagonal tile)
    Yt = stage("Yt", Up @ M.T)
    Zt = stage("Zt", Yt @ M)
    S = Yt @ Yt.T
    S[np.arange(kp), np.arange(kp)] += np.concatenate([1.0 / p["X"], np.ones(kp - k)])
    S = stage("S", S)
    Ssym = np.tril(S) + np.tril(S, -1).T
    Ms = np.tril(stage("Ms", np.tril(sla.solve_triangular(np.linalg.cholesky(Ssym), np.eye(kp), lower=True))))
    rhs = stage("rhs_w", ap + bp)
    y = stage("y", (M.T @ (M @ rhs.T)).T)
    w = (Up @ y.T).T - tp
    w[:, k:] = 0.0
    w = stage("w", w)
    zeta = stage("zeta", (Ms.T @ (Ms @ w.T)).T)
    dx = y - (Zt.T @ zeta.T).T
    dx[:, n:] = 0.0
    stage("dx", dx)
    for name in ("M", "S", "Ms"):
        A = out[name]
        tiles = np.arange(len(A)) // TB
        A[tiles[None, :] > tiles[:, None]] = np.nan
    return out


def restate_solve(p):
    """The same block elimination in float64 with substitutions instead of explicit inverses (unpadded): (dx, S)."""
    L = np.linalg.cholesky(p["H"])
    rhs = (p["a"] + p["b"]).T
    y = sla.cho_solve((L, True), rhs)
    Zt = sla.cho_solve((L, True), p["U"].T).T
    Yt = sla.solve_triangular(L, p["U"].T, lower=True).T
    S = Yt @ Yt.T + np.diag(1.0 / p["X"])
    w = p["U"] @ y - p["t"].T
    zeta = sla.cho_solve((np.linalg.cholesky(S), True), w)
    return (y - Zt.T @ zeta).T, S


def dd_solution(p):
    """(H_w + U' X U)^-1 ((a + b) + U' X t) in double-double (oracle/ddlin.c), as a long double array (nrhs, n)."""
    from oracle import ddlin
    n = p["n"]
    rhs = (p["a"].astype(LD) + p["b"].astype(LD)) + (p["X"].astype(LD) * p["t"].astype(LD)) @ p["U"].astype(LD)
    hi = rhs.astype(np.float64)
    lo = (rhs - hi.astype(LD)).astype(np.float64)
    Hh, Hl = np.ascontiguousarray(p["H"], dtype=np.float64).copy(), np.zeros((n, n))
    ddlin.rank_k(np.ascontiguousarray(p["U"]), np.ascontiguousarray(p["X"]), Hh, Hl)
    d0 = np.diag(Hh).copy()
    assert ddlin.chol(Hh, Hl, 1e-28, d0) == 0, "the double-double factorisation replaced a pivot"
    Bh, Bl = np.ascontiguousarray(hi.T), np.ascontiguousarray(lo.T)
    ddlin.cho_solve(Hh, Hl, Bh, Bl)
    return Bh.T.astype(LD) + Bl.T.astype(LD)


def relmax(x, ref):
    return float(np.abs(x.astype(LD) - ref).max() / np.abs(ref).max())


def end_to_end(p, dx):
    """dx (nrhs, n) against the double-double solution: (error of dx, error of the float64 restatement, cond of its S, S is SPD)."""
    ref = dd_solution(p)
    rs, S = restate_solve(p)
    ev = np.linalg.eigvalsh(S)
    return relmax(dx, ref), relmax(rs, ref), float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf, bool(ev[0] > 0)


class Report:
    """fractions: stage -> worst error as a fraction of its bound; failures: (stage, what) pairs."""

    def __init__(self):
        self.fractions, self.failures = {}, []

    def fail(self, stage, what):
        self.failures.append((stage, what))

    def failed_stages(self):
        return sorted({s for s, _ in self.failures}, key=STAGES.index)

    def bounded(self, stage, got, ref, bound):
        got = np.asarray(got)
        if not np.isfinite(got).all():
            self.fail(stage, "not finite")
            self.fractions[stage] = np.inf
            return
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        bound = np.asarray(bound, dtype=np.float64)
        frac = float(np.max(np.where(err == 0.0, 0.0, err / np.where(bound > 0.0, bound, np.finfo(float).tiny))))
        self.fractions[stage] = max(self.fractions.get(stage, 0.0), frac)
        if frac > 1.0:
            i = np.unravel_index(np.argmax(err - bound), err.shape)
            self.fail(stage, "entry %s off by %.3g, bound %.3g (%.3g of the bound at worst)" % (i, err[i], bound[i], frac))

    def exact(self, stage, got, want, what):
        got = np.asarray(got)
        if got.size and not np.array_equal(got, np.broadcast_to(want, got.shape)):
            self.fail(stage, what)


def _inverse_factor(rep, stage, A, Minv):
    """Minv (lower tiles valid) as the inverse Cholesky factor of the symmetric A: test_cholesky_and_inverse's bounds."""
    q = len(A)
    tiles = np.arange(q) // TB
    if not np.isfinite(Minv[np.tril_indices(q)]).all():
        rep.fail(stage, "not finite in the lower triangle")
        return
    same_tile_above = (tiles[None, :] == tiles[:, None]) & (np.arange(q)[None, :] > np.arange(q)[:, None])
    rep.exact(stage, Minv[same_tile_above], 0.0, "nonzero above the diagonal inside a diagonal tile")
    M = np.tril(Minv)
    L = np.linalg.cholesky(A)
    e_inv = float(np.abs(M @ L - np.eye(q)).max())
    c = np.random.default_rng(q).standard_normal(q)
    e_res = float(np.linalg.norm(A @ (M.T @ (M @ c)) - c) / np.linalg.norm(c))
    rep.fractions[stage] = max(e_inv / CHOL_INV_TOL, e_res / CHOL_RESID_TOL)
    if e_inv > CHOL_INV_TOL:
        rep.fail(stage, "|M L - I| = %.3g > %.3g" % (e_inv, CHOL_INV_TOL))
    if e_res > CHOL_RESID_TOL:
        rep.fail(stage, "|A x - c| / |c| = %.3g > %.3g" % (e_res, CHOL_RESID_TOL))


def stage_checks(p, kp, out, stages=STAGES):
    """Hold one lane's intermediates `out` (padded, as mbfir.test_capsolve returns them) to the stage bounds of this file's
    docstring; p: the problem, kp: the size the launches carried.  Returns a Report."""
    n, k = p["n"], p["k"]
    npad = pad64(n)
    Hp, Up, ap, bp, tp = _pad_inputs(p, kp)
    rep = Report()
    g_prod = gamma(npad + 8)
    fin = {name: bool(np.isfinite(np.tril(out[name]) if name in ("M", "S", "Ms") else out[name]).all()) for name in STAGES}
    # (np.tril: the lower triangle with zeros elsewhere -- what the kernels make of the inverse factors)
    Ml, Msl = np.tril(out["M"]), np.tril(out["Ms"])
    Yt, Zt = out["Yt"], out["Zt"]

    def ready(stage, *needs):
        bad = [x for x in needs if not fin[x]]
        if bad:
            rep.fail(stage, "input %s is not finite" % bad[0])
        return not bad

    if "M" in stages:
        _inverse_factor(rep, "M", Hp, out["M"])
    if "Yt" in stages and ready("Yt", "M"):
        rep.bounded("Yt", Yt[:k], Up[:k].astype(LD) @ Ml.T.astype(LD), g_prod * (np.abs(Up[:k]) @ np.abs(Ml).T))
        rep.exact("Yt", Yt[k:], 0.0, "a padding row is not exactly zero")
    if "Zt" in stages and ready("Zt", "M", "Yt"):
        rep.bounded("Zt", Zt[:k], Yt[:k].astype(LD) @ Ml.astype(LD), g_prod * (np.abs(Yt[:k]) @ np.abs(Ml)))
        rep.exact("Zt", Zt[k:], 0.0, "a padding row is not exactly zero")
    if "S" in stages and ready("S", "Yt"):
        S = out["S"]
        tiles = np.arange(kp) // TB
        low = tiles[None, :] <= tiles[:, None]                                  # the lower tiles, diagonal tiles whole
        core = low & (np.arange(kp)[:, None] < k) & (np.arange(kp)[None, :] < k)
        xinv = np.concatenate([1.0 / p["X"].astype(LD), np.zeros(kp - k, dtype=LD)])
        ref = Yt.astype(LD) @ Yt.T.astype(LD) + np.diag(xinv)
        bound = g_prod * (np.abs(Yt) @ np.abs(Yt).T) + 2.0 * U_ROUND * np.diag(xinv.astype(np.float64))
        rep.bounded("S", S[core], ref[core], bound[core])
        pad = low & ~core
        rep.exact("S", S[pad], np.eye(kp)[pad], "padding: the diagonal is not exactly 1 or another entry not exactly 0")
    if "Ms" in stages and ready("Ms", "S"):
        Ssym = np.tril(out["S"]) + np.tril(out["S"], -1).T
        _inverse_factor(rep, "Ms", Ssym, out["Ms"])
    if "rhs_w" in stages:
        s = ap.astype(LD) + bp.astype(LD)
        rep.bounded("rhs_w", out["rhs_w"][:, :n], s[:, :n], U_ROUND * np.abs(s[:, :n]).astype(np.float64))
        rep.exact("rhs_w", out["rhs_w"][:, n:], 0.0, "an entry past n is not exactly zero")

    def two_sided(stage, Minv, b, got, K):
        bl = b.astype(LD)
        ref = (Minv.T.astype(LD) @ (Minv.astype(LD) @ bl.T)).T
        bound = 3.0 * gamma(K + 40) * (np.abs(Minv).T @ (np.abs(Minv) @ np.abs(b).T)).T
        rep.bounded(stage, got, ref, bound)

    if "y" in stages and ready("y", "M", "rhs_w"):
        two_sided("y", Ml, out["rhs_w"], out["y"], npad)
    if "w" in stages and ready("w", "y"):
        y = out["y"]
        ref = (Up[:k, :n].astype(LD) @ y[:, :n].T.astype(LD)).T - tp[:, :k].astype(LD)
        bound = gamma(n + 8) * ((np.abs(Up[:k, :n]) @ np.abs(y[:, :n]).T).T + np.abs(tp[:, :k]))
        rep.bounded("w", out["w"][:, :k], ref, bound)
        rep.exact("w", out["w"][:, k:], 0.0, "a padding row is not exactly zero")
    if "zeta" in stages and ready("zeta", "Ms", "w"):
        two_sided("zeta", Msl, out["w"], out["zeta"], kp)
    if "dx" in stages and ready("dx", "Zt", "zeta", "y"):
        y, zeta = out["y"], out["zeta"]
        ref = y[:, :n].astype(LD) - (Zt[:k, :n].T.astype(LD) @ zeta[:, :k].T.astype(LD)).T
        bound = gamma(k + 40) * ((np.abs(Zt[:k, :n]).T @ np.abs(zeta[:, :k]).T).T + np.abs(y[:, :n]))
        rep.bounded("dx", out["dx"][:, :n], ref, bound)
        rep.exact("dx", out["dx"][:, n:], 0.0, "an entry past n is not exactly zero")
    return rep
