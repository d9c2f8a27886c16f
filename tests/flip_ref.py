"""Reference of the root-flip search's arithmetic (csrc/flip.hip, k_flip_score) for mbfir.test_flip_stages, stage by stage.
tests/test_flipstages_gpu.py holds the device to it, tests/test_flipstages_cpu.py holds a float64 twin to a quarter of it and shows
that it rejects planted errors.  NumPy only (numpy.longdouble, 64-bit mantissa here); nothing here needs a GPU, and nothing is shared
with flip.hip, flipzero.py or oracle/slr.py.

What is computed (the header of flip.hip):
    build   coef = c0 (n - nz coefficients, leading first, zero-padded to n), then for j = 0, 1, .. nz-1:
            coef[k] -= r_j coef[k - 1] (k >= 1), r_j = zf[j] if factor j is flipped else z[j]
    scale   DC rule: beta = coef * target / sum(coef);  npoly rule: beta = coef / max_k |FFT_nn(coef)_k| * bsf, nn = 2^ceil(log2 n)
    bf      |fft(beta, 8n)|, times 1 / (1e-8 + max) when max >= 1
    xl      log(sqrt(1 - bf^2))
    xlfp    fft(xl)(0 : 4n), doubled except at 0 and 4n
    afa     exp(ifft(xlfp zero-extended to 8n))
    a       (fft(afa)(0 : n-1) / 8n) reversed
    theta   for i = n .. 1: q = b_i / a_i, c = 1 / sqrt(1 + |q|^2), s = conj(c q), theta_i = atan2(|s|, c) (|rf_i| = 2 theta_i),
            a <- (c a + s b)(2 : i), b <- (-conj(s) a + c b)(1 : i-1);   peak = 2 max_i theta_i

Transforms: every DFT here is a sum over twiddles exp(-2 pi i m / N) taken from a table built in long double by octant reduction
(the argument of sin / cos never exceeds pi / 4) and indexed by the integer (j k) mod N.  Lengths up to DIRECT are summed directly;
longer ones are split by their smallest prime factor p into p transforms of length N / p (decimation in time), down to direct
leaves.  `dft_direct` is the plain sum and the CPU tests hold the split to it.

Stage checks (`stage_fractions`).  Every stage after beta takes the DEVICE's (or twin's) output of the stage before it as exact
input, so a failure names one stage and each bound is that stage's own rounding, counted from the kernel's expressions with
u = 2^-53 and the reference's own magnitudes (first order in u).  The counting rules: one rounding costs u times the magnitude of
its result; a complex product costs 2 sqrt(2) u |x||y| in modulus (2 u per component: two products, one sum); a sum of K terms in
ANY order (the kernel's strided per-thread sums, wave and block trees) costs (K - 1) u times the sum of the terms' magnitudes; a table
twiddle (sincospi of an exactly representable argument) is within 2 u; hypot, log, exp, sincos, atan2, sqrt and division are
taken at 2 u, 1 u ... as listed.  Fused multiply-adds only remove roundings, so the count holds whatever the compiler contracts.
    beta   step j rounds coefficient k by at most l_j[k] = u (2 sqrt2 |r_j| |coef_j[k-1]| + |coef_{j+1}[k]|) (k >= 1), and the factors
           that follow carry it on linearly:  E = sum_j |T_j| * l_j, T_j = prod_{i > j} (x - r_i), * the convolution -- the running
           sum of the magnitudes of the intermediate coefficients, weighted by the tails they still pass through.  DC rule: the sum is off by dS = (n-1) u sum|coef| + sum E, the quotient by
           8 u, the product by 2 sqrt2 u:  |f| E + |beta| (dS / |S| + 8 u + 2 sqrt2 u).  npoly rule: each FFT_nn bin is off by
           (n + 6) u sum|coef| + sum E (+ 2 u for hypot), max is 1-Lipschitz, two roundings scale: E bsf / m + |beta| (dM / m + 2 u).
    bf     dA = (n + 5) u sum|beta| for a bin (n products, n - 1 additions, the twiddles), 2 u for hypot; with the clip three more
           roundings and the error dm = dA + 2 u m of the maximum:  sc (dA + 2 u |B|) + bf (4 u + dm sc), sc = 1 / (1e-8 + m).
    xl     t = 1 - bf^2 is off by u bf^2 + u t, so log(sqrt(t)) by half of that over t -- the factor 1 / (1 - bf^2) -- plus u for
           the square root and 2 u |xl| for the logarithm:  (u bf^2 / t + u) / 2 + u + 2 u |xl|.
    xlfp   eight sub-sums of n real x complex terms, then seven complex products and additions:  g (n + 16) u sum|xl|, g = 1 or 2.
    afa    sub-sums of at most n / 2 + 1 terms and the same combine, dAcc = (n / 2 + 18) u sum|xlfp|; the scale by 1 / 8n is two
           roundings, exp and sincos 2 u each, the product one:  |afa| (2 dAcc / 8n + 2 u (|re| + |im|) + 8 u).
    a      8n products and additions and the scale:  (8n + 5) u mean|afa| + 2 u |a|.
    theta  first-order propagation through the recursion, EA = EB = 0 at the start (a and beta are the device's own):
           dq = (EB_i + |q| EA_i) / |a_i| + 8 u |q|,  dc = c^3 |q| dq + 4 u c,  ds = c dq + |q| dc + u |s|,
           dtheta = c^2 dq + 6 u + 2 u theta,
           EA'[k-1] = c EA[k] + |s| EB[k] + dc |a_k| + ds |b_k| + 4 u (c |a_k| + |s| |b_k|),  EB' alike with c and s exchanged.
The peak of a candidate must equal 2 max_i theta_i of its own thetas exactly.

End to end (`chain`): the same stages run from the long-double beta without rounding in between, with the stage bounds carried
forward to first order (|d bf| <= sum E; d xl <= bf / (1 - bf^2) d bf; d xlfp <= g sum d xl; d afa <= |afa| mean-type sum of d xlfp;
d a <= mean d afa; the recursion started at EA = d a, EB = E).  This gives every candidate's peak a bound of its own, used for the
search launch's peaks and to decide whether a winner index may be compared: only where the reference's runner-up is further away
than the two peak bounds together.

What the inputs must satisfy for all this to mean something (`conditions`, asserted by the CPU tests for every case): the clip
decision is not within rounding of 1 (max|B| <= 0.99 or >= 1.5), every pivot |a_i| of the recursion is at least 1e-6 max|a|, and the
DC sum is at least 1e-3 sum|coef|.
"""
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
PI = LD("3.14159265358979323846264338327950288")
SQ2 = float(np.sqrt(2.0))
DIRECT = 192                      # transforms up to this length are summed directly
STAGES = ("beta", "bf", "xl", "xlfp", "afa", "a", "theta")
CLIP_LOW, CLIP_HIGH, PIVOT_MIN, DC_MIN = 0.99, 1.5, 1e-6, 1e-3


# ---- transforms ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def tw_ld(N):
    """exp(-2 pi i m / N), m = 0 .. N-1, in long double: the angle is k pi / 2 +- t with t in [0, pi / 4] by integer arithmetic."""
    m = np.arange(N, dtype=np.int64)
    q, rem = np.divmod(8 * m, N)
    odd = (q & 1) == 1
    rem = np.where(odd, N - rem, rem)
    t = PI / 4 * rem.astype(LD) / LD(N)
    c, s = np.cos(t), np.sin(t)
    s = np.where(odd, -s, s)
    k = ((q + 1) // 2) & 3
    cr = np.select([k == 0, k == 1, k == 2], [c, -s, -c], s)
    sr = np.select([k == 0, k == 1, k == 2], [s, c, -s], -c)
    w = np.empty(N, dtype=CLD)
    w.real, w.imag = cr, -sr
    w.setflags(write=False)
    return w


def dft_direct(x, sign=-1, kout=None):
    """X[k] = sum_j x[j] exp(sign 2 pi i j k / N) over the last axis, the plain sum with exact integer phases."""
    x = np.asarray(x, dtype=CLD)
    N = x.shape[-1]
    k = np.arange(N if kout is None else kout, dtype=np.int64)
    w = tw_ld(N)
    W = w[(np.arange(N, dtype=np.int64)[:, None] * k[None, :]) % N]
    return x @ (W if sign < 0 else np.conj(W))


def _smallest_factor(N):
    p = 2
    while p * p <= N:
        if N % p == 0:
            return p
        p += 1
    return N


def dft_ld(x, sign=-1):
    """The same transform, split by the smallest prime factor while the length exceeds DIRECT."""
    x = np.asarray(x, dtype=CLD)
    N = x.shape[-1]
    p = _smallest_factor(N)
    if N <= DIRECT or p == N:
        return dft_direct(x, sign)
    M = N // p
    k = np.arange(N, dtype=np.int64)
    w = tw_ld(N) if sign < 0 else np.conj(tw_ld(N))
    out = np.zeros(x.shape, dtype=CLD)
    for r in range(p):
        out += w[(r * k) % N] * dft_ld(x[..., r::p], sign)[..., k % M]
    return out


def _pad(x, N):
    out = np.zeros(x.shape[:-1] + (N,), dtype=CLD)
    out[..., :x.shape[-1]] = x
    return out


# ---- candidates ---------------------------------------------------------------------------------------------------------------
def enum_flips(nz, ncand, enum_bits=None):
    """flips[c, j] of the enumerated candidates: bit (e_j >> 1) of c equals e_j & 1; default e_j = (nz - 1 - j) << 1."""
    eb = np.asarray([(nz - 1 - j) << 1 for j in range(nz)] if enum_bits is None else enum_bits, dtype=np.int64).reshape(nz)
    c = np.arange(ncand, dtype=np.int64)[:, None]
    return (((c >> (eb >> 1)[None, :]) & 1) == (eb & 1)[None, :]).astype(np.int64)


def build(case, flips, reverse=False, dtype=CLD):
    """The candidates of `flips` (B x nz) after the build and the scale rule, with the counted bound of the kernel's build (B x n) and
    the DC ratio |sum coef| / sum|coef|.  dtype complex128 is the float64 twin (reverse: factors multiplied on in reverse order)."""
    c0 = np.asarray(case["c0"], dtype=np.complex128)
    z, zf = np.asarray(case["z"], dtype=np.complex128), np.asarray(case["zf"], dtype=np.complex128)
    nz, n = len(z), len(c0) + len(z)
    flips = np.asarray(flips)
    B = flips.shape[0]
    flips = flips.reshape(B, nz)
    coef = np.zeros((B, n), dtype=dtype)
    coef[:, :len(c0)] = c0
    order = list(range(nz - 1, -1, -1) if reverse else range(nz))
    roots, local = [], []
    for j in order:
        r = np.where(flips[:, j] == 1, zf[j], z[j]).astype(dtype)
        new = coef.copy()
        new[:, 1:] -= r[:, None] * coef[:, :-1]
        loc = np.zeros((B, n))
        loc[:, 1:] = U * (2 * SQ2 * np.abs(r)[:, None] * np.abs(coef[:, :-1]) + np.abs(new[:, 1:])).astype(np.float64)
        roots.append(r)
        local.append(loc)
        coef = new
    E = np.zeros((B, n))                                   # each step's rounding, carried through the factors that follow it
    tail = np.ones((B, 1), dtype=dtype)
    for j in range(nz - 1, -1, -1):
        ta = np.abs(tail).astype(np.float64)
        for m in range(min(tail.shape[1], n)):
            E[:, m:] += ta[:, m:m + 1] * local[j][:, :n - m]
        nt = np.zeros((B, tail.shape[1] + 1), dtype=dtype)
        nt[:, :-1] = tail
        nt[:, 1:] -= roots[j][:, None] * tail
        tail = nt
    A1 = np.abs(coef).sum(axis=1).astype(np.float64)
    S = coef.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        dc_ratio = np.abs(S).astype(np.float64) / A1
        if case["rule"] == 0:
            f = dtype(case["target"]) / S
            beta = coef * f[:, None]
            dS = (n - 1) * U * A1 + E.sum(axis=1)
            fa = np.abs(f).astype(np.float64)[:, None]
            bound = fa * E + np.abs(beta).astype(np.float64) * (dS / np.abs(S).astype(np.float64) + (8 + 2 * SQ2) * U)[:, None]
        else:
            nn = 1
            while nn < n:
                nn <<= 1
            F = np.fft.fft(coef, nn, axis=1) if dtype is np.complex128 else dft_ld(_pad(coef, nn))
            m = np.abs(F).max(axis=1)
            mf = m.astype(np.float64)
            scale = (LD(case["bsf"]) if dtype is CLD else case["bsf"]) / m
            beta = coef * scale[:, None]
            dM = (n + 6) * U * A1 + E.sum(axis=1) + 2 * U * mf
            bound = E * (case["bsf"] / mf)[:, None] + np.abs(beta).astype(np.float64) * (dM / mf + 2 * U)[:, None]
    return beta, bound, dc_ratio


# ---- the chain, one stage at a time (inputs: the stage before, any precision; outputs long double) ------------------------------
def ref_bf(beta, clip_eps=1e-8):
    beta = np.asarray(beta, dtype=CLD)
    n = beta.shape[-1]
    F = np.abs(dft_ld(_pad(beta, 8 * n)))
    m = F.max(axis=-1, keepdims=True)
    clipped = m >= 1
    sc = np.where(clipped, 1 / (LD(clip_eps) + m), LD(1))
    bf = F * sc
    A1 = np.abs(beta).sum(axis=-1, keepdims=True)
    dA = (n + 5) * U * A1
    plain = dA + 2 * U * F
    clip = sc * plain + bf * (4 * U + (dA + 2 * U * m) * sc)
    return bf, np.where(clipped, clip, plain).astype(np.float64), m[..., 0].astype(np.float64)


def ref_xl(bf):
    bf = np.asarray(bf, dtype=LD)
    t = (1 - bf) * (1 + bf)
    xl = np.log(t) / 2
    return xl, (0.5 * (U * bf * bf / t + U) + U + 2 * U * np.abs(xl)).astype(np.float64)


def ref_xlfp(xl):
    xl = np.asarray(xl, dtype=LD)
    N = xl.shape[-1]
    n = N // 8
    g = np.full(4 * n + 1, 2.0)
    g[0] = g[4 * n] = 1.0
    X = dft_ld(xl.astype(CLD))[..., :4 * n + 1] * g
    bound = g * ((n + 16) * U * np.abs(xl).sum(axis=-1, keepdims=True)).astype(np.float64)
    return X, bound


def ref_afa(xlfp):
    xlfp = np.asarray(xlfp, dtype=CLD)
    n = (xlfp.shape[-1] - 1) // 4
    N = 8 * n
    w = dft_ld(_pad(xlfp, N), sign=+1) / N
    afa = np.exp(w.real) * (np.cos(w.imag) + 1j * np.sin(w.imag))
    dAcc = (n / 2 + 18) * U * np.abs(xlfp).sum(axis=-1, keepdims=True)
    bound = np.abs(afa) * (2 * dAcc / N + 2 * U * (np.abs(w.real) + np.abs(w.imag)) + 8 * U)
    return afa, bound.astype(np.float64)


def ref_a(afa):
    afa = np.asarray(afa, dtype=CLD)
    N = afa.shape[-1]
    n = N // 8
    a = (dft_ld(afa)[..., :n] / N)[..., ::-1]
    bound = (N + 5) * U * np.abs(afa).mean(axis=-1, keepdims=True) + 2 * U * np.abs(a)
    return a, bound.astype(np.float64)


def ref_theta(a, beta, EA=None, EB=None, want_rf=False):
    """theta (B x n, theta[:, i - 1] of step i), its bound, and the smallest pivot ratio |a_i| / max|a| over the steps."""
    A = np.atleast_2d(np.asarray(a, dtype=CLD)).copy()
    Bp = np.atleast_2d(np.asarray(beta, dtype=CLD)).copy()
    nb, n = A.shape
    EA = np.zeros((nb, n), dtype=LD) if EA is None else np.asarray(EA, dtype=LD).copy()
    EB = np.zeros((nb, n), dtype=LD) if EB is None else np.asarray(EB, dtype=LD).copy()
    amax = np.abs(A).max(axis=1)
    theta, dth = np.zeros((nb, n), dtype=LD), np.zeros((nb, n))
    rf, drf = np.zeros((nb, n), dtype=CLD), np.zeros((nb, n))
    pivot = np.full(nb, np.inf)
    for i in range(n, 0, -1):
        ai, bi = A[:, i - 1], Bp[:, i - 1]
        pivot = np.minimum(pivot, (np.abs(ai) / amax).astype(np.float64))
        q = bi / ai
        qa = np.abs(q)
        c = 1 / np.sqrt(1 + qa * qa)
        s = np.conj(c * q)
        sa = np.abs(s)
        th = np.arctan2(sa, c)
        dq = (EB[:, i - 1] + qa * EA[:, i - 1]) / np.abs(ai) + 8 * U * qa
        dc = c ** 3 * qa * dq + 4 * U * c
        ds = c * dq + qa * dc + U * sa
        theta[:, i - 1] = th
        dth[:, i - 1] = (c * c * dq + 6 * U + 2 * U * th).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            unit = np.where(sa > 0, s / sa, 1)             # slr.hip: rf_i = 2 theta (cos psi + i sin psi), psi = atan2(s.y, s.x)
            lever = np.where(sa > 0, th / sa, 1)           # theta / sin(theta) <= pi / 2: the phase error of s as an error of rf
        rf[:, i - 1] = 2 * th * unit
        drf[:, i - 1] = (2 * dth[:, i - 1] + 2 * lever * ds + 2 * th * 16 * U).astype(np.float64)
        aa, ba = np.abs(A[:, :i]), np.abs(Bp[:, :i])
        cc, ss, dcc, dss = c[:, None], sa[:, None], dc[:, None], ds[:, None]
        nEA = cc * EA[:, :i] + ss * EB[:, :i] + dcc * aa + dss * ba + 4 * U * (cc * aa + ss * ba)
        nEB = ss * EA[:, :i] + cc * EB[:, :i] + dss * aa + dcc * ba + 4 * U * (ss * aa + cc * ba)
        An = c[:, None] * A[:, :i] + s[:, None] * Bp[:, :i]
        Bn = -np.conj(s)[:, None] * A[:, :i] + c[:, None] * Bp[:, :i]
        A[:, :i - 1], Bp[:, :i - 1] = An[:, 1:], Bn[:, :i - 1]
        EA[:, :i - 1], EB[:, :i - 1] = nEA[:, 1:], nEB[:, :i - 1]
    if want_rf:
        return rf, drf, pivot
    return theta, dth, pivot


def stage_fractions(got, case=None, flips=None):
    """got: the stages of B candidates as float64 arrays (st_beta .. st_theta, st_peak).  Every stage's worst |got - ref| / bound,
    the reference taken from got's own stage before (beta: from the case, when given).  Also the conditions the inputs must meet."""
    out, cond = {}, {}
    frac = lambda g, r, b: float(np.max(np.abs(np.asarray(g, dtype=r.dtype) - r).astype(np.float64) / b))      # noqa: E731
    if case is not None:
        beta, bb, dc = build(case, flips)
        out["beta"] = frac(got["st_beta"], beta, bb)
        cond["dc_ratio"] = float(dc.min()) if case["rule"] == 0 else 1.0
    bf, b, m = ref_bf(got["st_beta"])
    out["bf"], cond["maxB"] = frac(got["st_bf"], bf, b), m
    xl, b = ref_xl(got["st_bf"])
    out["xl"] = frac(got["st_xl"], xl, b)
    X, b = ref_xlfp(got["st_xl"])
    out["xlfp"] = frac(got["st_xlfp"], X, b)
    afa, b = ref_afa(got["st_xlfp"])
    out["afa"] = frac(got["st_afa"], afa, b)
    a, b = ref_a(got["st_afa"])
    out["a"] = frac(got["st_a"], a, b)
    th, b, piv = ref_theta(got["st_a"], got["st_beta"])
    out["theta"], cond["pivot"] = frac(got["st_theta"], th, b), float(piv.min())
    return out, cond


def conditions_ok(cond):
    m = np.asarray(cond["maxB"])
    return bool(np.all((m <= CLIP_LOW) | (m >= CLIP_HIGH))) and cond["pivot"] >= PIVOT_MIN and cond.get("dc_ratio", 1.0) >= DC_MIN


def chain(case, flips):
    """End to end from the long-double beta: peak and its first-order bound per candidate (and the stages, for the curious)."""
    beta, Eb, _ = build(case, flips)
    n = beta.shape[-1]
    N = 8 * n
    bf, b_bf, m = ref_bf(beta)
    mm = m[:, None]
    clipped = mm >= 1
    sc = np.where(clipped, 1 / (1e-8 + mm), 1.0)
    sumE = Eb.sum(axis=1, keepdims=True)
    bff = bf.astype(np.float64)
    d_bf = b_bf + sc * sumE * np.where(clipped, 1.0 + bff, 1.0)
    # the clipped maximum itself is m / (1e-8 + m): the bin's error and the maximum's are one number and all but cancel
    d_m = (n + 5) * U * np.abs(beta).sum(axis=1, keepdims=True).astype(np.float64) + 2 * U * mm + sumE
    at_max = clipped & (bff == bff.max(axis=1, keepdims=True))
    d_bf = np.where(at_max, 4 * U + sc * (1 - bff) * d_m, d_bf)
    xl, b_xl = ref_xl(bf)
    d_xl = b_xl + bff / (1 - bff * bff) * d_bf
    X, b_X = ref_xlfp(xl)
    g = np.full(4 * n + 1, 2.0)
    g[0] = g[4 * n] = 1.0
    d_X = b_X + g * d_xl.sum(axis=1, keepdims=True)
    afa, b_afa = ref_afa(X)
    d_afa = b_afa + np.abs(afa).astype(np.float64) * d_X.sum(axis=1, keepdims=True) / N
    a, b_a = ref_a(afa)
    d_a = b_a + d_afa.mean(axis=1, keepdims=True)
    th, d_th, piv = ref_theta(a, beta, EA=d_a, EB=Eb)
    return dict(beta=beta, bf=bf, xl=xl, xlfp=X, afa=afa, a=a, theta=th, peak=2 * th.max(axis=1).astype(np.float64),
                peak_bound=2 * d_th.max(axis=1), maxB=m, pivot=piv)


# ---- the same chain as slr.hip runs it (k_dft_any / wg_dft, k_slr_logmag, k_slr_exp, ab2rf_recursion), end to end -----------------
ROT = 5 * 255 + 2          # a twiddle after at most 255 rotations from an exact seed: 2 u, plus (2 sqrt2 + 2) u < 5 u per rotation


def slr_chain(b):
    """mbfir.b2a / ab2rf / b2rf / b2rf_batch have no hook, so they are held end to end: the long-double chain from the caller's beta
    (exact input), the bounds recounted for those kernels' own sums and carried forward to first order.  A direct sum of N terms
    whose twiddles come from a rotation recurrence reseeded exactly every 256 terms is off by (N + 3 + ROT) u sum|x|: N - 1
    additions, the product, and the worst twiddle.  k_slr_logmag scales re and im (not the modulus) and sums the squares: five
    roundings on |bf|^2 before the subtraction.  Returns a, its bound, rf = ab2rf(a, b), its bound (the recursion started at
    EA = the bound of a), and rf's bound when a is given exactly (mbfir.ab2rf of a float64 a: ref_theta alone)."""
    b = np.atleast_2d(np.asarray(b, dtype=CLD))
    n = b.shape[-1]
    N = 8 * n
    K = (N + 3 + ROT) * U
    F = dft_ld(_pad(b, N))
    Fa = np.abs(F)
    m = Fa.max(axis=-1, keepdims=True)
    clipped = m >= 1
    sc = np.where(clipped, 1 / (LD(1e-8) + m), LD(1))
    bf = (Fa * sc).astype(np.float64)
    scf, mf = sc.astype(np.float64), m.astype(np.float64)
    D1 = K * np.abs(b).sum(axis=-1, keepdims=True).astype(np.float64)
    dm = D1 + 2 * U * mf
    d_bf = np.where(clipped, scf * D1 + bf * (3 * U + dm * scf), D1)
    d_bf = np.where(clipped & (bf == bf.max(axis=-1, keepdims=True)), 4 * U + scf * (1 - bf) * dm, d_bf)
    t = ((1 - Fa * sc) * (1 + Fa * sc))
    xl = np.log(t) / 2
    tf = t.astype(np.float64)
    d_xl = 0.5 * (2 * bf * d_bf + 5 * U * bf * bf + U * tf) / tf + U + 2 * U * np.abs(xl).astype(np.float64)
    g = np.full(4 * n + 1, 2.0)
    g[0] = g[4 * n] = 1.0
    X = dft_ld(xl.astype(CLD))[..., :4 * n + 1] * g
    d_X = g * (K * np.abs(xl).sum(axis=-1, keepdims=True).astype(np.float64) + d_xl.sum(axis=-1, keepdims=True))
    w = dft_ld(_pad(X, N), sign=+1) / N
    d_w = (K * np.abs(X).sum(axis=-1, keepdims=True).astype(np.float64) + d_X.sum(axis=-1, keepdims=True)) / N \
        + 2 * U * np.abs(w).astype(np.float64)
    afa = np.exp(w.real) * (np.cos(w.imag) + 1j * np.sin(w.imag))
    afa_abs = np.abs(afa).astype(np.float64)
    d_afa = afa_abs * (2 * d_w + 8 * U)
    a = (dft_ld(afa)[..., :n] / N)[..., ::-1]
    d_a = (K * afa_abs.sum(axis=-1, keepdims=True) + d_afa.sum(axis=-1, keepdims=True)) / N + 2 * U * np.abs(a).astype(np.float64)
    rf, d_rf, piv = ref_theta(a, b, EA=d_a, want_rf=True)
    return dict(a=a, d_a=d_a, rf=rf, d_rf=d_rf, maxB=mf[..., 0], pivot=piv)


def slr_input(n, level, seed, real=False):
    """A beta of n taps with max|B| = level on the 8n grid: a windowed sinc under a ramp, times a few factors off the circle."""
    nz = min(6, n - 1)
    case = make_case(n, nz, "real" if real else "complex", 0, level, seed)
    beta = build(case, pick_flips(case, 2, seed)[1:])[0][0]
    return beta.astype(np.complex128)


def reference_winner(peaks, bounds, flips, tie_high=False):
    """(index, decided): the reference's winner -- among the candidates with the best one's flip pattern (the same polynomial, so the
    same bits on the device) the lowest index, or the highest with tie_high -- and whether it is decided: the best candidate of any
    other pattern further away than the two peak bounds together."""
    flips = np.asarray(flips).reshape(len(peaks), -1)
    best = int(np.argmin(peaks))
    same = np.all(flips == flips[best], axis=1)
    idx = np.nonzero(same)[0]
    win = int(idx.max() if tie_high else idx.min())
    if same.all():
        return win, True
    other = np.nonzero(~same)[0]
    ru = other[np.argmin(peaks[other])]
    return win, bool(peaks[ru] - peaks[best] > bounds[ru] + bounds[best])


# ---- the float64 twin: the same algorithm on NumPy's FFT (another summation order), with switches that plant errors ---------------
PLANTS = ("window4n", "kmax", "edge", "conj", "clip", "order")


def twin(case, flips, plant=None):
    """Every stage in float64, each computed from the twin's own stage before: the dict stage_fractions takes."""
    beta = build(case, flips, reverse=plant == "order", dtype=np.complex128)[0]
    return twin_chain(beta, plant)


def _log_sqrt_one_minus_sq(a):
    """log(sqrt(1 - a^2)) with the square's rounding error put back (Veltkamp / Dekker split) and the logarithm itself taken in
    long double: the xl bound is the kernel's own three roundings and one ulp of the logarithm, so a plain float64 evaluation of the
    same expression has no factor of four to spare."""
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    hi = a * a
    lo = ((ah * ah - hi) + 2 * ah * al) + al * al
    return (0.5 * (np.log1p(-hi.astype(LD)) - lo / (1 - hi))).astype(np.float64)


def twin_chain(beta, plant=None):
    beta = np.atleast_2d(np.asarray(beta, dtype=np.complex128))
    B, n = beta.shape
    N = 8 * n
    F = np.abs(np.fft.fft(beta, N, axis=1))
    m = F.max(axis=1, keepdims=True)
    bf = F * np.where(m >= 1.0, 1.0 / ((1e-7 if plant == "clip" else 1e-8) + m), 1.0)
    xl = _log_sqrt_one_minus_sq(bf)
    g = np.full(4 * n + 1, 2.0)
    g[0] = 1.0
    g[4 * n] = 2.0 if plant == "window4n" else 1.0
    xlfp = np.fft.fft(xl, axis=1)[:, :4 * n + 1] * g
    X = np.zeros((B, N), dtype=np.complex128)
    X[:, :4 * n + 1] = xlfp
    if plant == "kmax":                                    # each sub-sum one term short: the last input of every residue class
        X[:, 4 * n - 7:4 * n + 1] = 0
    afa = np.exp(np.fft.ifft(X, axis=1))
    a = (np.fft.fft(afa, axis=1)[:, :n] / N)[:, ::-1].copy()
    A, Bp = a.copy(), beta.copy()
    theta = np.zeros((B, n))
    for i in range(n, 0, -1):
        q = Bp[:, i - 1] / A[:, i - 1]
        c = np.sqrt(1.0 / (1.0 + np.abs(q) ** 2))
        s = c * q if plant == "conj" else np.conj(c * q)
        theta[:, i - 1] = np.arctan2(np.abs(s), c)
        An = c[:, None] * A[:, :i] + s[:, None] * Bp[:, :i]
        Bn = -np.conj(s)[:, None] * A[:, :i] + c[:, None] * Bp[:, :i]
        keep = i - 2 if plant == "edge" else i - 1         # the last kept coefficient of b left as it was
        A[:, :i - 1] = An[:, 1:]
        Bp[:, :max(keep, 0)] = Bn[:, :max(keep, 0)]
    return dict(st_beta=beta, st_bf=bf, st_xl=xl, st_xlfp=xlfp, st_afa=afa, st_a=a, st_theta=theta, st_peak=2 * theta.max(axis=1))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_case(n, nz, kind, rule, level, seed, criterion="rf"):
    """c0: a windowed sinc of n - nz coefficients under a ramp (complex kind: modulated); nz flip factors spread round the circle at radius
    0.85 .. 0.95, every other one outside (complex), or on the real axis with alternating sign (real).  Kind "ordered": half the
    factors near +1, then half near -1 -- in this order the intermediate coefficients stay below the final ones, in the reverse
    order they pass through values 2^(nz / 2) times larger, so the build's order shows in the result far above its bound.  DC rule: the target puts
    max|B| on the kernel's 8n grid at `level` for every candidate (a flip scales |B(w)| by a constant, the DC rule takes it out);
    npoly rule: bsf = level."""
    rng = np.random.default_rng(seed)
    n0 = n - nz
    t = np.arange(n0) - (n0 - 1) / 2
    c0 = (np.sinc(t / 8) * np.hamming(n0) if n0 > 2 else np.array([1.0, 0.6])[:n0]).astype(np.complex128)
    c0 = c0 * (1 + 0.4 * (t + 0.5) / n0)                  # not symmetric: flipping every factor is no mirror image of the whole
    if kind == "complex":
        c0 = c0 * np.exp(0.07j * (t + 1.5))
        z = rng.uniform(0.85, 0.95, nz) * np.exp(2j * np.pi * (np.arange(nz) + rng.uniform(0.2, 0.8, nz)) / max(nz, 1))
        z = np.where(np.arange(nz) % 2 == 1, 1 / np.conj(z), z)
        bits = max(nz - 1, 1).bit_length()                 # van der Corput order of the angles: partial products stay small
        z = z[np.argsort([int(format(j, "0%db" % bits)[::-1], 2) for j in range(nz)], kind="stable")]
    elif kind == "ordered":                               # differencing factors first, summing factors last: see make_case
        z = np.concatenate([rng.uniform(0.85, 0.95, nz // 2), -rng.uniform(0.85, 0.95, nz - nz // 2)]).astype(np.complex128)
    else:
        z = (rng.uniform(0.5, 0.9, nz) * np.where(np.arange(nz) % 2 == 0, -1.0, 1.0)).astype(np.complex128)
    zf = 1 / np.conj(z)
    case = dict(n=n, nz=nz, c0=c0, z=z, zf=zf, rule=rule, criterion=criterion, kind=kind, level=level)
    if rule == 1:
        case["bsf"] = float(level)
    else:
        case.update(rule=1, bsf=1.0)
        b0 = build(case, np.zeros((1, nz), dtype=int))[0][0]
        case.pop("bsf")
        mx = np.abs(dft_ld(_pad(b0, 8 * n))).max()
        case.update(rule=0, target=complex(LD(level) * b0.sum() / mx))
    return case


def pick_flips(case, ncand, seed):
    """ncand explicit mask columns (B x nz), the first all-unflipped."""
    rng = np.random.default_rng(seed)
    f = (rng.random((ncand, case["nz"])) < 0.5).astype(np.int64)
    f[0] = 0
    return f


# name: (n, nz, kind, rule, level, candidates) -- candidates "enum" (all 2^nz, enum_bits NULL), "bits" (64 enumerated through given
# enum_bits), "masks" (16 explicit columns).  Every n, nz, kind, rule, level and candidate form of the issue's list occurs.
STAGE_CASES = {
    "n2_nz0": (2, 0, "complex", 0, 0.5, "enum"),
    "n2_nz1_real": (2, 1, "real", 0, 0.985, "enum"),
    "n3_nz1": (3, 1, "complex", 1, 0.5, "masks"),
    "n3_nz2_real_clip": (3, 2, "real", 0, 1.7, "bits"),
    "n8_nz0": (8, 0, "real", 1, 0.9, "enum"),
    "n8_nz7": (8, 7, "complex", 0, 0.5, "masks"),
    "n8_nz3": (8, 3, "complex", 1, 0.9, "enum"),
    "n8_nz1_real": (8, 1, "real", 0, 0.985, "masks"),
    "n44_ordered": (44, 20, "ordered", 1, 0.9, "masks"),
    "n63_nz31": (63, 31, "complex", 0, 0.985, "masks"),
    "n63_nz62": (63, 62, "complex", 1, 0.5, "masks"),
    "n64_nz32_clip": (64, 32, "complex", 0, 1.7, "masks"),
    "n64_nz33": (64, 33, "complex", 1, 0.9, "bits"),
    "n65_nz33": (65, 33, "complex", 0, 0.985, "masks"),
    "n65_nz1_real": (65, 1, "real", 1, 0.5, "enum"),
    "n65_nz64": (65, 64, "complex", 0, 0.5, "masks"),
    "n130_nz32": (130, 32, "complex", 0, 0.985, "masks"),
    "n130_nz0": (130, 0, "complex", 1, 0.9, "enum"),
    "n130_nz129_clip": (130, 129, "complex", 0, 1.7, "masks"),
}
NSEL = 8


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """(case, flips of every candidate (ncand x nz), call keywords for mbfir.test_flip_stages, selected candidate indices)."""
    n, nz, kind, rule, level, cand = STAGE_CASES[name]
    seed = 100 + sorted(STAGE_CASES).index(name)
    case = make_case(n, nz, kind, rule, level, seed)
    if cand == "enum":
        flips, kw = enum_flips(nz, 2 ** nz), {}
    elif cand == "bits":
        eb = [((j % 6) << 1) | (j & 1) for j in range(nz)]
        flips, kw = enum_flips(nz, 64, eb), dict(enum_bits=eb, ncand=64)
    else:
        flips = pick_flips(case, 16, seed)
        kw = dict(masks=flips.T.copy())
    ncand = flips.shape[0]
    sel = np.unique(np.linspace(0, ncand - 1, min(NSEL, ncand)).astype(np.int64))
    return case, flips, kw, sel


def size_case(n, seed=7):
    """The case of a mode-threshold size: 16 flip factors on a windowed sinc, npoly rule at 0.7, 8 explicit masks."""
    case = make_case(n, 16 if n > 17 else n - 1, "complex", 1, 0.7, seed + n)
    flips = pick_flips(case, 8, seed + n)
    return case, flips


def call_args(case):
    kw = dict(criterion=case["criterion"])
    if case["rule"] == 0:
        kw["target"] = case["target"]
    else:
        kw["bsf"] = case["bsf"]
    return (case["c0"], case["z"], case["zf"]), kw


# ---- the mode a search chooses, restated from flip_search_run -----------------------------------------------------------------
def mode_of(n, lds_limit):
    nn = 1
    while nn < n:
        nn <<= 1
    red, work, tabs = 16 * 16, (14 * n + 1) * 16, (8 * n + nn) * 16
    return 0 if red + work + tabs <= lds_limit else 1 if red + work <= lds_limit else 2


def mode_sizes(lds_limit, nmax=1024):
    """largest n of mode 0, smallest and largest of mode 1, smallest of mode 2 (None where a mode does not occur up to nmax)."""
    modes = np.array([mode_of(n, lds_limit) for n in range(2, nmax + 1)])
    ns = np.arange(2, nmax + 1)
    pick = lambda m, f: int(f(ns[modes == m])) if np.any(modes == m) else None          # noqa: E731
    return dict(last0=pick(0, np.max), first1=pick(1, np.min), last1=pick(1, np.max), first2=pick(2, np.min))
