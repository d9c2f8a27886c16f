"""Reference of the Parks-McClellan exchange of csrc/remez.hip, iterate by iterate (DESIGN.md sections 8e and 8e-1): plain NumPy
longdouble, dense, restated from the description of the algorithm and not from the kernel.  tests/test_remezstages_cpu.py checks
this file on the host, tests/test_remezstages_gpu.py holds the kernel against it.

How the iterates are seen.  With maxiter = k the kernel returns the extremal set it solved on in iteration k (`ext`, as
frequencies), that iteration's delta and the taps of that iteration's interpolant.  `check_sweep` takes the runs maxiter = 1 .. K_s
of one spec (K_s = the iteration at which the long-double replay repeats its set) and checks, for every k: the start set (k = 1),
status and iteration count, delta_k against solve(ext_k), ext_{k+1} against exchange(solve(ext_k)) index for index, h_k against
taps(ext_k) and its exact symmetry, and the alternation certificate at K_s.  Every check raises a *named* assertion (`Miss.name`),
so the host test can tell which one caught a planted change.

Bounds.  u = 2^-53; each is a count of roundings times u times the sum of absolute terms, on the reference's own magnitudes.

  delta.  gamma_k is a product of n1 - 1 factors 2 (x_k - x_j), an inverse and exact scalings: counted at n1 + 2 roundings.  The
      numerator sum gamma_k D_k is summed in double-double, so it carries only the weights' error, (n1 + 2) u sum |gamma_k D_k|;
      the denominator sum gamma_k (-1)^k / W_k has terms of one sign: (n1 + 2 + 16) u relative (its quotient and a 256-way sum).
      The node data is not exact either: f may differ by an ulp (lo + i delf contracted into an fma or not), cos(pi f) and, for
      type II, cos(pi f / 2) by an ulp, D by five roundings.  To first order a residual r_k in the k-th interpolation condition
      moves delta by gamma_k r_k / den, so that part is sum |gamma_k| r_k / |den| with
      r_k = eD_k + |delta| e(1 / W_k) + |P'(x_k)| ex_k.  The envelope is reported relative to |delta|, with its amplification
      sum |gamma D| / |sum gamma D| beside it.
  E.  The second barycentric form: every term gamma_k / (x - x_k) C_k carries n1 + 2 + 4 roundings and the two sums n1 more, so
      |dA| <= (2 n1 + 6) u (sum |t_k C_k| + |A| sum |t_k|) / |sum t_k|, plus the interpolant's response to the node errors
      r_k + env_delta / W_k (the same sum with |t_k| as weights), plus the grid point's own x.  E = W (D - A) adds W eD and
      three roundings.  It is computed only where an exchange differs (the near-tie allowance).
  taps.  The kernel recovers them in double-double from its fp64 grid data (weights, a delta and node values of their own, the
      sampling of the interpolant), so what remains is the response of the interpolant to the node data.  Three parts: the error
      on the 2L - 1 point cosine grid, sum_k |l_k(y)| (3 u (|D_k| + |delta / W_k|) + r_k) with l_k the Lagrange functions, plus
      |Q(y)| env_delta for the spurious degree-L part that an error of delta leaves behind (Q the interpolant of (-1)^k / W_k),
      plus the point's own x and the rounding of P; the O(L) cosine transform, (L + 4) u (2 / M) sum |P_j|; and the tap formulas
      (3 u).  `taps_envelope` returns it.  Measured on the host (test_remezstages_cpu.py prints it): over the 208 (spec,
      iteration) pairs it lies a median of 120 times above what the restatement achieves, within two decades in 43 % of the pairs
      and up to 7000 times above (the sums over |l_k| and the worst-case delta are patterns that roundings do not form), and as a
      first-order estimate it is itself exceeded where delta is tiny (w1e4_101, iterations 1 and 2: delta = 1e-7).  THE TAPS
      THEREFORE USE THE FALLBACK BOUND: ten times the distance of the restatement (`Kern64`, below) from the long-double
      reference for the same spec and extremal set, with the floor 1e-15 max|h| (`taps_bound`).  Ten because the restatement and
      the kernel sum in different orders.
"""
import importlib.util
import math
import os

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI = LD("3.14159265358979323846264338327950288")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    path = os.path.join(ROOT, "tests", "golden", "make_golden_conventional.py")
    sp = importlib.util.spec_from_file_location("make_golden_conventional", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    return mod


gold = _generator()
dense_grid, amplitude = gold.grid, gold.amplitude


class Miss(AssertionError):
    """A named check of check_sweep that did not hold."""

    def __init__(self, name, *what):
        super().__init__("%s: %s" % (name, " ".join(str(w) for w in what)))
        self.name = name


def need(ok, name, *what):
    if not ok:
        raise Miss(name, *what)


# ---- the certificate (moved here from tests/test_conventional_gpu.py) ---------------------------------------------------------
def weighted_error(h, f, numtaps, edges, desired, weight):
    """E = W (D - A) at frequencies f (Nyquist units), A from the taps, D / W of the band each f lies in."""
    f = np.asarray(f, dtype=np.float64)
    A = amplitude(h, f)
    D, W = np.zeros(len(f)), np.zeros(len(f))
    for b in range(len(weight)):
        lo, hi = edges[2 * b], edges[2 * b + 1]
        m = (f >= lo) & (f <= hi)
        D[m] = desired[2 * b] + (desired[2 * b + 1] - desired[2 * b]) * ((f[m] - lo) / (hi - lo) if hi > lo else 0)
        W[m] = weight[b]
    return W * (D - A)


# The certificate resolves |E| to 1e-8 |delta|.  The tolerance dates from the fp64 tap recovery, whose sampling of the interpolant
# carried about 1e-13 absolute error where the extremal set leaves gaps (transition bands): weighted by W / delta it reached 5.8e-9
# |delta| on the device for lp519_w300 (W = 300) and the sloped design.  With the double-double recovery
# the device stays below 5e-10 on every fixture and on the spec with a weight ratio of 1e4.
CERT_TOL = 1e-8


def certify(h, info, numtaps, edges, desired, weight, tol=CERT_TOL, density=16):
    """Optimality on the grid, from the taps alone: the L + 1 returned frequencies alternate with |E| = |delta|, and no grid
    point exceeds |delta|."""
    L, f, D, W, B = dense_grid(numtaps, edges, desired, weight, density)
    ad = abs(info["delta"])
    Ee = weighted_error(h, info["ext"], numtaps, edges, desired, weight)
    assert len(Ee) == L + 1
    assert np.all(np.abs(np.abs(Ee) - ad) <= tol * ad), np.abs(np.abs(Ee) - ad).max() / ad
    assert np.all(np.sign(Ee[1:]) != np.sign(Ee[:-1]))
    E = W * (D - amplitude(h, f))
    assert np.abs(E).max() <= ad * (1 + tol), np.abs(E).max() / ad - 1


# ---- the grid -----------------------------------------------------------------------------------------------------------
class Grid:
    pass


def half_len(numtaps):
    return (numtaps + 1) // 2 if numtaps % 2 else numtaps // 2


def grid(numtaps, edges, desired, weight, density=16, keep_f1=False):
    """The dense grid: per band max(1, int((hi - lo) / delf + 0.5)) points lo + i delf, the last one moved onto hi, delf =
    1 / (density L).  f is fp64 (it defines the grid); x = cos(pi f), D and W are long double, for type II divided / multiplied by
    cos(pi f / 2), and f = 1 is dropped only when the last edge is 1.  eD, eIW (relative, of 1 / W) and ex are the node-data
    errors of the module docstring."""
    g = Grid()
    g.numtaps, g.density, g.type2 = int(numtaps), int(density), numtaps % 2 == 0
    g.spec = (int(numtaps), [float(v) for v in edges], [float(v) for v in desired], [float(v) for v in weight])
    L = g.L = half_len(numtaps)
    g.n1 = L + 1
    delf = 1.0 / (density * L)
    f, D, W, B, S, starts = [], [], [], [], [], [0]
    for b in range(len(weight)):
        lo, hi = float(edges[2 * b]), float(edges[2 * b + 1])
        k = max(1, int((hi - lo) / delf + 0.5))
        fb = lo + np.arange(k) * delf
        fb[-1] = hi
        d0, d1 = LD(float(desired[2 * b])), LD(float(desired[2 * b + 1]))
        t = (fb.astype(LD) - LD(lo)) / (LD(hi) - LD(lo)) if hi > lo else np.zeros(k, dtype=LD)
        f.append(fb)
        D.append(d0 + (d1 - d0) * t)
        W.append(np.full(k, float(weight[b]), dtype=LD))
        B.append(np.full(k, b))
        S.append(np.full(k, abs(float(d1 - d0)) / (hi - lo) if hi > lo else 0.0))
        starts.append(starts[-1] + k)
    f, D, W, B, S = (np.concatenate(v) for v in (f, D, W, B, S))
    if g.type2 and float(edges[-1]) == 1.0 and not keep_f1:
        f, D, W, B, S = f[:-1], D[:-1], W[:-1], B[:-1], S[:-1]
        starts[-1] -= 1
    fl = f.astype(LD)
    g.f, g.band, g.starts, g.G = f, B, np.array(starts), len(f)
    g.x = np.cos(PI * fl)
    df = 2 * U * f
    relc = np.zeros(g.G)
    if g.type2:
        c = np.cos(PI * fl / 2)
        D, W = D / c, W * c
        S = S / np.abs(c).astype(np.float64)
        relc = (math.pi / 2) * np.abs(np.tan(PI * fl / 2)).astype(np.float64) * df + 2 * U
    g.D, g.W = D, W
    g.eD = np.abs(D).astype(np.float64) * (5 * U + relc) + S * df
    g.eIW = relc + 2 * U
    g.ex = 2 * U * np.abs(g.x).astype(np.float64) + math.pi * np.sin(math.pi * f) * df
    return g


def start_set(G, L):
    return np.array([(k * (G - 1)) // L for k in range(L + 1)])


def index_of(g, f_dev):
    """Grid indices of returned frequencies: the nearest grid point each (device code may contract lo + i delf into an fma, so the
    grids can differ by an ulp), every distance at most 4 ulp of f, indices strictly ascending."""
    f_dev = np.asarray(f_dev, dtype=np.float64)
    need(len(f_dev) == g.n1 and np.all(np.isfinite(f_dev)), "ext", "length or non-finite", len(f_dev))
    j = np.clip(np.searchsorted(g.f, f_dev), 1, g.G - 1)
    j = np.where(np.abs(g.f[j - 1] - f_dev) <= np.abs(g.f[j] - f_dev), j - 1, j)
    dist = np.abs(g.f[j] - f_dev)
    need(np.all(dist <= 4 * np.spacing(np.maximum(np.abs(f_dev), 1e-300))), "ext", "not a grid point", dist.max())
    need(np.all(np.diff(j) > 0), "ext", "indices not strictly ascending")
    return j


# ---- one iteration ---------------------------------------------------------------------------------------------------------
class Sol:
    pass


def _bary(xq, x, gam, C):
    """The interpolant at xq (second barycentric form; on a node its value C_k), and the terms t_k = gamma_k / (xq - x_k)."""
    d = xq[:, None] - x[None, :]
    hit = d == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        t = gam[None, :] / np.where(hit, LD(1), d)
    t[hit.any(axis=1)] = 0
    t[hit] = 1
    return (t @ C) / t.sum(axis=1), t


def solve(g, ext, sign=1):
    """Barycentric weights, delta, node values C and E on the whole grid for the extremal set ext (grid indices); on the nodes E is
    exactly (-1)^k delta.  Also the envelope of delta (absolute: env_delta; relative: env_rel; amplification: amp)."""
    s = Sol()
    s.g, s.ext = g, np.asarray(ext)
    n1 = len(s.ext)
    x, D, W = g.x[s.ext], g.D[s.ext], g.W[s.ext]
    d = x[:, None] - x[None, :]
    np.fill_diagonal(d, LD(0.5))
    gam = 1 / np.prod(2 * d, axis=1)
    gam = gam / np.abs(gam).max()
    sg = sign * np.where(np.arange(n1) % 2, LD(-1), LD(1))
    num, den = (gam * D).sum(), (gam * sg / W).sum()
    s.delta = num / den
    s.x, s.gam, s.sg = x, gam, sg
    s.C = D - sg * s.delta / W
    A, _ = _bary(g.x, x, gam, s.C)
    s.E = g.W * (g.D - A)
    s.E[s.ext] = sg * s.delta
    # P'(x_k) on the nodes (barycentric differentiation)
    np.fill_diagonal(d, LD(1))
    q = (gam[None, :] / gam[:, None]) * (s.C[None, :] - s.C[:, None]) / d
    np.fill_diagonal(q, LD(0))
    dP = np.abs(q.sum(axis=1)).astype(np.float64)
    ag = np.abs(gam).astype(np.float64)
    s.r = g.eD[s.ext] + abs(float(s.delta)) * g.eIW[s.ext] / np.abs(W).astype(np.float64) + dP * g.ex[s.ext]
    cg = n1 + 2
    sabs = float(np.abs(gam * D).sum())
    s.amp = sabs / max(abs(float(num)), 1e-4000)
    s.env_delta = (cg * U * sabs + float((ag * s.r).sum())) / abs(float(den)) + abs(float(s.delta)) * (cg + 17) * U
    s.env_rel = s.env_delta / abs(float(s.delta))
    return s


def _response(s, xq, ex_q):
    """(P, envelope of P) at the points xq whose own x carries ex_q: the E / taps part 1 formula of the module docstring."""
    n1 = len(s.ext)
    P, t = _bary(xq, s.x, s.gam, s.C)
    at = np.abs(t)
    st = np.abs(t.sum(axis=1))
    dC = (s.r + s.env_delta / np.abs(s.g.W[s.ext]).astype(np.float64)).astype(LD)
    h = LD(1e-9)
    dP = np.abs(_bary(xq + h, s.x, s.gam, s.C)[0] - _bary(xq - h, s.x, s.gam, s.C)[0]) / (2 * h)
    env = (2 * n1 + 6) * U * (at @ np.abs(s.C) + np.abs(P) * at.sum(axis=1)) / st + (at @ dC) / st + dP * ex_q
    return P, env.astype(np.float64)


def e_envelope(s):
    """Envelope of E on the whole grid (module docstring); zero on the nodes, where E is delta by definition."""
    g = s.g
    _, envP = _response(s, g.x, g.ex)
    env = np.abs(g.W).astype(np.float64) * (envP + g.eD) + np.abs(s.E).astype(np.float64) * (g.eIW + 3 * U)
    env[s.ext] = s.env_delta
    return env


def candidates(g, E, delta):
    """Pass 1: in-band local extrema with |E| >= |delta| (>= towards the left neighbour, > towards the right; a band's first and
    last point have no neighbour on that side)."""
    G = len(E)
    sE = np.where(E > 0, E, -E)
    ok = (sE >= abs(delta)) & (E != 0)
    sgn = np.where(E > 0, 1, -1)
    first = np.zeros(G, dtype=bool)
    last = np.zeros(G, dtype=bool)
    first[g.starts[:-1]] = True
    last[g.starts[1:] - 1] = True
    left = np.ones(G, dtype=bool)
    left[1:] = sgn[1:] * E[1:] >= sgn[1:] * E[:-1]
    right = np.ones(G, dtype=bool)
    right[:-1] = sgn[:-1] * E[:-1] > sgn[:-1] * E[1:]
    return np.nonzero(ok & (first | left) & (last | right))[0]


def exchange(g, E, delta, first_of_equal=True):
    """The three passes: candidates; the largest of each run of equal sign (the first of equal ones); trim to L + 1 by dropping the
    smaller end, the high end on a tie.  None when fewer than L + 1 survive."""
    cand = candidates(g, E, delta)
    alt = []
    for j in cand:
        if alt and (E[alt[-1]] > 0) == (E[j] > 0):
            if abs(E[j]) > abs(E[alt[-1]]) or (not first_of_equal and abs(E[j]) == abs(E[alt[-1]])):
                alt[-1] = j
        else:
            alt.append(j)
    if len(alt) < g.n1:
        return None
    lo, hi = 0, len(alt) - 1
    while hi - lo > g.L:
        if abs(E[alt[lo]]) < abs(E[alt[hi]]):
            lo += 1
        else:
            hi -= 1
    return np.array(alt[lo:hi + 1])


def _tap_formulas(a, L, type2, shift=0):
    """Cosine coefficients a_0 .. a_{L-1} to taps: type I h[L-1] = a_0, h[L-1 +- k] = a_k / 2; type II b_1 = a_0 + a_1 / 2,
    b_n = (a_{n-1} + a_n) / 2, b_L = a_{L-1} / 2, h[L-n] = h[L-1+n] = b_n / 2."""
    if not type2:
        return np.concatenate([a[:0:-1] / 2, a[:1], a[1:] / 2])
    b = np.zeros(L + 1, dtype=a.dtype)
    for n in range(1, L + 1):
        if n == 1:
            b[n] = a[0] + (a[1] / 2 if L > 1 else 0)
        elif n < L:
            b[n] = (a[n - 1 - shift] + a[n - shift]) / 2
        else:
            b[n] = a[L - 1] / 2
    return np.concatenate([b[:0:-1] / 2, b[1:] / 2])


def taps(s):
    """Taps of the interpolant of s: sampled on the 2L - 1 point cosine grid, inverse cosine transform, tap formulas; long double."""
    L = s.g.L
    M = 2 * L - 1
    j = np.arange(L)
    P, _ = _bary(np.cos(2 * PI * j.astype(LD) / M), s.x, s.gam, s.C)
    ck = np.cos(2 * PI * ((j[:, None] * j[None, :]) % M).astype(LD) / M)
    a = (P[0] + 2 * (ck[:, 1:] @ P[1:])) / M
    a[1:] *= 2
    return _tap_formulas(a, L, s.g.type2)


def taps_envelope(s):
    """The three-part envelope of the taps (module docstring), absolute."""
    g, L = s.g, s.g.L
    M = 2 * L - 1
    y = np.cos(2 * PI * np.arange(L).astype(LD) / M)
    P, t = _bary(y, s.x, s.gam, s.C)
    ell = np.abs(t / t.sum(axis=1)[:, None]).astype(np.float64)
    W = np.abs(g.W[s.ext]).astype(np.float64)
    dC = 3 * U * (np.abs(g.D[s.ext]).astype(np.float64) + abs(float(s.delta)) / W) + s.r
    Q = np.abs(_bary(y, s.x, s.gam, s.sg / g.W[s.ext])[0]).astype(np.float64)
    h = LD(1e-9)
    dP = (np.abs(_bary(y + h, s.x, s.gam, s.C)[0] - _bary(y - h, s.x, s.gam, s.C)[0]) / (2 * h)).astype(np.float64)
    aP = np.abs(P).astype(np.float64)
    envP = ell @ dC + Q * s.env_delta + dP * 2 * U * np.abs(y).astype(np.float64) + U * aP
    e_a = (2.0 / M) * (envP[0] + 2 * envP[1:].sum()) + (L + 4) * U * (2.0 / M) * (aP[0] + 2 * aP[1:].sum())
    return 0.5 * e_a * (1 + 3 * U) + 3 * U * float(np.abs(taps(s)).max())


# ---- the fp64 restatement of the kernel's arithmetic -------------------------------------------------------------------------
def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp / Dekker)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _block_sum(v, threads=256):
    """A sum in the order of the kernel's 256-thread reduction: thread t adds its entries t, t + 256, ... in turn, each wave of 64
    folds by strides 32, 16, .. 1, and the four waves are added in turn."""
    pd = np.zeros(threads)
    for j0 in range(0, len(v), threads):
        c = v[j0:j0 + threads]
        pd[:len(c)] = pd[:len(c)] + c
    w = pd.reshape(-1, 64).copy()
    o = 32
    while o:
        w[:, :o] = w[:, :o] + w[:, o:2 * o]
        o //= 2
    t = 0.0
    for x in w[:, 0]:
        t = t + x
    return float(t)


class Kern64:
    """The kernel's arithmetic in NumPy fp64: grid data in fp64, weights scaled by frexp every 16 factors, the numerator of delta
    summed exactly (the kernel: double-double), its denominator in the order of the kernel's block reduction (so that delta, and
    with it the node values C, come out with the kernel's own roundings wherever the grid data agree bit for bit), E by the second barycentric form in fp64, the taps from weights and barycentric
    sums in long double (the kernel: double-double) and the cosine transform in fp64.  `mut`
    plants one of the changes of tests/test_remezstages_cpu.py: 'pass2', 'start', 'keep_f1', 'sign', 'tapshift'."""

    def __init__(self, numtaps, edges, desired, weight, density=16, mut=None):
        self.mut = mut
        g = self.g = grid(numtaps, edges, desired, weight, density, keep_f1=mut == "keep_f1")
        self.f = g.f
        self.x = g.x.astype(np.float64)                       # cospi: the correctly rounded value
        D, W = np.zeros(g.G), np.zeros(g.G)
        for b in range(len(weight)):
            m = g.band == b
            lo, hi = float(edges[2 * b]), float(edges[2 * b + 1])
            d0, d1 = float(desired[2 * b]), float(desired[2 * b + 1])
            D[m] = d0 + (d1 - d0) * ((g.f[m] - lo) / (hi - lo)) if hi > lo else d0
            W[m] = float(weight[b])
        if g.type2:
            c = np.cos(PI * g.f.astype(LD) / 2).astype(np.float64)
            D, W = D / c, W * c
        self.D, self.W = D, W

    def start(self):
        G, L = self.g.G, self.g.L
        if self.mut == "start":
            return np.array([min(G - 1, (k * G) // L) for k in range(L + 1)])
        return start_set(G, L)

    def solve(self, ext):
        s = Sol()
        s.ext = ext = np.asarray(ext)
        n1 = len(ext)
        x, D, W = self.x[ext], self.D[ext], self.W[ext]
        d = 2.0 * (x[:, None] - x[None, :])
        np.fill_diagonal(d, 1.0)
        p, ex = np.ones(n1), np.zeros(n1, dtype=np.int64)
        for j0 in range(0, n1, 16):
            for j in range(j0, min(n1, j0 + 16)):
                p = p * d[:, j]
            p, e = np.frexp(p)
            ex += e
        gam = np.ldexp(1.0 / p, (-ex - (-ex).max()).astype(np.int32))
        sg = np.where(np.arange(n1) % 2, -1.0, 1.0) * (-1.0 if self.mut == "sign" else 1.0)
        pr, er = _two_prod(gam, D)
        num = math.fsum(list(pr) + list(er))
        den = _block_sum(gam * sg / W)
        s.delta = num / den
        s.x, s.gam, s.sg = x, gam, sg
        s.C = D - sg * s.delta / W
        dq = self.x[:, None] - x[None, :]
        hit = dq == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            t = gam[None, :] / np.where(hit, 1.0, dq)
            s.E = self.W * (self.D - (t * s.C[None, :]).sum(axis=1) / t.sum(axis=1))
        s.E[ext] = sg * s.delta
        return s

    def taps(self, s):
        """The kernel recovers the taps from weights, a delta and node values of its own in double-double, on its fp64 grid data (x,
        D, W), samples the interpolant in double-double and transforms in fp64; here: long double in place of double-double."""
        L = self.g.L
        M = 2 * L - 1
        j = np.arange(L)
        y = np.cos(2 * PI * j.astype(LD) / M).astype(np.float64)
        x, D, W = s.x.astype(LD), self.D[s.ext].astype(LD), self.W[s.ext].astype(LD)
        d = x[:, None] - x[None, :]
        np.fill_diagonal(d, LD(0.5))
        gam = 1 / np.prod(2 * d, axis=1)
        gam = gam / np.abs(gam).max()
        sg = s.sg.astype(LD)
        C = D - sg * ((gam * D).sum() / (gam * sg / W).sum()) / W
        P = _bary(y.astype(LD), x, gam, C)[0].astype(np.float64)
        ck = np.cos(2 * PI * ((j[:, None] * j[None, :]) % M).astype(LD) / M).astype(np.float64)
        a = (P[0] + 2.0 * (ck[:, 1:] * P[None, 1:]).sum(axis=1)) / M
        a[1:] *= 2.0
        return _tap_formulas(a, L, self.g.type2, shift=1 if self.mut == "tapshift" else 0)

    def sweep(self, kmax=25):
        """The runs maxiter = 1 .. (the iteration that converges, or kmax): {k: run}, each run what the kernel returns for that
        maxiter -- dict(h, status, iterations, delta, ext)."""
        runs, ext = {}, self.start()
        for k in range(1, kmax + 1):
            s = self.solve(ext)
            nxt = exchange(self.g, s.E, s.delta, first_of_equal=self.mut != "pass2") if np.isfinite(s.delta) else None
            status = "failed" if nxt is None else "converged" if np.array_equal(nxt, ext) else "not converged"
            h = self.taps(s)
            runs[k] = dict(h=h, status=status, iterations=k, delta=float(s.delta), ext=self.f[ext].copy())
            if status != "not converged":
                break
            ext = nxt
        return runs


# ---- the spec table ----------------------------------------------------------------------------------------------------------
def gap_for(numtaps, a, G, density):
    """t such that the grid of [0 a a+t 1] has exactly G points."""
    L = half_len(numtaps)
    delf = 1.0 / (density * L)
    for j in range(-12, 13):
        t = round(1.0 - G * delf + j * delf / 4, 12)
        if t > 0 and grid(numtaps, [0, a, a + t, 1], [1, 1, 0, 0], [1, 1], density).G == G:
            return t
    raise ValueError("no gap gives G = %d" % G)


def _specs():
    lp, one = [1.0, 1.0, 0.0, 0.0], [1.0, 1.0]
    S = {}
    for n in (3, 4, 5):
        S["tiny%d" % n] = (n, [0, .3, .6, 1], lp, one, 16)
    S["tiny6_below1"] = (6, [0, .3, .5, .9], lp, one, 16)
    for n in (29, 30, 31, 32):
        S["frexp%d" % n] = (n, [0, .2, .3, 1], lp, one, 16)
    for n in (509, 511, 512, 513):
        S["nodes%d" % n] = (n, [0, .05, .06, 1], lp, [1.0, 10.0], 16)
    S["bp60_type2_below1"] = (60, [.1, .2, .3, .5, .6, .9], [0, 0, 1, 1, 0, 0], [5.0, 1.0, 5.0], 16)
    S["hp41"] = (41, [0, .5, .6, 1], [0, 0, 1, 1], one, 16)
    S["point45"] = (45, [0, .2, .25, .25, .3, 1], [1, 1, 0, 0, 0, 0], [1.0, 50.0, 1.0], 16)
    S["oneband21"] = (21, [0, 1], [1, 0], [1.0], 16)
    S["eight121"] = (121, [0, .05, .08, .15, .18, .3, .33, .45, .48, .6, .63, .75, .78, .9, .93, 1],
                     [1, .9, 0, 0, .5, .7, 0, 0, 1, .8, 0, 0, .3, .5, 0, 0], [1.0, 30.0, 2.0, 35.0, 1.0, 30.0, 2.0, 35.0], 16)
    e64 = [v for b in range(64) for v in (2 * b / 127, (2 * b + 0.6) / 127)]
    S["comb64"] = (513, e64, [float(1 - b % 2) for b in range(64) for _ in (0, 1)], [1.0 if b % 2 == 0 else 10.0 for b in range(64)], 16)
    S["w1e4_101"] = (101, [0, .1, .2, 1], lp, [1.0, 1e4], 16)
    # the compaction chunk ceil(G / 256) going 1 -> 2 -> 3.  33 taps at density 16 have at most 273 grid points, so G = 512 and 513
    # take density 32 (they run in the density-32 launch)
    for G, dens in ((255, 16), (256, 16), (257, 16), (512, 32), (513, 32)):
        a = 0.3
        S["G%d" % G] = (33, [0, a, a + gap_for(33, a, G, dens), 1], lp, one, dens)
    for dens in (8, 32):
        S["frexp31_d%d" % dens] = S["frexp31"][:4] + (dens,)
        S["bp60_d%d" % dens] = S["bp60_type2_below1"][:4] + (dens,)
    return {k: (v[0], [float(x) for x in v[1]], [float(x) for x in v[2]], [float(x) for x in v[3]], v[4]) for k, v in S.items()}


SPECS = _specs()
NAMES = list(SPECS)
SMALL = [k for k in NAMES if SPECS[k][0] < 40]              # the near-tie allowance is never granted below 40 taps
_GRID, _SOL, _TAPS, _K64, _REPLAY, _BOUND = {}, {}, {}, {}, {}, {}


def spec_grid(name):
    if name not in _GRID:
        _GRID[name] = grid(*SPECS[name])
    return _GRID[name]


def ref_solve(name, ext):
    """solve() on a spec's grid, cached per (spec, set): the long-double work is paid once."""
    key = (name, np.asarray(ext).tobytes())
    if key not in _SOL:
        _SOL[key] = solve(spec_grid(name), ext)
    return _SOL[key]


def ref_taps(name, ext):
    key = (name, np.asarray(ext).tobytes())
    if key not in _TAPS:
        _TAPS[key] = taps(ref_solve(name, ext))
    return _TAPS[key]


def kern64(name):
    if name not in _K64:
        _K64[name] = Kern64(*SPECS[name])
    return _K64[name]


def taps_bound(name, ext):
    """The fallback bound of the taps for (spec, set): ten times the distance of the fp64 restatement from the long-double
    reference, at least 1e-15 max|h|.  Returns (bound, the restatement's distance)."""
    key = (name, np.asarray(ext).tobytes())
    if key not in _BOUND:
        k = kern64(name)
        href = ref_taps(name, ext)
        s64 = k.solve(ext)
        d = float(np.abs(k.taps(s64).astype(LD) - href).max())
        _BOUND[key] = (max(10 * d, 1e-15 * float(np.abs(href).max())), d, float(s64.delta))
    return _BOUND[key][:2]


def kern64_delta(name, ext):
    """The restatement's delta for (spec, set)."""
    taps_bound(name, ext)
    return _BOUND[(name, np.asarray(ext).tobytes())][2]


def replay(name, kmax=25):
    """The long-double replay: start set, then solve and exchange until the set repeats.  Returns (sets, K_s): sets[k - 1] is the
    set iteration k solves on; K_s = None when it does not repeat within kmax."""
    if name not in _REPLAY:
        g = spec_grid(name)
        sets, ext = [], start_set(g.G, g.L)
        K = None
        for k in range(1, kmax + 1):
            sets.append(ext)
            s = ref_solve(name, ext)
            nxt = exchange(g, s.E, s.delta)
            if nxt is None:
                break
            if np.array_equal(nxt, ext):
                K = k
                break
            ext = nxt
        _REPLAY[name] = (sets, K)
    return _REPLAY[name]


def replay_taps(numtaps, edges, desired, weight, density=16, kmax=25):
    """Taps (fp64-rounded) of the converged long-double replay of any spec."""
    g = grid(numtaps, edges, desired, weight, density)
    ext = start_set(g.G, g.L)
    for _ in range(kmax):
        s = solve(g, ext)
        nxt = exchange(g, s.E, s.delta)
        need(nxt is not None, "reference", "the exchange lost the alternation")
        if np.array_equal(nxt, ext):
            return taps(s).astype(np.float64)
        ext = nxt
    raise Miss("reference", "the long-double replay does not converge")


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def near_tie(g, s, want, got):
    """The near-tie allowance: every position where the sets differ holds a point of the same sign run of the reference's E (same
    sign, no candidate of the other sign between the two), whose reference |E| is within the E envelope of the reference's pick."""
    if got is None or want is None or len(got) != len(want):
        return False
    env = e_envelope(s)
    cand = candidates(g, s.E, s.delta)
    for a, b in zip(want, got):
        if a == b:
            continue
        lo, hi = min(a, b), max(a, b)
        if (s.E[a] > 0) != (s.E[b] > 0):
            return False
        between = cand[(cand > lo) & (cand < hi)]
        if np.any((s.E[between] > 0) != (s.E[a] > 0)):
            return False
        if abs(float(abs(s.E[a]) - abs(s.E[b]))) > env[a] + env[b]:
            return False
    return True


def check_sweep(name, runs, default_run=None, allow_ties=True, stats=None):
    """Hold the runs maxiter = 1 .. K of one spec (runs[k] = dict(h, status, iterations, delta, ext); K = the first k whose status
    is not 'not converged') against the reference, as the module docstring lists.  default_run: the run at the default maxiter,
    bit-identical to runs[K].  Returns the statistics (worst error / bound of delta and of the taps, pairs, ties used, pairs whose
    delta equals the restatement's bit for bit); a dict given as `stats` is filled as the sweep goes, so it is there after a miss."""
    g = spec_grid(name)
    numtaps, edges, desired, weight, density = SPECS[name]
    sets, Ks = replay(name)
    need(Ks is not None, "reference", "the long-double replay does not converge on", name)
    st = stats if stats is not None else {}
    st.update(pairs=0, ties=0, delta=0.0, taps=0.0, amp=0.0, env_rel=0.0, K=Ks, same_delta=0)
    want, tied = start_set(g.G, g.L), False
    for k in range(1, Ks + 1):
        need(k in runs, "status", "no run at maxiter", k, "(converged early: expected K_s = %d)" % Ks)
        r = runs[k]
        idx = index_of(g, r["ext"])
        if k == 1:
            need(np.array_equal(idx, want), "start_set", "first differing entry", int(np.argmax(idx != want)) if len(idx) == len(want) else -1)
        s = ref_solve(name, idx)
        nxt = exchange(g, s.E, s.delta)
        # status and iteration count (K_s follows the device's path only after a granted near-tie)
        last = (nxt is not None and np.array_equal(nxt, idx)) if tied else k == Ks
        need(r["iterations"] == k, "status", "iterations", r["iterations"], "at maxiter", k)
        need(r["status"] == ("converged" if last else "not converged"), "status", r["status"], "at maxiter %d, K_s = %d" % (k, Ks))
        # delta
        err = abs(float(LD(r["delta"]) - s.delta))
        st["pairs"] += 1
        st["delta"] = max(st["delta"], err / s.env_delta)
        st["amp"], st["env_rel"] = max(st["amp"], s.amp), max(st["env_rel"], s.env_rel)
        need(err <= s.env_delta, "delta", "iteration %d: |error| / envelope %.3g (relative envelope %.3g, amplification %.3g)"
             % (k, err / s.env_delta, s.env_rel, s.amp))
        # taps
        h = np.asarray(r["h"], dtype=np.float64)
        need(len(h) == numtaps and np.array_equal(h, h[::-1]), "symmetry", "iteration", k)
        bound, _ = taps_bound(name, idx)
        st["same_delta"] += int(r["delta"] == kern64_delta(name, idx))
        herr = float(np.abs(h.astype(LD) - ref_taps(name, idx)).max())
        st["taps"] = max(st["taps"], herr / bound)
        need(herr <= bound, "taps", "iteration %d: |error| / bound %.3g" % (k, herr / bound))
        if last:
            need(k == Ks or tied, "status", "converged at", k, "reference at", Ks)
            try:
                certify(h, dict(delta=r["delta"], ext=r["ext"]), numtaps, edges, desired, weight, density=density)
            except Miss:
                raise
            except AssertionError as e:
                raise Miss("certify", e) from None
            break
        # the exchange, seen through the next run's set
        need(k + 1 in runs, "status", "no run at maxiter", k + 1)
        got = index_of(g, runs[k + 1]["ext"])
        if nxt is None or not np.array_equal(got, nxt):
            ok = allow_ties and name not in SMALL and near_tie(g, s, nxt, got)
            need(ok, "exchange", "iteration %d -> %d: sets differ at %s" % (k, k + 1, np.nonzero(got != nxt)[0][:8] if nxt is not None else "all"))
            st["ties"] += 1
            tied = True
    if default_run is not None:
        K = max(runs) if tied else Ks
        a, b = runs[K], default_run
        need(np.array_equal(a["h"], b["h"]) and a["delta"] == b["delta"] and np.array_equal(a["ext"], b["ext"])
             and b["status"] == "converged" and b["iterations"] == a["iterations"], "default", "maxiter = 25 differs from maxiter = K_s")
    return st


# ---- fmp in long double --------------------------------------------------------------------------------------------------
FMP_LENGTHS = (31, 33, 63, 65, 127, 129, 255, 257)          # lp = 256 .. 4096; l = 3, 5 (lp = 32, 64) beside them


def fmp_input(l):
    """The Parks-McClellan spec whose design is the fmp input of length l (ripple about 0.06 for l >= 31)."""
    return (l, [0, .3, .6, 1], [1, 1, 0, 0], [1, 1]) if l <= 5 else (l, [0, .2, .2 + 2.0 / l, 1], [1, 1, 0, 0], [1, 1])


def _dft(v, sign):
    n = len(v.real)
    k = np.arange(n)
    ph = (2 * PI / n) * ((k[:, None] * k[None, :]) % n).astype(LD)
    c, s = np.cos(ph), sign * np.sin(ph)
    return c @ v.real - s @ v.imag, c @ v.imag + s @ v.real


def fmp_ref(h):
    """fmp.m (make_golden_conventional.fmp_np) restated in long double with dense DFTs, for lp = 8 * 2^ceil(log2 l) <= 512; fp64
    fmp_np beyond.  Returns complex128 (real and imaginary part each rounded from long double)."""
    h = np.asarray(h, dtype=np.complex128)
    l = len(h)
    lp = 8 * 2 ** int(math.ceil(math.log2(l))) if l > 1 else 8
    if lp > 512:
        return gold.fmp_np(h)
    lo = (lp - l + 1) // 2
    hp = np.zeros(lp, dtype=np.complex128)
    hp[lo:lo + l] = h

    class Z:                                                   # a long-double complex vector
        def __init__(self, re, im):
            self.real, self.imag = np.asarray(re, dtype=LD), np.asarray(im, dtype=LD)

    sh = np.fft.fftshift(np.arange(lp))
    fr, fi = _dft(Z(hp.real[sh], hp.imag[sh]), -1)
    fr, fi = fr[sh], fi[sh]                                    # hpf
    fr = fr - fr.min() * LD("1.000001")
    xl = np.log(np.sqrt(np.hypot(fr, fi)))                     # mag2mp(sqrt(abs(hpfs))): the log of the root
    xr, xi = _dft(Z(xl, np.zeros(lp)), -1)
    m = np.zeros(lp, dtype=LD)
    m[0] = m[lp // 2] = 1
    m[1:lp // 2] = 2
    ar, ai = _dft(Z(xr * m, xi * m), +1)
    ar, ai = ar / lp, ai / lp
    er, ei = np.exp(ar) * np.cos(ai), np.exp(ar) * np.sin(ai)  # hpfmp
    br, bi = _dft(Z(er[sh], -ei[sh]), +1)                      # ifft(fftshift(conj(hpfmp)))
    n = (l + 1) // 2
    return (br[:n] / lp).astype(np.float64) + 1j * (bi[:n] / lp).astype(np.float64)
