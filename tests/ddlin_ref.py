"""The reference of the double-double dense kernels (csrc/ddlin.hip: k_dd_syrk, k_ddchol_diag / _trsm / _update, k_dd_blockinv, k_dd_trsv,
k_dd_trsv_mw, k_dd_trsv_bi) for mbfir.test_ddstages: tests/test_ddlin_gpu.py holds the device to it stage by stage,
tests/test_ddlin_ref_cpu.py holds the oracle's C twin (oracle/ddlin.c) and a NumPy restatement of the block-inverse form to it, checks
that planted errors fail their own stage alone and that the replaced-pivot inputs decide far from rounding, without a GPU.

Every stage is handed the device's own earlier outputs as exact, so a wrong kernel fails alone.  A double-double number hi + lo is a
dyadic rational: the sums of products a stage forms are evaluated EXACTLY, as Python integers on the doubles' mantissas over one
common power of two (what an mpmath sum tends to as its precision grows; test_ddlin_ref_cpu.py compares them with plain mpmath sums at
240 bits, the precision of ddkkt_ref.mp_dd), so that |device - reference| loses nothing; the quotients, square roots and reciprocals are
mpmath at 240 bits.  A quotient is compared through |L_ij - N / L_jj| = |L_ij L_jj - N| / L_jj, numerator exact.

Bounds: K_DD(terms) EPS_DD envelope, EPS_DD = 2^-102, K_DD(t) = 3 t + 4 of ddkkt_ref: a double-double operation errs by at most
4 u^2 = 2^-104 of its operands (u = 2^-53), three operations a term, the project's margin of 4.  (The rigorous constants of the
operations in dd_dev.h -- Joldes, Muller, Popescu, "Tight and rigorous error bounds for basic building blocks of double-word
arithmetic", ACM TOMS 44 (2017): the sum 3 u^2, the product with fused multiply-adds 5 u^2, 6 .. 7 u^2 without -- are within that
count: a term costs one product and one sum, 8 .. 10 u^2 against the 48 u^2 it is given.)  The envelope is the sum of the absolute
values of the terms, in float64 from the stage's inputs (its own rounding, terms x 2^-53 relative, is nothing next to the margin),
never from the stage's output; it holds for any order of summation -- right-looking panels, the unscaled Schur complement of
k_ddchol_diag, partial sums folded by shuffles, both tile sizes.  No constant is taken from a device result; the measured fractions
quoted below are the CPU twin's (test_ddlin_ref_cpu.py prints them).

  update   Hh + sum_r X[r] U[r, i] U[r, j] for every entry of the lower-triangle tiles (the entries above the diagonal inside a
           diagonal tile included: the kernel writes them): K_DD(k + 1) EPS_DD (|Hh| + sum_r X |u_i| |u_j|).  The kernel starts from
           (Hh, 0): an incoming low word is discarded by design -- Hl goes in holding the sentinel and comes back finite; with k = 0 the
           low word is exactly 0 and the high word unchanged.  The tiles strictly above the diagonal tiles (32 or 64 wide, MBFIR_DD_TILE)
           keep Hh as given and Hl's sentinel.  Past n: the identity exactly.           (twin: 0.015 of the bound at worst)
  d0       the diagonal of Hh after the update, bit for bit.
  factor   entry by entry from the device's own earlier columns, H the device's updated matrix:
           off the diagonal N = H_ij - sum_{c<j} L_ic L_jc, ref = N / L_jj: K_DD(j + 2) EPS_DD (|H_ij| + sum |L_ic| |L_jc|) / L_jj
           (j products and sums, H_ij, the scaling by 1 / L_jj);
           on the diagonal p = H_jj - sum L_jc^2, ref = sqrt(p): the same envelope / (2 L_jj) + C_DIAG EPS_DD L_jj.  The kernel forms
           x = 1 / sqrt(p.h) in double (the hardware's estimate and two Newton steps: the last one's three roundings leave x within
           e <= 3 u), then e1 = 1 - p x^2 by a two-term product and three fused multiply-adds and ri = x + x e1 / 2.  |e1| <= 2 e + u
           = 7 u; the Newton step's own error 3/8 e1^2 = 18.4 u^2, the three roundings of e1 (each u |e1|, halved) 10.5 u^2, the
           product x e1 / 2 (two roundings of 3.5 u) 7 u^2, the dropped p.l t2.l 0.5 u^2: ri = (1 + d) / sqrt(p), |d| <= 36.4 u^2.
           L_jj = p ri (a product: 5 u^2) errs by 41.4 u^2 = 2.6 EPS_DD: C_DIAG = 4 x 2.6 -> 11.         (twin: 0.013, all of factor)
           A pivot with !(p > pivtol d0[j]) is replaced by max(d0[j], 1e-300) (the rule of oracle/ddlin.c), p the exact one: the
           inputs keep every decision 1e10 away from rounding (asserted on the CPU); the replaced diagonal is sqrt of that.
           ri: 1 / L_jj within C_RI EPS_DD relative: ri L_jj = (1 + d)^2 (1 + 5 u^2) = 1 + 77.8 u^2 = 1 + 4.9 EPS_DD, C_RI = 4 x 4.9
           -> 20.                                          (twin: its reciprocal is a dd division)
           Lt: the transpose of L bit for bit, both words; its strict lower part keeps the sentinel; the strict upper part of
           (Lh, Ll) is what the update left there, bit for bit.
  blockinv for each 64 x 64 diagonal block, row by row from the device's own earlier rows of X:
           ref_ij = -(sum_{j<=k<i} L_ik X_kj) ri_i within K_DD(i - j + 1) EPS_DD (sum |L_ik| |X_kj|) |ri_i| (i - j terms in four partial
           sums, the scaling); the diagonal equals ri bit for bit, the strict upper triangle is exactly zero.  A form without the
           inverses leaves dinv's sentinel.                                                (NumPy restatement: 0.019)
  solve    backward error on the device's factor, b the (hi, lo) right-hand side, y = L'x exactly:
           substitution (single, mw): (L + dL) yy = b, (L' + dL') x = yy with |dL| <= gamma |L| gives
               |b - L (L' x)| <= gamma (|L| |L' x| + |L| |L'| |x|),   gamma = K_DD(np + 2) EPS_DD
           entrywise, to first order (np terms a row, the right-hand side, the product with ri).  The kernels multiply by ri where
           the analysis divides by L_qq: rho_q = |ri_q L_qq - 1|, exact from the device's own ri, adds rho |L_qq| |y_q| to row q of the
           forward sweep and |L| (rho |L_qq| |x_q|) to the backward one -- 4.9 EPS_DD at most with a correct ri, and a wrong ri fails
           the factor stage, not this one.
           block inverses (bi): block b forms w_b = b_b - sum_c L_bc y_c by substitution-like sums and y_b = X_b w_b, a product of 64
           terms: L_bb y_b = w_b + (L_bb X_b - I) w_b + L_bb delta, |delta| <= g64 |X_b| |w_b|, g64 = K_DD(64 + 1) EPS_DD; with
           |w_b| = |L_bb y_b| <= |L_bb| |y_b| to first order a block row of the forward sweep errs by
               gamma (|L| |y|)_b + (E_b + g64 |L_bb| |X_b|) |L_bb| |y_b|,     E_b = |L_bb X_b - I|
           and of the backward sweep (x_b = X_b' v_b) by the same with L_bb', X_b', F_b = |X_b L_bb - I|' and x; together
               |b - L (L' x)| <= gamma (|L| |L' x| + |L| |L'| |x|) + D[(E + g64 |L_bb| |X_b|) |L_bb| |L' x|_b]
                                 + |L| D[(F + g64 |L_bb'| |X_b'|) |L_bb'| |x_b|]
           (D[.]: block by block).  E and F are evaluated exactly from the device's own X, an input of this stage: a wrong block
           inverse fails the blockinv stage and not this one; with a correct one E <= K_DD(65) EPS_DD |L_bb| |X_b|.  The extra factor
           |L_bb| |X_b| is the price of multiplying by an inverse: up to the condition number of a diagonal block looser than the
           substitution's bound.                                  (twin: 2.6e-4 substitution, 6.5e-5 block inverses)
           The padding rows of x are exactly zero, an all-zero right-hand side gives exact zeros, rows past nrhs keep the sentinel,
           the solutions of repeated solves (epochs 1 .. nsolve on one flag array) are the same bit for bit, the nrhs = 1 solution
           equals column 0 of nrhs = 2 bit for bit in every form.  single and mw do NOT sum in one order -- k_dd_trsv walks a row's
           columns ascending in one chain, k_dd_trsv_mw keeps eight partial sums a row (columns q mod 8 of every block) and folds them
           by shuffles -- so each is held to the bound and no bit-equality between them is asserted.
  counter  replaced pivots: the device's count equals the reference's plan and the twin's; no DD_SYNC_LOST (2^20) in it.

Inputs (inputs()): H = B'B, B (n + 30) x n standard normal; U k x n standard normal, every third row a copy of its predecessor to
1e-9 (nearly dependent), a few exact zeros (the twin skips them, the device does not); X = 10^U(8, 16); b standard normal with low
words of 1e-17.  Replaced pivots, lower=(j, ...): H[j][j] is lowered to half its neighbour's, H[z][z] / 2 with z = j - 1, so d0[j] > 0
stays of the order of the matrix.  Lowering alone does not do: the replaced pivot d0[j] divides a column of the Schur complement that
is then far too large, every later pivot turns negative in its turn, and the entries square from column to column (measured with
H[j][j] = 3 at n = 150: 101 .. 129 pivots replaced with k = 9, an overflow with k = 0).  So row and column j are tied to their
neighbour: H[j][c] = H[z][c] for c < j, H[i][j] = H[i][z] + N(0, 1) for i > j, columns z and j of U exactly zero (the update adds
nothing to them).  Then column j of the matrix above the diagonal is its leading block times e_z, whatever was replaced before: the
pivot is exactly H[j][j] - H[z][z] = -H[z][z] / 2 -- negative by half a diagonal entry, nowhere near rounding -- the column below it
is the N(0, 1) noise over sqrt d0[j], and the later pivots move by 1e-2: one replaced pivot per lowered entry, nothing grows.
j = 0: the first pivot IS d0[0] and the rule keeps it; H[0][0] and column 0 are halved (still positive definite): the plan is empty.
"""
import math
import zlib

import numpy as np

import cone_ref as CR
from ddkkt_ref import EPS_DD, k_dd

C_DIAG, C_RI = 11.0, 20.0
DIB, DNB = 64, 32
SYNC_LOST = 1 << 20
STAGES = ("update", "d0", "factor", "blockinv", "solve", "counter")
FORMS = ("single", "mw", "bi")


def mpm():
    import mpmath as mp
    mp.mp.prec = 240
    return mp


# ---- exact arithmetic on doubles -----------------------------------------------------------------------------------------------------
def _emin(*arrs):
    """the exponent e with a / 2^e an integer for every entry of the arrays"""
    e = 0
    for a in arrs:
        a = np.asarray(a, dtype=np.float64)
        nz = a[a != 0]
        if nz.size:
            e = min(e, int(np.frexp(nz)[1].min()) - 53)
    return e


def _ints(a, e):
    """a / 2^e as an object array of Python integers (exact; a finite)"""
    a = np.asarray(a, dtype=np.float64)
    m, ex = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64).astype(object)
    sh = np.where(a != 0, ex.astype(np.int64) - 53 - e, 0).astype(object)
    return mi << sh


def xdd(h, l=None):
    """(integers, e): the exact value h + l = integers x 2^e"""
    e = _emin(h) if l is None else _emin(h, l)
    v = _ints(h, e)
    return (v if l is None else v + _ints(l, e)), e


def _align(a, ea, b, eb):
    e = min(ea, eb)
    return a * (1 << (ea - e)), b * (1 << (eb - e)), e


def _flt(d, e):
    """float of the integer d x 2^e (truncated to 64 bits first: an error measure needs no more)"""
    bl = d.bit_length()
    try:
        if bl > 64:
            return math.ldexp(float(d >> (bl - 64)), e + bl - 64)
        return math.ldexp(float(d), e)
    except OverflowError:
        return math.inf if d > 0 else -math.inf


_vflt = np.frompyfunc(_flt, 2, 1)


def flt(a, e):
    return np.asarray(_vflt(a, e), dtype=np.float64)


def _abs(a):
    return np.asarray(np.frompyfunc(abs, 1, 1)(a), dtype=object) if np.ndim(a) else abs(a)


def is_sent(a, sentinel=np.nan):
    a = np.asarray(a)
    return bool(np.all(np.isnan(a) if np.isnan(sentinel) else a == sentinel))


def same_bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
# name -> (n, k, lowered diagonal entries).  Every n at two values of k, every k at n = 150; the replaced pivots at n = 150, k = 0 and 9.
CASES = {
    "n30_k0": (30, 0, ()), "n30_k9": (30, 9, ()),
    "n64_k7": (64, 7, ()), "n64_k8": (64, 8, ()),
    "n65_k1": (65, 1, ()), "n65_k20": (65, 20, ()),
    "n150_k0": (150, 0, ()), "n150_k1": (150, 1, ()), "n150_k7": (150, 7, ()), "n150_k8": (150, 8, ()), "n150_k9": (150, 9, ()),
    "n150_k20": (150, 20, ()),
}
PIVOTS = {"p0": (0,), "p31": (31,), "p32": (32,), "p63": (63,), "p64": (64,), "p149": (149,), "p31_64": (31, 64)}
for _k in (0, 9):
    for _nm, _js in PIVOTS.items():
        CASES["n150_k%d_%s" % (_k, _nm)] = (150, _k, _js)
PIVTOL = 1e-28
_IN = {}


def npad(n):
    return -(-n // DIB) * DIB


def inputs(name, rhs="random"):
    """dict(n, k, H, U, X, b, bl) of a case (deterministic).  rhs: 'random' | 'zero' (an all-zero second column)."""
    key = (name, rhs)
    if key not in _IN:
        n, k, lower = CASES[name]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        B = rng.standard_normal((n + 30, n))
        H = B.T @ B
        H = 0.5 * (H + H.T)
        U = rng.standard_normal((k, n))
        if k:
            m = len(U[1::3])
            U[1::3] = U[0::3][:m] * (1 + 1e-9 * rng.standard_normal((m, 1)))     # nearly dependent rows
            U[rng.integers(0, k, 5), rng.integers(0, n, 5)] = 0.0                 # a few exact zeros
        X = 10.0 ** rng.uniform(8, 16, k)
        b = rng.standard_normal((2, n))
        bl = 1e-17 * rng.standard_normal((2, n))
        for j in sorted(lower):
            U[:, j] = 0.0
            if j == 0:
                H[0, 0] *= 0.5
                H[1:, 0] *= 0.5
                H[0, 1:] = H[1:, 0]
                continue
            z = j - 1
            U[:, z] = 0.0
            H[j, :j] = H[z, :j]
            H[:j, j] = H[j, :j]
            H[j, j] = 0.5 * H[z, z]
            H[j + 1:, j] = H[j + 1:, z] + rng.standard_normal(n - j - 1)
            H[j, j + 1:] = H[j + 1:, j]
        if rhs == "zero":
            b[1], bl[1] = 0.0, 0.0
        _IN[key] = dict(n=n, k=k, H=H, U=U, X=X, b=b, bl=bl)
    return _IN[key]


def padded(inp):
    """(H, U, b, bl) at the padded size: the identity past n, zero coupling"""
    n, k = inp["n"], inp["k"]
    q = npad(n)
    Hp, Up, bp, blp = np.eye(q), np.zeros((k, q)), np.zeros((2, q)), np.zeros((2, q))
    Hp[:n, :n], Up[:, :n], bp[:, :n], blp[:, :n] = inp["H"], inp["U"], inp["b"], inp["bl"]
    return Hp, Up, bp, blp


def tile_mask(q, tile):
    """entries of the lower-triangle tiles (those the update kernel writes)"""
    t = np.arange(q) // tile
    return t[:, None] >= t[None, :]


# ---- the stages ----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _key(*arrs):
    return tuple(zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrs) + tuple(np.shape(a) for a in arrs)


def _cached(stage, key, fn):
    """a stage's (fractions, failures) per input: the forms, the tile sizes and the repeated calls share them"""
    if (stage, key) not in _CACHE:
        rec = CR.Rec()
        extra = fn(rec)
        _CACHE[(stage, key)] = (dict(rec.frac), list(rec.failed), extra)
    return _CACHE[(stage, key)]


def _merge(rec, got):
    frac, failed, extra = got
    for kk, v in frac.items():
        rec.frac[kk] = max(rec.frac.get(kk, 0.0), v)
    rec.failed += failed
    return extra


def check_update(rec, inp, o, tile=32, sentinel=np.nan):
    Hp, Up, _, _ = padded(inp)
    n, k, X = inp["n"], inp["k"], inp["X"]
    q = len(Hp)
    Hh, Hl = o["Hh"], o["Hl"]

    def run(rec):
        low = tile_mask(q, tile)
        rec.exact("update", "finite in the lower-triangle tiles", np.isfinite(Hh[low]).all() and np.isfinite(Hl[low]).all())
        rec.exact("update", "tiles above the diagonal: Hh as given, Hl untouched", np.array_equal(Hh[~low], Hp[~low]) and is_sent(Hl[~low], sentinel))
        pad = low.copy()
        pad[:n, :n] = False
        rec.exact("update", "past n the identity exactly", np.array_equal(Hh[pad], np.eye(q)[pad]) and np.all(Hl[pad] == 0.0))
        if k == 0:
            rec.exact("update", "k = 0: the high word unchanged, the low word exactly 0", np.array_equal(Hh[low], Hp[low]) and np.all(Hl[low] == 0.0))
        Hs, Hls = np.where(low, Hh, 0.0), np.where(low & np.isfinite(Hl), Hl, 0.0)
        dev, ed = xdd(Hs, Hls)
        h0, eh = xdd(Hp)
        ux, eu = xdd(Up)
        xx, ex = xdd(X)
        ref = (ux.T * xx) @ ux if k else np.zeros((q, q), dtype=object) + 0
        et = ex + 2 * eu
        e = min(ed, eh, et)
        diff = dev * (1 << (ed - e)) - h0 * (1 << (eh - e)) - ref * (1 << (et - e))
        err = np.abs(flt(diff, e))
        env = np.abs(Hp) + (np.abs(Up).T * X) @ np.abs(Up)
        rec.add("update", "H + U'XU", err[low], k_dd(k + 1) * EPS_DD * env[low])
    _merge(rec, _cached("update", _key(Hp, Up, X, Hh, Hl) + (tile,), run))
    return rec


def check_d0(rec, o):
    rec.exact("d0", "the diagonal of Hh after the update", np.array_equal(o["d0"], np.diag(o["Hh"])))
    return rec


def check_factor(rec, o, pivtol=PIVTOL, sentinel=np.nan):
    """the factor, ri and Lt.  Returns facts: replaced (the reference's plan), and the margins of the decisions: keep = the smallest
    p / (pivtol d0) of a kept pivot, drop = the largest p / d0 of a replaced one (negative)."""
    Hh, Hl, Lh, Ll, d0, ri = o["Hh"], o["Hl"], o["Lh"], o["Ll"], o["d0"], o["ri"]
    q = len(Hh)

    def run(rec):
        mp = mpm()
        tri, stri = np.tril(np.ones((q, q), dtype=bool)), np.tril(np.ones((q, q), dtype=bool), -1)
        ok = bool(np.isfinite(Lh[tri]).all() and np.isfinite(Ll[tri]).all() and np.isfinite(Hh[tri]).all() and np.isfinite(Hl[tri]).all()
                  and np.isfinite(ri).all() and np.isfinite(d0).all())
        rec.exact("factor", "finite", ok)
        rec.exact("factor", "above the diagonal what the update left", same_bits(Lh[~tri], Hh[~tri]) and same_bits(Ll[~tri], Hl[~tri]))
        rec.exact("factor", "Lt = L' bit for bit", same_bits(o["Lth"][tri.T], Lh.T[tri.T]) and same_bits(o["Ltl"][tri.T], Ll.T[tri.T]))
        rec.exact("factor", "Lt below the diagonal untouched", is_sent(o["Lth"][stri], sentinel) and is_sent(o["Ltl"][stri], sentinel))
        if not ok:
            rec.add("factor", "L", np.inf, 1.0)
            return dict(replaced=[], keep=np.inf, drop=-np.inf)
        Hx, eh = xdd(np.where(tri, Hh, 0.0), np.where(tri, Hl, 0.0))
        Lx, el = xdd(np.where(tri, Lh, 0.0), np.where(tri, Ll, 0.0))
        La, Ha = np.abs(np.where(tri, Lh, 0.0)), np.abs(Hh)
        e = min(eh, 2 * el)
        sh, sl = 1 << (eh - e), 1 << (2 * el - e)
        err_o, bnd_o = np.zeros((q, q)), np.ones((q, q))
        err_d, bnd_d, err_r = np.zeros(q), np.ones(q), np.zeros(q)
        replaced, keep, drop = [], np.inf, -np.inf
        for j in range(q):
            S = Lx[j:, :j] @ Lx[j, :j] if j else np.zeros(q - j, dtype=object) + 0
            N = Hx[j:, j] * sh - S * sl                                    # (x 2^e): H_ij - sum_{c<j} L_ic L_jc, i = j .. q-1
            env = Ha[j:, j] + La[j:, :j] @ La[j, :j]
            ljj = float(Lh[j, j])
            # the pivot
            p = N[0]
            ti, et = xdd(np.array([pivtol * d0[j]]))                        # (the threshold as the kernel forms it: one double product)
            pa, ta, _ = _align(p, e, int(ti[0]), et)
            bad = not pa > ta
            pf = _flt(p, e)
            if bad:
                replaced.append(j)
                drop = max(drop, pf / d0[j] if d0[j] > 0 else np.inf)
                pm, extra = mp.mpf(float(d0[j]) if d0[j] > 1e-300 else 1e-300), 0.0
            else:
                keep = min(keep, pf / (pivtol * d0[j]) if d0[j] > 0 else np.inf)
                pm, extra = mp.ldexp(mp.mpf(int(p)), e), k_dd(j + 2) * EPS_DD * env[0] / (2 * ljj)
            lm = mp.mpf(float(Lh[j, j])) + mp.mpf(float(Ll[j, j]))
            err_d[j], bnd_d[j] = float(abs(lm - mp.sqrt(pm))), extra + C_DIAG * EPS_DD * ljj
            rm = mp.mpf(float(ri[0, j])) + mp.mpf(float(ri[1, j]))
            err_r[j] = float(abs(rm * lm - 1))
            # the column below it: |L_ij L_jj - N| / L_jj, the numerator exact
            if j + 1 < q:
                d = Lx[j + 1:, j] * Lx[j, j] * sl - N[1:]
                err_o[j + 1:, j] = np.abs(flt(d, e)) / ljj
                bnd_o[j + 1:, j] = k_dd(j + 2) * EPS_DD * env[1:] / ljj
        rec.add("factor", "off the diagonal", err_o[stri], bnd_o[stri])
        rec.add("factor", "diagonal", err_d, bnd_d)
        rec.add("factor", "ri", err_r, C_RI * EPS_DD)
        return dict(replaced=replaced, keep=keep, drop=drop)
    return _merge(rec, _cached("factor", _key(Hh, Hl, Lh, Ll, o["Lth"], o["Ltl"], d0, ri) + (pivtol,), run))


def _blocks(o):
    q = len(o["Lh"])
    for b in range(q // DIB):
        s = slice(b * DIB, (b + 1) * DIB)
        yield b, s, np.tril(o["Lh"][s, s]), np.tril(o["Ll"][s, s]), o["dinv"][0, b], o["dinv"][1, b]


def check_blockinv(rec, o, form, sentinel=np.nan):
    if form != "bi":
        rec.exact("blockinv", "no inverses in this form: dinv untouched", is_sent(o["dinv"], sentinel))
        return rec
    ri = o["ri"]

    def run(rec):
        up = np.triu(np.ones((DIB, DIB), dtype=bool), 1)
        for b, s, Lh, Ll, Xh, Xl in _blocks(o):
            fin = bool(np.isfinite(Xh).all() and np.isfinite(Xl).all())
            rec.exact("blockinv", "finite", fin)
            rec.exact("blockinv", "strict upper triangle exactly zero", np.all(Xh[up] == 0.0) and np.all(Xl[up] == 0.0))
            rec.exact("blockinv", "the diagonal is ri bit for bit", np.array_equal(np.diag(Xh), ri[0, s]) and np.array_equal(np.diag(Xl), ri[1, s]))
            if not fin:
                rec.add("blockinv", "X", np.inf, 1.0)
                continue
            Lx, el = xdd(Lh, Ll)
            Xx, ex = xdd(Xh, Xl)
            rx, er = xdd(ri[0, s], ri[1, s])
            La, Xa, ra = np.abs(Lh), np.abs(Xh), np.abs(ri[0, s])
            err, bnd = np.zeros((DIB, DIB)), np.ones((DIB, DIB))
            for i in range(1, DIB):
                # X_ij = -(sum_{j<=k<i} L_ik X_kj) ri_i, j < i: the earlier rows of X are lower triangular, so the sum may start at 0
                S = Lx[i, :i] @ Xx[:i, :i]                                      # (x 2^(el + ex))
                a, c, e = _align(Xx[i, :i], ex, -S * rx[i], el + ex + er)
                err[i, :i] = np.abs(flt(a - c, e))
                terms = i - np.arange(i)
                bnd[i, :i] = k_dd(terms + 1) * EPS_DD * (La[i, :i] @ Xa[:i, :i]) * ra[i]
            lo = np.tril(np.ones((DIB, DIB), dtype=bool), -1)
            rec.add("blockinv", "X", err[lo], bnd[lo])
    _merge(rec, _cached("blockinv", _key(o["Lh"], o["Ll"], o["dinv"], ri), run))
    return rec


def _inverse_residuals(o):
    """E_b = |L_bb X_b - I| and F_b = |X_b L_bb - I| of every block, exact, as float64"""
    def run(rec):
        out = []
        for b, s, Lh, Ll, Xh, Xl in _blocks(o):
            Lx, el = xdd(Lh, Ll)
            Xx, ex = xdd(np.nan_to_num(np.tril(Xh)), np.nan_to_num(np.tril(Xl)))
            one = np.zeros((DIB, DIB), dtype=object) + 0
            one[np.arange(DIB), np.arange(DIB)] = 1 << -(el + ex)
            out.append((np.abs(flt(Lx @ Xx - one, el + ex)), np.abs(flt(Xx @ Lx - one, el + ex))))
        return out
    return _cached("invres", _key(o["Lh"], o["Ll"], o["dinv"]), run)[2]


def check_solve(rec, inp, o, form, nrhs=2, sentinel=np.nan):
    """the solves of one call: the first against the backward-error bound, the others bit-identical to it"""
    _, _, bp, blp = padded(inp)
    n = inp["n"]
    q = bp.shape[1]
    xh, xl = o["xh"], o["xl"]
    rec.exact("solve", "rows past nrhs untouched", is_sent(xh[:, nrhs:], sentinel) and is_sent(xl[:, nrhs:], sentinel))
    rec.exact("solve", "repeated solves bit-identical", all(same_bits(xh[s], xh[0]) and same_bits(xl[s], xl[0]) for s in range(1, len(xh))))
    xh, xl = xh[0, :nrhs], xl[0, :nrhs]
    fin = bool(np.isfinite(xh).all() and np.isfinite(xl).all())
    rec.exact("solve", "finite", fin)
    if not fin:
        rec.add("solve", "b - L L'x", np.inf, 1.0)
        return rec
    rec.exact("solve", "padding rows exactly zero", np.all(xh[:, n:] == 0.0) and np.all(xl[:, n:] == 0.0))
    for v in range(nrhs):
        if not bp[v].any() and not blp[v].any():
            rec.exact("solve", "an all-zero right-hand side gives exact zeros", np.all(xh[v] == 0.0) and np.all(xl[v] == 0.0))
    Lh, Ll = np.tril(o["Lh"]), np.tril(o["Ll"])
    Lx, el = xdd(Lh, Ll)
    La = np.abs(Lh)
    gamma, g64 = k_dd(q + 2) * EPS_DD, k_dd(DIB + 1) * EPS_DD
    res = _inverse_residuals(o) if form == "bi" else None
    # rho_q = |ri_q L_qq - 1|, exact, from the device's own ri: the substitutions multiply by ri where the analysis divides by L_qq
    rx, er = xdd(o["ri"][0], o["ri"][1])
    dg = np.arange(q)
    one = 1 << -(er + el)
    rho_l = np.abs(flt(rx * Lx[dg, dg] - one, er + el)) * La[dg, dg]
    for v in range(nrhs):
        xx, ex = xdd(xh[v], xl[v])
        bx, eb = xdd(bp[v], blp[v])
        y = Lx.T @ xx                                                   # (x 2^(el + ex)), exact
        Ly = Lx @ y
        a, c, e = _align(bx, eb, Ly, 2 * el + ex)
        err = np.abs(flt(a - c, e))
        ya, xa = np.abs(flt(y, el + ex)), np.abs(xh[v])
        bnd = gamma * (La @ ya + La @ (La.T @ xa))
        if form == "bi":
            back = np.zeros(q)
            for (b, s, Lbh, _, Xh, _), (E, F) in zip(_blocks(o), res):
                Lb, Xb = np.abs(Lbh), np.abs(np.nan_to_num(np.tril(Xh)))
                bnd[s] += (E + g64 * Lb @ Xb) @ (Lb @ ya[s])
                back[s] = (F.T + g64 * Lb.T @ Xb.T) @ (Lb.T @ xa[s])
            bnd += La @ back
        else:
            bnd += rho_l * ya + La @ (rho_l * xa)
        rec.add("solve", "b - L L'x", err, bnd + 1e-300)
    return rec


def check_counter(rec, o, replaced, twin_count=None):
    c = [int(v) for v in o["counter"]]
    rec.exact("counter", "no hand-off lost", c[0] < SYNC_LOST and c[1] < SYNC_LOST and c[0] >= 0)
    rec.exact("counter", "the solves add nothing to it", c[1] == c[0])
    rec.exact("counter", "replaced pivots as the reference plans", c[0] == len(replaced))
    if twin_count is not None:
        rec.exact("counter", "replaced pivots as the twin counts", c[0] == twin_count)
    return rec


def check_all(inp, o, form, nrhs=2, tile=32, pivtol=PIVTOL, sentinel=np.nan, twin_count=None):
    """every stage of one call of the hook (or of the twin).  Returns (rec, facts of the factor stage)."""
    rec = CR.Rec()
    check_update(rec, inp, o, tile, sentinel)
    check_d0(rec, o)
    facts = check_factor(rec, o, pivtol, sentinel)
    check_blockinv(rec, o, form, sentinel)
    check_solve(rec, inp, o, form, nrhs, sentinel)
    check_counter(rec, o, facts["replaced"], twin_count)
    return rec, facts


def failing(rec):
    """the stages a record fails: a fraction above 1 or a failed exact check"""
    return sorted({st for (st, _), _ in rec.over()} | {st for st, _ in rec.failed})


def report(rec, tag):
    w = rec.worst()
    print("ddlin %-34s %s" % (tag, "  ".join("%s %.2g" % (st, w[st]) for st in STAGES if st in w)))


def assert_held(rec, tag):
    report(rec, tag)
    assert not rec.over(), (tag, rec.over())
    assert not rec.failed, (tag, rec.failed)


# ---- the CPU twin: oracle/ddlin.c, and NumPy double-double where it has no counterpart ---------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ah, al, bh, bl):
    sh, sl = _two_sum(ah, bh)
    th, tl = _two_sum(al, bl)
    sh, sl = _quick(sh, sl + th)
    return _quick(sh, sl + tl)


def dd_mul(ah, al, bh, bl):
    ph, pl = _two_prod(ah, bh)
    return _quick(ph, pl + (ah * bl + al * bh))


def dd_div(ah, al, bh, bl):
    q1 = ah / bh
    rh, rl = dd_add(ah, al, *(-t for t in dd_mul(bh, bl, q1, 0.0 * q1)))
    q2 = rh / bh
    rh, rl = dd_add(rh, rl, *(-t for t in dd_mul(bh, bl, q2, 0.0 * q2)))
    q3 = rh / bh
    return dd_add(*_quick(q1, q2), q3, 0.0 * q3)


def dd_sqrt(ah, al):
    x = 1.0 / np.sqrt(ah)
    ax = ah * x
    sh, sl = _two_prod(ax, ax)
    eh, _ = dd_add(ah, al, -sh, -sl)
    return _two_sum(ax, eh * (x * 0.5))


def np_chol(Hh, Hl, pivtol, d0, corrupt=None, at=0):
    """oracle/ddlin.c's dd_chol in NumPy double-double, a column at a time (left-looking, sums over c ascending), with the planted errors
    of test_ddlin_ref_cpu: 'pivot_low' ignores the low word of pivot `at`, 'column_low' zeroes the low words of column `at` below the
    diagonal once it is formed; everything after is computed from the wrong values, as a wrong kernel would."""
    q = len(Hh)
    Lh, Ll = Hh.copy(), Hl.copy()
    nfix = 0
    for j in range(q):
        ah, al = Lh[j:, j].copy(), Ll[j:, j].copy()
        for c in range(j):
            ph, pl = dd_mul(Lh[j:, c], Ll[j:, c], Lh[j, c], Ll[j, c])
            ah, al = dd_add(ah, al, -ph, -pl)
        ph, pl = ah[0], al[0]
        if not ph > pivtol * d0[j]:
            ph, pl, nfix = (d0[j] if d0[j] > 1e-300 else 1e-300), 0.0, nfix + 1
        if corrupt == "pivot_low" and j == at:
            pl = 0.0
        rh, rl = dd_sqrt(np.float64(ph), np.float64(pl))
        vh, vl = dd_div(ah[1:], al[1:], rh, rl)
        if corrupt == "column_low" and j == at:
            vl = np.zeros_like(vl)
        Lh[j, j], Ll[j, j] = rh, rl
        Lh[j + 1:, j], Ll[j + 1:, j] = vh, vl
    return Lh, Ll, nfix


def np_blockinv(Lh, Ll, rih, ril):
    """the product form's inverse of one 64 x 64 block: row i of X from the earlier rows, X_ij = -(sum_k L_ik X_kj) ri_i"""
    m = len(Lh)
    Xh, Xl = np.zeros((m, m)), np.zeros((m, m))
    for i in range(m):
        ah, al = np.zeros(i), np.zeros(i)
        for k in range(i):
            ph, pl = dd_mul(Xh[k, :i], Xl[k, :i], Lh[i, k], Ll[i, k])
            ah, al = dd_add(ah, al, -ph, -pl)
        Xh[i, :i], Xl[i, :i] = dd_mul(ah, al, rih[i], ril[i])
        Xh[i, i], Xl[i, i] = rih[i], ril[i]
    return Xh, Xl


def np_solve_bi(Lh, Ll, dinv, bh, bl):
    """(L L')^-1 b on 64-row blocks with the inverses of the diagonal blocks, one right-hand side"""
    q = len(Lh)
    nb = q // DIB
    yh, yl = bh.copy(), bl.copy()
    for ps in range(2):
        Th, Tl = (Lh, Ll) if ps == 0 else (Lh.T, Ll.T)
        for bb in (range(nb) if ps == 0 else range(nb - 1, -1, -1)):
            s = slice(bb * DIB, (bb + 1) * DIB)
            wh, wl = yh[s].copy(), yl[s].copy()
            for c in (range(bb * DIB) if ps == 0 else range((bb + 1) * DIB, q)):
                ph, pl = dd_mul(Th[s, c], Tl[s, c], yh[c], yl[c])
                wh, wl = dd_add(wh, wl, -ph, -pl)
            Xh, Xl = (dinv[0, bb], dinv[1, bb]) if ps == 0 else (dinv[0, bb].T, dinv[1, bb].T)
            oh, ol = np.zeros(DIB), np.zeros(DIB)
            for c in range(DIB):
                ph, pl = dd_mul(Xh[:, c], Xl[:, c], wh[c], wl[c])
                oh, ol = dd_add(oh, ol, ph, pl)
            yh[s], yl[s] = oh, ol
    return yh, yl


CORRUPTIONS = {"update_low": "update", "pivot_low": "factor", "column_low": "factor", "inverse_low": "blockinv", "solve_low": "solve"}


def twin(inp, form, nrhs=2, nsolve=1, tile=32, pivtol=PIVTOL, corrupt=None, at=0, sentinel=np.nan):
    """what mbfir.test_ddstages returns, from oracle/ddlin.c (rank_k, chol, cho_solve) and the NumPy restatements above; `corrupt`
    plants one of CORRUPTIONS where a wrong kernel would make it, everything downstream computed from the wrong values."""
    from oracle import ddlin
    Hp, Up, bp, blp = padded(inp)
    q, k = len(Hp), inp["k"]
    low, tri = tile_mask(q, tile), np.tril(np.ones((q, q), dtype=bool))
    Hh, Hl = Hp.copy(), np.zeros((q, q))
    if k:
        ddlin.rank_k(np.ascontiguousarray(Up), inp["X"], Hh, Hl)
    Hh, Hl = np.where(tri, Hh, Hh.T), np.where(tri, Hl, Hl.T)           # (the kernel writes both halves of a diagonal tile)
    if corrupt == "update_low":
        Hl[:] = 0.0
    Hh, Hl = np.where(low, Hh, Hp), np.where(low, Hl, sentinel)
    d0 = np.diag(Hh).copy()
    if corrupt in ("pivot_low", "column_low"):
        Lh, Ll, nfix = np_chol(np.ascontiguousarray(Hh), np.nan_to_num(Hl), pivtol, d0, corrupt, at)
    else:
        Lh, Ll = np.ascontiguousarray(Hh).copy(), np.ascontiguousarray(np.nan_to_num(Hl))
        nfix = ddlin.chol(Lh, Ll, pivtol, d0)
    Lh, Ll = np.where(tri, Lh, Hh), np.where(tri, Ll, Hl)
    Lth, Ltl = np.where(tri.T, Lh.T, sentinel), np.where(tri.T, Ll.T, sentinel)
    dg = np.arange(q)
    rih, ril = dd_div(np.ones(q), np.zeros(q), Lh[dg, dg], Ll[dg, dg])
    ri = np.stack([rih, ril])
    dinv = np.full((2, q // DIB, DIB, DIB), sentinel)
    if form == "bi":
        for b in range(q // DIB):
            s = slice(b * DIB, (b + 1) * DIB)
            dinv[0, b], dinv[1, b] = np_blockinv(np.tril(Lh[s, s]), np.tril(Ll[s, s]), rih[s], ril[s])
        if corrupt == "inverse_low":
            dinv[1, at] = np.where(np.eye(DIB, dtype=bool), dinv[1, at], 0.0)
    Lsh, Lsl = np.tril(Lh), np.tril(Ll)
    if corrupt == "solve_low":
        Lsl = np.zeros_like(Lsl)
    xh, xl = np.full((nsolve, 2, q), sentinel), np.full((nsolve, 2, q), sentinel)
    if form == "bi":
        for v in range(nrhs):
            xh[0, v], xl[0, v] = np_solve_bi(Lsh, Lsl, np.nan_to_num(dinv), bp[v], blp[v])
    else:
        Bh, Bl = np.ascontiguousarray(bp[:nrhs].T), np.ascontiguousarray(blp[:nrhs].T)
        ddlin.cho_solve(np.ascontiguousarray(Lsh), np.ascontiguousarray(Lsl), Bh, Bl)
        xh[0, :nrhs], xl[0, :nrhs] = Bh.T, Bl.T
    xh[1:], xl[1:] = xh[0], xl[0]
    return dict(Hh=Hh, Hl=Hl, d0=d0, Lh=Lh, Ll=Ll, Lth=Lth, Ltl=Ltl, ri=ri, dinv=dinv, xh=xh, xl=xl, counter=np.array([nfix, nfix], dtype=np.int32))

