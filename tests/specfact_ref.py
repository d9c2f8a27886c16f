"""Reference of the tap extraction's arithmetic (csrc/specfact.hip: k_specfact, kind 0, and k_fmp, kind 1) for
mbfir.test_specfact_stages, stage by stage.  tests/test_specfactstages_gpu.py holds the device to it, tests/test_specfactstages_cpu.py
holds a float64 twin to it and shows that it rejects planted errors.  NumPy only (numpy.longdouble, 64-bit mantissa here), the
transforms and twiddles are flip_ref's (dft_ld, tw_ld); nothing here needs a GPU and nothing is shared with specfact.hip or
oracle/specfact.py.

What is computed (fir_ap_cvx.m:185-186, 264-304; fmp.m:12-23), lp = 8 * 2^ceil(log2 l), hlp = lp / 2, L = log2 lp:
    in      kind 0: x (2n - 1 reals) -> r, the two-sided Hermitian autocorrelation of l = 2n - 1 lags; kind 1: h, l complex taps
    hpf     fft(fftshift(hp)), hp = [zeros(ceil((lp - l) / 2)), r or h, zeros(floor((lp - l) / 2))]: the centre tap lands on index 0,
            so for kind 0 hpf is real up to rounding.  Stored as the transform leaves it (bin k of the unshifted transform).
    lift    kind 1: 1.000001 min_k real(hpf_k) (one product, the minimum is exact); kind 0: 0
    xl      xl_i = log(sqrt(|hpf_{(i + hlp) mod lp} - lift|))
    xlfp    fft(xl), bins 1 .. hlp - 1 doubled, bins above hlp zero, DC and hlp as they are
    a       exp(ifft(xlfp))
    h       ifft(fftshift(conj(a)))(0 : m), m = n (kind 0) or (l + 1) / 2 (kind 1)

Stage checks (`stage_fractions`).  Every stage's reference is computed in long double from the DEVICE's (or twin's) output of the
stage before (hpf: from the input), so a failure names one stage, conditioning cannot hide an error or excuse one, and each bound
is that stage's own rounding, to first order in u = 2^-53.  A stage is held to TWO bounds and its fraction is the larger ratio.

The transforms.  fft_inplace is a bit reversal (exact) and L levels of butterflies  u +- w t,  w = sincospi of a dyadic (exactly
representable) argument, correct to 2 u per component (flip_ref's budget for this device's sincospi), so 2 sqrt2 u in modulus.
    per entry: a level multiplies what passes through it by the twiddle (2 sqrt2 u for its own error, 2 sqrt2 u for the complex
        product: flip_ref's rule) and adds (one rounding per component, sqrt2 u in modulus), and no partial sum exceeds the sum of
        the magnitudes below it:   |y^_k - y_k| <= L 5 sqrt2 u sum_j |x_j|.
    in norm: Higham, Accuracy and Stability of Numerical Algorithms, theorem 24.2 (radix-2 Cooley-Tukey, twiddles within mu):
        ||y^ - y||_2 <= L eta ||y||_2,  eta = mu + gamma_4 (sqrt2 + mu) = (2 sqrt2 + 4 sqrt2) u to first order,  ||y||_2 = sqrt(lp) ||x||_2.
        Roundings are independent, so a correct transform sits near 1 / (eta sqrt L) of this bound where the entry-wise bound, which
        must allow every rounding to line up, leaves a factor sqrt(lp) unused: the norm is what catches a slightly wrong twiddle.
    The scale 1 / lp of the inverse transforms is a power of two: exact.
The pointwise stages, from their operation sequences (the function budgets are flip_ref's: hypot 2 u, sqrt 1 u, log 2 u |log|,
exp 2 u, sincos 2 u per component):
    lift    one rounding: u |lift|.
    xl      the subtraction (kind 1 only) moves |hpf - lift| by at most u of itself, hypot by 2 u, the root halves both and adds u of
            its own, the logarithm turns relative into absolute and adds 2 u |xl|:   ((2 + s) / 2 + 1) u + 2 u |xl|,  s = 1 for kind 1.
            Where the modulus is exactly 0 the reference is -inf and the device must give -inf.
    xlfp    the transform's bounds times the window (1 or 2; doubling is exact); entries above hlp must be exactly 0.
    a       with w = ifft(xlfp) off by dw (the transform's bound over lp):  |a| (dw + (2 + 2 sqrt2 + 1) u)  -- exp, sincos in modulus,
            the product; in norm the same for the vector (a^ - a) / |a|.
    h       the transform's bounds over lp; in norm over the m taps kept (a part of the vector cannot exceed the whole).

End to end (`chain`): the same stages in long double from the input without rounding in between, and the bounds of stages 2 .. 5
carried forward to first order (d xlfp <= g sum d xl; d w <= sum d xlfp / lp; d a <= |a| d w; d h <= sum d a / lp).  Stage 1 is
not carried forward linearly: where the spectrum touches zero, log |hpf| is not Lipschitz, and how far the taps move under the
stage-1 bound is the input's own property.  `spread` measures it on the reference itself: the chain's taps with hpf moved by
+- the stage-1 entry-wise bound per sample, random signs, eight draws, the largest movement of any tap.  The taps are then held to
2 spread + the carried-forward bound; the factor 2 covers the directions eight draws do not sample.
"""
import functools
import json
import os

import numpy as np

import flip_ref as fr

LD, CLD, U, SQ2 = fr.LD, fr.CLD, fr.U, fr.SQ2
STAGES = ("hpf", "xl", "xlfp", "a", "h")
C_ENTRY = 5 * SQ2 * U             # per butterfly level, entry-wise, times sum |x|
ETA = 6 * SQ2 * U                 # per butterfly level, in norm (Higham 24.2 with mu = 2 sqrt2 u)
C_EXP = (3 + 2 * SQ2) * U         # exp, sincos (modulus) and the product, relative to |a|
LIFT = LD(np.float64(1.000001))   # the kernel's constant is the double nearest to 1.000001
NDRAW = 8


def lp_of(l):
    p = 1
    while p < l:
        p <<= 1
    return 8 * p


def taps_of(kind, n):
    """(l, m): the length that is padded and the number of taps kept; n is the order (kind 0) or the filter length (kind 1)."""
    return (2 * n - 1, n) if kind == 0 else (n, (n + 1) // 2)


def _f(x):
    return np.asarray(x).astype(np.float64)


def _norm2(x, axis=-1):
    x = np.abs(np.asarray(x)).astype(LD)
    return _f(np.sqrt((x * x).sum(axis=axis)))


def place(kind, inp, n):
    """fftshift(hp) in long double (placement only: exact).  inp: lanes x (2n - 1) reals (kind 0) or lanes x l complex (kind 1)."""
    l, _ = taps_of(kind, n)
    lp = lp_of(l)
    if kind == 0:
        x = np.atleast_2d(np.asarray(inp, dtype=np.float64)).astype(LD)
        r = np.zeros((x.shape[0], n), dtype=CLD)
        r.real[:, 0] = x[:, 0]
        r.real[:, 1:], r.imag[:, 1:] = x[:, 1:n], x[:, n:]
        v = np.concatenate([np.conj(r[:, :0:-1]), r], axis=1)
    else:
        v = np.atleast_2d(np.asarray(inp)).astype(CLD)
    assert v.shape[1] == l
    pad = lp - l
    hp = np.zeros((v.shape[0], lp), dtype=CLD)
    hp[:, -(-pad // 2):-(-pad // 2) + l] = v
    return np.roll(hp, -(lp // 2), axis=1)


def _levels(lp):
    return int(lp).bit_length() - 1


def fft_bounds(x):
    """(entry-wise, in norm) bounds of one radix-2 transform of x (.. x lp) as the kernel runs it, both of shape (.., 1)."""
    lp = x.shape[-1]
    L = _levels(lp)
    ent = L * C_ENTRY * _f(np.abs(x).sum(axis=-1, keepdims=True))
    nrm = L * ETA * np.sqrt(lp) * _norm2(x)[..., None]
    return ent, nrm


def ref_hpf(B0):
    B0 = np.asarray(B0, dtype=CLD)
    return (fr.dft_ld(B0),) + fft_bounds(B0)


def ref_lift(kind, hpf):
    """The lift the kernel takes from ITS hpf, and the bound of its one rounding."""
    hpf = np.asarray(hpf)
    if kind == 0:
        z = np.zeros(hpf.shape[:-1], dtype=LD)
        return z, _f(z)
    lift = hpf.real.min(axis=-1).astype(LD) * LIFT
    return lift, U * _f(np.abs(lift))


def ref_xl(kind, hpf, lift):
    hpf = np.asarray(hpf).astype(CLD)
    lp = hpf.shape[-1]
    v = np.roll(hpf, -(lp // 2), axis=-1)
    with np.errstate(divide="ignore"):
        xl = np.log(np.hypot(v.real - np.asarray(lift, dtype=LD)[..., None], v.imag)) / 2
    s = 1.0 if kind == 1 else 0.0
    with np.errstate(invalid="ignore"):
        bound = ((2 + s) / 2 + 1) * U + 2 * U * _f(np.abs(xl))
    return xl, bound


def window(lp):
    g = np.zeros(lp)
    g[0] = g[lp // 2] = 1.0
    g[1:lp // 2] = 2.0
    return g


def ref_xlfp(xl):
    xl = np.asarray(xl).astype(CLD)
    g = window(xl.shape[-1])
    ent, nrm = fft_bounds(xl)
    return fr.dft_ld(xl) * g, g * ent, 2 * nrm


def ref_a(xlfp):
    xlfp = np.asarray(xlfp).astype(CLD)
    lp = xlfp.shape[-1]
    w = fr.dft_ld(xlfp, sign=+1) / lp
    a = np.exp(w.real) * (np.cos(w.imag) + 1j * np.sin(w.imag))
    ent, nrm = fft_bounds(xlfp)
    # entry-wise |a^ - a| <= |a| (dw + C_EXP); in norm || (a^ - a) / |a| ||_2 <= ||dw||_2 + C_EXP sqrt(lp)
    return a, _f(np.abs(a)) * (ent / lp + C_EXP), nrm / lp + C_EXP * np.sqrt(lp)


def ref_h(a, m):
    a = np.asarray(a).astype(CLD)
    lp = a.shape[-1]
    B2 = np.conj(np.roll(a, -(lp // 2), axis=-1))
    ent, nrm = fft_bounds(B2)
    return (fr.dft_ld(B2, sign=+1) / lp)[..., :m], ent / lp, nrm / lp


def _ratio(err, bound):
    """max err / bound over everything; no error is ratio 0 whatever the bound (the window's zeros), a nan counts as inf."""
    err = _f(err)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(np.where(np.isnan(q), np.inf, q))) if q.size else 0.0


def _diff(got, ref):
    """|got - ref| in long double; nan where got and ref are the same infinity is turned into 0."""
    got, ref = np.asarray(got), np.asarray(ref)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(ref.dtype) - ref)
    same_inf = np.isinf(_f(np.abs(ref))) & (_f(got.real) == _f(ref.real)) & (_f(np.imag(got)) == _f(np.imag(ref)))
    return np.where(same_inf, 0, d)


def stage_fractions(got, kind, inp, n, stages=None):
    """got: the stages of every lane (st_hpf, st_xl, st_xlfp, st_a, st_h as lanes x .. arrays, lift per lane) as mbfir.test_specfact_stages
    returns them.  For each stage the worst of |got - ref| / entry-wise bound and ||got - ref||_2 / norm bound per lane (an array
    over the lanes), the reference taken from got's own stage before.  kind 1 adds "lift".  Also what must hold exactly."""
    _, m = taps_of(kind, n)
    out, exact = {}, {}
    want = STAGES if stages is None else stages
    per_lane = lambda d, ent, nrm: np.maximum(                                     # noqa: E731
        np.array([_ratio(d[q], np.broadcast_to(ent, d.shape)[q]) for q in range(d.shape[0])]), _norm2(d) / nrm[..., 0])
    if "hpf" in want:
        hpf, ent, nrm = ref_hpf(place(kind, inp, n))
        out["hpf"] = per_lane(_diff(got["st_hpf"], hpf), ent, nrm)
        if kind == 0:                                                             # r is Hermitian: the spectrum is real
            exact["hpf_imag"] = bool(np.all(np.abs(got["st_hpf"].imag) <= ent))
    lift = np.asarray(got["lift"], dtype=np.float64)
    if kind == 1:
        rl, bl = ref_lift(kind, got["st_hpf"])
        out["lift"] = _f(np.abs(lift.astype(LD) - rl)) / bl
    else:
        exact["lift"] = bool(np.all(lift == 0.0))
    if "xl" in want:
        xl, b = ref_xl(kind, got["st_hpf"], lift)
        out["xl"] = np.array([_ratio(_diff(got["st_xl"][q], xl[q]), b[q]) for q in range(len(xl))])
    if "xlfp" in want:
        X, ent, nrm = ref_xlfp(got["st_xl"])
        out["xlfp"] = per_lane(_diff(got["st_xlfp"], X), ent, nrm)
        lp = X.shape[-1]
        exact["xlfp_zero"] = bool(np.all(got["st_xlfp"][..., lp // 2 + 1:] == 0))
    if "a" in want:
        a, ent, nrm = ref_a(got["st_xlfp"])
        d = _diff(got["st_a"], a)
        rel = _f(d) / _f(np.abs(a))
        out["a"] = np.maximum(np.array([_ratio(d[q], ent[q]) for q in range(len(d))]), _norm2(rel) / nrm[..., 0])
    if "h" in want:
        h, ent, nrm = ref_h(got["st_a"], m)
        out["h"] = per_lane(_diff(got["st_h"], h), ent, nrm)
    return out, exact


def chain(kind, inp, n, hpf=None):
    """End to end in long double from the input (or from a given hpf, for `spread`).  Returns the stages, the taps and the bound of
    stages 2 .. 5 carried forward to first order (per tap)."""
    _, m = taps_of(kind, n)
    b1 = None
    if hpf is None:
        hpf, b1, _ = ref_hpf(place(kind, inp, n))
    lp = hpf.shape[-1]
    lift, bl = ref_lift(kind, hpf)
    xl, b_xl = ref_xl(kind, hpf, lift)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_arg = bl[..., None] / _f(np.abs(np.roll(hpf, -(lp // 2), axis=-1) - lift[..., None]))   # the lift's rounding, seen by the log
    d_xl = b_xl + d_arg / 2
    X, b_X, _ = ref_xlfp(xl)
    d_X = b_X + window(lp) * d_xl.sum(axis=-1, keepdims=True)
    a, b_a, _ = ref_a(X)
    d_a = b_a + _f(np.abs(a)) * d_X.sum(axis=-1, keepdims=True) / lp
    h, b_h, _ = ref_h(a, m)
    d_h = b_h + d_a.sum(axis=-1, keepdims=True) / lp
    return dict(hpf=hpf, b_hpf=b1, lift=lift, xl=xl, xlfp=X, a=a, h=h, h_bound=np.broadcast_to(d_h, h.shape))


def spread(kind, inp, n, seed=0):
    """Per lane: how far the long-double chain's taps move when its hpf takes +- the stage-1 entry-wise bound per sample (random
    signs, NDRAW draws, the largest movement of any tap).  The reference's own sensitivity; nothing of the code under test enters.
    kind 0 moves the real part (the spectrum of a Hermitian r is real), kind 1 both parts.  Returns (spread, the unmoved chain)."""
    base = chain(kind, inp, n)
    lanes, lp = base["hpf"].shape
    rng = np.random.default_rng(seed)
    sg = rng.choice([-1.0, 1.0], size=(NDRAW, lanes, lp))
    if kind == 1:
        sg = sg + 1j * rng.choice([-1.0, 1.0], size=(NDRAW, lanes, lp))
    moved = (base["hpf"][None] + (sg * base["b_hpf"][None]).astype(CLD)).reshape(NDRAW * lanes, lp)
    with np.errstate(all="ignore"):
        h = chain(kind, None, n, hpf=moved)["h"].reshape(NDRAW, lanes, -1)
        worst = np.fmax.reduce(_f(np.abs(h - base["h"][None]).max(axis=-1)), axis=0)
    return worst, base


# ---- the float64 twin: the kernel's order (bit reversal, radix-2 levels) in NumPy, with switches that plant errors ---------------
PLANTS = ("tw32", "twrot", "nyq2", "dc2", "zero_hlp", "padfloor", "noconj", "nosqrt", "inv2", "inv0", "lift5", "minabs")


def _twiddles(m, sign, plant):
    half = m // 2
    if plant == "twrot" and half > 1:                     # one rotation per step across the whole level
        w1 = complex(fr.tw_ld(m)[1])
        w = np.empty(half, dtype=np.complex128)
        w[0] = 1.0
        for j in range(1, half):
            w[j] = w[j - 1] * w1
    else:
        w = fr.tw_ld(m)[:half].astype(np.complex128)
    if plant == "tw32":
        w = w.astype(np.complex64).astype(np.complex128)
    return w if sign < 0 else np.conj(w)


def twin_fft(a, sign, plant=None):
    a = np.array(a, dtype=np.complex128)
    lp = a.shape[-1]
    L = _levels(lp)
    idx = np.arange(lp)
    rev = np.zeros(lp, dtype=np.int64)
    for b in range(L):
        rev |= ((idx >> b) & 1) << (L - 1 - b)
    a = a[..., rev]
    for s in range(1, L + 1):
        m, half = 1 << s, 1 << (s - 1)
        w = _twiddles(m, sign, plant)
        v = a.reshape(a.shape[:-1] + (lp // m, m))
        u, t = v[..., :half], w * v[..., half:]
        a = np.concatenate([u + t, u - t], axis=-1).reshape(a.shape)
    return a


def twin(kind, inp, n, plant=None):
    """Every stage in float64, each from the twin's own stage before: the dict stage_fractions takes."""
    l, m = taps_of(kind, n)
    lp = lp_of(l)
    hlp = lp // 2
    B0 = place(kind, inp, n).astype(np.complex128)
    if plant == "padfloor":                               # pad_lo = floor((lp - l) / 2): the centre tap one sample early
        B0 = np.roll(B0, -1, axis=-1)
    hpf = twin_fft(B0, -1, plant)
    if kind == 1:
        mn = np.abs(hpf).min(axis=-1) if plant == "minabs" else hpf.real.min(axis=-1)
        lift = mn * (1.00001 if plant == "lift5" else 1.000001)
    else:
        lift = np.zeros(hpf.shape[0])
    v = np.roll(hpf, -hlp, axis=-1)
    with np.errstate(divide="ignore"):
        mod = np.hypot(v.real - lift[:, None], v.imag).astype(LD)      # the logarithm in long double: its bound has no factor to spare
        xl = (np.log(mod) if plant == "nosqrt" else np.log(mod) / 2).astype(np.float64)
    X = twin_fft(xl, -1, plant)
    i = np.arange(lp)
    dbl = (i >= 1) & (i <= hlp if plant == "nyq2" else i < hlp)
    if plant == "dc2":
        dbl |= i == 0
    zero = i >= hlp if plant == "zero_hlp" else i > hlp
    with np.errstate(invalid="ignore"):
        xlfp = np.where(zero, 0, np.where(dbl, 2 * X, X))
        w = twin_fft(xlfp, +1, plant) / lp
        a = np.exp(w)
        B2 = np.roll(a, -hlp, axis=-1)
        if plant != "noconj":
            B2 = np.conj(B2)
        h = twin_fft(B2, +1, plant)[..., :m] * {"inv2": 1.0 / lp / lp, "inv0": 1.0}.get(plant, 1.0 / lp)
    return dict(st_hpf=hpf, lift=lift, st_xl=xl, st_xlfp=xlfp, st_a=a, st_h=h)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def autocorr_x(n, seed=None, scale=1.0):
    """(A): the autocorrelation of n random complex taps as the designers' x, as test_spectral_factorisation_matches_oracle builds it."""
    rng = np.random.default_rng(n if seed is None else seed)
    h0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    r = np.correlate(h0, h0, mode="full")[n - 1:] * scale
    return np.concatenate([[r[0].real], r[1:].real, r[1:].imag])


ZERO_X = np.array([2.0, -1.0, 0.0])                        # (D): r = [-1, 2, -1], hpf_0 = 0 exactly
N_MAX = 4096                                               # the largest n with lp <= 65536
SIZES = (1, 2, 3, 16, 17, 33, 64, 65, 257, 512, 2048, N_MAX)
T_LEVELS = (1e-6, 1e-9, 1e-12, 1e-15, 0.0)
FMP_SIZES = (3, 5, 31, 33, 129)


def fmp_input(l, cplx):
    """A symmetric low-pass of odd length l (a windowed sinc over a ripple floor), modulated when cplx."""
    t = np.arange(l) - (l - 1) / 2
    h = np.sinc(t / 4) * np.hamming(l) / 4
    return h * np.exp(0.3j * t) if cplx else h


def touch(x, n, t):
    """(C): x with x[0] shifted (every sample of hpf moves by the same amount) so that the sample of smallest |real hpf| sits at
    t max|hpf|, in long double.  The spectrum crosses zero in several places, so putting ONE sample there may push another one closer;
    the shift taken is the smallest d = -v_k +- t max for which no sample ends up nearer to zero than t max (t = 0: d = -v_k of the
    sample nearest to zero)."""
    v = ref_hpf(place(0, x, n))[0][0].real
    lvl = LD(t) * np.abs(v).max()
    cand = np.concatenate([-v + lvl, -v - lvl])
    for d in cand[np.argsort(np.abs(cand))]:
        if np.abs(v + d).min() >= lvl * (1 - LD(1e-9)):
            break
    out = np.array(x, dtype=np.float64)
    out[0] = np.float64(LD(out[0]) + d)
    return out


# ---- the cases both test files run (section "inputs" above; the multi-lane launches are put together from these by the GPU test) ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (kind, input, n): (A) A_n<n> and A_n33_tiny, (B) B_<name>, (C) C_<name>_<t>, (D) D_zero, k_fmp: F_<l>_real / _cplx and
    F_<design> (the conventional fixtures' equiripple filters, the 2047-tap one among them)."""
    out = {}
    for n in SIZES:
        out["A_n%d" % n] = (0, autocorr_x(n), n)
    out["A_n33_tiny"] = (0, autocorr_x(33, scale=1e-12), 33)
    with np.load(os.path.join(GOLDEN, "specfact_cases.npz")) as z:
        for k in z.files:
            x = z[k]
            out[k.replace("/", "_")] = (0, x, (len(x) + 1) // 2)
    out["D_zero"] = (0, ZERO_X, 2)
    for l in FMP_SIZES:
        out["F_%d_real" % l] = (1, fmp_input(l, False), l)
        out["F_%d_cplx" % l] = (1, fmp_input(l, True), l)
    with open(os.path.join(GOLDEN, "conventional.json")) as fh:
        conv = json.load(fh)
    with np.load(os.path.join(GOLDEN, "conventional.npz")) as z:
        for k in sorted(conv["fmp"]):
            hh = z["remez/" + k]
            l = conv["remez"][k]["numtaps"]
            out["F_" + k] = (1, np.concatenate([hh, hh[::-1][l % 2:]]), l)
    l = conv["remez"]["dzlp2047"]["numtaps"]
    out["F_dzlp2047_cplx"] = (1, out["F_dzlp2047"][1] * np.exp(0.01j * np.arange(l)), l)
    return out


def family(name):
    return name[0]


def strict(name):
    """The cases whose spread must stay below STRICT max|h|: all of (A), and (C) with t >= 1e-6."""
    return family(name) == "A" or (family(name) == "C" and float(name.rsplit("_", 1)[1]) >= 1e-6)


STRICT, LOOSE = 1e-9, 1e-5


@functools.lru_cache(maxsize=None)
def reference(name):
    """(spread, chain) of a case, computed once per process: the long-double transforms of the longest cases take seconds."""
    kind, inp, n = cases()[name]
    return spread(kind, inp, n)
