"""Echo-planar spin-echo spectral-spatial pulses: rf_tools/dzepse.m and the pieces it stands on.

    rf = dzepse(ang, gx, tbx, tgx, ngx, sbw, srip1, srip2, stype)   # rf_tools/dzepse.m   2D inverse SLR
    rfs = dzepse_batch(specs)                                        # many designs, grouped device launches
    beta = dzbeta(np, tb, ptype, ftype, d1, d2)                      # rf_tools/dzbeta.m   dzrf without the inverse SLR
    rfv = verse(g, rf), versec(g, rf)                                # rf_tools/verse.m, versec.m
    y = fftc(x), hf = fftcp(h, n)                                    # rf_tools/fftc.m, fftcp.m
    ab2ex, ab2se, ab2inv, ab2sat, ab2st                              # rf_tools/ab2*.m profiles of (a, b)

The two inverse-SLR stages of dzepse run on the device, each as ONE mbfir.b2rf_batch launch (rows, then columns); the pm / min /
max spectral filters go through the device Parks-McClellan batch.  Everything else is host NumPy: a few small FFTs and an
interpolation.  The one intended difference from the reference: an unknown ptype or ftype raises instead of printing and
returning nothing, and so does an odd gradient length, which dzepse.m cannot index.
"""
import math
import sys

import numpy as np

from . import slrclassic

_pkg = sys.modules[__package__]          # the package (bindings looked up at call time)


# ---- centred FFTs --------------------------------------------------------------------------------------------
def fftc(x):
    """`y = fftc(x)` (fftc.m): the FFT taken about the centre of the array, fftshift(fft(fftshift(x)))."""
    return np.fft.fftshift(np.fft.fft(np.fft.fftshift(np.asarray(x, dtype=np.complex128).ravel())))


def fftcp(h, n):
    """`hf = fftcp(h, n)` (fftcp.m): fftc of h padded with ceil(n/2 - l/2) zeros in front and floor(n/2 - l/2) behind."""
    h = np.asarray(h, dtype=np.complex128).ravel()
    l = len(h)
    return fftc(np.concatenate([np.zeros(int(math.ceil(n / 2 - l / 2))), h, np.zeros(int(math.floor(n / 2 - l / 2)))]))


# ---- dzbeta.m --------------------------------------------------------------------------------------------------
def _beta_filter(np_, tb, ftype, d1, d2, res=None, ctx=None):
    """The filter of dzbeta.m:40-57 (ripples already mapped).  res: the remez_batch result of a pm / min / max design, else it
    is designed here."""
    if ftype == "ms":
        return slrclassic.msinc(np_, tb / 4)
    if ftype == "ls":
        return slrclassic.dzls(np_, tb, d1, d2)
    if ftype not in ("pm", "min", "max"):
        raise ValueError("dzbeta: unrecognized filter design method %r; options are ms, pm, min, max and ls" % (ftype,))
    if res is None:
        spec = (slrclassic.dzlp_spec if ftype == "pm" else slrclassic.dzmp_spec)(np_, tb, d1, d2)
        res = slrclassic.remez_batch([spec], ctx=ctx)[0]
    b, info = res
    if info["status"] != "converged":
        raise _pkg.MbfirError("dzbeta: remez %s after %d iterations" % (info["status"], info["iterations"]))
    if ftype == "pm":
        return b
    return slrclassic.fmp(b, ctx=ctx)[::-1 if ftype == "min" else 1]     # 'min' is the reversed factor (:48-50)


def _remez_spec(np_, tb, ftype, d1, d2):
    return (slrclassic.dzlp_spec if ftype == "pm" else slrclassic.dzmp_spec)(np_, tb, d1, d2)


def dzbeta(np_, tb, ptype="st", ftype="ls", d1=0.01, d2=0.01, pclsfrac=1.5, *, ctx=None):
    """`beta = dzbeta(np, tb, ptype, ftype, d1, d2)` (rf_tools/dzbeta.m): the beta polynomial dzrf would invert -- the filter of
    ftype ms | pm | ls | min | max with dzrf.m's ripple mapping for ptype st | ex | se | inv | sat, times bsf unless 'st'.
    pclsfrac is accepted and unused, as in the reference."""
    r1, r2, bsf = slrclassic.ptype_ripples(ptype, d1, d2)
    b = _beta_filter(np_, tb, ftype, r1, r2, ctx=ctx)
    return b if ptype == "st" else bsf * b


# ---- verse.m / versec.m ------------------------------------------------------------------------------------------
def _as_columns(rf):
    """rf as the reference's matrix (a 1D array is a MATLAB row vector), transposed (conj(rf') = rf.') when it has fewer rows than
    columns (verse.m:13-16, versec.m:3-6)."""
    rf = np.asarray(rf)
    if rf.ndim == 1:
        rf = rf[None, :]
    if rf.shape[0] < rf.shape[1]:
        rf = rf.T
    return rf


def _spline_slopes(x, y):
    """Node slopes of the not-a-knot cubic spline through (x, y) (MATLAB's spline, scipy's CubicSpline 'not-a-knot'); y is
    (m, ncol), m >= 2."""
    m = len(x)
    dx = np.diff(x)[:, None]
    sl = np.diff(y, axis=0) / dx
    if m == 2:
        return np.vstack([sl, sl])
    if m == 3:                                             # one parabola through the three points
        A = np.array([[1.0, 1.0, 0.0], [dx[1, 0], 2 * (dx[0, 0] + dx[1, 0]), dx[0, 0]], [0.0, 1.0, 1.0]])
        rhs = np.vstack([2 * sl[0], 3 * (dx[1] * sl[0] + dx[0] * sl[1]), 2 * sl[1]])
        return np.linalg.solve(A, rhs)
    # tridiagonal system: sub[i] s[i-1] + dia[i] s[i] + sup[i] s[i+1] = rhs[i]
    sub, dia, sup = np.zeros(m), np.zeros(m), np.zeros(m)
    rhs = np.zeros((m,) + y.shape[1:], dtype=y.dtype)
    dia[1:-1] = 2 * (dx[:-1, 0] + dx[1:, 0])
    sup[1:-1] = dx[:-1, 0]
    sub[1:-1] = dx[1:, 0]
    rhs[1:-1] = 3 * (dx[1:] * sl[:-1] + dx[:-1] * sl[1:])
    d = x[2] - x[0]                                        # not-a-knot at the first interior node
    dia[0], sup[0] = dx[1, 0], d
    rhs[0] = ((dx[0] + 2 * d) * dx[1] * sl[0] + dx[0] ** 2 * sl[1]) / d
    d = x[-1] - x[-3]                                      # ... and at the last
    dia[-1], sub[-1] = dx[-2, 0], d
    rhs[-1] = (dx[-1] ** 2 * sl[-2] + (2 * d + dx[-1]) * dx[-2] * sl[-1]) / d
    # Thomas elimination (the system is diagonally dominant apart from its end rows, which pivot fine for spline data)
    cp = np.zeros(m)
    dp = np.zeros_like(rhs)
    cp[0] = sup[0] / dia[0]
    dp[0] = rhs[0] / dia[0]
    for i in range(1, m):
        den = dia[i] - sub[i] * cp[i - 1]
        cp[i] = sup[i] / den if i < m - 1 else 0.0
        dp[i] = (rhs[i] - sub[i] * dp[i - 1]) / den
    s = np.zeros_like(rhs)
    s[-1] = dp[-1]
    for i in range(m - 2, -1, -1):
        s[i] = dp[i] - cp[i] * s[i + 1]
    return s


def spline_interp(x, y, xq):
    """interp1(x, y, xq, 'spline'): not-a-knot cubic spline, extrapolated by the end pieces outside [x(1), x(end)].  y: (m,) or
    (m, ncol); returns (len(xq),) or (len(xq), ncol)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y)
    vec = y.ndim == 1
    y2 = y[:, None] if vec else y
    if len(x) < 2 or len(x) != y2.shape[0]:
        raise ValueError("spline: need at least two points and one value per point")
    s = _spline_slopes(x, y2)
    xq = np.asarray(xq, dtype=np.float64).ravel()
    i = np.clip(np.searchsorted(x, xq, side="right") - 1, 0, len(x) - 2)
    h = (x[i + 1] - x[i])[:, None]
    t = (xq - x[i])[:, None]
    sl = (y2[i + 1] - y2[i]) / h
    c2 = (3 * sl - 2 * s[i] - s[i + 1]) / h
    c3 = (s[i] + s[i + 1] - 2 * sl) / (h * h)
    out = y2[i] + t * (s[i] + t * (c2 + t * c3))
    return out[:, 0] if vec else out


def _verse_axis(g, m):
    g = np.asarray(g, dtype=np.float64).ravel()
    k = np.cumsum(g)
    k = (m - 1) * k / np.max(k)
    return k, m * g / np.sum(g)


def verse(g, rf):
    """`rfv = verse(g, rf)` (verse.m): rf resampled onto the time-varying gradient g.  Literal restatement: the samples sit at
    1 .. m while k = (m - 1) cumsum(g) / max(cumsum(g)) runs up to m - 1 and below 1, so interp1's spline extrapolates there.
    rf: a vector (a MATLAB row, so transposed) or an (m, n) matrix whose columns are resampled; returns (len(g), n)."""
    rf = _as_columns(np.asarray(rf, dtype=np.complex128) if np.iscomplexobj(rf) else np.asarray(rf, dtype=np.float64))
    m = rf.shape[0]
    k, gs = _verse_axis(g, m)
    return gs[:, None] * spline_interp(np.arange(1, m + 1, dtype=np.float64), rf, k)


def versec(g, rf):
    """`rfv = versec(g, rf)` (versec.m): as verse, on the grid 0 .. m - 1 with linear interpolation (interp1's default; NaN
    outside the grid).  Returns (len(g), n): column j is the reference's j-th block of rfv."""
    rf = _as_columns(np.asarray(rf, dtype=np.complex128) if np.iscomplexobj(rf) else np.asarray(rf, dtype=np.float64))
    m = rf.shape[0]
    k, gs = _verse_axis(g, m)
    grid = np.arange(m, dtype=np.float64)
    cols = [np.interp(k, grid, rf[:, j], left=np.nan, right=np.nan) for j in range(rf.shape[1])]
    return gs[:, None] * np.stack(cols, axis=1)


# ---- ab2*.m ------------------------------------------------------------------------------------------------------------
def _split_ab(a, b):
    if b is not None:
        return np.asarray(a), np.asarray(b)
    ab = np.asarray(a)
    n = ab.shape[1]
    return ab[:, :n // 2], ab[:, n // 2:]


def ab2ex(a, b=None):
    """`mxy = ab2ex(a, b)` or `ab2ex([a b])` (ab2ex.m): excitation profile 2 conj(a) b."""
    a, b = _split_ab(a, b)
    return 2 * np.conj(a) * b


def ab2se(a, b=None):
    """`mxy = ab2se(a, b)` or `ab2se([a b])` (ab2se.m): spin-echo profile i b^2."""
    a, b = _split_ab(a, b)
    return 1j * b * b


def ab2inv(a, b=None):
    """`mz = ab2inv(a, b)` or `ab2inv([a b])` (ab2inv.m): inversion profile 1 - 2 |b|^2."""
    a, b = _split_ab(a, b)
    return 1 - 2 * (np.conj(b) * b).real


def ab2sat(a, b=None):
    """`mz = ab2sat(a, b)` or `ab2sat([a b])` (ab2sat.m): saturation profile 1 - 2 |b|^2."""
    a, b = _split_ab(a, b)
    return 1 - 2 * (np.conj(b) * b).real


def ab2st(a, b=None):
    """`mxy = ab2st(a, b)` (ab2st.m): the straight-through term i a^2; with one argument the first column of a is used."""
    a = np.asarray(a)
    if b is None:
        a = a[:, 0]
    return 1j * a * a


# ---- dzepse.m --------------------------------------------------------------------------------------------------------
_SPEC_NAMES = ("ang", "gx", "tbx", "tgx", "ngx", "sbw", "srip1", "srip2", "stype")
_SPEC_DEFAULTS = {"srip1": 0.01, "srip2": 0.01, "stype": "pm"}


def _norm_spec(s):
    if isinstance(s, dict):
        missing = [k for k in _SPEC_NAMES[:6] if k not in s]
        if missing:
            raise ValueError("dzepse: missing argument(s) %s" % ", ".join(missing))
        s = tuple(s.get(k, _SPEC_DEFAULTS.get(k)) for k in _SPEC_NAMES)
    s = tuple(s)
    if not 6 <= len(s) <= 9:
        raise ValueError("dzepse: takes 6 to 9 arguments (ang, gx, tbx, tgx, ngx, sbw[, srip1, srip2, stype])")
    s = s + tuple(_SPEC_DEFAULTS[k] for k in _SPEC_NAMES[len(s):])
    ang, gx, tbx, tgx, ngx, sbw, srip1, srip2, stype = s
    gx = np.asarray(gx, dtype=np.float64).ravel()
    lgx, ngx = len(gx), int(ngx)
    if lgx < 2 or lgx % 2:
        raise ValueError("dzepse: the gradient lobe needs an even number of samples >= 2 (dzepse.m indexes 0.5 lgx + 1 : 1.5 lgx); "
                         "got %d" % lgx)
    if ngx != s[4] or not 2 <= ngx <= 2048:
        raise ValueError("dzepse: ngx must be an integer in [2, 2048]")
    if lgx > 2048:
        raise ValueError("dzepse: at most 2048 samples per lobe")
    if stype not in ("ms", "pm", "ls", "min", "max"):
        raise ValueError("dzepse: unrecognized spectral filter type %r; options are ms, pm, min, max and ls" % (stype,))
    if not np.all(np.isfinite(gx)) or np.max(np.cumsum(gx)) <= 0 or np.sum(gx) == 0:
        raise ValueError("dzepse: the gradient lobe must be finite with a positive area")
    tbs = (ngx - 1) * float(tgx) * float(sbw)                     # dzepse.m:30-31
    r1, r2, _ = slrclassic.ptype_ripples("se", srip1, srip2)
    return dict(ang=float(ang), gx=gx, lgx=lgx, tbx=float(tbx), ngx=ngx, tbs=tbs, stype=stype, r1=r1, r2=r2)


def _stage2_poly(col, m):
    """p2 of dzepse.m:45-46 for one column of rn1: fftcp(sin(rn1(:, j)' / 2), 2m) / (2m), middle m samples."""
    p2 = fftcp(np.sin(np.conj(col) / 2), m * 2) / (2 * m)
    return p2[m // 2:m // 2 + m]


def dzepse_batch(specs, *, ctx=None):
    """Many dzepse designs with the device work grouped: every pm / min / max spectral filter of the batch in one remez_batch
    launch, every stage-1 polynomial of one length in one b2rf_batch launch, and likewise for stage 2.  specs: tuples of dzepse's
    positional arguments or dicts of its argument names.  Returns the list of pulses, each bit-identical to its single call."""
    P = [_norm_spec(s) for s in specs]
    if not P:
        return []
    ctx = ctx or _pkg.get_context()
    # spectral k-space weightings kws = dzbeta(ngx, tbs, 'se', stype, srip1, srip2)          (dzepse.m:33-34)
    jobs = [_remez_spec(p["ngx"], p["tbs"], p["stype"], p["r1"], p["r2"]) for p in P if p["stype"] in ("pm", "min", "max")]
    res = iter(slrclassic.remez_batch(jobs, ctx=ctx)) if jobs else iter(())
    for p in P:
        kws = _beta_filter(p["ngx"], p["tbs"], p["stype"], p["r1"], p["r2"],
                           res=next(res) if p["stype"] in ("pm", "min", "max") else None, ctx=ctx)
        p["kws"] = 1.0 * np.asarray(kws)                                 # bsf = 1 for 'se' (dzbeta.m:76-80)
        # x profile (dzepse.m:24-27): kwx = dzbeta(lgx, tbx, 'se'), its centred 2 lgx spectrum, the middle lgx samples
        lgx = p["lgx"]
        pwx = fftcp(dzbeta(lgx, p["tbx"], "se", ctx=ctx), 2 * lgx)[lgx // 2:lgx // 2 + lgx]
        p["r"] = np.outer(np.conj(pwx), p["kws"]) * math.sin(p["ang"] / 2)   # r = pwx' * kws * sin(ang/2)   (:36)
    # stage 1: b2rf of every row of r (:39-42), grouped by row length ngx
    _grouped_b2rf(P, "r", "rn1", ctx)
    # stage 2: b2rf of p2 of every column of rn1 (:44-49); rn2(:, j) = b2rf(p2)'
    for p in P:
        m = p["lgx"]
        p["p2"] = np.stack([_stage2_poly(p["rn1"][:, j], m) for j in range(p["ngx"])])
    _grouped_b2rf(P, "p2", "rf2", ctx)
    out = []
    for p in P:
        rn2 = np.conj(p["rf2"]).T                                         # m x n, column j = b2rf(p2_j)'
        rfv = versec(p["gx"], rn2)                                        # (:52)
        out.append(rfv.ravel(order="F"))                                  # rf = rfv(:).'   (:55)
    return out


def _grouped_b2rf(P, src, dst, ctx):
    lengths = sorted({p[src].shape[1] for p in P})
    for n in lengths:
        group = [p for p in P if p[src].shape[1] == n]
        rows = _pkg.b2rf_batch(np.concatenate([p[src] for p in group], axis=0), ctx=ctx)
        o = 0
        for p in group:
            c = p[src].shape[0]
            p[dst] = rows[o:o + c]
            o += c


def dzepse(ang, gx, tbx, tgx, ngx, sbw, srip1=0.01, srip2=0.01, stype="pm", *, ctx=None):
    """`rf = dzepse(ang, gx, tbx, tgx, ngx, sbw, srip1, srip2, stype)` (rf_tools/dzepse.m:19-57): an echo-planar spin-echo
    spectral-spatial pulse by a 2D inverse SLR transform.  ang flip angle (radians), gx one gradient lobe (even length lgx), tbx the
    spatial time-bandwidth, tgx the lobe duration (ms), ngx the number of lobes, sbw the spectral bandwidth (kHz), srip1 / srip2
    the spectral ripples, stype the spectral filter (ms | pm | ls | min | max).  Returns the lgx * ngx samples, radians per sample,
    lobe after lobe (the versed columns of rn2, column-major as rfv(:).')."""
    return dzepse_batch([(ang, gx, tbx, tgx, ngx, sbw, srip1, srip2, stype)], ctx=ctx)[0]
