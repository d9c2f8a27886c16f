"""Conventional single-band SLR pulses: the designers of rf_tools/dzrf.m and the pieces they stand on.

    rf = dzrf(np, tb, ptype, ftype, d1, d2)      # rf_tools/dzrf.m
    h = dzlp(n, tb, d1, d2)                      # rf_tools/dzlp.m   Parks-McClellan, linear phase
    h = dzmp(n, tb, d1, d2)                      # rf_tools/dzmp.m   Parks-McClellan at 2n - 1 taps, then fmp
    h = dzls(n, tb, d1, d2)                      # rf_tools/dzls.m   least squares (firls)
    h = msinc(n, m)                              # rf_tools/msinc.m
    hmp = fmp(h)                                 # rf_tools/fmp.m
    df, mxy, mz = sim_rf_scale(rf, dt, ...)      # sim_rf_scale.m without its plots

The Parks-McClellan exchange (remez, remez_batch) and fmp run on the device (csrc/remez.hip, csrc/specfact.hip k_fmp), b2rf is
the existing device inverse SLR.  firls_lp and msinc are closed forms solved on the host: milliseconds at these sizes.
The one intended difference from the reference: an unknown ptype or ftype raises instead of printing and returning nothing.
"""
import ctypes as C
import math
import sys

import numpy as np

from .spec import dinf

_pkg = sys.modules[__package__]          # the package (bindings looked up at call time, so tests may replace them)

STATUS = {0: "converged", 1: "not converged", 2: "failed"}

# ptype -> (bsf, d1 rule, d2 rule): dzrf.m:38-60
_PTYPES = {
    "st": (1.0, lambda d1: d1, lambda d2: d2),
    "ex": (math.sqrt(0.5), lambda d1: math.sqrt(d1 / 2), lambda d2: d2 / math.sqrt(2)),
    "se": (1.0, lambda d1: d1 / 4, lambda d2: math.sqrt(d2)),
    "inv": (1.0, lambda d1: d1 / 8, lambda d2: math.sqrt(d2 / 2)),
    "sat": (math.sqrt(0.5), lambda d1: d1 / 2, lambda d2: math.sqrt(d2)),
}
_FTYPES = ("ms", "pm", "ls", "min", "max")


def ptype_ripples(ptype, d1=0.01, d2=0.01):
    """(d1, d2, bsf) of the beta filter for a pulse type (dzrf.m:38-60)."""
    if ptype not in _PTYPES:
        raise ValueError("dzrf: unrecognized pulse type %r; recognized types are st, ex, se, inv and sat" % (ptype,))
    bsf, r1, r2 = _PTYPES[ptype]
    return r1(float(d1)), r2(float(d2)), bsf


# ---- Parks-McClellan on the device ------------------------------------------------------------------------
def _remez_job(numtaps, edges, desired, weight, kind):
    if kind not in (None, "bandpass"):
        raise ValueError("remez: only symmetric (bandpass) filters; %r (antisymmetric taps) is out of scope" % (kind,))
    numtaps = int(numtaps)
    e, d, w = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for v in (edges, desired, weight))
    if len(e) % 2 or len(e) == 0:
        raise ValueError("remez: edges must hold two entries per band")
    nb = len(e) // 2
    if len(d) != 2 * nb or len(w) != nb:
        raise ValueError("remez: desired needs 2 entries per band and weight one")
    if not 3 <= numtaps <= 2047:
        raise ValueError("remez: numtaps must be in [3, 2047] (got %d)" % numtaps)
    if np.any(e < 0) or np.any(e > 1) or np.any(np.diff(e) < 0):
        raise ValueError("remez: band edges must ascend within [0, 1] (1 = Nyquist)")
    L = (numtaps + 1) // 2 if numtaps % 2 else numtaps // 2
    return dict(numtaps=numtaps, e=e, d=d, w=w, nb=nb, L=L, h=np.zeros(numtaps), ext=np.zeros(L + 1))


def remez_batch(jobs, *, grid_density=16, maxiter=25, ctx=None):
    """Many Parks-McClellan designs in one device launch (mbfir_remez_batch).  jobs: (numtaps, edges, desired, weight) tuples,
    edges in Nyquist units as MATLAB's remez takes them (numtaps = its order + 1), desired at both edges of every band.
    Returns [(h, info)], info = dict(status ('converged' / 'not converged' / 'failed'), iterations, delta, ext)."""
    prep = [_remez_job(*j[:4], j[4] if len(j) > 4 else None) for j in jobs]
    if not prep:
        return []
    ctx = ctx or _pkg.get_context()
    arr = (_pkg.RemezJob * len(prep))()
    for a, p in zip(arr, prep):
        a.numtaps, a.nband, a.type = p["numtaps"], p["nb"], 0
        a.edges, a.desired, a.weight = (p[k].ctypes.data_as(_pkg._dp) for k in ("e", "d", "w"))
        a.h, a.ext = p["h"].ctypes.data_as(_pkg._dp), p["ext"].ctypes.data_as(_pkg._dp)
    opts = _pkg.RemezOpts(int(grid_density), int(maxiter))
    rc = _pkg.load_library().mbfir_remez_batch(ctx._h, arr, len(prep), C.byref(opts))
    if rc == _pkg.E_ARG:
        raise ValueError("remez: %s" % ctx.last_error())
    if rc != 0:
        raise _pkg.MbfirError("mbfir_remez_batch failed (%d): %s" % (rc, ctx.last_error()))
    return [(p["h"], dict(status=STATUS.get(a.status, "failed"), iterations=a.iterations, delta=a.delta, ext=p["ext"]))
            for a, p in zip(arr, prep)]


def remez(numtaps, edges, desired, weight, *, grid_density=16, maxiter=25, info=False, ctx=None):
    """`h = remez(numtaps - 1, edges, desired, weight)` on the device.  With info=True returns (h, info) whatever the status;
    without it a design that did not converge raises (its last iterate is not a result)."""
    (h, inf), = remez_batch([(numtaps, edges, desired, weight)], grid_density=grid_density, maxiter=maxiter, ctx=ctx)
    if info:
        return h, inf
    if inf["status"] != "converged":
        raise _pkg.MbfirError("remez: %s after %d iterations" % (inf["status"], inf["iterations"]))
    return h


def fmp(h, *, ctx=None):
    """`hmp = fmp(h)` (rf_tools/fmp.m) on the device: minimum-phase factor of an odd-length equiripple filter, (l + 1) / 2 taps."""
    hre, him = _pkg._split(h)
    n = len(hre)
    if n % 2 == 0:
        raise ValueError("fmp: filter length must be odd (got %d)" % n)
    if n > 2047:
        raise ValueError("fmp: filter length at most 2047 (got %d)" % n)
    ctx = ctx or _pkg.get_context()
    m = (n + 1) // 2
    ore, oim = np.zeros(m), np.zeros(m)
    rc = _pkg.load_library().mbfir_fmp(ctx._h, n, _pkg._ptr(hre), _pkg._ptr(him), _pkg._ptr(ore), _pkg._ptr(oim))
    if rc == _pkg.E_ARG:
        raise ValueError("fmp: %s" % ctx.last_error())
    if rc != 0:
        raise _pkg.MbfirError("mbfir_fmp failed (%d): %s" % (rc, ctx.last_error()))
    return ore + 1j * oim


# ---- host closed forms ------------------------------------------------------------------------------------
def msinc(n, m):
    """Hamming-windowed sinc of length n with m cycles, time-bandwidth 4 m (rf_tools/msinc.m)."""
    x = (np.arange(n) - n / 2) / (n / 2)
    a = m * 2 * np.pi * x + 0.00001
    return np.sin(a) / a * (0.54 + 0.46 * np.cos(np.pi * x)) * 4 * m / n


def _int_cos(t, lo, hi):
    """integral of cos(pi f t) df over [lo, hi] (t an array, may hold 0)."""
    return hi * np.sinc(hi * t) - lo * np.sinc(lo * t)


def _int_fcos(t, lo, hi):
    """integral of f cos(pi f t) df over [lo, hi]."""
    out = np.full(t.shape, (hi * hi - lo * lo) / 2)
    nz = t != 0
    w = np.pi * t[nz]
    F = lambda f: f * np.sin(w * f) / w + np.cos(w * f) / (w * w)      # noqa: E731
    out[nz] = F(hi) - F(lo)
    return out


def firls_lp(numtaps, edges, desired, weight=None):
    """Least-squares linear-phase FIR with MATLAB firls semantics (`firls(numtaps - 1, edges, desired, weight)`): minimises
    sum_b weight_b * integral over band b of (A(f) - D(f))^2 df, D linear between the band edges (Nyquist = 1), transition bands
    left free.  Odd numtaps gives type I, even type II.  Solved by the normal equations on the host."""
    numtaps = int(numtaps)
    e = np.asarray(edges, dtype=np.float64).ravel()
    d = np.asarray(desired, dtype=np.float64).ravel()
    nb = len(e) // 2
    w = np.ones(nb) if weight is None else np.asarray(weight, dtype=np.float64).ravel()
    if len(e) % 2 or len(d) != len(e) or len(w) != nb:
        raise ValueError("firls_lp: edges / desired need two entries per band, weight one")
    if numtaps < 1 or numtaps > 2047:
        raise ValueError("firls_lp: numtaps must be in [1, 2047]")
    if np.any(e < 0) or np.any(e > 1) or np.any(np.diff(e) < 0):
        raise ValueError("firls_lp: band edges must ascend within [0, 1]")
    L = (numtaps + 1) // 2
    tau = np.arange(L, dtype=np.float64) + (0.0 if numtaps % 2 else 0.5)
    Q = np.zeros((L, L))
    q = np.zeros(L)
    tm = tau[:, None] - tau[None, :]
    tp = tau[:, None] + tau[None, :]
    for b in range(nb):
        lo, hi, wb = e[2 * b], e[2 * b + 1], w[b]
        if hi <= lo:
            continue
        Q += wb * 0.5 * (_int_cos(tm, lo, hi) + _int_cos(tp, lo, hi))
        s = (d[2 * b + 1] - d[2 * b]) / (hi - lo)
        q += wb * ((d[2 * b] - s * lo) * _int_cos(tau, lo, hi) + s * _int_fcos(tau, lo, hi))
    c = np.linalg.solve(Q, q)
    if numtaps % 2:
        return np.concatenate([c[:0:-1] / 2, c[:1], c[1:] / 2])
    return np.concatenate([c[::-1] / 2, c / 2])


# ---- the dz* designers ------------------------------------------------------------------------------------
def _bands(n, tb, di):
    """f = [0 (1-w)(tb/2) (1+w)(tb/2) (n/2)] / (n/2), w = di / tb (dzlp.m:10-11, dzls.m:16-17, dzmp.m:11-12)."""
    w = di / tb
    return [0.0, (1 - w) * (tb / 2) / (n / 2), (1 + w) * (tb / 2) / (n / 2), 1.0]


def dzlp_spec(n, tb, d1, d2):
    """(numtaps, edges, desired, weight) of the remez call of dzlp.m."""
    return int(n), _bands(n, tb, dinf(d1, d2)), [1.0, 1.0, 0.0, 0.0], [1.0, d1 / d2]


def dzmp_spec(n, tb, d1, d2):
    """(numtaps, edges, desired, weight) of the remez call of dzmp.m: 2n - 1 taps, ripples 2 d1 and d2^2 / 2."""
    di = 0.5 * dinf(2 * d1, 0.5 * d2 * d2)
    return 2 * int(n) - 1, _bands(n, tb, di), [1.0, 1.0, 0.0, 0.0], [1.0, 2 * d1 / (0.5 * d2 * d2)]


dzls_spec = dzlp_spec          # dzls.m:15-20 builds the same band vectors and weights for firls


def dzlp(n, tb, d1=0.01, d2=0.01, *, ctx=None):
    """Equiripple linear-phase filter of n taps (rf_tools/dzlp.m)."""
    return remez(*dzlp_spec(n, tb, d1, d2), ctx=ctx)


def dzmp(n, tb, d1=0.01, d2=0.01, *, ctx=None):
    """Minimum-phase filter of n taps: a 2n - 1 tap equiripple design factored by fmp (rf_tools/dzmp.m)."""
    return fmp(remez(*dzmp_spec(n, tb, d1, d2), ctx=ctx), ctx=ctx)


def dzls(n, tb, d1=0.01, d2=0.01):
    """Least-squares linear-phase filter of n taps (rf_tools/dzls.m), on the host."""
    return firls_lp(*dzls_spec(n, tb, d1, d2))


def dzrf(np_, tb, ptype="st", ftype="ls", d1=0.01, d2=0.01, pclsfrac=1.5, *, ctx=None):
    """`rf = dzrf(np, tb, ptype, ftype, d1, d2, pclsfrac)` (rf_tools/dzrf.m): an np-sample SLR pulse of time-bandwidth tb.
    ptype st | ex | se | inv | sat, ftype ms | pm | ls | min | max.  Returns beta itself for 'st', else b2rf(bsf * beta) in radians
    per sample.  pclsfrac is accepted and unused, as in the reference."""
    return dzrf_batch([(np_, tb, ptype, ftype, d1, d2)], ctx=ctx)[0]


def dzrf_batch(specs, *, ctx=None):
    """Many dzrf calls; every pm / min / max exchange goes into one remez_batch launch.  specs: tuples (np, tb[, ptype[, ftype[, d1[,
    d2]]]]) or dicts of dzrf's argument names (np under 'np').  Returns the list of pulses."""
    norm = []
    for s in specs:
        if isinstance(s, dict):
            s = (s["np"], s["tb"], s.get("ptype", "st"), s.get("ftype", "ls"), s.get("d1", 0.01), s.get("d2", 0.01))
        n, tb, ptype, ftype, d1, d2 = tuple(s) + ("st", "ls", 0.01, 0.01)[len(s) - 2:]
        if ftype not in _FTYPES:
            raise ValueError("dzrf: unrecognized filter design method %r; options are ms, pm, min, max and ls" % (ftype,))
        norm.append((n, tb, ptype, ftype) + ptype_ripples(ptype, d1, d2))       # dzrf.m:38-60
    jobs = [(dzlp_spec if f == "pm" else dzmp_spec)(n, tb, r1, r2) for n, tb, _, f, r1, r2, _ in norm if f in ("pm", "min", "max")]
    res = iter(remez_batch(jobs, ctx=ctx))
    out = []
    for n, tb, ptype, ftype, r1, r2, bsf in norm:                              # dzrf.m:62-80
        if ftype == "ms":
            b = msinc(n, tb / 4)
        elif ftype == "ls":
            b = dzls(n, tb, r1, r2)
        else:
            b, info = next(res)
            if info["status"] != "converged":
                raise _pkg.MbfirError("dzrf: remez %s after %d iterations" % (info["status"], info["iterations"]))
            if ftype != "pm":
                b = fmp(b, ctx=ctx)[::-1 if ftype == "min" else 1]            # 'min' is the reversed factor (:67-69)
        out.append(b if ptype == "st" else _pkg.b2rf(bsf * b, ctx=ctx))
    return out


# ---- sim_rf_scale.m -----------------------------------------------------------------------------------------
def sim_rf_axis(f=None, bw=None, n=2048):
    """The frequency axis of sim_rf_scale.m (Hz): bw (kHz, the 7-argument form) -> [-3 bw, 3 bw]; f (band edges in kHz, the
    9-argument form) -> [f(1) - 300, f(end) + 300]; 2048 points."""
    if (f is None) == (bw is None):
        raise ValueError("sim_rf_scale: give either bw (passband bandwidth, kHz) or f (band edges, kHz)")
    if bw is not None:
        BW = float(bw) * 1e3
        lo, hi = -3 * BW, 3 * BW
    else:
        fv = np.asarray(f, dtype=np.float64).ravel() * 1e3
        lo, hi = fv[0] - 300, fv[-1] + 300
    return np.linspace(lo, hi, n)


def sim_rf_scale(rf, dt, scale=None, nucleus="C-13", f=None, bw=None, *, ctx=None):
    """The computation of sim_rf_scale.m without its plots: the pulse rf (Gauss) with sampling interval dt (ms), scaled by each
    entry of `scale` (default 0.8 .. 1.2), simulated by mbfir.bloch (T1 = T2 = 1000 s, on resonance in space) over the
    2048-point axis of sim_rf_axis.  Returns (df [Hz], mxy [len(scale), 2048] complex, mz [len(scale), 2048])."""
    if nucleus not in ("C-13", "H-1"):
        raise ValueError("sim_rf_scale: nucleus must be 'H-1' or 'C-13'")
    df = sim_rf_axis(f, bw)
    scale = [0.8, 0.9, 1.0, 1.1, 1.2] if scale is None or len(scale) == 0 else list(scale)
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    g = np.zeros(len(rf))
    mxy = np.zeros((len(scale), len(df)), dtype=np.complex128)
    mz = np.zeros((len(scale), len(df)))
    for k, s in enumerate(scale):
        mx, my, m_z = _pkg.bloch(rf * s, g, dt * 1e-3, 1e3, 1e3, df, 0.0, 0, nucleus=nucleus, ctx=ctx)
        mxy[k] = np.asarray(mx).ravel() + 1j * np.asarray(my).ravel()
        mz[k] = np.asarray(m_z).ravel()
    return df, mxy, mz


def sim_rf_scale_batch(pulses, dts, scale=None, nucleus="C-13", f=None, bw=None, *, ctx=None):
    """sim_rf_scale of many pulses from one mbfir.bloch_batch call (every pulse at every scale in one launch).  pulses: rf arrays
    (Gauss); dts: one sampling interval (ms) or one per pulse; f (band edges, kHz) and bw (kHz): one value, or a list with one per
    pulse (None where a pulse takes the other).  Returns one (df, mxy, mz) per pulse, as sim_rf_scale returns it."""
    if nucleus not in ("C-13", "H-1"):
        raise ValueError("sim_rf_scale: nucleus must be 'H-1' or 'C-13'")
    rfs = [np.asarray(rf, dtype=np.complex128).ravel() for rf in pulses]
    P = len(rfs)
    dts = np.broadcast_to(np.asarray(dts, dtype=np.float64), (P,))
    fs = list(f) if isinstance(f, list) and len(f) == P and all(v is None or np.ndim(v) >= 1 for v in f) else [f] * P
    bws = list(bw) if isinstance(bw, (list, tuple)) else [bw] * P
    if len(bws) != P:
        raise ValueError("sim_rf_scale: bw must be one value or one per pulse")
    axes = [sim_rf_axis(fv, bv) for fv, bv in zip(fs, bws)]
    scale = [0.8, 0.9, 1.0, 1.1, 1.2] if scale is None or len(scale) == 0 else list(scale)
    res = _pkg.bloch_batch([(rf, np.zeros(len(rf)), dt * 1e-3, 1e3, 1e3, nucleus) for rf, dt in zip(rfs, dts)], axes, 0.0,
                           scales=scale, ctx=ctx)
    return [(df, mx[:, :, 0] + 1j * my[:, :, 0], m_z[:, :, 0]) for df, (mx, my, m_z) in zip(axes, res)]
