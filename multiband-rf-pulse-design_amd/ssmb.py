"""Multiband spectral-spatial pulses: a multiband spectral beta designed as dzrf_mb designs it, times a spatial slice profile,
inverted by the device 2D SLR (mbfir.slr2d_batch) -- the metabolite-specific excitations of hyperpolarized C-13 imaging.

    rf, g, info = dzss_mb(gx, dt, ngx, mb_cf, mb_range, mb_FA, mb_ripple, ...)   # one pulse, rf in Gauss, g in G/cm
    out = dzss_mb_batch(specs)                                                   # many, grouped device work
    fold = fold_bands(mb_cf, mb_range, mb_FA, mb_ripple, fs)                     # bands into the spectral window

The design is separable, beta(x, f) = P(x) B(f): B is the beta dzrf_mb(ngx, Ts, ...) hands to b2rf (sampled once per subpulse,
Ts apart, with sin(FA / 2) per band already in it), P the spatial profile of dzepse.m:24-27 from dzbeta(lgx, tbx, 'st', ...).
r = conj(P) B^T goes through the 2D inverse SLR with the hard-pulse middle stage, and every column of its result is versed onto
the gradient lobe.  The 2D SLR conjugates its pulses as dzepse.m:48 does, which puts B(f) at -f; the pulse is conjugated once
more so that B(f) answers at +f, as dzrf_mb's 1D pulses do.  Symmetric EPI plays a subpulse on every lobe, the lobes alternating in sign; flyback plays them on the
positive lobes only, with the rewinder gfb (RF off) in between.  DESIGN.md section 8g has the physics and the measured figures.
"""
import math
import sys

import numpy as np

from . import spec as _spec
from .dzrf import GAMMA
from .epse import dzbeta, fftcp, versec

_pkg = sys.modules[__package__]          # the package (bindings looked up at call time)

_FTYPES = ("ap_cvx", "ap_minstopripple_cvx", "ap_minorder_cvx", "ap_mintran_cvx", "ap_mintran_minorder_cvx", "lp_minorder",
           "qp_cvx")
# fixed-order designs (dzrf_mb.m:166-169, 204-206): one solve_batch job each
_FIXED = {"ap_cvx": lambda n, f, a, d, Peak: ("fir_ap_cvx", (n, f, a, d, 1.0, Peak)),
          "ap_minstopripple_cvx": lambda n, f, a, d, Peak: ("fir_ap_cvx", (n, f, a, d, 1e4, Peak)),
          "qp_cvx": lambda n, f, a, d, Peak: ("fir_qp_cvx", (n, f, a, d, 120.0, 1e6))}

_NAMES = ("gx", "dt", "ngx", "mb_cf", "mb_range", "mb_FA", "mb_ripple", "ptype", "ftype", "nucleus", "tbx", "xftype", "xd1", "xd2",
          "gfb", "Peak", "flip_zero", "min_order", "opts")
_KWONLY = ("min_tran", "probes", "flip_criterion", "flip_candidates", "flip_seed", "downsampling", "shift_f")
_DEFAULTS = {"ptype": "ex", "ftype": "ap_cvx", "nucleus": "C-13", "tbx": 4.0, "xftype": "ls", "xd1": 0.01, "xd2": 0.01,
             "gfb": None, "Peak": 1e-3, "flip_zero": 0, "min_order": 0.9, "opts": None, "min_tran": 0.85, "probes": 1,
             "flip_criterion": "beta", "flip_candidates": "reference", "flip_seed": None, "downsampling": 1, "shift_f": 0}


def fold_bands(mb_cf, mb_range, mb_FA, mb_ripple, fs):
    """Fold every band into the spectral window [-fs/2, fs/2) of a pulse sampled at fs (kHz) and sort the bands by frequency.
    mb_cf: per band a centre or a (lo, hi) range in kHz (rf_bandedge's form); mb_range: per-band widths added around it, or None.
    A band moves by the multiple of fs that puts its centre in the window.  Returns dict(mb_cf, mb_range, mb_FA, mb_ripple, order):
    the folded spec in rf_bandedge's form, sorted, and order[i] = the input index of folded band i.  Raises ValueError naming
    the bands when one straddles +-fs/2 after folding or two folded bands overlap."""
    k = len(mb_cf)
    if len(mb_FA) != k or len(mb_ripple) != k or (mb_range is not None and len(mb_range) != k):
        raise ValueError("fold_bands: mb_cf, mb_FA, mb_ripple (and mb_range) need one entry per band")
    if not fs > 0:
        raise ValueError("fold_bands: the spectral sampling rate must be positive")
    cf, lo, hi = [], np.zeros(k), np.zeros(k)
    for i, c in enumerate(mb_cf):
        c = np.ravel(np.asarray(c, dtype=np.float64))
        l, h = float(c[0]), float(c[-1])
        if not (np.isfinite(l) and np.isfinite(h)) or h < l:
            raise ValueError("fold_bands: band %d has no valid frequency range" % i)
        w = 0.0 if mb_range is None else float(mb_range[i])
        shift = math.floor((l + h) / 2 / fs + 0.5) * fs
        cf.append((l - shift, h - shift) if len(c) > 1 else l - shift)
        lo[i], hi[i] = l - shift - w / 2, h - shift + w / 2
    bad = [i for i in range(k) if lo[i] < -fs / 2 or hi[i] > fs / 2]
    if bad:
        raise ValueError("fold_bands: band(s) %s straddle +-fs/2 = +-%.6g kHz after folding" % (", ".join(map(str, bad)), fs / 2))
    order = sorted(range(k), key=lambda i: (lo[i] + hi[i]) / 2)
    clash = [(i, j) for a, i in enumerate(order) for j in order[a + 1:] if lo[j] < hi[i] and lo[i] < hi[j]]
    if clash:
        raise ValueError("fold_bands: folded bands overlap: %s" % ", ".join("%d and %d" % p for p in clash))
    return dict(mb_cf=[cf[i] for i in order], mb_range=None if mb_range is None else [float(mb_range[i]) for i in order],
                mb_FA=[mb_FA[i] for i in order], mb_ripple=[mb_ripple[i] for i in order], order=order)


def _norm_spec(s):
    """A spec (tuple of dzss_mb's positional arguments or dict of its argument names) -> dict of every argument, checked, with the
    band folding, the spectral band spec (f, a, d) and the spatial profile filled in."""
    if isinstance(s, dict):
        unknown = sorted(set(s) - set(_NAMES) - set(_KWONLY))
        if unknown:
            raise ValueError("dzss_mb: unknown argument(s) %s" % ", ".join(unknown))
        missing = [k for k in _NAMES[:7] if k not in s]
        if missing:
            raise ValueError("dzss_mb: missing argument(s) %s" % ", ".join(missing))
        p = {k: s.get(k, _DEFAULTS.get(k)) for k in _NAMES + _KWONLY}
    else:
        s = tuple(s)
        if not 7 <= len(s) <= len(_NAMES):
            raise ValueError("dzss_mb: takes 7 to %d positional arguments (gx, dt, ngx, mb_cf, mb_range, mb_FA, mb_ripple, ...)"
                             % len(_NAMES))
        p = dict(zip(_NAMES, s))
        p.update({k: _DEFAULTS[k] for k in _NAMES[len(s):] + _KWONLY})
    gx = np.asarray(p["gx"], dtype=np.float64).ravel()
    lgx = len(gx)
    if lgx < 2 or lgx % 2 or lgx > 2048:
        raise ValueError("dzss_mb: the gradient lobe needs an even number of samples in [2, 2048]; got %d" % lgx)
    if not np.all(np.isfinite(gx)) or np.any(gx < 0) or not np.sum(gx) > 0:
        raise ValueError("dzss_mb: the gradient lobe must be finite, non-negative and of positive area")
    dt = float(p["dt"])
    if not dt > 0:
        raise ValueError("dzss_mb: dt must be positive")
    ngx = p["ngx"]
    if int(ngx) != ngx or not 2 <= int(ngx) <= 2048:
        raise ValueError("dzss_mb: ngx must be an integer in [2, 2048]")
    gfb = None if p["gfb"] is None else np.asarray(p["gfb"], dtype=np.float64).ravel()
    if gfb is not None and (len(gfb) < 1 or not np.all(np.isfinite(gfb))):
        raise ValueError("dzss_mb: the flyback rewinder gfb must be a non-empty finite array")
    if (p["downsampling"] or 1) != 1:
        raise ValueError("dzss_mb: downsampling != 1 is not supported")
    if (p["shift_f"] or 0) != 0:
        raise ValueError("dzss_mb: shift_f != 0 is not supported")
    if p["ftype"] not in _FTYPES:
        raise ValueError("dzss_mb: unrecognized ftype %r; options are %s" % (p["ftype"], ", ".join(_FTYPES)))
    if p["ptype"] not in ("ex", "se", "sat", "inv"):
        raise ValueError("dzss_mb: ptype must be ex, se, sat or inv (got %r)" % (p["ptype"],))
    if p["nucleus"] not in GAMMA:
        raise ValueError("dzss_mb: no such option for nucleus. Options are H-1 and C-13")
    Ts = (lgx + (0 if gfb is None else len(gfb))) * dt                  # ms
    fold = fold_bands(list(p["mb_cf"]), p["mb_range"], list(p["mb_FA"]), list(p["mb_ripple"]), 1.0 / Ts)
    p.update(gx=gx, lgx=lgx, dt=dt, ngx=int(ngx), gfb=gfb, Ts=Ts, fs=1.0 / Ts, fold=fold, gamma=GAMMA[p["nucleus"]])
    # the spectral band spec at ngx taps, as dzrf_mb.m:101-121 forms it
    p["f"], p["a"], p["d"] = _spec.band_spec(p["ngx"], Ts, fold["mb_cf"], fold["mb_range"], fold["mb_FA"], fold["mb_ripple"],
                                             p["ptype"])
    # spatial profile (dzepse.m:24-27 with ptype 'st'): the middle lgx samples of the centred 2 lgx spectrum
    kwx = dzbeta(lgx, float(p["tbx"]), "st", p["xftype"], float(p["xd1"]), float(p["xd2"]))
    p["pwx"] = fftcp(kwx, 2 * lgx)[lgx // 2:lgx // 2 + lgx]
    return p


def _dzrf_mb(p):
    """The spectral design of a search ftype, through dzrf_mb itself: (beta, b_spec) or (None, b_spec) when it fails."""
    fold = p["fold"]
    _, b, _, b_spec = _pkg.dzrf_mb(p["ngx"], p["Ts"], fold["mb_cf"], fold["mb_range"], fold["mb_FA"], fold["mb_ripple"],
                                   p["ptype"], p["ftype"], p["nucleus"], p["flip_zero"], 1, p["Peak"], 0, p["min_order"],
                                   p["min_tran"], 0, opts=p["opts"], probes=p["probes"], flip_criterion=p["flip_criterion"],
                                   flip_candidates=p["flip_candidates"], flip_seed=p["flip_seed"])
    return (b if len(b) else None), b_spec


def _finish_beta(p, h):
    """dzrf_mb.m:220-225 on a fixed-order design: the taps reversed, then the optional zero flip."""
    b = np.asarray(h, dtype=np.complex128).ravel()[::-1]
    if p["flip_zero"]:
        b = _pkg.fir_flip_zero(b, 0, seed=p["flip_seed"], criterion=p["flip_criterion"], candidates=p["flip_candidates"])
    return b


def _spectral(P):
    """Every design's spectral beta: the fixed-order ones in one solve_batch per options object, the search ones one by one."""
    groups = {}
    for q, p in enumerate(P):
        if p["ftype"] in _FIXED:
            groups.setdefault(id(p["opts"]), []).append(q)
    for qs in groups.values():
        jobs = [_FIXED[P[q]["ftype"]](P[q]["ngx"], P[q]["f"], P[q]["a"], P[q]["d"], P[q]["Peak"]) for q in qs]
        for q, (h, status) in zip(qs, _pkg.solve_batch(jobs, opts=P[qs[0]]["opts"])):
            P[q]["beta"] = _finish_beta(P[q], h) if status == "Solved" else None
            P[q]["b_spec"] = dict(f=P[q]["f"], a=P[q]["a"], d=P[q]["d"])
    for p in P:
        if p["ftype"] not in _FIXED:
            p["beta"], p["b_spec"] = _dzrf_mb(p)


def _gradient(p, n):
    """The gradient waveform (G/cm) of n subpulses and the sample index of every subpulse's first sample."""
    gx, lgx = p["gx"], p["lgx"]
    if p["gfb"] is None:
        return np.concatenate([gx * (-1.0) ** k for k in range(n)]), np.arange(n) * lgx
    step = lgx + len(p["gfb"])
    return np.concatenate([gx] + [np.concatenate([p["gfb"], gx]) for _ in range(n - 1)]), np.arange(n) * step


def dzss_mb_batch(specs, *, ctx=None):
    """Many dzss_mb designs with the device work grouped: the fixed-order spectral designs (ap_cvx, ap_minstopripple_cvx, qp_cvx)
    in one mbfir.solve_batch, the search ftypes one by one, every 2D SLR of one (lgx, n) shape in one slr2d_batch call.  specs:
    tuples of dzss_mb's positional arguments or dicts of its argument names (the keyword-only ones included).  Returns the list of
    (rf, g, info), each bit-identical to its single call."""
    P = [_norm_spec(s) for s in specs]
    if not P:
        return []
    ctx = ctx or _pkg.get_context()
    _spectral(P)
    live = [p for p in P if p["beta"] is not None]
    for p in live:
        if len(p["beta"]) < 2:
            raise ValueError("dzss_mb: the spectral design has %d tap(s); the 2D SLR needs at least 2" % len(p["beta"]))
        p["r"] = np.outer(np.conj(p["pwx"]), p["beta"])                 # beta(x, f) = P(x) B(f): rows x, columns subpulses
    for shape in sorted({p["r"].shape for p in live}):
        group = [p for p in live if p["r"].shape == shape]
        rn2 = _pkg.slr2d_batch(np.stack([p["r"] for p in group]), ctx=ctx)
        for p, r in zip(group, rn2):
            p["rn2"] = r
    out = []
    for p in P:
        fold = p["fold"]
        info = dict(status="Failed" if p["beta"] is None else "Solved", ngx=p["ngx"], Ts=p["Ts"], fs=p["fs"], dt=p["dt"],
                    mb_cf=fold["mb_cf"], mb_range=fold["mb_range"], mb_FA=fold["mb_FA"], mb_ripple=fold["mb_ripple"],
                    order=fold["order"], b_spec=p["b_spec"], pwx=p["pwx"], nucleus=p["nucleus"],
                    thk=float(p["tbx"]) / (p["gamma"] * np.sum(p["gx"]) * p["dt"]))        # cm: tbx / (gamma * lobe area)
        if p["beta"] is None:                                           # dzrf_mb.m:216-218: empty pulse
            info.update(beta=np.zeros(0, dtype=np.complex128))
            out.append((np.zeros(0, dtype=np.complex128), np.zeros(0), info))
            continue
        n = len(p["beta"])
        g, starts = _gradient(p, n)
        sub = versec(p["gx"], p["rn2"])                                 # (lgx, n): column j is subpulse j, radians per sample
        rf = np.zeros(len(g), dtype=np.complex128)
        for j, s0 in enumerate(starts):
            rf[s0:s0 + p["lgx"]] = sub[:, j]
        rf = np.conj(rf) / (2 * np.pi * p["gamma"] * p["dt"])           # Gauss (rfscaleg.m:12-16); conj: B(f) at +f
        info.update(ngx=n, beta=p["beta"])
        out.append((rf, g, info))
    return out


def dzss_mb(gx, dt, ngx, mb_cf, mb_range, mb_FA, mb_ripple, ptype="ex", ftype="ap_cvx", nucleus="C-13", tbx=4.0, xftype="ls",
            xd1=0.01, xd2=0.01, gfb=None, Peak=1e-3, flip_zero=0, min_order=0.9, opts=None, *, min_tran=0.85, probes=1,
            flip_criterion="beta", flip_candidates="reference", flip_seed=None, downsampling=1, shift_f=0, ctx=None):
    """`rf, g, info = dzss_mb(...)`: a multiband spectral-spatial pulse.
    gx: one gradient lobe (G/cm, even length <= 2048, non-negative, positive area) sampled every dt ms.  gfb None: symmetric EPI,
    a subpulse on every lobe, lobes alternating in sign, Ts = lgx dt; gfb an array: flyback, the rewinder (sampled at dt, RF off)
    after every lobe but the last, Ts = (lgx + len(gfb)) dt.  ngx: the number of subpulses = the spectral filter's length.
    mb_cf / mb_range / mb_FA / mb_ripple / ptype / ftype / nucleus / Peak / flip_zero / min_order / opts and the keyword-only flip
    and search options: dzrf_mb's, applied to the bands folded into [-fs/2, fs/2), fs = 1 / Ts (fold_bands).  tbx, xftype, xd1,
    xd2: the spatial profile dzbeta(lgx, tbx, 'st', xftype, xd1, xd2).  downsampling != 1 and shift_f != 0 raise ValueError.
    Returns rf (Gauss) and g (G/cm) of the same length, and info: status, ngx (the length used; the search ftypes may shorten
    it), Ts (ms), fs (kHz), the folded spec (mb_cf, mb_range, mb_FA, mb_ripple, order), b_spec (f, a, d), beta (the spectral
    beta), pwx (the spatial profile), thk (the slice thickness in cm, tbx / (gamma * lobe area)).  A failed spectral design
    returns empty rf and g with info['status'] = 'Failed'."""
    return dzss_mb_batch([dict(gx=gx, dt=dt, ngx=ngx, mb_cf=mb_cf, mb_range=mb_range, mb_FA=mb_FA, mb_ripple=mb_ripple,
                               ptype=ptype, ftype=ftype, nucleus=nucleus, tbx=tbx, xftype=xftype, xd1=xd1, xd2=xd2, gfb=gfb,
                               Peak=Peak, flip_zero=flip_zero, min_order=min_order, opts=opts, min_tran=min_tran, probes=probes,
                               flip_criterion=flip_criterion, flip_candidates=flip_candidates, flip_seed=flip_seed,
                               downsampling=downsampling, shift_f=shift_f)], ctx=ctx)[0]
