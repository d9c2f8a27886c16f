"""Generate tests/golden/epse.json (specs) and epse.npz (vectors) -- fixtures of the spectral-spatial designer rf_tools/dzepse.m and
of verse.m / versec.m.

Everything is computed on the CPU, independently of the package:
  dzepse   a NumPy restatement of dzepse.m:19-57: dzbeta.m's filters from scipy.signal.firls ('ls') and scipy.signal.remez ('pm',
           and 'min' through the fmp.m restatement of make_golden_conventional.py), fftcp.m, both inverse-SLR stages through
           oracle.slr.b2rf row by row, versec.m by np.interp.  Six designs: spectral filters pm, ls and min, lobes of 32 to 128
           samples (trapezoid and sinusoid), 8 to 24 lobes, flip angles pi/2 and pi.
  verse    scipy.interpolate.CubicSpline (not-a-knot) evaluated with extrapolation on verse.m's 1 .. m grid.
  versec   np.interp on versec.m's 0 .. m - 1 grid, NaN outside.
Run:  python tests/golden/make_golden_epse.py
"""
import importlib.util
import json
import math
import os
import sys

import numpy as np
import scipy.interpolate as si
import scipy.signal as ss

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import slr  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_conventional", os.path.join(HERE, "make_golden_conventional.py"))
conv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(conv)


def trapezoid(n):
    """A trapezoidal lobe of n samples: ramps of n / 4 samples, a flat top in between."""
    r = n // 4
    t = np.ones(n)
    t[:r] = (np.arange(r) + 0.5) / r
    t[n - r:] = t[:r][::-1]
    return t


def sinusoid(n):
    return np.sin(np.pi * (np.arange(n) + 0.5) / n)


GRADS = {"trap": trapezoid, "sin": sinusoid}

# name: (ang, lobe shape, lgx, tbx, tgx [ms], ngx, sbw [kHz], srip1, srip2, stype)
DESIGNS = {
    "pm_trap32_n8_90": (math.pi / 2, "trap", 32, 4.0, 0.6, 8, 0.6, 0.01, 0.01, "pm"),
    "pm_sin64_n16_180": (math.pi, "sin", 64, 4.0, 0.6, 16, 0.3, 0.01, 0.01, "pm"),
    "ls_trap64_n13_180": (math.pi, "trap", 64, 6.0, 0.5, 13, 0.4, 0.01, 0.01, "ls"),
    "ls_sin128_n23_90": (math.pi / 2, "sin", 128, 8.0, 0.4, 23, 0.3, 0.02, 0.005, "ls"),
    "min_trap48_n10_180": (math.pi, "trap", 48, 4.0, 0.5, 10, 0.5, 0.01, 0.01, "min"),
    "min_sin96_n20_90": (math.pi / 2, "sin", 96, 6.0, 0.5, 20, 0.3, 0.01, 0.01, "min"),
}


def fftc(x):
    return np.fft.fftshift(np.fft.fft(np.fft.fftshift(x)))


def fftcp(h, n):
    h = np.asarray(h, dtype=np.complex128)
    l = len(h)
    return fftc(np.concatenate([np.zeros(int(math.ceil(n / 2 - l / 2))), h, np.zeros(int(math.floor(n / 2 - l / 2)))]))


def firls(n, edges, desired, weight):
    """MATLAB firls(n - 1, ...): scipy.signal.firls for odd n; for even n (type II, which SciPy does not design) the same
    weighted least-squares problem with its band integrals taken by 1024-point Gauss-Legendre quadrature."""
    if n % 2:
        return ss.firls(n, edges, desired, weight=weight)
    tau = np.arange(n // 2) + 0.5
    xg, wg = np.polynomial.legendre.leggauss(1024)
    Q = np.zeros((n // 2, n // 2))
    q = np.zeros(n // 2)
    for b in range(len(weight)):
        lo, hi = edges[2 * b], edges[2 * b + 1]
        f = lo + (hi - lo) * (xg + 1) / 2
        w = weight[b] * wg * (hi - lo) / 2
        D = desired[2 * b] + (desired[2 * b + 1] - desired[2 * b]) * (f - lo) / (hi - lo)
        C = np.cos(np.pi * np.outer(f, tau))
        Q += C.T @ (w[:, None] * C)
        q += C.T @ (w * D)
    c = np.linalg.solve(Q, q)
    return np.concatenate([c[::-1] / 2, c / 2])


def dzbeta_se(n, tb, ftype, d1, d2):
    """dzbeta(n, tb, 'se', ftype, d1, d2): d1 / 4, sqrt(d2), bsf = 1."""
    d1, d2 = d1 / 4, math.sqrt(d2)
    if ftype == "ls":
        return firls(n, conv.bands(n, tb, conv.dinf(d1, d2)), [1, 1, 0, 0], [1, d1 / d2])
    h, _ = conv.scipy_remez(*(conv.dzlp_spec if ftype == "pm" else conv.dzmp_spec)(n, tb, d1, d2))
    assert h is not None, (n, tb, ftype)
    return h if ftype == "pm" else conv.fmp_np(h)[::-1 if ftype == "min" else 1]


def versec(g, rf):
    m, n = rf.shape
    if m < n:
        rf = rf.T
        m, n = rf.shape
    k = np.cumsum(g)
    k = (m - 1) * k / np.max(k)
    g = m * g / np.sum(g)
    return np.stack([g * np.interp(k, np.arange(m), rf[:, j], left=np.nan, right=np.nan) for j in range(n)], axis=1)


def verse(g, rf):
    m, n = rf.shape
    if m < n:
        rf = rf.T
        m, n = rf.shape
    k = np.cumsum(g)
    k = (m - 1) * k / np.max(k)
    g = m * g / np.sum(g)
    return np.stack([g * si.CubicSpline(np.arange(1, m + 1), rf[:, j], bc_type="not-a-knot", extrapolate=True)(k)
                     for j in range(n)], axis=1)


def dzepse(ang, gx, tbx, tgx, ngx, sbw, srip1, srip2, stype):
    lgx = len(gx)
    pwx = fftcp(dzbeta_se(lgx, tbx, "ls", 0.01, 0.01), 2 * lgx)[lgx // 2:lgx // 2 + lgx]
    kws = dzbeta_se(ngx, (ngx - 1) * tgx * sbw, stype, srip1, srip2)
    r = np.outer(np.conj(pwx), kws) * math.sin(ang / 2)
    m, n = r.shape
    rn1 = np.stack([slr.b2rf(r[j]) for j in range(m)])
    cols = []
    for j in range(n):
        p2 = fftcp(np.sin(np.conj(rn1[:, j]) / 2), m * 2) / (2 * m)
        cols.append(np.conj(slr.b2rf(p2[m // 2:m // 2 + m])))
    rn2 = np.stack(cols, axis=1)
    return versec(gx, rn2).ravel(order="F")


def build():
    meta = {"dzepse": {}, "verse": {}}
    vec = {}
    for name, (ang, shape, lgx, tbx, tgx, ngx, sbw, d1, d2, stype) in DESIGNS.items():
        gx = GRADS[shape](lgx)
        meta["dzepse"][name] = {"ang": ang, "shape": shape, "lgx": lgx, "tbx": tbx, "tgx": tgx, "ngx": ngx, "sbw": sbw,
                                "srip1": d1, "srip2": d2, "stype": stype}
        vec["dzepse/%s/gx" % name] = gx
        vec["dzepse/%s/rf" % name] = dzepse(ang, gx, tbx, tgx, ngx, sbw, d1, d2, stype)
    rng = np.random.default_rng(7)
    for name, (shape, lg, m, n) in {"trap40_m24_n3": ("trap", 40, 24, 3), "sin33_m17_n1": ("sin", 33, 17, 1),
                                     "trap16_m64_n2": ("trap", 16, 64, 2)}.items():
        g = GRADS[shape](lg)
        rf = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
        meta["verse"][name] = {"shape": shape, "lg": lg, "m": m, "n": n}
        vec["verse/%s/rf" % name] = rf
        vec["verse/%s/verse" % name] = verse(g, rf)
        vec["verse/%s/versec" % name] = versec(g, rf)
    return meta, vec


def main():
    meta, vec = build()
    with open(os.path.join(HERE, "epse.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    np.savez_compressed(os.path.join(HERE, "epse.npz"), **vec)
    print("wrote epse.json / .npz: %d dzepse designs, %d verse cases" % (len(meta["dzepse"]), len(meta["verse"])))


if __name__ == "__main__":
    main()
