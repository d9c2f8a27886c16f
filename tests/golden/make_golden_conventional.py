"""Generate tests/golden/conventional.json (specs) and conventional.npz (vectors) -- fixtures of the conventional SLR designers (rf_tools/dzrf.m and what it calls).

Everything is computed on the CPU, independently of the package's device code:
  remez    scipy.signal.remez (bands in Nyquist units / 2, one desired value per band) for numtaps 21 .. 2047, types I and II,
           2 to 4 bands, weight ratios up to 1e3, and the dzlp / dzmp band vectors of bSSFP_pulse_sb_mb.m:93,
           specsat_minripple_C13.m:59 and specsat_H1_dualband_conventional.m:40-43.  A design is kept only when SciPy converged:
           its taps must pass the alternation certificate on the dense grid (>= L + 1 alternating extrema within 1e-7 of the
           largest weighted error).  delta = that largest weighted error.  The designs SciPy does not converge on (its
           type II at 2046 taps among them) are kept under certify_only: the device result is checked by the certificate alone.
  firls    scipy.signal.firls for the dzls designs (odd lengths; SciPy weights the band integrals the way MATLAB's firls does).
  fmp      a NumPy restatement of fmp.m (fftc, mag2mp) applied to every odd-length remez fixture (real part stored).
Symmetric taps are stored as their first half.
  dzrf     the chain of dzrf.m for every ptype x ftype at n = 65: beta from the fixtures above (msinc.m in closed form),
           reversed for 'min', times bsf, then oracle.slr.b2rf.
Run:  python tests/golden/make_golden_conventional.py
"""
import json
import math
import os
import sys
import warnings

import numpy as np
import scipy.signal as ss

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import slr  # noqa: E402


def dinf(d1, d2):
    a1, a2, a3, a4, a5, a6 = 5.309e-3, 7.114e-2, -4.761e-1, -2.66e-3, -5.941e-1, -4.278e-1
    l1, l2 = math.log10(d1), math.log10(d2)
    return (a1 * l1 * l1 + a2 * l1 + a3) * l2 + (a4 * l1 * l1 + a5 * l1 + a6)


def bands(n, tb, di):
    w = di / tb
    return [0.0, (1 - w) * (tb / 2) / (n / 2), (1 + w) * (tb / 2) / (n / 2), 1.0]


def dzlp_spec(n, tb, d1, d2):
    return n, bands(n, tb, dinf(d1, d2)), [1.0, 1.0, 0.0, 0.0], [1.0, d1 / d2]


def dzmp_spec(n, tb, d1, d2):
    return 2 * n - 1, bands(n, tb, 0.5 * dinf(2 * d1, 0.5 * d2 * d2)), [1.0, 1.0, 0.0, 0.0], [1.0, 2 * d1 / (0.5 * d2 * d2)]


PTYPES = {"st": (1.0, lambda a: a, lambda b: b), "ex": (math.sqrt(0.5), lambda a: math.sqrt(a / 2), lambda b: b / math.sqrt(2)),
          "se": (1.0, lambda a: a / 4, lambda b: math.sqrt(b)), "inv": (1.0, lambda a: a / 8, lambda b: math.sqrt(b / 2)),
          "sat": (math.sqrt(0.5), lambda a: a / 2, lambda b: math.sqrt(b))}


def grid(numtaps, edges, desired, weight, density=16):
    """The dense grid (Nyquist units) with the true (not type II divided) D and W, and each point's band."""
    L = (numtaps + 1) // 2 if numtaps % 2 else numtaps // 2
    delf = 1.0 / (density * L)
    f, D, W, B = [], [], [], []
    for b in range(len(weight)):
        lo, hi = edges[2 * b], edges[2 * b + 1]
        k = max(1, int((hi - lo) / delf + 0.5))
        fb = lo + np.arange(k) * delf
        fb[-1] = hi
        f.append(fb)
        D.append(desired[2 * b] + (desired[2 * b + 1] - desired[2 * b]) * ((fb - lo) / (hi - lo) if hi > lo else 0 * fb))
        W.append(np.full(k, float(weight[b])))
        B.append(np.full(k, b))
    f, D, W, B = (np.concatenate(v) for v in (f, D, W, B))
    if numtaps % 2 == 0:
        keep = f != 1.0
        f, D, W, B = f[keep], D[keep], W[keep], B[keep]
    return L, f, D, W, B


def amplitude(h, f):
    """A(f) of symmetric taps, summed in extended precision: the phases pi f k reach 1000 pi at 2047 taps, and their fp64
    rounding alone would move E by more than the 1e-9 |delta| the certificate of tests/test_conventional_gpu.py resolves."""
    f = np.asarray(f, dtype=np.longdouble)
    k = np.arange(len(h), dtype=np.longdouble) - np.longdouble(len(h) - 1) / 2
    pi = np.longdouble("3.14159265358979323846264338327950288")
    return (np.cos(pi * np.outer(f, k)) @ np.asarray(h, dtype=np.longdouble)).astype(np.float64)


def alternation(E, B, tol):
    """Number of alternating local extrema (within bands) with |E| >= (1 - tol) max|E|."""
    m = np.abs(E).max()
    idx = []
    for j in range(len(E)):
        if abs(E[j]) < (1 - tol) * m:
            continue
        s = np.sign(E[j])
        if j > 0 and B[j - 1] == B[j] and s * E[j] < s * E[j - 1]:
            continue
        if j + 1 < len(E) and B[j + 1] == B[j] and s * E[j] <= s * E[j + 1]:
            continue
        if idx and np.sign(E[idx[-1]]) == s:
            continue
        idx.append(j)
    return len(idx), m


def fmp_np(h, noise=0.0, seed=0):
    """fmp.m restated: fftc, the lift by the most negative real part, mag2mp, the inverse transform.  noise > 0 adds that much
    (times max|hpf|, fixed seed) to the spectrum: how far the result moves then measures its conditioning."""
    h = np.asarray(h, dtype=np.complex128)
    l = len(h)
    lp = 8 * 2 ** int(math.ceil(math.log2(l)))
    lo = (lp - l + 1) // 2
    hp = np.zeros(lp, dtype=np.complex128)
    hp[lo:lo + l] = h
    hpf = np.fft.fftshift(np.fft.fft(np.fft.fftshift(hp)))
    hpf = hpf + noise * np.abs(hpf).max() * np.random.default_rng(seed).standard_normal(lp) if noise else hpf
    hpfs = hpf - np.min(hpf.real) * 1.000001
    hpfmp = slr.mag2mp(np.sqrt(np.abs(hpfs)))
    hpmp = np.fft.ifft(np.fft.fftshift(np.conj(hpfmp)))
    return hpmp[:(l + 1) // 2]


def msinc(n, m):
    x = (np.arange(n) - n / 2) / (n / 2)
    a = m * 2 * np.pi * x + 0.00001
    return np.sin(a) / a * (0.54 + 0.46 * np.cos(np.pi * x)) * 4 * m / n


def half(h):
    """The first ceil(n / 2) taps of an exactly symmetric filter (the rest is their mirror image)."""
    h = np.asarray(h, dtype=np.float64)
    assert np.array_equal(h, h[::-1])
    return h[:(len(h) + 1) // 2]


def scipy_remez(numtaps, edges, desired, weight):
    """SciPy's design, or None when it did not converge (error, or the certificate fails)."""
    if any(desired[2 * b] != desired[2 * b + 1] for b in range(len(weight))):
        return None, None
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            h = ss.remez(numtaps, np.asarray(edges) / 2, desired[::2], weight=weight, maxiter=25, grid_density=16)
    except Exception:                                   # noqa: BLE001  (SciPy's failure to converge)
        return None, None
    L, f, D, W, B = grid(numtaps, edges, desired, weight)
    E = W * (D - amplitude(h, f))
    nalt, m = alternation(E, B, 1e-7)
    return (h, m) if nalt >= L + 1 else (None, None)


def h1_bands():
    B0 = 3.0015
    f1, f2, f3 = (np.array(v) * B0 * 42.577e-3 for v in ([1.8, 2.5], [3, 4.1], [4.8, 5.4]))
    fr = f3.mean()
    f1, f2, f3 = f1 - fr, f2 - fr, f3 - fr
    bw1 = ((f1[1] + f2[0]) / 2 - f1.mean()) * 2
    bw2 = (f3.mean() - (f2[1] + f3[0]) / 2) * 2
    return bw1, bw2


def main():
    bw1, bw2 = h1_bands()
    d1e, d2e, _ = (math.sqrt(0.3 * 0.01 / 2), 0.005 / math.sqrt(2), 0)          # bSSFP 'ex' with 0.3 d1
    cand = {
        "lp21": (21, [0, 0.2, 0.3, 1], [1, 1, 0, 0], [1, 1]),
        "lp48_w10": (48, [0, 0.2, 0.3, 1], [1, 1, 0, 0], [1, 10]),
        "bp100_3band": (100, [0, 0.1, 0.15, 0.4, 0.45, 1], [0, 0, 1, 1, 0, 0], [10, 1, 10]),
        "bs255_4band_w1e3": (255, [0, 0.1, 0.12, 0.3, 0.32, 0.6, 0.62, 1], [1, 1, 0, 0, 1, 1, 0, 0], [1, 100, 1, 1000]),
        "lp519_w300": (519, [0, 0.03, 0.05, 1], [1, 1, 0, 0], [1, 300]),
        "dzlp1023": dzlp_spec(1023, 6, 0.001, 0.001),
        "dzlp2046": dzlp_spec(2046, 40, 0.01, 0.01),
        "dzlp2047": dzlp_spec(2047, 12, 0.01, 0.001),
        "dzmp_bssfp_100": dzmp_spec(100, 4 * 0.65, d1e, d2e),
        "dzmp_c13_150": dzmp_spec(150, 10 * 0.25, 0.05 / 2, math.sqrt(0.5 * 1e-3)),
        "dzmp_h1_260_bw1": dzmp_spec(260, 26 * bw1, 0.0008, 0.03),
        "dzmp_h1_260_bw2": dzmp_spec(260, 26 * bw2, 0.0008, 0.03),
    }
    out = {"remez": {}, "firls": {}, "fmp": [], "dzrf": {}, "certify_only": {}}
    vec = {}
    for name, (n, e, d, w) in cand.items():
        sp = {"numtaps": n, "edges": list(map(float, e)), "desired": list(map(float, d)), "weight": list(map(float, w))}
        h, delta = scipy_remez(n, sp["edges"], sp["desired"], sp["weight"])
        if h is None:
            out["certify_only"][name] = sp
            print("certificate only (SciPy did not converge):", name)
            continue
        out["remez"][name] = dict(sp, delta=float(delta))
        vec["remez/" + name] = half(h)
        if n % 2:
            out["fmp"].append(name)
            vec["fmp/" + name] = fmp_np(h).real        # the imaginary part of a real symmetric filter's factor is rounding
        print("remez", name, n, "delta %.3e" % delta)
    for name, (n, tb, a, b) in {"dzls65": (65, 6, 0.01, 0.01), "dzls129": (129, 8, 0.01, 0.001), "dzls255": (255, 4, 0.001, 0.01)}.items():
        e = bands(n, tb, dinf(a, b))
        out["firls"][name] = {"numtaps": n, "edges": e, "desired": [1, 1, 0, 0], "weight": [1, a / b], "tb": tb, "d1": a, "d2": b}
        vec["firls/" + name] = half(ss.firls(n, e, [1, 1, 0, 0], weight=[1, a / b]))
    n, tb, d1, d2 = 65, 6.0, 0.01, 0.01
    for ptype, (bsf, r1, r2) in PTYPES.items():
        a, b = r1(d1), r2(d2)
        for ftype in ("ms", "ls", "pm", "min", "max"):
            if ftype == "ms":
                beta = msinc(n, tb / 4)
            elif ftype == "ls":
                beta = ss.firls(n, bands(n, tb, dinf(a, b)), [1, 1, 0, 0], weight=[1, a / b])
            else:
                hl, _ = scipy_remez(*(dzlp_spec if ftype == "pm" else dzmp_spec)(n, tb, a, b))
                assert hl is not None, (ptype, ftype)
                beta = hl if ftype == "pm" else fmp_np(hl)[::-1 if ftype == "min" else 1]
            key = "%s_%s" % (ptype, ftype)
            out["dzrf"][key] = {"np": n, "tb": tb, "ptype": ptype, "ftype": ftype, "d1": d1, "d2": d2}
            vec["dzrf/" + key] = beta if ptype == "st" else slr.b2rf(bsf * np.asarray(beta, dtype=np.complex128))
    with open(os.path.join(HERE, "conventional.json"), "w") as fh:
        json.dump(out, fh)
    np.savez_compressed(os.path.join(HERE, "conventional.npz"), **{k: np.asarray(v) for k, v in vec.items()})
    print("wrote conventional.json / .npz: %d remez, %d fmp, %d firls, %d dzrf" % (len(out["remez"]), len(out["fmp"]),
                                                                                 len(out["firls"]), len(out["dzrf"])))


if __name__ == "__main__":
    main()
