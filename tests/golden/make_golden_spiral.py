"""Generate tests/golden/spiral.json -- fixtures of the spiral 2D designer rf_tools/dz2d.m with csg.m.

Everything is computed on the CPU, independently of the package (mbfir.spiral is not imported): csg.m:19-44 and dz2d.m:26-55 are
restated here sample by sample, with the linear interpolation written out as (1 - w) k_j + w k_{j+1} on the bracketing knots
(mbfir.spiral goes through np.interp, which evaluates k_j + slope (t - t_j)), the gradient by explicit differences and the Bessel
function from scipy.special.j1 (mbfir.spiral calls jv(1, .)).  A query within 1e-12 (relative) of an end knot takes that knot's
value, the documented rule of mbfir.spiral.csg; one further outside is NaN as interp1 returns it.

Five designs (nt, bw, tbp, ns, mxg, mxs): the reference's example `dz2d(8, 1, 4, 512, 1, 2)`; one held by the gradient amplitude
over most of its length (mxg 0.3); one held by the slew rate alone (mxg 4 is never reached); an odd ns; two turns on 64 samples.
Stored per design: the arguments, the time-warped trajectory k (csg's output for the linear spiral), rf, g and the duration in ms.
Run:  python tests/golden/make_golden_spiral.py
"""
import json
import math
import os

import numpy as np
from scipy.special import j1

HERE = os.path.dirname(os.path.abspath(__file__))
GAMMA = 4.26            # csg.m:25, :36
RTOL = 1e-12

DESIGNS = {
    "example_8turn_512": (8, 1.0, 4.0, 512, 1.0, 2.0),
    "amplitude_limited": (6, 1.0, 4.0, 200, 0.3, 20.0),
    "slew_limited": (6, 1.0, 4.0, 200, 4.0, 0.5),
    "odd_ns_151": (5, 1.5, 3.0, 151, 1.0, 2.0),
    "two_turns_64": (2, 1.0, 2.0, 64, 1.0, 2.0),
}


def interp1(tk, yk, tq):
    """linear interp1 of complex yk on ascending knots tk, NaN outside (end knots within RTOL count as inside)"""
    out = np.empty(len(tq), dtype=np.complex128)
    for i, t in enumerate(tq):
        if t < tk[0]:
            out[i] = yk[0] if tk[0] - t <= RTOL * abs(tk[0]) else complex(math.nan, math.nan)
        elif t > tk[-1]:
            out[i] = yk[-1] if t - tk[-1] <= RTOL * abs(tk[-1]) else complex(math.nan, math.nan)
        else:
            j = min(int(np.searchsorted(tk, t, side="right")) - 1, len(tk) - 2)
            w = (t - tk[j]) / (tk[j + 1] - tk[j])
            out[i] = (1.0 - w) * yk[j] + w * yk[j + 1]
    return out


def csg(k, mxg, mxs):
    n = len(k)
    g = np.zeros(n, dtype=np.complex128)
    for i in range(1, n):
        g[i] = (k[i] - k[i - 1]) / (GAMMA * (1.0 / n))
    s = np.empty(n, dtype=np.complex128)
    for i in range(n - 1):
        s[i] = (g[i + 1] - g[i]) / (1.0 / n)
    s[n - 1] = s[n - 2]
    t1 = np.cumsum(np.sqrt(np.abs(s / mxs))) * 1.0 / n
    q = np.arange(1, n + 1)
    nk = interp1(t1, k, q * t1[n - 1] / n)
    g = np.zeros(n, dtype=np.complex128)
    for i in range(1, n):
        g[i] = (nk[i] - nk[i - 1]) / (GAMMA * (t1[n - 1] / n))
    t2 = np.cumsum(np.maximum(np.abs(g), mxg)) * t1[n - 1] / (mxg * n)
    return interp1(t2, nk, q * t2[n - 1] / n), float(t2[n - 1])


def dz2d(nt, bw, tbp, ns, mxg, mxs):
    t = np.arange(1, ns + 1) / ns
    kl = t * np.exp(1j * 2 * np.pi * t * nt) * bw / 2
    k, dur = csg(kl, mxg, mxs)
    kr = np.abs(k) / (bw / 2)
    z = kr * np.pi * tbp / 2 + 0.0001
    rf = j1(z) / z * np.exp(-kr * kr * 2)
    g = np.empty(ns, dtype=np.complex128)
    g[0] = k[0]
    g[1:] = k[1:] - k[:-1]
    omt = 2 * np.pi * nt
    rf = rf * ((omt * kr) / np.sqrt(omt * omt * kr * kr + 1)) * np.abs(g)
    rf = rf[::-1]
    return k, rf / np.sum(rf), g[::-1] * 2 * np.pi, dur


def main():
    out = {}
    for name, args in DESIGNS.items():
        k, rf, g, dur = dz2d(*args)
        assert np.all(np.isfinite(k)) and np.all(np.isfinite(rf)), name
        out[name] = dict(args=list(args), duration_ms=dur, k_re=k.real.tolist(), k_im=k.imag.tolist(), rf=rf.tolist(),
                         g_re=g.real.tolist(), g_im=g.imag.tolist())
        print("%-20s ns %4d  duration %.4f ms  max|g| %.4f G/cm" % (name, args[3], dur, np.abs(g).max() / (2 * np.pi) /
                                                                   (GAMMA * dur / args[3])))
    with open(os.path.join(HERE, "spiral.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
