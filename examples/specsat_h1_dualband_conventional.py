"""specsat_H1_dualband_conventional.m on the MI355X: a dual-band H-1 spectral saturation pulse at 3 T built the conventional
way: two minimum-phase equiripple filters (dzmp, 519-tap Parks-McClellan designs factored by fmp) scaled to sin(FA/2), the
NAA one shifted to its band, summed into one beta, then b2a / ab2rf (:36-55, :95-99).  Prints the pulse numbers and the
simulated Mz in each band; no plots.

    python examples/specsat_h1_dualband_conventional.py
"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

n, B0, T, d1, d2, FA1, FA2, gamma = 260, 3.0015, 26.0, 0.0008, 0.03, 120.0, 90.0, 4.2576     # :8-19
dt = T / n
f1, f2, f3 = (np.array(v) * B0 * 42.577e-3 for v in ([1.8, 2.5], [3.0, 4.1], [4.8, 5.4]))    # kHz
fr = f3.mean()
f1, f2, f3 = f1 - fr, f2 - fr, f3 - fr
BW1 = ((f1[1] + f2[0]) / 2 - f1.mean()) * 2
BW2 = (f3.mean() - (f2[1] + f3[0]) / 2) * 2

t0 = time.time()
b1 = math.sin(0.5 * FA1 * math.pi / 180) * mbfir.dzmp(n, T * BW1, d1, d2)
b2 = math.sin(0.5 * FA2 * math.pi / 180) * mbfir.dzmp(n, T * BW2, d1, d2)
t_axis = np.arange(n) * dt
b = b1 * np.exp(-1j * 2 * np.pi * f1.mean() * t_axis) + b2
rf = mbfir.rfscaleg(mbfir.ab2rf(mbfir.b2a(b), b), T, gamma)
print("computation time: %.4f s" % (time.time() - t0))
print("pulse duration:   %.3f ms" % (len(rf) * dt))
print("total power:      %.4f G^2*ms" % (np.sum(np.abs(rf) ** 2) * dt))
print("peak amplitude:   %.4f G" % np.max(np.abs(rf)))
fs = 1 / dt
fk = np.linspace(-fs / 2, fs / 2, 2048)
_, be = mbfir.abr(rf * (2 * np.pi * gamma * dt), fk * len(rf) * dt)
mz = 1 - 2 * np.abs(be) ** 2                                                # abr.m:12
for name, (lo, hi), target in (("NAA", f1, math.cos(FA1 * math.pi / 180)), ("3-4.1 ppm", f2, 1.0),
                               ("water", f3, math.cos(FA2 * math.pi / 180))):
    m = (fk >= lo) & (fk <= hi)
    print("  %-9s [%7.3f, %7.3f] kHz: Mz in [%.4f, %.4f]   target %.4f" % (name, lo, hi, mz[m].min(), mz[m].max(), target))
