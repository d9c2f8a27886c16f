"""specsat_minripple_C13.m on the MI355X: a C-13 spectral saturation pulse at 3 T (alanine saturated, lactate untouched)
designed as a multiband arbitrary-phase pulse with the smallest stopband ripple (`ap_minstopripple_cvx`), against the
conventional maximum-phase SLR pulse `dzrf(n, T*BW, 'sat', 'max', d1, 0.5*d2)` (:57-63), both simulated over transmit-gain
errors of -20 .. +20 % (sim_rf_scale.m, :90-92).  Prints the reference's comparison numbers; no plots.

    python examples/specsat_minripple_c13.py
"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

B0, n, T, FA, d1, d2, gamma = 3.0, 150, 10.0, 90.0, 0.05, 1e-3, 1.0705      # :6-17
cf = mbfir.spec.spectrum_c13(B0)[[2, 1]]                                   # alanine, lactate (pick_compound = [3 2])
mb_cf = list((cf - cf[0]) * 1e-3)                                           # kHz
mb_range, mb_FA, mb_ripple = [0.05, 0.05], [FA, 0], [d1, d2]
dt = T / n
if abs(dt / 4e-3 - round(dt / 4e-3)) > 1e-9:                               # :41-45
    dt = 4e-3 * math.floor(dt / 4e-3)
    T = n * dt
fs = 1 / dt

t0 = time.time()
rf, _, rf_spec, _ = mbfir.dzrf_mb(n, dt, mb_cf, mb_range, mb_FA, mb_ripple, "sat", "ap_minstopripple_cvx", "C-13", 0, 1, 1e-3, 0)
t1 = time.time()
BW = 0.25                                                                   # kHz
rf2 = mbfir.dzrf(n, T * BW, "sat", "max", d1, 0.5 * d2)
rf2 = rf2 * (FA * math.pi / 180) / np.sum(rf2)
rf2 = mbfir.rfscaleg(rf2, T, gamma)
t2 = time.time()
if len(rf) == 0:
    sys.exit("Filter design failed.")
dt2 = dt
n1, n2 = "mb-ap-SLR", "sb-mp-SLR"
print("%s vs. %s" % (n1, n2))
print("%s computation time: %.4f s" % (n1, t1 - t0))
print("%s computation time: %.4f s" % (n2, t2 - t1))
print("%s pulse duration: %.3f ms" % (n1, len(rf) * dt))
print("%s pulse duration: %.3f ms" % (n2, len(rf2) * dt2))
p1, p2 = np.sum(np.abs(rf) ** 2) * dt, np.sum(np.abs(rf2) ** 2) * dt2
print("%s pulse power: %.4f G^2*ms" % (n1, p1))
print("%s pulse power: %.4f G^2*ms" % (n2, p2))
print("power ratio: %.4f" % (p1 / p2))
print("%s pulse peak amplitude: %.4f G" % (n1, np.abs(rf).max()))
print("%s pulse peak amplitude: %.4f G" % (n2, np.abs(rf2).max()))
print("amplitude ratio: %.4f" % (np.abs(rf).max() / np.abs(rf2).max()))

scale = [0.8, 0.9, 1.0, 1.1, 1.2]
f = np.asarray(rf_spec["f"]) * fs / 2                                       # kHz, the 9-argument form of sim_rf_scale
for name, pulse, step in ((n1, rf, dt), (n2, rf2, dt2)):
    df, mxy, mz = mbfir.sim_rf_scale(pulse, step, scale, "C-13", f=f)
    print("%s, Mz over the bands at each transmit gain:" % name)
    for k, s in enumerate(scale):
        cells = []
        for i in range(len(rf_spec["d"])):
            m = (df >= f[2 * i] * 1e3) & (df <= f[2 * i + 1] * 1e3)
            cells.append("band %d [%.4f, %.4f]" % (i, mz[k, m].min(), mz[k, m].max()))
        print("  %+4.0f%%  %s" % ((s - 1) * 100, "   ".join(cells)))
