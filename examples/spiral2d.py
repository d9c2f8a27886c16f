"""A 2D excitation on an inward spiral (mbfir.dz2d): the reference's example dz2d(8, 1, 4, 512, 1, 2), "an 8 ms 8 turn spiral" that
reaches 0.5 cycles/cm within 1 G/cm and 2 (G/cm)/ms, scaled to 90 degrees.  One mbfir.abr2_batch call simulates it over a 65 x 65
grid of +-8 cm at five transmit gains; prints |Mxy| along the x axis and the pass-disc minimum and stop-ring maximum over the whole
grid for every gain.  No plots.

    python examples/spiral2d.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

rf, g, ms = mbfir.dz2d(8, 1, 4, 512, 1, 2)
dt = ms / len(rf)                                                   # ms per sample
k = np.cumsum(g[::-1]) / (2 * np.pi)                                # the trajectory walked outwards, cycles/cm
# csg.m warps time with gamma = 4.26 kHz/G and a first-order rule for the slew rate, which its result overshoots; ktog / ktos
# (4.257) measure what the waveform has
print("dz2d: %d samples, %.4f ms, reaches %.3f cycles/cm; max gradient %.3f G/cm, max slew rate %.2f (G/cm)/ms"
      % (len(rf), ms, abs(k[-1]), np.abs(mbfir.ktog(k, dt)).max(), np.abs(mbfir.ktos(k, dt)).max()))

scales = [0.8, 0.9, 1.0, 1.1, 1.2]
x = np.linspace(-8, 8, 65)                                          # cm
(a, b), = mbfir.abr2_batch([(rf * np.pi / 2, g)], x, x, scales=scales, convention="abr")
mxy = np.abs(2 * np.conj(a) * b)                                    # (5, 65, 65)
r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
cols = [32, 34, 36, 40, 44, 48, 56, 64]
print("|Mxy| along y = 0:")
print("  gain   " + "".join("x=%-6.2f" % x[c] for c in cols) + " min r<=1  max 3.5<=r<=8")
for s, m in zip(scales, mxy):
    print("  %.2f   " % s + "".join("%-8.4f" % m[c, 32] for c in cols) + " %-9.4f %.4f" % (m[r <= 1].min(), m[(r >= 3.5) & (r <= 8)].max()))
