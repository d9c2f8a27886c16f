"""A metabolite-specific C-13 excitation at 3 T as a multiband spectral-spatial pulse (mbfir.dzss_mb): pyruvate at 10 degrees,
lactate at 30, alanine and bicarbonate held at 0, a slice of tbx = 4 on flyback gradients (a 0.32 ms trapezoid, a 0.16 ms
rewinder of equal area).  The pulse is simulated by mbfir.bloch over slice position x frequency; prints |Mxy| at the slice centre
in every band and the slice profile's pass and stop bands at every band centre.  No plots.

    python examples/ssmb_c13.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402


def trap(n, ramp, amp):
    t = np.full(n, float(amp))
    t[:ramp] = amp * (np.arange(ramp) + 0.5) / ramp
    t[n - ramp:] = t[:ramp][::-1]
    return t


cs = mbfir.spec.spectrum_c13(3.0) * 1e-3                            # kHz relative to pyruvate
names = ["pyruvate", "alanine", "lactate", "bicarbonate"]
mb_cf = [cs[0], cs[2], cs[1], cs[4]]
mb_FA = [10, 0, 30, 0]
dt = 0.004                                                          # ms
gx, gfb = trap(80, 16, 4.0), -trap(40, 8, 8.0)                      # G/cm

t0 = time.time()
rf, g, info = mbfir.dzss_mb(gx, dt, 25, mb_cf, [0.06] * 4, mb_FA, [0.01] * 4, "ex", "ap_cvx", "C-13", gfb=gfb)
t1 = time.time()
assert info["status"] == "Solved", info["status"]
print("designed in %.0f ms: %d subpulses, Ts %.3f ms (fs %.3f kHz), %.2f ms in all, peak %.3f G, slice %.2f cm"
      % ((t1 - t0) * 1e3, info["ngx"], info["Ts"], info["fs"], len(rf) * dt, np.abs(rf).max(), info["thk"]))

thk = info["thk"]
x = np.linspace(-3 * thk, 3 * thk, 121)                            # cm
df = np.linspace(-600.0, 600.0, 241)                                # Hz
mx, my, _ = mbfir.bloch(rf, g, dt * 1e-3, 1e6, 1e6, df, x)          # no relaxation over the pulse
mxy = np.abs(mx + 1j * my)                                          # (frequency, position)
centre = np.argmin(np.abs(x))
for name, c, fa in zip(names, mb_cf, mb_FA):
    k = np.argmin(np.abs(df - c * 1e3))
    inner, outer = np.abs(x) <= 0.35 * thk, np.abs(x) >= 1.5 * thk
    print("%-12s %+7.1f Hz  FA %2d: |Mxy| at x = 0 %.4f (sin FA %.4f); within +-0.35 thk %.4f .. %.4f, beyond 1.5 thk <= %.4f"
          % (name, c * 1e3, fa, mxy[k, centre], np.sin(np.radians(fa)), mxy[k, inner].min(), mxy[k, inner].max(),
             mxy[k, outer].max()))
