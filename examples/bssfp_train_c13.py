"""What a balanced-SSFP train of the 60-degree lactate pulse of bssfp_pulse_sb_mb.py does to hyperpolarised C-13 magnetisation, echo
by echo.  The magnetisation starts far above equilibrium and never comes back, so the steady state says nothing here: what counts is
the signal the excited metabolite gives at each echo and how much of the metabolites left alone survives the train.  One period is
the pulse and the dead time of one repetition, the dead time as two zero-b1 samples so that the echo is read in its middle;
mbfir.bloch_train_batch plays it 64 times with the RF phase alternated and the first repetition at half the amplitude (alpha / 2
catalysation), at the transmit gains 0.9, 1.0 and 1.1, with meq = 0 (the thermal magnetisation is nothing beside the hyperpolarised
one) from m0 = [0 0 1].  Prints per band the echo signal |Mxy| of the first, the middle and the last repetition and the fraction of
Mz left after the train.  No plots.

    python examples/bssfp_train_c13.py [--tr 6.0] [--ntr 64] [--t1 30] [--t2 2]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--ntr", type=int, default=64)
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
args = ap.parse_args()
B0, n, T, FA, d1, d2 = 14.0, 100, 4.0, 60.0, 0.01, 0.005               # bSSFP_pulse_sb_mb.m:9-15
pick, sel = [5, 0, 2, 3, 1], 4                                          # urea, pyruvate, alanine, pyruvate hydrate, lactate
names = ["urea", "pyruvate", "alanine", "pyr. hydrate", "lactate"]
cf = mbfir.spec.spectrum_c13(B0)[pick] * 1e-3                           # kHz
cf = cf - cf[sel]
dt = T / n
rf, _, rf_spec, _ = mbfir.dzrf_mb(n, dt, list(cf), [0.1] * 5, [FA if i == sel else 0.0 for i in range(5)],
                                  [d1 if i == sel else d2 for i in range(5)], "ex", "ap_minorder_cvx", "C-13", 0, 1, None, 0, 58,
                                  probes=4)
if len(rf) == 0:
    sys.exit("Filter design failed.")
nrf = len(rf)
dead = args.tr - nrf * dt
if dead <= 0:
    sys.exit("TR is shorter than the pulse.")
scales, N = (0.9, 1.0, 1.1), args.ntr
f = np.asarray(rf_spec["f"]) * (1 / dt) / 2                             # band edges, kHz
K = 17                                                                  # points per band
df = np.concatenate([np.linspace(f[2 * i], f[2 * i + 1], K) for i in range(5)]) * 1e3          # Hz
b1 = np.concatenate([rf, [0.0, 0.0]])                                   # the pulse, then the dead time in two halves
tp = np.concatenate([np.full(nrf, dt), [dead / 2, dead / 2]]) * 1e-3    # s
period = (b1, None, tp, args.t1, args.t2, "C-13")
gains = np.append(0.5, np.ones(N - 1))                                  # alpha / 2, then alpha
((mx, my, mz), (fx, fy, fz)), = mbfir.bloch_train_batch([period], df, 0.0, N, phases=np.pi, gains=gains, echo=nrf + 1, scales=scales,
                                                        meq=0.0, final=True)
mxy = np.hypot(mx, my)[:, :, :, 0]                                      # (3 gains, N echoes, 5 K points)
left = fz[:, :, 0]                                                      # m0 = [0 0 1]: Mz after the train is the fraction left
print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), echo %.3f ms after the pulse, T1 %.0f s, T2 %.1f s"
      % (N, nrf * dt, dead, args.tr, dead / 2, args.t1, args.t2))
print("per band: the smallest .. largest value over its %d points" % K)
for si, s in enumerate(scales):
    print("transmit gain %.1f" % s)
    for i, name in enumerate(names):
        b = slice(i * K, (i + 1) * K)
        row = ["%.4f .. %.4f" % (mxy[si, k, b].min(), mxy[si, k, b].max()) for k in (0, N // 2, N - 1)]
        print("  %-13s |Mxy| echo 1: %s   echo %d: %s   echo %d: %s   Mz left: %.4f .. %.4f"
              % (name, row[0], N // 2 + 1, row[1], N, row[2], left[si, b].min(), left[si, b].max()))
