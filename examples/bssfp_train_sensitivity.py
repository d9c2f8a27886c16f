"""How sensitive the lactate train of bssfp_train_c13.py is, echo by echo, to two things that go wrong in practice: an amplitude
droop of 1 % across the pulse (the amplifier sags: v_t = -0.01 (t / n) b1_t) and a magnetisation that the previous block left 1 %
off the z axis (dm_0 = [0.01 0 0]).  Both are directions of mbfir.bloch_train_jvp_batch, the tangent of the train, so one call gives
the first-order change of every echo of every band at the transmit gains 0.9, 1.0 and 1.1: no step size, no second and third
train.  Prints per band the change of the echo signal |Mxy| at the first, the middle and the last repetition for each of the two
perturbations.  No plots.

    python examples/bssfp_train_sensitivity.py [--tr 6.0] [--ntr 64] [--t1 30] [--t2 2]
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
droop = -0.01 * np.concatenate([np.arange(nrf) / nrf, [0.0, 0.0]]) * b1
v = np.stack([droop, np.zeros_like(b1)])                                # direction 0: the droop; direction 1: m0 alone
zero = np.zeros((2, len(df), 1))
tilt = zero.copy()
tilt[1] = 0.01
(((mx, my, mz), (dx, dy, dz)),) = mbfir.bloch_train_jvp_batch([period], df, 0.0, N, [v], tangents_m0=[(tilt, zero, zero)],
                                                              phases=np.pi, gains=gains, echo=nrf + 1, scales=scales, meq=0.0,
                                                              primal=True)
mxy = np.hypot(mx, my)[:, :, :, 0]                                      # (3 gains, N echoes, 5 K points)
dmxy = ((mx * dx + my * dy)[:, :, :, :, 0] / np.maximum(mxy, 1e-300))   # d|Mxy| per direction: (2, 3 gains, N echoes, 5 K points)
print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), echo %.3f ms after the pulse" % (N, nrf * dt, dead, args.tr, dead / 2))
print("first-order change of |Mxy| per band: the smallest .. largest value over its %d points" % K)
for k, what in enumerate(("a 1 %% amplitude droop across the pulse", "m0 tilted by 0.01 towards x")):
    print(what % ())
    for si, s in enumerate(scales):
        print("  transmit gain %.1f" % s)
        for i, name in enumerate(names):
            b = slice(i * K, (i + 1) * K)
            row = ["%+.2e .. %+.2e" % (dmxy[k, si, e, b].min(), dmxy[k, si, e, b].max()) for e in (0, N // 2, N - 1)]
            print("    %-13s echo 1: %s   echo %d: %s   echo %d: %s   (|Mxy| at echo %d: %.4f .. %.4f)"
                  % (name, row[0], N // 2 + 1, row[1], N, row[2], N, mxy[si, N - 1, b].min(), mxy[si, N - 1, b].max()))
