"""The variable-flip-angle schedule of bssfp_train_vfa.py designed with dense Levenberg-Marquardt steps instead of L-BFGS.  A
schedule of N repetitions has N gains, so the whole Jacobian of the echoes in the gains is one mbfir.bloch_train_jacobian_sched_batch
call (the period is swept twice whatever N is, a direction then costs two 3 x 3 products per repetition and point)
and a step is an N x N solve on the host.  The residual is the band-integrated echo amplitude of every repetition less its mean over
the repetitions; its squared norm over N - 1 is the variance that bssfp_train_vfa.py lowers.  Starting from the same textbook schedule
it prints the schedule and the variance before and after; run bssfp_train_vfa.py for the L-BFGS figures on the same train.  No plots.

    python examples/bssfp_train_vfa_gn.py [--tr 6.0] [--ntr 16] [--t1 30] [--t2 2] [--steps 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--ntr", type=int, default=16)
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--steps", type=int, default=5, help="Levenberg-Marquardt steps (one Jacobian each)")
args = ap.parse_args()
B0, n, T, FA, d1, d2 = 14.0, 100, 4.0, 60.0, 0.01, 0.005               # bSSFP_pulse_sb_mb.m:9-15
pick, sel = [5, 0, 2, 3, 1], 4                                          # urea, pyruvate, alanine, pyruvate hydrate, lactate
cf = mbfir.spec.spectrum_c13(B0)[pick] * 1e-3                           # kHz
cf = cf - cf[sel]
dt = T / n
rf, _, rf_spec, _ = mbfir.dzrf_mb(n, dt, list(cf), [0.1] * 5, [FA if i == sel else 0.0 for i in range(5)],
                                  [d1 if i == sel else d2 for i in range(5)], "ex", "ap_minorder_cvx", "C-13", 0, 1, None, 0, 58,
                                  probes=4)
if len(rf) == 0:
    sys.exit("Filter design failed.")
nrf, N = len(rf), args.ntr
dead = args.tr - nrf * dt
if dead <= 0:
    sys.exit("TR is shorter than the pulse.")
f = np.asarray(rf_spec["f"]) * (1 / dt) / 2                             # band edges, kHz
lo, hi = f[2 * sel], f[2 * sel + 1]
df = np.linspace(lo - (hi - lo) / 2, hi + (hi - lo) / 2, 33) * 1e3      # Hz: the lactate band and half a band of its skirts
pulse = (np.concatenate([rf, [0.0, 0.0]]), None, np.concatenate([np.full(nrf, dt), [dead / 2, dead / 2]]) * 1e-3, args.t1, args.t2,
         "C-13")                                                         # the pulse, then the dead time in two halves
kw = dict(phases=np.pi, echo=nrf + 1, meq=0.0)
theta = np.arctan(1.0 / np.sqrt(np.maximum(N - np.arange(N) - 1, 1e-30)))             # the last one is 90 degrees
gains = theta / np.deg2rad(FA)


def signal(g):
    """The band-integrated echo amplitude of every repetition, (N,)"""
    (mx, my, _), = mbfir.bloch_train_batch([pulse], df, np.zeros(1), N, gains=g, **kw)
    return np.hypot(mx[0, :, :, 0].mean(1), my[0, :, :, 0].mean(1))


def signal_and_jacobian(g):
    """(s (N,), ds/dgains (N, N)): one call, the primal echoes with bloch_train_batch's bits next to the 2 N tangents"""
    ((mx, my, _), (dx, dy, _)), = mbfir.bloch_train_jacobian_sched_batch([pulse], df, np.zeros(1), N, gains=g, primal=True, **kw)
    X, Y = mx[0, :, :, 0].mean(1), my[0, :, :, 0].mean(1)
    dX, dY = dx[:N, 0, :, :, 0].mean(2), dy[:N, 0, :, :, 0].mean(2)      # (direction j, repetition k): the gains' half
    s = np.hypot(X, Y)
    return s, ((X * dX + Y * dY) / s).T


def show(tag, g):
    s = signal(g)
    print("%s: variance of the echo amplitude %.3e (mean %.4f, min %.4f, max %.4f)" % (tag, s.var(ddof=1), s.mean(), s.min(), s.max()))
    print("  flip angles (degrees): " + " ".join("%.1f" % v for v in g * FA))
    print("  echo amplitudes:       " + " ".join("%.4f" % v for v in s))


print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), T1 %.0f s, T2 %.1f s, %d points over the lactate band"
      % (N, nrf * dt, dead, args.tr, args.t1, args.t2, len(df)))
show("textbook schedule atan(1 / sqrt(N - k - 1))", gains)
C = np.eye(N) - 1.0 / N                                                  # takes the mean over the repetitions out
mu, calls = 1e-4, 0
for step in range(args.steps):
    s, J = signal_and_jacobian(gains)
    r, Jr = C @ s, C @ J
    calls += 1
    while True:                                                          # Levenberg-Marquardt on 1/2 |r|^2
        d = np.linalg.solve(Jr.T @ Jr + mu * np.eye(N), -Jr.T @ r)
        trial = C @ signal(gains + d)
        calls += 1
        if trial @ trial < r @ r:
            gains, mu = gains + d, mu / 3
            break
        mu *= 4
        if mu > 1e6:
            break
    print("  step %d: variance %.3e (mu %.1e)" % (step + 1, min(trial @ trial, r @ r) / (N - 1), mu))
show("after %d Levenberg-Marquardt steps on the gains (%d device calls)" % (args.steps, calls), gains)
