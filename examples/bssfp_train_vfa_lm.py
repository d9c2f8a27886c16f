"""The variable-flip-angle schedule of bssfp_train_vfa.py refined by mbfir.refine_bloch_train_sched_batch: dense
Levenberg-Marquardt on the gains with the loss, its gradient and the N x N normal matrix formed on the device.  Where
bssfp_train_vfa_gn.py brings the echoes of every repetition and their 2 N tangents to the host and can afford that only on its 33
points, here nothing echo-sized crosses the bus in either direction: the targets are demodulated and broadcast, one point-sized plane
used at every repetition, and what comes back per step is N numbers, or N x N for the matrix.  The fit asks every repetition for the
same transverse magnetisation at the lactate points: the target is the mean over the repetitions of the demodulated echo of the
textbook schedule, point by point, so a flat echo train has zero loss.  Starting from that schedule it prints the schedule, the
losses of the accepted steps and the echo amplitudes before and after.  A result, not a criterion.  No plots.

    python examples/bssfp_train_vfa_lm.py [--tr 6.0] [--ntr 16] [--t1 30] [--t2 2] [--steps 5] [--solver host|device] [--magnitude]

--solver device takes the steps through mbfir.refine_bloch_train_sched_lm_batch: conjugate gradients on the
device in the call that evaluates the trial, one call and one set of propagator sweeps per accepted step.
With --magnitude the goal is one constant |Mxy| for every echo: the target is the mean over the repetitions and
the points of the textbook schedule's echo amplitude, one number, and the echo's phase is free; every call is made with
magnitude=True and pairs (xy, z).
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
ap.add_argument("--steps", type=int, default=5, help="accepted Levenberg-Marquardt steps at the most")
ap.add_argument("--solver", choices=("host", "device"), default="host", help="dense Cholesky on the host, or CG on the device")
ap.add_argument("--magnitude", action="store_true", help="fit one constant |Mxy| for every echo instead of (mx, my)")
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
df = np.linspace(lo, hi, 33) * 1e3                                      # Hz: the lactate band
pos = np.zeros(1)
pulse = (np.concatenate([rf, [0.0, 0.0]]), None, np.concatenate([np.full(nrf, dt), [dead / 2, dead / 2]]) * 1e-3, args.t1, args.t2,
         "C-13")                                                         # the pulse, then the dead time in two halves
kw = dict(phases=np.pi, echo=nrf + 1, meq=0.0, demod=True)
theta = np.arctan(1.0 / np.sqrt(np.maximum(N - np.arange(N) - 1, 1e-30)))             # the last one is 90 degrees
gains = theta / np.deg2rad(FA)


def echoes(g):
    """The demodulated echoes of every repetition, (mx, my) each (N, nf)"""
    (mx, my, _), = mbfir.bloch_train_batch([pulse], df, pos, N, gains=g, **kw)
    return mx[0, :, :, 0], my[0, :, :, 0]


def show(tag, g):
    mx, my = echoes(g)
    s = np.hypot(mx.mean(1), my.mean(1))
    print("%s: band-integrated echo amplitude mean %.4f, min %.4f, max %.4f, variance %.3e" % (tag, s.mean(), s.min(), s.max(), s.var(ddof=1)))
    print("  flip angles (degrees): " + " ".join("%.1f" % v for v in g * FA))
    print("  echo amplitudes:       " + " ".join("%.4f" % v for v in s))


print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), T1 %.0f s, T2 %.1f s, %d points over the lactate band"
      % (N, nrf * dt, dead, args.tr, args.t1, args.t2, len(df)))
show("textbook schedule atan(1 / sqrt(N - k - 1))", gains)
mx, my = echoes(gains)
target = (mx.mean(0)[:, None], my.mean(0)[:, None], 0.0)                # (nf, npos) planes: the same at every repetition
weights, mag = (1.0, 1.0, 0.0), {}                                      # the transverse components only
if args.magnitude:                                                      # one constant |Mxy| for every echo and point; pairs (xy, z)
    target, weights = (float(np.hypot(mx, my).mean()), 0.0), (1.0, 0.0)
    mag = dict(magnitude=True)
    print("magnitude target: |Mxy| = %.4f at every echo and point" % target[0])
if args.solver == "host":
    (sch,), (info,) = mbfir.refine_bloch_train_sched_batch([pulse], df, pos, N, [target], [weights], vary=("gains",), iters=args.steps,
                                                           gains=gains, **kw, **mag)
else:
    (sch,), (info,) = mbfir.refine_bloch_train_sched_lm_batch([pulse], df, pos, N, [target], [weights], vary=("gains",),
                                                              iters=args.steps, gains=gains, solver="device", cg=N, **kw, **mag)
print("losses of the accepted steps: " + " ".join("%.4e" % v for v in info["losses"]))
print("status %s, %d refused steps, last mu %.2e, device calls: %d lsq, %d gn" % (info["status"], info["refused"], info["mu"],
                                                                                   info["calls"]["lsq"], info["calls"]["gn"])
      + (", %d lm" % info["calls"]["lm"] if "lm" in info["calls"] else ""))
show("after refine_bloch_train_sched_batch on the gains" if args.solver == "host" else
     "after refine_bloch_train_sched_lm_batch(solver='device') on the gains", sch[0])
