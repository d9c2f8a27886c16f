"""The train of bssfp_train_refine.py fitted by Levenberg-Marquardt on the fused products (mbfir.refine_bloch_train_batch, DESIGN
section 8ab) instead of L-BFGS over the adjoint.  The 60-degree lactate pulse of bssfp_pulse_sb_mb.py, played 64 times with
alternating phase and an alpha / 2 first repetition on hyperpolarised C-13 magnetisation (meq = 0), gives a lactate signal that
changes from echo to echo.  The fit asks for the same thing as bssfp_train_refine.py in least-squares form:
    echo term:  at the lactate points the demodulated echo (Mx, My) of every repetition after the first --skip ones should be the
                mean over those repetitions of the starting pulse's demodulated echoes: one target per (gain, point), used at
                every repetition, so only point-sized planes go up to the device and nothing echo-sized comes back;
    final term: at the other bands' points Mz after the train should be 1, weighted by --weight.
rep_weights leaves the first --skip echoes of the transient out.  refine_bloch_train_batch moves every sample of the period, the two
dead-time samples included (bssfp_train_refine.py moves the pulse's samples only): the peak |b1| line shows what that costs.
Prints the figures of bssfp_train_refine.py before and after, whose "largest deviation" line is the one to set against its L-BFGS
result at the same --tr, --ntr and --weight, and the losses and device calls of the fit.  The figures are a result, not a
criterion.  No plots.  --solver host (the default) runs the CG recurrence on the host, one bloch_train_gn_batch call per iteration
(56 device calls at the defaults); --solver device solves and tries every step in one bloch_train_lm_step_batch call
(mbfir.refine_bloch_train_lm_batch).  The last line counts the device calls of the fit.
With --magnitude the echo term asks for |Mxy| alone: at the lactate points the echo amplitude of every
repetition after the first --skip ones should be the mean amplitude over those repetitions of the starting pulse, the echo's phase
being free, and the final term is the same Mz = 1; every call of the fit is made with magnitude=True and pairs (xy, z).

    python examples/bssfp_train_lm.py [--tr 6.0] [--ntr 64] [--iters 5] [--cg 8] [--weight 10] [--skip 8] [--solver host|device]
                                      [--magnitude]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--ntr", type=int, default=64)
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--cg", type=int, default=8)
ap.add_argument("--weight", type=float, default=10.0)
ap.add_argument("--skip", type=int, default=8)
ap.add_argument("--solver", choices=("host", "device"), default="host")
ap.add_argument("--magnitude", action="store_true", help="fit (|Mxy|, mz) of the echoes instead of (mx, my, mz)")
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
dp = np.zeros(1)
tp = np.concatenate([np.full(nrf, dt), [dead / 2, dead / 2]]) * 1e-3    # the pulse, then the dead time in two halves, s
gains = np.append(0.5, np.ones(N - 1))                                  # alpha / 2, then alpha
lac = slice(sel * K, (sel + 1) * K)
b1 = np.concatenate([np.asarray(rf, dtype=np.complex128), np.zeros(2)])
kw = dict(phases=np.pi, gains=gains, echo=nrf + 1, scales=scales, meq=0.0)
rw = np.append(np.zeros(args.skip), np.ones(N - args.skip))


def pulse(b):
    return (b, None, tp, args.t1, args.t2, "C-13")


def report(title, b):
    ((mx, my, _), (_, _, fz)), = mbfir.bloch_train_batch([pulse(b)], df, dp, N, final=True, **kw)
    mxy, left = np.hypot(mx, my)[..., 0], fz[..., 0]
    print("%s: peak |b1| %.4f G" % (title, float(np.abs(b).max())))
    for si, s in enumerate(scales):
        print("transmit gain %.1f" % s)
        for i, name in enumerate(names):
            b_ = slice(i * K, (i + 1) * K)
            row = ["%.4f .. %.4f" % (mxy[si, k, b_].min(), mxy[si, k, b_].max()) for k in (0, N // 2, N - 1)]
            print("  %-13s |Mxy| echo 1: %s   echo %d: %s   echo %d: %s   Mz left: %.4f .. %.4f"
                  % (name, row[0], N // 2 + 1, row[1], N, row[2], left[si, b_].min(), left[si, b_].max()))
    sig = mxy[:, :, lac]
    print("  lactate |Mxy|: largest deviation from its mean over the echoes %.4f" % np.abs(sig - sig.mean(1, keepdims=True)).max())
    sig = sig[:, args.skip:]
    print("  the same after the first %d echoes %.4f" % (args.skip, np.abs(sig - sig.mean(1, keepdims=True)).max()))


print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), T1 %.0f s, T2 %.1f s; per band the smallest .. largest value "
      "over its %d points" % (N, nrf * dt, dead, args.tr, args.t1, args.t2, K))
report("before", b1)
(ex, ey, _), = mbfir.bloch_train_batch([pulse(b1)], df, dp, N, demod=True, **kw)
S, nf = len(scales), len(df)
on = np.zeros((S, nf, 1))
on[:, lac] = 1.0
target = (ex[:, args.skip:].mean(1) * on, ey[:, args.skip:].mean(1) * on, 0.0)       # the mean demodulated echo, per (gain, point)
weight, target_final, weight_final, mag = (on, on, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, args.weight * (1 - on)), {}
if args.magnitude:                                                      # the mean echo amplitude, per (gain, point); pairs (xy, z)
    target, weight = (np.hypot(ex, ey)[:, args.skip:].mean(1) * on, 0.0), (on, 0.0)
    target_final, weight_final, mag = (0.0, 1.0), (0.0, args.weight * (1 - on)), dict(magnitude=True)
t0 = time.perf_counter()
(b1_lm,), (info,) = mbfir.refine_bloch_train_lm_batch([pulse(b1)], df, dp, N, [target], [weight], rep_weights=rw,
                                                       targets_final=[target_final], weights_final=[weight_final], demod=True,
                                                       iters=args.iters, cg=args.cg, solver=args.solver, **kw, **mag)
ms = (time.perf_counter() - t0) * 1e3
print("Levenberg-Marquardt (%s solver): %d accepted steps, %d refused, losses %s, calls %s: %d device calls, %.1f ms" %
      (args.solver, len(info["losses"]) - 1, info["refused"], " ".join("%.6g" % v for v in info["losses"]), info["calls"],
       sum(info["calls"].values()), ms))
report("after Levenberg-Marquardt on the fused products", b1_lm)
