"""A variable-flip-angle schedule for the hyperpolarised C-13 train of bssfp_train_c13.py, designed through the train's own
derivative.  The magnetisation is not renewed (meq = 0, T1 decay), so a train of N echoes has to spend it evenly.  For ideal,
perfectly spoiled pulses the constant-signal schedule is the textbook theta_k = atan(1 / sqrt(N - k - 1)); the real train is
balanced (the transverse magnetisation is carried on, the RF phase alternates), T1 and T2 are finite, and the 58-sample lactate pulse
has a slice profile across its band.  Starting from the textbook schedule as gains[k] = theta_k / 60 degrees of the 60-degree pulse,
a few L-BFGS steps on the gains through mbfir.torchsim.bloch_train (backward: one mbfir.bloch_train_vjp_sched_batch call, DESIGN
section 8ad) lower the variance over k of the band-integrated echo amplitude.  Prints the schedule and the variance before and after.
No plots.

    python examples/bssfp_train_vfa.py [--tr 6.0] [--ntr 16] [--t1 30] [--t2 2] [--steps 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--ntr", type=int, default=16)
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--steps", type=int, default=5, help="L-BFGS steps")
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
b1 = torch.tensor(np.concatenate([rf, [0.0, 0.0]]), dtype=torch.complex128)          # the pulse, then the dead time in two halves
tp = np.concatenate([np.full(nrf, dt), [dead / 2, dead / 2]]) * 1e-3    # s
theta = np.arctan(1.0 / np.sqrt(np.maximum(N - np.arange(N) - 1, 1e-30)))             # the last one is 90 degrees
gains = torch.tensor(theta / np.deg2rad(FA), dtype=torch.float64, requires_grad=True)


def signal(g):
    """The band-integrated echo amplitude of every repetition, (N,)"""
    mx, my, _ = mbfir.torchsim.bloch_train(b1, None, tp, args.t1, args.t2, df, 0.0, N, nucleus="C-13", phases=np.pi, gains=g,
                                           echo=nrf + 1, meq=0.0)
    return torch.hypot(mx[0, :, :, 0].mean(1), my[0, :, :, 0].mean(1))


def show(tag, g):
    with torch.no_grad():
        s = signal(g)
    print("%s: variance of the echo amplitude %.3e (mean %.4f, min %.4f, max %.4f)" % (tag, s.var().item(), s.mean().item(),
                                                                                      s.min().item(), s.max().item()))
    print("  flip angles (degrees): " + " ".join("%.1f" % v for v in g.detach().numpy() * FA))
    print("  echo amplitudes:       " + " ".join("%.4f" % v for v in s.numpy()))


print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), T1 %.0f s, T2 %.1f s, %d points over the lactate band"
      % (N, nrf * dt, dead, args.tr, args.t1, args.t2, len(df)))
show("textbook schedule atan(1 / sqrt(N - k - 1))", gains)
opt = torch.optim.LBFGS([gains], lr=1.0, max_iter=args.steps, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    loss = signal(gains).var()
    loss.backward()
    return loss


opt.step(closure)
show("after %d L-BFGS steps on the gains" % args.steps, gains)
