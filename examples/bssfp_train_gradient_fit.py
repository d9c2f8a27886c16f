"""Fit of a gradient gain error and a B0 offset from the echo train of a hyperpolarised balanced-SSFP acquisition, through the
gradients mbfir.torchsim.bloch_train has in gr and df: examples/bssfp_steady_gradient_fit.py moved to a train with meq = 0, where
the magnetisation never recovers and the steady state says nothing.
A slice-selective excitation (mbfir.dzrf, time-bandwidth 6) is reshaped onto a trapezoid by mbfir.verse, between two rewinders of half
its area and followed by the dead time of the repetition; the train plays that period --ntr times with alternating phase after a
half-angle first repetition, and the echo is read at the centre of the pulse.  The "measured" echoes are that train with the gradient
times 1.03 (the moment is then no longer balanced) and every off-resonance plus 7 Hz; two scalars, the gain and the offset, are then
recovered from their nominal values 1 and 0 by torch.optim.LBFGS on sum |echo - measured|^2, whose backward is one
mbfir.bloch_train_vjp_gr_batch call per evaluation.  Prints both with the loss before and after: the answer is
known, so this shows the plumbing.  No plots.

    python examples/bssfp_train_gradient_fit.py [--gain 1.03] [--offset 7] [--steps 30] [--ntr 32] [--t1 30] [--t2 2] [--tr 8e-3] [--flip 30]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gain", type=float, default=1.03)
ap.add_argument("--offset", type=float, default=7.0, help="Hz")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--ntr", type=int, default=32, help="repetitions")
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--tr", type=float, default=8e-3, help="s, the period: pulse, rewinders and dead time")
ap.add_argument("--flip", type=float, default=30.0, help="degrees")
args = ap.parse_args()

n, tb, dt, thk = 128, 6.0, 20e-6, 0.5                                   # samples, time-bandwidth, s, cm
ramp, nrew = 16, 32
gamma = mbfir.GAMMA_C13
shape = np.concatenate([(np.arange(ramp) + 0.5) / ramp, np.ones(n - 2 * ramp), (np.arange(ramp)[::-1] + 0.5) / ramp])
rf = mbfir.verse(shape, mbfir.dzrf(n, tb, "st", "ls"))[:, 0]            # radians per sample, on the trapezoid
rf = rf * (np.deg2rad(args.flip) / rf.sum().real)
amp = tb / (shape.sum() * dt) / (gamma / (2 * np.pi) * thk)             # G/cm: the trapezoid's area covers tb cycles over thk
# one period: the pulse on its trapezoid, a rewinder of minus half its area before and after (balanced), the dead time
rew = -0.5 * shape.sum() / nrew * np.ones(nrew)
gz = amp * np.concatenate([rew, shape, rew, [0.0]])
b1 = np.concatenate([np.zeros(nrew), rf / (gamma * dt), np.zeros(nrew), [0.0]])          # G
nt = len(b1)
tp = np.append(np.full(nt - 1, dt), args.tr - (nt - 1) * dt)
gr0 = np.stack([np.zeros(nt), np.zeros(nt), gz], 1)                     # the slice is along z
df0 = np.array([-40.0, -20.0, 0.0, 20.0, 40.0])                        # Hz, inside the pass band of 1 / TR
dp = np.stack([np.zeros(65), np.zeros(65), np.linspace(-1.0, 1.0, 65)], 1)
train = dict(phases=np.pi * np.arange(args.ntr), gains=np.append(0.5, np.ones(args.ntr - 1)), echo=nrew + n // 2, meq=0.0)
measured, = mbfir.bloch_train_batch([(b1, args.gain * gr0, tp, args.t1, args.t2, "C-13")], df0 + args.offset, dp, args.ntr, **train)
measured = [torch.tensor(v) for v in measured]

b1t = torch.tensor(b1, dtype=torch.complex128)
g0, d0 = torch.tensor(gr0), torch.tensor(df0)
p = torch.tensor([1.0, 0.0], dtype=torch.float64, requires_grad=True)   # gain, offset / 10 Hz


def loss_of(p):
    e = mbfir.torchsim.bloch_train(b1t, p[0] * g0, tp, args.t1, args.t2, d0 + 10.0 * p[1], dp, args.ntr, nucleus="C-13", **train)
    return sum(((a - b) ** 2).sum() for a, b in zip(e, measured))


opt = torch.optim.LBFGS([p], lr=1.0, max_iter=args.steps, history_size=10, line_search_fn="strong_wolfe",
                        tolerance_grad=1e-12, tolerance_change=1e-14)
evals = [0]


def closure():
    opt.zero_grad()
    loss = loss_of(p)
    loss.backward()
    evals[0] += 1
    return loss


with torch.no_grad():
    first = float(loss_of(p))
opt.step(closure)
with torch.no_grad():
    last = float(loss_of(p))
gain, off = (float(v) for v in p.detach())
print("%d samples in a period of %.2f ms, %d repetitions, %.3f G/cm on the flat top, %d x %d points, T1 %.0f s, T2 %.1f s, meq 0, "
      "flip %.0f degrees" % (nt, args.tr * 1e3, args.ntr, amp, len(df0), dp.shape[0], args.t1, args.t2, args.flip))
print("gradient gain: true %.6f, nominal 1, fitted %.6f" % (args.gain, gain))
print("B0 offset:     true %.4f Hz, nominal 0, fitted %.4f Hz" % (args.offset, 10.0 * off))
print("loss %.6g -> %.3g in %d evaluations" % (first, last, evals[0]))
