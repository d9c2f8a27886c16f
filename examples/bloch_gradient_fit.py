"""Fit of a gradient gain error and a B0 offset under relaxation, through the gradients mbfir.torchsim.bloch has in gr and df.
A slice-selective excitation (mbfir.dzrf, time-bandwidth 6) is reshaped onto a trapezoid by mbfir.verse and simulated with T1 / T2
by mbfir.bloch_batch.  The "measured" profile is that simulation with the gradient times 1.03 and every off-resonance plus 7 Hz; two
scalars, the gain and the offset, are then recovered from their nominal values 1 and 0 by torch.optim.LBFGS on sum |m - measured|^2,
whose backward is one mbfir.bloch_vjp_gr_batch call per evaluation.  Prints both with the loss before and after:
the answer is known, so this shows the plumbing.  No plots.

    python examples/bloch_gradient_fit.py [--gain 1.03] [--offset 7] [--steps 30] [--t1 1.0] [--t2 0.02]
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
ap.add_argument("--t1", type=float, default=1.0, help="s")
ap.add_argument("--t2", type=float, default=0.02, help="s")
args = ap.parse_args()

n, tb, dt, thk = 128, 6.0, 40e-6, 0.5                                   # samples, time-bandwidth, s, cm
ramp = 16
shape = np.concatenate([(np.arange(ramp) + 0.5) / ramp, np.ones(n - 2 * ramp), (np.arange(ramp)[::-1] + 0.5) / ramp])
rf = mbfir.verse(shape, mbfir.dzrf(n, tb, "ex", "ls"))[:, 0]            # radians per sample, on the trapezoid
b1 = rf / (mbfir.GAMMA_H1 * dt)                                         # G
amp = tb / (shape.sum() * dt) / (mbfir.GAMMA_H1 / (2 * np.pi) * thk)    # G/cm: the trapezoid's area covers tb cycles over thk
gr0 = np.stack([np.zeros(n), np.zeros(n), amp * shape], 1)              # the slice is along z
df0 = np.array([-20.0, 0.0, 20.0])                                      # Hz
dp = np.stack([np.zeros(65), np.zeros(65), np.linspace(-1.0, 1.0, 65)], 1)
measured, = mbfir.bloch_batch([(b1, args.gain * gr0, dt, args.t1, args.t2, "H-1")], df0 + args.offset, dp)
measured = [torch.tensor(v) for v in measured]

b1t = torch.tensor(b1, dtype=torch.complex128)
g0, d0 = torch.tensor(gr0), torch.tensor(df0)
p = torch.tensor([1.0, 0.0], dtype=torch.float64, requires_grad=True)   # gain, offset / 10 Hz


def loss_of(p):
    m = mbfir.torchsim.bloch(b1t, p[0] * g0, dt, args.t1, args.t2, d0 + 10.0 * p[1], dp, nucleus="H-1")
    return sum(((a - b) ** 2).sum() for a, b in zip(m, measured))


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
print("%d samples, %.2f ms, %.3f G/cm on the flat top, %d x %d points, T1 %.2f s, T2 %.0f ms"
      % (n, n * dt * 1e3, amp, len(df0), dp.shape[0], args.t1, args.t2 * 1e3))
print("gradient gain: true %.6f, nominal 1, fitted %.6f" % (args.gain, gain))
print("B0 offset:     true %.4f Hz, nominal 0, fitted %.4f Hz" % (args.offset, 10.0 * off))
print("loss %.6g -> %.3g in %d evaluations" % (first, last, evals[0]))
