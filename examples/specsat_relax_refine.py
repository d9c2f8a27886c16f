"""Refinement of the dual-band H-1 saturation pulse of specsat_h1_dualband.py under relaxation.  The pulse lasts 26 ms; it is
designed without relaxation, and in vivo T2 is a few tens of ms, so the Mz it leaves in its bands is not the Mz of its design.
mbfir.bloch_batch simulates it with T1 / T2 at the transmit gains s = 0.9, 1.0 and 1.1; a few torch.optim.LBFGS steps through
mbfir.torchsim.bloch, whose backward is one mbfir.bloch_vjp_batch call, then lower sum w (mz - target)^2 over the three bands, with
target cos(s FA) per band (FA 120, 0 and 90 degrees), w = 1 in the two saturation bands and --wpass in the untouched one.  Prints
the worst in-band |mz - target| per band and gain without relaxation, with it, and after the refinement.  No plots.

    python examples/specsat_relax_refine.py [--steps 20] [--t1 1.0] [--t2 0.06] [--wpass 1] [--n 260]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--t1", type=float, default=1.0, help="s")
ap.add_argument("--t2", type=float, default=0.06, help="s")
ap.add_argument("--wpass", type=float, default=1.0, help="weight of the untouched band")
ap.add_argument("--n", type=int, default=260)
args = ap.parse_args()
n, T, d1, d2 = args.n, 26.0, 0.05, 0.001                                # specsat_H1_dualband.m:4-13
B0 = 127794577 / (42.577e6)
bands = [(1.8, 2.5), (3.0, 4.1), (4.8, 5.4)]                            # ppm; the last one is water
ref = sum(bands[2]) / 2
mb_cf = [[(lo - ref) * B0 * 42.577e-3, (hi - ref) * B0 * 42.577e-3] for lo, hi in bands]   # kHz
mb_FA, mb_range, mb_ripple = [120, 0, 90], [0.01] * 3, [d1, d2, d1]
dt = T / n
if abs(dt / 4e-3 - round(dt / 4e-3)) > 1e-9:                            # :38-43
    dt = 4e-3 * math.floor(dt / 4e-3)
rf0, _, rf_spec, _ = mbfir.dzrf_mb(n, dt, mb_cf, mb_range, mb_FA, mb_ripple, "sat", "ap_mintran_cvx", "H-1", 0, 1, None, 0, None,
                                   0.95, 1, probes=3)
if len(rf0) == 0:
    sys.exit("Filter design failed.")
scales = (0.9, 1.0, 1.1)
f = np.asarray(rf_spec["f"]) * (1 / dt) / 2                             # band edges, kHz
K = 33                                                                  # points per band
df = np.concatenate([np.linspace(f[2 * i], f[2 * i + 1], K) for i in range(3)]) * 1e3          # Hz
target = np.stack([np.repeat([math.cos(s * fa * math.pi / 180) for fa in mb_FA], K) for s in scales])[:, :, None]
w = np.broadcast_to(np.repeat([1.0, args.wpass, 1.0], K)[None, :, None], target.shape).copy()
target, w = torch.tensor(target), torch.tensor(w)
gr, tp = np.zeros(len(rf0)), dt * 1e-3


def report(name, mz):
    e = np.abs(np.asarray(mz) - target.numpy())[:, :, 0]
    print("%-22s loss %10.3f" % (name, float((w.numpy()[:, :, 0] * e ** 2).sum()))
          + "".join("   gain %.1f: %s" % (s, " ".join("%.4f" % e[k, K * i:K * (i + 1)].max() for i in range(3)))
                    for k, s in enumerate(scales)))


print("worst |mz - cos(s FA)| in the bands %s kHz, %d samples, %.2f ms:"
      % (", ".join("[%.3f, %.3f]" % (f[2 * i], f[2 * i + 1]) for i in range(3)), len(rf0), len(rf0) * dt))
(_, _, mz), = mbfir.bloch_batch([(rf0, gr, tp, 1e3, 1e3, "H-1")], df, 0.0, scales=scales)
report("no relaxation", mz)
(_, _, mz), = mbfir.bloch_batch([(rf0, gr, tp, args.t1, args.t2, "H-1")], df, 0.0, scales=scales)
report("T1 %.2f s, T2 %.0f ms" % (args.t1, args.t2 * 1e3), mz)

b1 = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
opt = torch.optim.LBFGS([b1], lr=1.0, max_iter=args.steps, history_size=10, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    mz = mbfir.torchsim.bloch(b1, gr, tp, args.t1, args.t2, df, 0.0, nucleus="H-1", scales=scales)[2]
    loss = (w * (mz - target) ** 2).sum()
    loss.backward()
    return loss


opt.step(closure)
with torch.no_grad():
    report("refined, %d steps" % args.steps, mbfir.torchsim.bloch(b1, gr, tp, args.t1, args.t2, df, 0.0, nucleus="H-1", scales=scales)[2])
print("peak |b1| %.5f -> %.5f G" % (np.abs(rf0).max(), float(b1.detach().abs().max())))
