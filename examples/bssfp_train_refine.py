"""Shapes the echo-by-echo signal of the train of bssfp_train_c13.py with its gradient.  The 60-degree lactate pulse of
bssfp_pulse_sb_mb.py, played 64 times with alternating phase and an alpha / 2 first repetition on hyperpolarised C-13 magnetisation
(meq = 0), gives a lactate signal that changes from echo to echo.  A few L-BFGS iterations through mbfir.torchsim.bloch_train (the
forward one mbfir.bloch_train_batch call, the backward one mbfir.bloch_train_vjp_batch call) move the pulse's
samples so that the lactate |Mxy| stays closer to its mean over the echoes, while the four metabolites that the pulse leaves alone
keep their Mz after the train.  The loss is
    sum over the lactate points and the echoes of (|Mxy| - mean over the echoes of |Mxy|)^2
  + weight x sum over the other bands' points of (1 - Mz after the train)^2
at the transmit gains 0.9, 1.0 and 1.1.  Prints per band the figures of bssfp_train_c13.py before and after.  The figures are a
result, not a criterion.  No plots.

    python examples/bssfp_train_refine.py [--tr 6.0] [--ntr 64] [--iters 20] [--weight 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--ntr", type=int, default=64)
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--weight", type=float, default=10.0)
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
tp = np.concatenate([np.full(nrf, dt), [dead / 2, dead / 2]]) * 1e-3    # the pulse, then the dead time in two halves, s
gains = np.append(0.5, np.ones(N - 1))                                  # alpha / 2, then alpha
lac = slice(sel * K, (sel + 1) * K)
rest = np.ones(5 * K, dtype=bool)
rest[lac] = False
rest = torch.from_numpy(rest)
rf = np.asarray(rf, dtype=np.complex128)
x = torch.tensor(np.stack([rf.real, rf.imag], 1), requires_grad=True)   # the pulse's samples (Re, Im): the dead time stays zero


def train(x):
    b1 = torch.cat([torch.view_as_complex(x), torch.zeros(2, dtype=torch.complex128)])
    (mx, my, mz), (fx, fy, fz) = mbfir.torchsim.bloch_train(b1, None, tp, args.t1, args.t2, df, 0.0, N, nucleus="C-13", phases=np.pi,
                                                            gains=gains, echo=nrf + 1, scales=scales, meq=0.0, final=True)
    return mx[:, :, :, 0], my[:, :, :, 0], fz[:, :, 0]                  # (3 gains, N echoes, 5 K points) twice, (3 gains, 5 K points)


def loss(x):
    mx, my, left = train(x)
    sig = torch.hypot(mx[:, :, lac], my[:, :, lac])
    return ((sig - sig.mean(1, keepdim=True)) ** 2).sum() + args.weight * ((1 - left[:, rest]) ** 2).sum()


def report(title, x):
    with torch.no_grad():
        mx, my, left = (v.numpy() for v in train(x))
        mxy = np.hypot(mx, my)
        print("%s: loss %.6g, peak |b1| %.4f G" % (title, float(loss(x)), float(torch.view_as_complex(x).abs().max())))
    for si, s in enumerate(scales):
        print("transmit gain %.1f" % s)
        for i, name in enumerate(names):
            b = slice(i * K, (i + 1) * K)
            row = ["%.4f .. %.4f" % (mxy[si, k, b].min(), mxy[si, k, b].max()) for k in (0, N // 2, N - 1)]
            print("  %-13s |Mxy| echo 1: %s   echo %d: %s   echo %d: %s   Mz left: %.4f .. %.4f"
                  % (name, row[0], N // 2 + 1, row[1], N, row[2], left[si, b].min(), left[si, b].max()))
    sig = mxy[:, :, lac]
    print("  lactate |Mxy|: largest deviation from its mean over the echoes %.4f" % np.abs(sig - sig.mean(1, keepdims=True)).max())


print("%d repetitions of %.3f ms pulse + %.3f ms dead time (TR %.1f ms), T1 %.0f s, T2 %.1f s; per band the smallest .. largest value "
      "over its %d points" % (N, nrf * dt, dead, args.tr, args.t1, args.t2, K))
report("before", x)
opt = torch.optim.LBFGS([x], max_iter=args.iters, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    v = loss(x)
    v.backward()
    return v


opt.step(closure)
report("after %d L-BFGS iterations" % args.iters, x)
