"""Refinement of the 60-degree lactate pulse of bssfp_pulse_sb_mb.py in the quantity a balanced-SSFP train sees: the steady state of
one repetition under T1 / T2.  The pulse is designed for its single-shot profile; for hyperpolarised C-13 (T1 of tens of seconds, TR
of a few ms) the fixed point of pulse + dead time is far from it.  One period here is two repetitions with the RF phase alternated,
[b, 0, -b, 0] with a zero-b1 sample of TR - T after each pulse (per-sample tp), built with torch.cat so that autograd ties the two
halves.  mbfir.bloch_batch(mode=1) gives the steady state at the transmit gains s = 0.9, 1.0 and 1.1; a few torch.optim.LBFGS steps
through mbfir.torchsim.bloch(steady_state=True), whose backward is one mbfir.bloch_ss_vjp_batch call, then lower the weighted
least-squares loss sum w_ex (|Mxy| - target_s)^2 over the excited band + w_pass sum (mx^2 + my^2 + (mz - 1)^2) over the four bands
left alone, target_s being the on-resonance bSSFP signal of the flip angle s FA.  Prints the worst in-band deviation per band and
gain before and after.  No plots.

    python examples/bssfp_steady_refine.py [--steps 20] [--tr 6.0] [--t1 30] [--t2 2] [--wpass 1]
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
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--wpass", type=float, default=1.0, help="weight of the bands left alone")
args = ap.parse_args()
B0, n, T, FA, d1, d2 = 14.0, 100, 4.0, 60.0, 0.01, 0.005               # bSSFP_pulse_sb_mb.m:9-15
pick, sel = [5, 0, 2, 3, 1], 4                                          # urea, pyruvate, alanine, pyruvate hydrate, lactate
names = ["urea", "pyruvate", "alanine", "pyr. hydrate", "lactate"]
cf = mbfir.spec.spectrum_c13(B0)[pick] * 1e-3                           # kHz
cf = cf - cf[sel]
dt = T / n
rf0, _, rf_spec, _ = mbfir.dzrf_mb(n, dt, list(cf), [0.1] * 5, [FA if i == sel else 0.0 for i in range(5)],
                                   [d1 if i == sel else d2 for i in range(5)], "ex", "ap_minorder_cvx", "C-13", 0, 1, None, 0, 58,
                                   probes=4)
if len(rf0) == 0:
    sys.exit("Filter design failed.")
nrf = len(rf0)
dead = args.tr - nrf * dt
if dead <= 0:
    sys.exit("TR is shorter than the pulse.")
scales = (0.9, 1.0, 1.1)
f = np.asarray(rf_spec["f"]) * (1 / dt) / 2                             # band edges, kHz
K = 17                                                                  # points per band
df = np.concatenate([np.linspace(f[2 * i], f[2 * i + 1], K) for i in range(5)]) * 1e3          # Hz
tp = np.concatenate([np.full(nrf, dt), [dead], np.full(nrf, dt), [dead]]) * 1e-3               # s: two repetitions
gr = np.zeros(len(tp))
ex = np.zeros(5 * K, dtype=bool)
ex[sel * K:(sel + 1) * K] = True
r12 = args.t1 / args.t2


def bssfp(alpha):
    """on-resonance bSSFP signal with alternated phase at TR << T2"""
    return math.sin(alpha) / ((r12 + 1) - math.cos(alpha) * (r12 - 1))


target = torch.tensor([bssfp(s * FA * math.pi / 180) for s in scales])[:, None]
zero = torch.zeros(1, dtype=torch.complex128)


def steady(b):
    """(mx, my, mz), each (3 gains, 5 K points): the steady state just before a +b pulse"""
    period = torch.cat([b, zero, -b, zero])
    m = mbfir.torchsim.bloch(period, gr, tp, args.t1, args.t2, df, 0.0, nucleus="C-13", scales=scales, steady_state=True)
    return tuple(v[:, :, 0] for v in m)


def loss_of(m):
    mx, my, mz = m
    mxy = torch.sqrt(mx * mx + my * my + 1e-24)
    lex = ((mxy[:, ex] - target) ** 2).sum()
    lpass = (mx[:, ~ex] ** 2 + my[:, ~ex] ** 2 + (mz[:, ~ex] - 1) ** 2).sum()
    return lex + args.wpass * lpass


def report(name, m):
    mx, my, mz = (v.detach().numpy() for v in m)
    mxy = np.hypot(mx, my)
    print("%-20s loss %.6f" % (name, float(loss_of(m))))
    for k, s in enumerate(scales):
        cells = []
        for i in range(5):
            a, z = mxy[k, i * K:(i + 1) * K], mz[k, i * K:(i + 1) * K]
            cells.append("%s |Mxy| [%.4f, %.4f] mz [%.4f, %.4f]" % (names[i], a.min(), a.max(), z.min(), z.max()))
        print("   gain %.1f (target |Mxy| %.4f in %s): %s" % (s, float(target[k]), names[sel], "; ".join(cells)))


print("steady state of %d samples (%.2f ms) in TR %.2f ms, T1 %.0f s, T2 %.1f s, phase alternated; %d points per band"
      % (nrf, nrf * dt, args.tr, args.t1, args.t2, K))
b1 = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
with torch.no_grad():
    report("designed", steady(b1))
opt = torch.optim.LBFGS([b1], lr=1.0, max_iter=args.steps, history_size=10, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    loss = loss_of(steady(b1))
    loss.backward()
    return loss


opt.step(closure)
with torch.no_grad():
    report("refined, %d steps" % args.steps, steady(b1))
print("peak |b1| %.5f -> %.5f G" % (np.abs(rf0).max(), float(b1.detach().abs().max())))
