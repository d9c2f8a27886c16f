"""Levenberg-Marquardt refinement of the 60-degree lactate pulse of bssfp_pulse_sb_mb.py on its balanced-SSFP steady state, the case
of bssfp_steady_refine.py: the 58-sample pulse in TR = 6 ms with the RF phase alternated, one period [b, 0, -b, 0] with a zero-b1
sample of TR - T after each pulse, T1 = 30 s, T2 = 2 s, 17 points per band, transmit gains 0.9 / 1.0 / 1.1.  The fit is a plain
weighted least squares in (mx, my, mz), which the fused products take as it is: the targets are the designed pulse's own steady state
at gain 1.0 inside the lactate band, at every gain (so that the excitation does not move with the gain), and (0, 0, 1) in the four
bands left alone, with unit weights.  Two optimisers run from the designed period on the same loss:
    mbfir.refine_bloch_ss_batch: CG on (H + mu I) d = -g with one bloch_ss_gn_batch call per iteration and one bloch_ss_lsq_batch
        call per trial step (--solver host, the default), or every step solved and tried in one bloch_ss_lm_step_batch call
        (--solver device: the same losses to the printed digits in a fraction of the device calls);
    torch.optim.LBFGS with a strong-Wolfe line search, its closure one bloch_ss_lsq_batch call.
Both move every sample of the period: the two halves are not tied to b and -b and the dead-time samples are free, which the report
shows (a tied design takes the chain rule g_b = g[first half] - g[second half] instead, as bssfp_steady_refine.py's autograd does).
Prints the losses, the worst in-band ranges per band and gain, and the device calls each optimiser made.  No plots.
With --magnitude the same goal is put on (|Mxy|, mz): the designed |Mxy| and mz at gain 1.0 in the lactate band, 0 and
1 elsewhere; the band's phase is then free.  Every call of both optimisers is made with magnitude=True.

    python examples/bssfp_steady_lm.py [--iters 6] [--cg 8] [--steps 20] [--tr 6.0] [--t1 30] [--t2 2] [--solver host] [--magnitude]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=6, help="accepted Levenberg-Marquardt steps")
ap.add_argument("--cg", type=int, default=8, help="CG iterations per step")
ap.add_argument("--steps", type=int, default=20, help="L-BFGS iterations")
ap.add_argument("--tr", type=float, default=6.0, help="ms")
ap.add_argument("--t1", type=float, default=30.0, help="s")
ap.add_argument("--t2", type=float, default=2.0, help="s")
ap.add_argument("--solver", choices=("host", "device"), default="host", help="where the Levenberg-Marquardt step is solved")
ap.add_argument("--magnitude", action="store_true", help="fit (|Mxy|, mz) instead of (mx, my, mz)")
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
period0 = np.concatenate([rf0, [0.0], -np.asarray(rf0), [0.0]]).astype(np.complex128)
rest = (gr, tp, args.t1, args.t2, "C-13")
calls = dict(forward=0, lsq=0)


def steady(b):
    calls["forward"] += 1
    m, = mbfir.bloch_batch([(b,) + rest], df, 0.0, scales=scales, mode=1)
    return tuple(v[:, :, 0] for v in m)                                 # each (3 gains, 5 K points)


designed = steady(period0)
target = tuple(np.where(ex[None, :], designed[c][1][None, :], 1.0 if c == 2 else 0.0)[:, :, None] * np.ones((3, 1, 1)) for c in range(3))
weight = (1.0, 1.0, 1.0)
mag = dict(magnitude=True) if args.magnitude else {}
if args.magnitude:
    target, weight = (np.hypot(target[0], target[1]), target[2]), (1.0, 1.0)


def lsq(b):
    calls["lsq"] += 1
    (L, g), = mbfir.bloch_ss_lsq_batch([(b,) + rest], df, 0.0, [target], [weight], scales=scales, **mag)
    return L, g


def report(name, b):
    mx, my, mz = steady(b)
    mxy = np.hypot(mx, my)
    print("%-28s loss %.6g" % (name, lsq(b)[0]))
    for k, s in enumerate(scales):
        cells = []
        for i in range(5):
            a, z = mxy[k, i * K:(i + 1) * K], mz[k, i * K:(i + 1) * K]
            cells.append("%s |Mxy| [%.4f, %.4f] mz [%.4f, %.4f]" % (names[i], a.min(), a.max(), z.min(), z.max()))
        print("   gain %.1f: %s" % (s, "; ".join(cells)))
    halves = np.abs(b[:nrf] + b[nrf + 1:2 * nrf + 1]).max() / np.abs(b).max()
    print("   peak |b1| %.5f G, dead-time samples |b1| %.3g and %.3g G, |first half + second half| / peak %.3g"
          % (np.abs(b).max(), abs(b[nrf]), abs(b[-1]), halves))


print("steady state of %d samples (%.2f ms) in TR %.2f ms, T1 %.0f s, T2 %.1f s, phase alternated; %d points per band; target: the"
      " designed steady state at gain 1.0 in %s, (0, 0, 1) elsewhere" % (nrf, nrf * dt, args.tr, args.t1, args.t2, K, names[sel]))
report("designed", period0)

(b_lm,), (info,) = mbfir.refine_bloch_ss_batch([(period0,) + rest], df, 0.0, [target], [weight], scales=scales, iters=args.iters,
                                               cg=args.cg, solver=args.solver, **mag)
print("Levenberg-Marquardt: losses %s; status %s, %d refused, last mu %.3g; device calls %s"
      % (" ".join("%.6g" % v for v in info["losses"]), info["status"], info["refused"], info["mu"], info["calls"]))
report("Levenberg-Marquardt, %d steps" % (len(info["losses"]) - 1), b_lm)

size = float(np.abs(period0).max())                                     # L-BFGS works on b1 / max|b1|
x = torch.tensor(np.concatenate([period0.real, period0.imag]) / size, requires_grad=True)
opt = torch.optim.LBFGS([x], lr=1.0, max_iter=args.steps, history_size=10, line_search_fn="strong_wolfe")
before, trace = calls["lsq"], []


def closure():
    v = x.detach().numpy() * size
    L, g = lsq(v[:len(period0)] + 1j * v[len(period0):])
    x.grad = torch.tensor(np.concatenate([g.real, g.imag]) * size)
    trace.append(L)
    return torch.tensor(L)


opt.step(closure)
lbfgs_calls = calls["lsq"] - before
v = x.detach().numpy() * size
print("L-BFGS: loss %.6g -> %.6g (lowest seen %.6g) in %d bloch_ss_lsq_batch calls" % (trace[0], trace[-1], min(trace), lbfgs_calls))
report("L-BFGS, %d iterations" % args.steps, v[:len(period0)] + 1j * v[len(period0):])
