"""The case of specsat_relax_refine.py (the 26 ms dual-band H-1 saturation pulse, refined under T1 / T2 at the transmit gains 0.9, 1.0
and 1.1) on the fused device products of the Bloch model: Levenberg-Marquardt by mbfir.refine_bloch_batch (one mbfir.bloch_lsq_batch
call per trial step, one mbfir.bloch_gn_batch call per conjugate-gradient iteration; with --solver device each step solved and
tried in one mbfir.bloch_lm_step_batch call, the host run repeated beside it for its call counts), and L-BFGS driven by
mbfir.bloch_lsq_batch alone, which returns the loss and its gradient in one call.  Prints the loss (sum w (mz - target)^2, as the other two examples
print it) and the device calls of each run beside the calls the two-call paths of specsat_relax_gauss_newton.py and
specsat_relax_refine.py take for the same products: two per loss and gradient (bloch_batch, bloch_vjp_batch) and two per
Gauss-Newton product (bloch_jvp_batch, bloch_vjp_batch).  On this case Gauss-Newton does not beat L-BFGS per simulation (DESIGN
8q); the two results are printed side by side so that this stays visible.  No plots.
With --magnitude the fit is on (|Mxy|, mz): |sin| of the scaled flip angle beside its cosine, the same weights on
both, every call made with magnitude=True; the printed loss is then sum w ((|Mxy| - target)^2 + (mz - target)^2).

    python examples/specsat_relax_lm.py [--steps 8] [--cg 12] [--lbfgs 20] [--t1 1.0] [--t2 0.06] [--wpass 1] [--n 260] [--solver host|device]
                                        [--magnitude]
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
ap.add_argument("--steps", type=int, default=8, help="Levenberg-Marquardt steps")
ap.add_argument("--cg", type=int, default=12, help="conjugate-gradient iterations per step at the most")
ap.add_argument("--lbfgs", type=int, default=20, help="L-BFGS iterations")
ap.add_argument("--t1", type=float, default=1.0, help="s")
ap.add_argument("--t2", type=float, default=0.06, help="s")
ap.add_argument("--wpass", type=float, default=1.0, help="weight of the untouched band")
ap.add_argument("--n", type=int, default=260)
ap.add_argument("--solver", choices=("host", "device"), default="host", help="where the step's conjugate gradients run")
ap.add_argument("--magnitude", action="store_true", help="fit (|Mxy|, mz) instead of mz alone")
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
gr, tp = np.zeros(len(rf0)), dt * 1e-3
rest = (gr, tp, args.t1, args.t2, "H-1")
targets, weights = (0.0, 0.0, target), (0.0, 0.0, w)                    # mz alone is fitted
mag = dict(magnitude=True) if args.magnitude else {}
if args.magnitude:
    txy = np.stack([np.repeat([abs(math.sin(s * fa * math.pi / 180)) for fa in mb_FA], K) for s in scales])[:, :, None]
    targets, weights = (txy, target), (w, w)
b0 = np.asarray(rf0, dtype=np.complex128)



def refine(solver):
    (b,), (i,) = mbfir.refine_bloch_batch([(b0,) + rest], df, 0.0, [targets], [weights], scales=scales, iters=args.steps, cg=args.cg,
                                          rtol=1e-4, solver=solver, **mag)
    return b, i


def count(c):
    return "%d device calls (%s)" % (sum(c.values()), ", ".join("%d %s" % (c[k], k) for k in ("lsq", "gn", "lm") if k in c))


b_lm, info = refine(args.solver)
print("Levenberg-Marquardt (refine_bloch_batch, solver %s), %d samples, %.2f ms, T1 %.2f s, T2 %.0f ms"
      % (args.solver, len(b0), len(b0) * dt, args.t1, args.t2 * 1e3))
for k, L in enumerate(info["losses"]):
    print("  %s loss %.6g" % ("start " if k == 0 else "step %d" % k, 2 * L))
calls = info["calls"]
print("  solver %-6s %s" % (args.solver, count(calls)))
if args.solver == "device":                                             # the host solver on the same case, for its calls
    print("  solver %-6s %s" % ("host", count(refine("host")[1]["calls"])))

tb = torch.tensor(b0, requires_grad=True)
opt = torch.optim.LBFGS([tb], lr=1.0, max_iter=args.lbfgs, history_size=10, line_search_fn="strong_wolfe")
evals = [0]


def closure():
    """sum w r^2 = 2 L and its gradient from one bloch_lsq_batch call"""
    evals[0] += 1
    (L, g), = mbfir.bloch_lsq_batch([(tb.detach().numpy(),) + rest], df, 0.0, [targets], [weights], scales=scales, **mag)
    tb.grad = torch.tensor(2 * g)
    return torch.tensor(2 * L)


opt.step(closure)
b_lb = tb.detach().numpy()
(L_lb, _), = mbfir.bloch_lsq_batch([(b_lb,) + rest], df, 0.0, [targets], [weights], scales=scales, **mag)
print("start                 loss %.6g" % (2 * info["losses"][0]))
print("Levenberg-Marquardt   loss %.6g   %s; %d refused steps; the two-call paths take %s%d; peak |b1| %.5f G"
      % (2 * info["losses"][-1], count(calls), info["refused"], "at most " if "lm" in calls else "", 2 * (calls["lsq"] + calls["gn"] + (1 + args.cg) * calls.get("lm", 0)),
         np.abs(b_lm).max()))
print("L-BFGS, %2d iterations loss %.6g   %d device calls (lsq); the two-call path takes %d; peak |b1| %.5f G"
      % (args.lbfgs, 2 * L_lb, evals[0], 2 * evals[0], np.abs(b_lb).max()))
