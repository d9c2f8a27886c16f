"""The case of specsat_relax_refine.py (the 26 ms dual-band H-1 saturation pulse, refined under T1 / T2 at the transmit gains 0.9, 1.0
and 1.1) by Levenberg-Marquardt instead of L-BFGS.  With r = mz - target and W the band weights, a step solves (J^H W J + mu I) d =
-J^H W r by conjugate gradients on the host, in the real inner product <u, v> = Re sum conj(u) v over the b1 samples: J v is the mz
plane of one mbfir.bloch_jvp_batch call and J^H c one mbfir.bloch_vjp_batch call with the cotangent (0, 0, c).  A step that lowers
sum w r^2 is kept and mu divided by 3; one that does not is dropped and mu multiplied by 4.  Prints the loss and the number of
simulations (forward, tangent and adjoint calls, one each) beside those of the L-BFGS run of specsat_relax_refine.py.  No plots.

    python examples/specsat_relax_gauss_newton.py [--steps 8] [--cg 12] [--lbfgs 20] [--t1 1.0] [--t2 0.06] [--wpass 1] [--n 260]
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
ap.add_argument("--lbfgs", type=int, default=20, help="L-BFGS iterations of the comparison run")
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
gr, tp = np.zeros(len(rf0)), dt * 1e-3
rest = (gr, tp, args.t1, args.t2, "H-1")
sims = dict(forward=0, tangent=0, adjoint=0)


def residual(b1):
    sims["forward"] += 1
    (_, _, mz), = mbfir.bloch_batch([(b1,) + rest], df, 0.0, scales=scales)
    return mz - target


def J(b1, v):
    sims["tangent"] += 1
    (_, (_, _, dmz)), = mbfir.bloch_jvp_batch([(b1,) + rest], df, 0.0, [v], scales=scales)
    return dmz


def JH(b1, c):
    sims["adjoint"] += 1
    g, = mbfir.bloch_vjp_batch([(b1,) + rest], df, 0.0, [(np.zeros_like(c), np.zeros_like(c), c)], scales=scales)
    return g


def dot(u, v):
    return float((np.conj(u) * v).real.sum())


def lm_step(b1, r, mu):
    """d of (J^H W J + mu I) d = -J^H W r by conjugate gradients from d = 0, until <res, res> <= 1e-4 <b, b>"""
    b = -JH(b1, w * r)
    d, res, p = np.zeros_like(b), b.copy(), b.copy()
    rr = bb = dot(b, b)
    for _ in range(args.cg):
        Hp = JH(b1, w * J(b1, p)) + mu * p
        a = rr / dot(p, Hp)
        d, res = d + a * p, res - a * Hp
        rn = dot(res, res)
        if rn <= 1e-4 * bb:
            break
        p, rr = res + (rn / rr) * p, rn
    return d


def loss_of(r):
    return float((w * r * r).sum())


b1 = np.asarray(rf0, dtype=np.complex128)
r = residual(b1)
loss = loss0 = loss_of(r)
mu = 1e-3 * dot(JH(b1, w * J(b1, b1)), b1) / dot(b1, b1)                  # a thousandth of the Rayleigh quotient of J^H W J at b1
print("Levenberg-Marquardt, %d samples, %.2f ms, T1 %.2f s, T2 %.0f ms: loss %.6g" % (len(b1), len(b1) * dt, args.t1, args.t2 * 1e3, loss))
for k in range(args.steps):
    d = lm_step(b1, r, mu)
    rn = residual(b1 + d)
    ln = loss_of(rn)
    kept = ln < loss
    if kept:
        b1, r, loss, mu = b1 + d, rn, ln, mu / 3
    else:
        mu *= 4
    print("  step %d: loss %.6g (%s), mu %.3g, simulations %d" % (k + 1, ln, "kept" if kept else "dropped", mu, sum(sims.values())))
lm_sims = dict(sims)

tb = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
tt, tw = torch.tensor(target), torch.tensor(w)
opt = torch.optim.LBFGS([tb], lr=1.0, max_iter=args.lbfgs, history_size=10, line_search_fn="strong_wolfe")
evals = [0]


def closure():
    opt.zero_grad()
    evals[0] += 1
    mz = mbfir.torchsim.bloch(tb, gr, tp, args.t1, args.t2, df, 0.0, nucleus="H-1", scales=scales)[2]
    val = (tw * (mz - tt) ** 2).sum()
    val.backward()
    return val


opt.step(closure)
lb = loss_of(residual(tb.detach().numpy()))
print("start                 loss %.6g" % loss0)
print("Levenberg-Marquardt   loss %.6g   %d simulations (%d forward, %d tangent, %d adjoint), peak |b1| %.5f G"
      % (loss, sum(lm_sims.values()), lm_sims["forward"], lm_sims["tangent"], lm_sims["adjoint"], np.abs(b1).max()))
print("L-BFGS, %2d iterations loss %.6g   %d simulations (%d forward, %d adjoint), peak |b1| %.5f G"
      % (args.lbfgs, lb, 2 * evals[0], evals[0], evals[0], float(tb.detach().abs().max())))
