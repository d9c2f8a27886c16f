"""Levenberg-Marquardt refinement of a 2D spiral excitation through mbfir.refine_batch: the problem of
examples/spiral2d_refine.py and examples/spiral2d_gauss_newton.py (the same pulse, grid, gains, target and weights), with every
product of the fit one device call: the loss and its gradient mbfir.abr2_lsq_batch, each CG iteration one mbfir.abr2_gn_batch
product, and nothing of grid size crossing the bus but the target and the weights.  The loop, its rules for mu and its CG stop are
those of spiral2d_gauss_newton.py, whose loss |r|^2 is twice the L = 1/2 sum w |Mxy - target|^2 of refine_batch; the lines below
print |r|^2 so that the two read side by side.  With --solver device each step is solved and tried in one
mbfir.abr2_lm_step_batch call instead: CG runs on the device and the host reads nothing between its iterations.  No torch.  No plots.

    python examples/spiral2d_lm.py [outer iterations] [CG iterations per step] [--solver host|device]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

argv = sys.argv[1:]
solver = "host"
if "--solver" in argv:
    k = argv.index("--solver")
    solver = argv[k + 1]
    del argv[k:k + 2]
outer = int(argv[0]) if len(argv) > 0 else 5
cg_max = int(argv[1]) if len(argv) > 1 else 8
rf0, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
rf0 = rf0 * np.pi / 2
scales = (0.9, 1.0, 1.1)
x = np.linspace(-8, 8, 65)                                          # cm
r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)

(a0, b0), = mbfir.abr2_batch([(rf0, g)], x, x, scales=scales)
m0 = 2 * np.conj(a0[1, 32, 32]) * b0[1, 32, 32]                     # the design's Mxy at the centre fixes the target's phase
phase = m0 / abs(m0)
target = np.stack([np.where(disc, phase * np.sin(s * np.pi / 2), 0.0) for s in scales])
w = (disc | ring).astype(np.float64)                                # one weight plane for every gain


def report(name, rf):
    (a, b), = mbfir.abr2_batch([(rf, g)], x, x, scales=scales)
    e = np.abs(2 * np.conj(a) * b - target)
    print("%-7s loss %.5f" % (name, float((w * e ** 2).sum()))
          + "".join("   gain %.1f: disc %.4f ring %.4f" % (s, e[k][disc].max(), e[k][ring].max()) for k, s in enumerate(scales)))


print("worst |Mxy - target| in the disc (r <= 1 cm) and in the ring (3.5 <= r <= 8 cm), %d samples, 65 x 65 points:" % len(rf0))
report("dz2d", rf0)
(rf,), (info,) = mbfir.refine_batch([(rf0, g)], x, x, [target], [w], profile="ex", scales=scales, iters=outer, cg=cg_max,
                                   solver=solver)
L = info["losses"]
for it in range(1, len(L)):
    print("iteration %d: loss %.5f -> %.5f" % (it, 2 * L[it - 1], 2 * L[it]))
print("%d steps refused, last mu %.3g, status %s" % (info["refused"], info["mu"], info["status"]))
report("refined", rf)
print("peak |rf| %.4f -> %.4f rad/sample" % (np.abs(rf0).max(), np.abs(rf).max()))
print("simulator calls: %d abr2_lsq_batch, %d abr2_gn_batch" % (info["calls"]["lsq"], info["calls"]["gn"])
      + (", %d abr2_lm_step_batch" % info["calls"]["lm"] if solver == "device" else ""))
