"""Gradient refinement of a 2D spiral excitation.  dz2d is a small-tip design: scaled to 90 degrees the disc profile of the
reference's example dz2d(8, 1, 4, 512, 1, 2) sags and its stop ring rises, and a transmit gain of 0.9 or 1.1 moves both.  A few
torch.optim.LBFGS steps on the simulated profile repair it: the loss is sum w |2 conj(a) b - target|^2 over the pass disc (r <= 1
cm, target sin(s pi / 2) with the phase of the design) and the stop ring (3.5 <= r <= 8 cm, target 0) at the gains s = 0.9, 1.0 and
1.1; mbfir.torchsim.abr2 simulates all three in one launch and its backward is one adjoint call (mbfir.abr2_vjp_batch).  Prints the
loss and the worst in-disc and out-of-disc errors before and after.  No plots.

    python examples/spiral2d_refine.py [steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rf0, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
rf0 = rf0 * np.pi / 2
scales = (0.9, 1.0, 1.1)
x = np.linspace(-8, 8, 65)                                          # cm
r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)

(a0, b0), = mbfir.abr2_batch([(rf0, g)], x, x, scales=scales)
m0 = 2 * np.conj(a0[1, 32, 32]) * b0[1, 32, 32]                     # the design's Mxy at the centre fixes the target's phase
phase = m0 / abs(m0)
target = torch.tensor(np.stack([np.where(disc, phase * np.sin(s * np.pi / 2), 0.0) for s in scales]))
w = torch.tensor(np.broadcast_to((disc | ring).astype(np.float64), target.shape).copy())


def profile(rf):
    a, b = mbfir.torchsim.abr2(rf, g, x, x, scales=scales)
    return 2 * a.conj() * b


def report(name, rf):
    with torch.no_grad():
        e = (profile(rf) - target).abs()
        loss = float((w * e ** 2).sum())
    e = e.numpy()
    print("%-7s loss %.5f" % (name, loss) + "".join("   gain %.1f: disc %.4f ring %.4f" % (s, e[k][disc].max(), e[k][ring].max())
                                                    for k, s in enumerate(scales)))


rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
print("worst |Mxy - target| in the disc (r <= 1 cm) and in the ring (3.5 <= r <= 8 cm), %d samples, 65 x 65 points:" % len(rf0))
report("dz2d", rf)
opt = torch.optim.LBFGS([rf], lr=1.0, max_iter=steps, history_size=10, line_search_fn="strong_wolfe")


def closure():
    opt.zero_grad()
    loss = (w * (profile(rf) - target).abs() ** 2).sum()
    loss.backward()
    return loss


opt.step(closure)
report("refined", rf)
print("peak |rf| %.4f -> %.4f rad/sample" % (np.abs(rf0).max(), float(rf.detach().abs().max())))
