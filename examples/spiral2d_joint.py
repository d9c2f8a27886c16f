"""Joint refinement of a 2D spiral excitation's rf and gradient waveform.  The setting is examples/spiral2d_refine.py's: dz2d(8, 1,
4, 512, 1, 2) scaled to 90 degrees, the loss sum w |2 conj(a) b - target|^2 over the pass disc (r <= 1 cm) and the stop ring (3.5 <=
r <= 8 cm) at the transmit gains 0.9, 1.0 and 1.1.  mbfir.torchsim.abr2 is differentiable in rf and in the complex gradient
waveform g (its backward is then one mbfir.abr2_vjp_rfg_batch call), so the same number of torch.optim.LBFGS iterations is run twice
from the design: on rf alone, and on rf and g together.  Prints both losses and the largest change of g.  No plots.

    python examples/spiral2d_joint.py [steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rf0, g0, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
rf0, g0 = rf0 * np.pi / 2, np.asarray(g0, dtype=np.complex128)
scales = (0.9, 1.0, 1.1)
x = np.linspace(-8, 8, 65)                                          # cm
r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)

(a0, b0), = mbfir.abr2_batch([(rf0, g0)], x, x, scales=scales)
m0 = 2 * np.conj(a0[1, 32, 32]) * b0[1, 32, 32]                     # the design's Mxy at the centre fixes the target's phase
phase = m0 / abs(m0)
target = torch.tensor(np.stack([np.where(disc, phase * np.sin(s * np.pi / 2), 0.0) for s in scales]))
w = torch.tensor(np.broadcast_to((disc | ring).astype(np.float64), target.shape).copy())


def loss_of(rf, g):
    a, b = mbfir.torchsim.abr2(rf, g, x, x, scales=scales)
    return (w * (2 * a.conj() * b - target).abs() ** 2).sum()


def refine(with_g):
    rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
    g = torch.tensor(g0, dtype=torch.complex128, requires_grad=with_g)
    opt = torch.optim.LBFGS([rf, g] if with_g else [rf], lr=1.0, max_iter=steps, history_size=10, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = loss_of(rf, g)
        loss.backward()
        return loss
    opt.step(closure)
    with torch.no_grad():
        return float(loss_of(rf, g)), rf.detach().numpy(), g.detach().numpy()


with torch.no_grad():
    start = float(loss_of(torch.tensor(rf0, dtype=torch.complex128), torch.tensor(g0)))
print("%d samples, 65 x 65 points, %d L-BFGS iterations each" % (len(rf0), steps))
print("dz2d        loss %.5f" % start)
loss_rf, _, _ = refine(False)
print("rf alone    loss %.5f" % loss_rf)
loss_j, rf_j, g_j = refine(True)
print("rf and g    loss %.5f" % loss_j)
print("largest change of g %.3e rad/cm per sample (largest |g| %.3e), peak |rf| %.4f -> %.4f rad/sample"
      % (np.abs(g_j - g0).max(), np.abs(g0).max(), np.abs(rf0).max(), np.abs(rf_j).max()))
