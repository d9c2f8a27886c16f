"""Gauss-Newton refinement of a 2D spiral excitation: the problem of examples/spiral2d_refine.py (the same pulse, grid, gains,
target and weights) as the nonlinear least-squares fit it is.  The residual is r = sqrt(w) (2 conj(a) b - target) over the pass
disc, the stop ring and the gains 0.9, 1.0 and 1.1, the loss |r|^2, and each Levenberg-Marquardt step solves
(J^T J + mu I) d = -J^T r by conjugate gradients on the real form of rf (Re rf, Im rf), with
    J v     one mbfir.abr2_jvp_batch call and the chain rule dM = 2 (conj(da) b + conj(a) db), which is real-linear in v, and
    J^T c   one mbfir.abr2_vjp_batch call with the cotangents (2 b conj(c'), 2 a c'), c' = sqrt(w) c.
mu shrinks after a step that lowers the loss and grows after one that does not.  No torch.  Prints the loss after every outer
iteration, the number of simulator calls, and the worst in-disc and out-of-disc errors that spiral2d_refine.py prints.  No plots.

    python examples/spiral2d_gauss_newton.py [outer iterations] [CG iterations per step]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbfir  # noqa: E402

outer = int(sys.argv[1]) if len(sys.argv) > 1 else 5
cg_max = int(sys.argv[2]) if len(sys.argv) > 2 else 8
rf0, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
rf0 = rf0 * np.pi / 2
scales = (0.9, 1.0, 1.1)
x = np.linspace(-8, 8, 65)                                          # cm
r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)
calls = dict(forward=0, jvp=0, vjp=0)


def simulate(rf):
    calls["forward"] += 1
    (a, b), = mbfir.abr2_batch([(rf, g)], x, x, scales=scales)
    return a, b


a0, b0 = simulate(rf0)
m0 = 2 * np.conj(a0[1, 32, 32]) * b0[1, 32, 32]                     # the design's Mxy at the centre fixes the target's phase
phase = m0 / abs(m0)
target = np.stack([np.where(disc, phase * np.sin(s * np.pi / 2), 0.0) for s in scales])
sw = np.sqrt(np.broadcast_to((disc | ring).astype(np.float64), target.shape))


def residual(a, b):
    return sw * (2 * np.conj(a) * b - target)


def J(rf, a, b, v):
    calls["jvp"] += 1
    (_, (da, db)), = mbfir.abr2_jvp_batch([(rf, g)], x, x, [v], scales=scales)
    return sw * 2 * (np.conj(da) * b + np.conj(a) * db)


def JT(rf, a, b, c):
    """the v with Re sum(conj(c) J w) = Re sum(conj(v) w) for every w"""
    calls["vjp"] += 1
    c = sw * c
    grad, = mbfir.abr2_vjp_batch([(rf, g)], x, x, [(2 * b * np.conj(c), 2 * a * c)], scales=scales)
    return grad


def dot(u, v):
    """the inner product of the real forms"""
    return float((np.conj(u) * v).real.sum())


def report(name, rf, a, b):
    e = np.abs(2 * np.conj(a) * b - target)
    print("%-7s loss %.5f" % (name, dot(residual(a, b), residual(a, b)))
          + "".join("   gain %.1f: disc %.4f ring %.4f" % (s, e[k][disc].max(), e[k][ring].max()) for k, s in enumerate(scales)))


print("worst |Mxy - target| in the disc (r <= 1 cm) and in the ring (3.5 <= r <= 8 cm), %d samples, 65 x 65 points:" % len(rf0))
report("dz2d", rf0, a0, b0)
rf, a, b = rf0.copy(), a0, b0
res = residual(a, b)
loss = dot(res, res)
mu = None
for it in range(outer):
    grad = JT(rf, a, b, res)                                        # J^T r: half the gradient of the loss
    if mu is None:
        jg = J(rf, a, b, grad)
        mu = 1e-3 * dot(jg, jg) / dot(grad, grad)                   # a Rayleigh quotient of J^T J sets the scale of mu
    while True:
        d, q = np.zeros_like(rf), -grad                             # CG on (J^T J + mu I) d = -J^T r from d = 0
        p, qq, n_cg = q.copy(), dot(q, q), 0
        while n_cg < cg_max and qq > 1e-6 * dot(grad, grad):
            jp = J(rf, a, b, p)
            ap = JT(rf, a, b, jp) + mu * p
            alpha = qq / dot(p, ap)
            d, q = d + alpha * p, q - alpha * ap
            qq, old = dot(q, q), qq
            p = q + (qq / old) * p
            n_cg += 1
        an, bn = simulate(rf + d)
        rn = residual(an, bn)
        new = dot(rn, rn)
        if new < loss:
            rf, a, b, res = rf + d, an, bn, rn
            print("iteration %d: loss %.5f -> %.5f   (%d CG iterations, mu %.3g)" % (it + 1, loss, new, n_cg, mu))
            loss, mu = new, mu / 3
            break
        mu *= 4
        print("iteration %d: step refused (loss %.5f), mu -> %.3g" % (it + 1, new, mu))
        if mu > 1e12:
            break
report("refined", rf, a, b)
print("peak |rf| %.4f -> %.4f rad/sample" % (np.abs(rf0).max(), np.abs(rf).max()))
print("simulator calls: %d abr2_batch, %d abr2_jvp_batch, %d abr2_vjp_batch" % (calls["forward"], calls["jvp"], calls["vjp"]))
