"""Cost of the magnitude least-squares calls of the Bloch simulator (magnitude=True on mbfir.bloch_lsq_batch, bloch_gn_batch,
bloch_lm_step_batch, their steady-state twins and the refiners) on the two shapes of the neighbouring sections: 64 pulses
of 64 samples on 85 points, and one 600-sample pulse on 16384 points, each at 3 transmit-gain scales, for the end point (mode 0) and
the steady state (mode 1).  Three comparisons per shape and model, all in one session:
    twins:   each magnitude call against its component twin (same staging, same launches: the difference is the sweep kernel's)
    routes:  the fused magnitude lsq and gn (K = 1) against the shipped routes they replace, the forward call or the tangent, the
             NumPy seed, then the adjoint
    solvers: one Levenberg-Marquardt iterate of the refiner with magnitude=True, solver="device" against solver="host"
Times are warm host clocks around calls that end in a stream synchronise (transfers and the NumPy between the calls included); the
calls of a comparison alternate; the minimum, the median and the spread (max - min) / min of --reps each.  One JSON line per shape
and model.

    python tools/gpu_blochmag.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SC = (0.9, 1.0, 1.1)


def shape(name, steady):
    """(pulses, df, dp, pairs of targets and weights, triples of weights, directions)"""
    rng = np.random.default_rng(0)
    if name == "64x64x85":
        P, n, dur, nf, npos = 64, 64, 4e-3, 1, 85
    else:
        P, n, dur, nf, npos = 1, 600, 26e-3, 2048, 8
    t1, t2 = (0.2, 40e-3) if steady else (1.0, 40e-3)
    pulses = []
    for _ in range(P):
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.2 / (2 * np.pi * 4257.6 * dur))
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, t1, t2, "H-1"))
    df, dp = np.linspace(-200, 200, nf) if nf > 1 else np.zeros(1), np.linspace(-2, 2, npos)
    w3 = [tuple(rng.uniform(0, 1, (3, len(SC), nf, npos))) for _ in range(P)]
    t2p = [(rng.uniform(0, 1, (len(SC), nf, npos)), rng.uniform(-1, 1, (len(SC), nf, npos))) for _ in range(P)]
    v = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(p[0]).max() for p in pulses]
    return pulses, df, dp, t2p, [(w[0], w[2]) for w in w3], w3, v


def clock(fns, reps):
    for _, f in fns:
        f()
    acc = {k: [] for k, _ in fns}
    for _ in range(reps):
        for k, f in fns:
            t0 = time.perf_counter()
            f()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(ms=min(v), median=float(np.median(v)), spread=(max(v) - min(v)) / min(v)) for k, v in acc.items()}


def measure(name, steady, reps):
    import mbfir
    ctx = mbfir.get_context()
    pulses, df, dp, t2p, w2, w3, v = shape(name, steady)
    kw = dict(scales=SC, ctx=ctx)
    if steady:
        fwd = lambda: mbfir.bloch_batch(pulses, df, dp, mode=1, **kw)
        lsq, gn, lm = mbfir.bloch_ss_lsq_batch, mbfir.bloch_ss_gn_batch, mbfir.bloch_ss_lm_step_batch
        jvp, vjp, refine = mbfir.bloch_ss_jvp_batch, mbfir.bloch_ss_vjp_batch, mbfir.refine_bloch_ss_batch
    else:
        fwd = lambda: mbfir.bloch_batch(pulses, df, dp, **kw)
        lsq, gn, lm = mbfir.bloch_lsq_batch, mbfir.bloch_gn_batch, mbfir.bloch_lm_step_batch
        jvp, vjp, refine = mbfir.bloch_jvp_batch, mbfir.bloch_vjp_batch, mbfir.refine_bloch_batch
    t3 = [(t[0], t[0], t[1]) for t in t2p]
    mu = [1e-3] * len(pulses)

    def direction(m):
        rho = np.sqrt(m[0] * m[0] + m[1] * m[1])
        safe = np.where(rho > 0, rho, 1.0)
        return rho, np.where(rho > 0, m[0] / safe, 0.0), np.where(rho > 0, m[1] / safe, 0.0)

    def lsq_route():
        seeds, L = [], []
        for m, t, w in zip(fwd(), t2p, w2):
            rho, ux, uy = direction(m)
            r, rz = rho - t[0], m[2] - t[1]
            L.append(0.5 * float((w[0] * r * r).sum() + (w[1] * rz * rz).sum()))
            seeds.append((w[0] * r * ux, w[0] * r * uy, w[1] * rz))
        return L, vjp(pulses, df, dp, seeds, **kw)

    def gn_route():
        seeds = []
        for (m, dm), w in zip(jvp(pulses, df, dp, v, **kw), w2):
            _, ux, uy = direction(m)
            a = ux * dm[0] + uy * dm[1]
            seeds.append((w[0] * a * ux, w[0] * a * uy, w[1] * dm[2]))
        return vjp(pulses, df, dp, seeds, **kw)
    row = dict(tool="gpu_blochmag", shape=name, steady=steady, pulses=len(pulses), samples=len(pulses[0][0]),
               points=len(df) * len(dp), scales=len(SC), reps=reps)
    row["twins"] = clock((("lsq_mag", lambda: lsq(pulses, df, dp, t2p, w2, magnitude=True, **kw)),
                          ("lsq", lambda: lsq(pulses, df, dp, t3, w3, **kw)),
                          ("gn_mag", lambda: gn(pulses, df, dp, v, w2, magnitude=True, **kw)),
                          ("gn", lambda: gn(pulses, df, dp, v, w3, **kw)),
                          ("lm_mag", lambda: lm(pulses, df, dp, v, w2, mu, targets=t2p, cg=4, rtol=0.0, magnitude=True, **kw)),
                          ("lm", lambda: lm(pulses, df, dp, v, w3, mu, targets=t3, cg=4, rtol=0.0, **kw))), reps)
    row["routes"] = clock((("lsq_mag", lambda: lsq(pulses, df, dp, t2p, w2, magnitude=True, **kw)), ("lsq_route", lsq_route),
                           ("gn_mag", lambda: gn(pulses, df, dp, v, w2, magnitude=True, **kw)), ("gn_route", gn_route)), reps)
    rkw = dict(scales=SC, iters=1, cg=4, magnitude=True, ctx=ctx)
    row["solvers"] = clock((("device", lambda: refine(pulses, df, dp, t2p, w2, solver="device", **rkw)),
                            ("host", lambda: refine(pulses, df, dp, t2p, w2, solver="host", **rkw))), max(3, reps // 4))
    (La, ga), (Lb, gb) = lsq(pulses, df, dp, t2p, w2, magnitude=True, **kw)[0], (lambda r: (r[0][0], r[1][0]))(lsq_route())
    gb = gb[0] if isinstance(gb, tuple) else gb
    row["lsq_vs_route_rel"] = max(abs(La - Lb) / abs(Lb), float(np.abs(ga - gb).max() / np.abs(gb).max()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for name in ("64x64x85", "600x16384"):
        for steady in (False, True):
            print(json.dumps(measure(name, steady, a.reps)), flush=True)


if __name__ == "__main__":
    main()
