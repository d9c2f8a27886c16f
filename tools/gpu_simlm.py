"""Cost of one tried Levenberg-Marquardt step solved on the device (mbfir.abr_lm_step_batch / abr2_lm_step_batch) against the host
loop of mbfir.refine_batch(solver="host") that it replaces, at cg = 8 and rtol = 0 (every iteration runs), for two shapes:
    spiral   the pulse of tools/gpu_simgn.py: dz2d(8, 1, 4, 512, 1, 2) at 90 degrees on 128 x 128 points at 3 gains, profile 'ex'
    short    a batch of 64 1D pulses of 64 samples on 65 points at 3 gains: the regime the host loop serves worst
Timed per shape:
    device   one lm_step call with targets: one upload, 2 cg + 4 launches, one download
    host     the same step as refine_batch's host solver takes it: 8 gn calls with the CG arithmetic in NumPy, then 1 lsq call
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the two alternate, minimum and median
of --reps each.  One JSON line.

    python tools/gpu_simlm.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CG = 8


def _dot(u, v):
    return float((np.conj(u) * v).real.sum())


def spiral(mbfir):
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    rf = rf * np.pi / 2
    x, sc = np.linspace(-8, 8, 128), (0.9, 1.0, 1.1)
    r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
    disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)
    target = np.stack([np.where(disc, np.sin(s * np.pi / 2) + 0j, 0.0) for s in sc])
    w = np.broadcast_to((disc | ring).astype(np.float64), target.shape)
    return True, [(rf, g)], (x, x), [target], [w], sc


def short(mbfir):
    n, x, sc = 64, np.linspace(-8, 8, 65), (0.9, 1.0, 1.1)
    win = np.hanning(n + 2)[1:-1] * np.sinc(np.linspace(-2, 2, n))
    band, stop = np.abs(x) <= 0.6, np.abs(x) >= 2.5
    pulses, targets, weights = [], [], []
    for flip in np.linspace(0.3 * np.pi, 0.6 * np.pi, 64):
        pulses.append(win * (flip / win.sum()) + 0j)
        targets.append(np.stack([np.where(band, 1j * np.sin(s * flip), 0.0) for s in sc]))
        weights.append((band | stop).astype(np.float64))
    return False, pulses, (x,), targets, weights, sc


def measure(mbfir, ctx, shape, reps):
    two, pulses, pos, targets, weights, sc = shape(mbfir)
    pre = "abr2_" if two else "abr_"
    lsq, gn, lm = (getattr(mbfir, pre + k) for k in ("lsq_batch", "gn_batch", "lm_step_batch"))
    kw = dict(scales=sc, ctx=ctx)
    b = [-g for _, g in lsq(pulses, *pos, targets, weights, **kw)]
    mu = [1e-3 * _dot(v, h) / _dot(v, v) for v, h in zip(b, gn(pulses, *pos, b, weights, **kw))]
    rfs = [p[0] if isinstance(p, tuple) else p for p in pulses]

    def device():
        return [d for d, _ in lm(pulses, *pos, b, weights, mu, targets=targets, cg=CG, rtol=0.0, **kw)]

    def host():                                                   # refine_batch's host solver, one tried step
        P = range(len(pulses))
        d = [np.zeros_like(v) for v in b]
        r = [v.copy() for v in b]
        p = [v.copy() for v in b]
        rr = [_dot(v, v) for v in r]
        for _ in range(CG):
            for q, hp in zip(P, gn(pulses, *pos, p, weights, **kw)):
                ap = hp + mu[q] * p[q]
                alpha = rr[q] / _dot(p[q], ap)
                d[q], r[q] = d[q] + alpha * p[q], r[q] - alpha * ap
                rr[q], old = _dot(r[q], r[q]), rr[q]
                p[q] = r[q] + (rr[q] / old) * p[q]
        trial = [(rfs[q] + d[q], pulses[q][1]) if isinstance(pulses[q], tuple) else rfs[q] + d[q] for q in P]
        lsq(trial, *pos, targets, weights, **kw)
        return d
    runs = (("device", device), ("host", host))
    out = {name: f() for name, f in runs}
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t0 = time.perf_counter()
            f()
            t[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(pulses=len(pulses), samples=len(rfs[0]), points=int(np.prod([len(v) for v in pos])), scales=len(sc), cg=CG)
    for name, _ in runs:
        row["ms_" + name] = min(t[name])
        row["ms_" + name + "_median"] = float(np.median(t[name]))
    row["speedup"] = row["ms_host"] / row["ms_device"]
    row["step_device_vs_host"] = max(float(np.abs(u - v).max() / np.abs(v).max()) for u, v in zip(out["device"], out["host"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import mbfir
    ctx = mbfir.get_context()
    print(json.dumps(dict(tool="gpu_simlm", reps=a.reps, spiral=measure(mbfir, ctx, spiral, a.reps),
                          short=measure(mbfir, ctx, short, a.reps))))


if __name__ == "__main__":
    main()
