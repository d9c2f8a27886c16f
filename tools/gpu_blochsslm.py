"""Cost of one tried Levenberg-Marquardt step of the steady state solved on the device (mbfir.bloch_ss_lm_step_batch) against the
host loop of mbfir.refine_bloch_ss_batch(solver="host") that it replaces, at cg = 8 and rtol = 0 (every iteration runs), for the two
shapes of tools/gpu_blochlm.py taken as steady-state periods:
    long     600 samples, 26 ms, T2 = 40 ms on 2048 frequencies x 8 positions at 3 gains
    short    a batch of 64 periods of 64 samples, 4 ms, T2 = 10 ms on 3 frequencies x 33 positions at 3 gains: the regime the host
             loop serves worst
Timed per shape:
    device   one bloch_ss_lm_step_batch call with targets: one upload, 2 cg + 5 launches (pass 0 once), one download
    host     the same step as the host solver takes it: 8 bloch_ss_gn_batch calls (pass 0 in each) with the CG arithmetic in NumPy,
             then 1 bloch_ss_lsq_batch call
    gn, lsq  one bloch_ss_gn_batch call and one bloch_ss_lsq_batch call alone, to say where the host solver's time goes
    fwd      one bloch_batch(mode=1) call: the kernel k_bloch_ss_lm_prep is to be read beside in a kernel trace
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the five alternate, minimum and median
of --reps each.  One JSON line.

    python tools/gpu_blochsslm.py [--reps 20] [--shape both]
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
SC = (0.9, 1.0, 1.1)


def _dot(u, v):
    return float((np.conj(u) * v).real.sum())


def long_pulse(mbfir):
    rng = np.random.default_rng(0)
    n, dur, nf, npos = 600, 26e-3, 2048, 8
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    w = tuple(rng.uniform(0, 1, (3, len(SC), nf, npos)))
    t = tuple(rng.uniform(-1, 1, (3, len(SC), nf, npos)))
    return pulses, df, dp, [t], [w]


def short(mbfir):
    n, dur = 64, 4e-3
    df, dp = np.linspace(-100, 100, 3), np.linspace(-3, 3, 33)
    win = np.hanning(n + 2)[1:-1]
    tz = np.where(np.abs(dp) < 1.0, 0.0, 1.0)[None, :] * np.ones((3, 1))
    w = np.where((np.abs(dp) > 0.8) & (np.abs(dp) < 1.2), 0.0, 1.0)[None, :] * np.ones((3, 1))
    pulses, targets, weights = [], [], []
    for flip in np.linspace(0.3 * np.pi, 0.6 * np.pi, 64):
        b1 = win * (flip / (mbfir.GAMMA_H1 * dur / n * win.sum())) + 0j
        pulses.append((b1, np.full(n, 0.05), dur / n, 1.0, 10e-3, "H-1"))
        targets.append((0.0, 0.0, tz))
        weights.append((0.1 * w, 0.1 * w, w))
    return pulses, df, dp, targets, weights


def measure(mbfir, ctx, shape, reps):
    pulses, df, dp, targets, weights = shape(mbfir)
    kw = dict(scales=SC, ctx=ctx)
    b = [-g for _, g in mbfir.bloch_ss_lsq_batch(pulses, df, dp, targets, weights, **kw)]
    mu = [1e-3 * _dot(v, h) / _dot(v, v) for v, h in zip(b, mbfir.bloch_ss_gn_batch(pulses, df, dp, b, weights, **kw))]

    def device():
        return [d for d, _ in mbfir.bloch_ss_lm_step_batch(pulses, df, dp, b, weights, mu, targets=targets, cg=CG, rtol=0.0, **kw)]

    def host():                                                   # refine_bloch_ss_batch's host solver, one tried step
        P = range(len(pulses))
        d = [np.zeros_like(v) for v in b]
        r = [v.copy() for v in b]
        p = [v.copy() for v in b]
        rr = [_dot(v, v) for v in r]
        for _ in range(CG):
            for q, hp in zip(P, mbfir.bloch_ss_gn_batch(pulses, df, dp, p, weights, **kw)):
                ap = hp + mu[q] * p[q]
                alpha = rr[q] / _dot(p[q], ap)
                d[q], r[q] = d[q] + alpha * p[q], r[q] - alpha * ap
                rr[q], old = _dot(r[q], r[q]), rr[q]
                p[q] = r[q] + (rr[q] / old) * p[q]
        mbfir.bloch_ss_lsq_batch([(pulses[q][0] + d[q],) + tuple(pulses[q][1:]) for q in P], df, dp, targets, weights, **kw)
        return d

    def gn():
        mbfir.bloch_ss_gn_batch(pulses, df, dp, b, weights, **kw)

    def lsq():
        mbfir.bloch_ss_lsq_batch(pulses, df, dp, targets, weights, **kw)

    def fwd():
        mbfir.bloch_batch(pulses, df, dp, mode=1, **kw)
    runs = (("device", device), ("host", host), ("gn", gn), ("lsq", lsq), ("fwd", fwd))
    out = {name: f() for name, f in runs}
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t0 = time.perf_counter()
            f()
            t[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(pulses=len(pulses), samples=len(pulses[0][0]), points=len(df) * len(dp), scales=len(SC), cg=CG)
    for name, _ in runs:
        row["ms_" + name] = min(t[name])
        row["ms_" + name + "_median"] = float(np.median(t[name]))
    row["speedup"] = row["ms_host"] / row["ms_device"]
    row["host_spread"] = row["ms_host_median"] / row["ms_host"]      # the device call is to be faster by more than this
    row["step_device_vs_host"] = max(float(np.abs(u - v).max() / np.abs(v).max()) for u, v in zip(out["device"], out["host"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", choices=("both", "long", "short"), default="both", help="one shape alone: for a kernel trace")
    a = ap.parse_args()
    import mbfir
    ctx = mbfir.get_context()
    shapes = dict(long=long_pulse, short=short)
    rows = {k: measure(mbfir, ctx, f, a.reps) for k, f in shapes.items() if a.shape in ("both", k)}
    print(json.dumps(dict(tool="gpu_blochsslm", reps=a.reps, **rows)))


if __name__ == "__main__":
    main()
