"""Batched Parks-McClellan timing (mbfir.remez_batch): one JSON line.
Two design sizes -- the 519-tap dzmp design of specsat_H1_dualband_conventional.m (n = 260) and a 2047-tap dzlp design -- each
solved as 1 design and as a batch of 256 (weights varied by a few per cent so the designs differ), timed warm as a host clock
around the call (it ends in a stream synchronise, and includes the transfers): ms per call, designs per second, iterations.
When SciPy is importable, scipy.signal.remez on one core solves the same designs one after another (the single design, and
--scipy-batch of the 256 extrapolated from that many).

    python tools/gpu_remez_batch.py [--reps 3] [--scipy-batch 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mbfir  # noqa: E402
from mbfir import slrclassic  # noqa: E402


def h1_spec():
    f1, f2, f3 = (np.array(v) * 3.0015 * 42.577e-3 for v in ([1.8, 2.5], [3.0, 4.1], [4.8, 5.4]))
    fr = f3.mean()
    f1, f2 = f1 - fr, f2 - fr
    bw1 = ((f1[1] + f2[0]) / 2 - f1.mean()) * 2
    return slrclassic.dzmp_spec(260, 26 * bw1, 0.0008, 0.03)


def batch(spec, k):
    n, e, d, w = spec
    rng = np.random.default_rng(1)
    return [(n, e, d, [w[0], w[1] * (1 + 0.05 * rng.random())]) for _ in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy-batch", type=int, default=8, help="SciPy designs timed for the 256-design estimate")
    a = ap.parse_args()
    try:
        import scipy.signal as ss
    except ImportError:
        ss = None
    ctx = mbfir.get_context()
    out = {"tool": "gpu_remez_batch", "cases": []}
    for name, spec in (("dzmp_h1_519", h1_spec()), ("dzlp_2047", slrclassic.dzlp_spec(2047, 12, 0.01, 0.001))):
        for k in (1, 256):
            jobs = batch(spec, k)
            res = mbfir.remez_batch(jobs, ctx=ctx)                       # warm-up
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = mbfir.remez_batch(jobs, ctx=ctx)
                ts.append((time.perf_counter() - t0) * 1e3)
            its = [r[1]["iterations"] for r in res]
            row = dict(case=name, numtaps=spec[0], designs=k, ms=min(ts), designs_per_s=k / (min(ts) * 1e-3),
                       iters_min=min(its), iters_max=max(its), converged=sum(r[1]["status"] == "converged" for r in res))
            if ss is not None:
                m = 1 if k == 1 else min(k, a.scipy_batch)
                t0 = time.perf_counter()
                for n, e, d, w in jobs[:m]:
                    ss.remez(n, np.asarray(e) / 2, d[::2], weight=w, maxiter=25)
                row["scipy_ms"] = (time.perf_counter() - t0) * 1e3 * k / m
                row["scipy_measured_designs"] = m
            out["cases"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
