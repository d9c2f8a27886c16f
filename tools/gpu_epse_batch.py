"""Spectral-spatial designer timing: one JSON line.
  b2rf_batch   1024 polynomials at n = 64 and 256 in one launch (mbfir.b2rf_batch), against a loop of mbfir.b2rf over the same rows
  abrm_2d      the 2D Cayley-Klein simulation of a 1024-sample pulse at 256 x 256 positions (mbfir.abrm with y), against the
               vectorised NumPy restatement of abrm.m:39-57 (timed on --np-rows of the 256 x rows and scaled)
  dzepse       one dzepse design alone, and dzepse_batch of 64 designs (spatial time-bandwidths varied) against 64 single calls
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the minimum of --reps.

    python tools/gpu_epse_batch.py [--reps 3] [--np-rows 16]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mbfir  # noqa: E402


def best(fn, reps):
    fn()                                                   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), out


def abrm2_np(rf, g, x, y):
    X, Y = np.meshgrid(x, y, indexing="ij")
    a = np.ones(X.shape, dtype=np.complex128)
    b = np.zeros(X.shape, dtype=np.complex128)
    for m in range(len(rf)):
        om = X * g[m].real + Y * g[m].imag
        phi = np.sqrt(abs(rf[m]) ** 2 + om ** 2)
        safe = np.where(phi > 0, phi, 1.0)
        av = np.cos(phi / 2) - 1j * (om / safe) * np.sin(phi / 2)
        bv = -1j * ((rf[m].real + 1j * rf[m].imag) / safe) * np.sin(phi / 2)
        a, b = av * a - np.conj(bv) * b, bv * a + np.conj(av) * b
    return a, b


def lobe(n):
    return np.sin(np.pi * (np.arange(n) + 0.5) / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np-rows", type=int, default=16, help="x rows of the 256 x 256 grid the NumPy restatement is timed on")
    a = ap.parse_args()
    ctx = mbfir.get_context()
    out = {"tool": "gpu_epse_batch", "cases": []}

    def emit(row):
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    rng = np.random.default_rng(1)
    for n in (64, 256):
        B = (rng.standard_normal((1024, n)) + 1j * rng.standard_normal((1024, n))) * 0.7 / math.sqrt(n)
        ms_b, rb = best(lambda: mbfir.b2rf_batch(B, ctx=ctx), a.reps)
        ms_l, rl = best(lambda: np.stack([mbfir.b2rf(r, ctx=ctx) for r in B]), 1)
        emit(dict(case="b2rf_batch", n=n, count=1024, ms_batch=ms_b, ms_loop=ms_l, speedup=ms_l / ms_b,
                  max_rel_diff=float(np.abs(rb - rl).max() / np.abs(rl).max())))

    npulse = 1024
    rf = (rng.standard_normal(npulse) + 1j * rng.standard_normal(npulse)) * 0.01
    g = np.tile(np.concatenate([lobe(64), -lobe(64)]), npulse // 128) * 2 * np.pi / 64 + 1j * 2 * np.pi * 4e-6
    x, y = np.linspace(-8, 8, 256), np.linspace(-2000, 2000, 256)
    ms_d, (ad, bd) = best(lambda: mbfir.abrm(rf, g, x, y, ctx=ctx), a.reps)
    t0 = time.perf_counter()
    an, bn = abrm2_np(rf, g, x[:a.np_rows], y)
    ms_n = (time.perf_counter() - t0) * 1e3 * 256 / a.np_rows
    emit(dict(case="abrm_2d", samples=npulse, nx=256, ny=256, ms_device=ms_d, ms_numpy=ms_n, numpy_rows_measured=a.np_rows,
              speedup=ms_n / ms_d, max_abs_diff=float(max(np.abs(ad[:a.np_rows] - an).max(), np.abs(bd[:a.np_rows] - bn).max()))))

    gx = lobe(64)
    spec = (math.pi, gx, 6.0, 0.5, 16, 0.3, 0.01, 0.01, "pm")
    ms_1, _ = best(lambda: mbfir.dzepse(*spec, ctx=ctx), a.reps)
    specs = [(math.pi, gx, 4.0 + 0.05 * k, 0.5, 16, 0.3, 0.01, 0.01, "pm") for k in range(64)]
    ms_b, rb = best(lambda: mbfir.dzepse_batch(specs, ctx=ctx), a.reps)
    ms_s, rs = best(lambda: [mbfir.dzepse(*s, ctx=ctx) for s in specs], 1)
    emit(dict(case="dzepse", lgx=64, ngx=16, ms_single=ms_1, designs=64, ms_batch=ms_b, ms_single_calls=ms_s, speedup=ms_s / ms_b,
              bit_identical=all(np.array_equal(p, q) for p, q in zip(rb, rs))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
