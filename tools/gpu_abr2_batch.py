"""Batched 2D Cayley-Klein simulation (mbfir.abr2_batch) against the loop of single 2D mbfir.abrm(rf * s, g, x, y) calls: one JSON line.
  epse6     the six dzepse pulses of tests/golden/epse.npz (832 .. 3072 samples) x 5 transmit-gain scales on 128 x 128 points
            (x in cycles of the spatial profile, y in Hz): one abr2_batch call against 30 abrm calls
  epse64    64 pulses from one dzepse_batch call (the designs of tools/gpu_epse_batch.py, 1024 samples each) x 3 scales on 64 x 64
            points: one abr2_batch call against 192 abrm calls
Times are warm host clocks around calls that end in a stream synchronise (transfers included); batch and loop alternate, the
minimum of --reps each.

    python tools/gpu_abr2_batch.py [--reps 5]
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


def alternate(batch, loop, reps):
    """(min ms of batch, min ms of loop, their last results): one warm-up each, then batch and loop in turn"""
    batch()
    loop()
    tb, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        rb = batch()
        tb.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rl = loop()
        tl.append((time.perf_counter() - t0) * 1e3)
    return min(tb), min(tl), rb, rl


def lobe_gradient(gx, ngx, tgx):
    """Re g: the lobes with alternating sign, 2 pi per lobe; Im g = 2 pi dt per sample (y in Hz); tgx in ms"""
    lobe = gx * 2 * np.pi / gx.sum()
    return np.concatenate([lobe * (-1) ** k for k in range(ngx)]) + 1j * 2 * np.pi * (tgx / len(gx) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = mbfir.get_context()
    out = {"tool": "gpu_abr2_batch", "cases": []}

    def run(case, pulses, x, y, scales):
        ms_b, ms_l, rb, rl = alternate(lambda: mbfir.abr2_batch(pulses, x, y, scales=scales, ctx=ctx),
                                       lambda: [mbfir.abrm(rf * s, g, x, y, ctx=ctx) for rf, g in pulses for s in scales], a.reps)
        flat = [ab[c][k] for ab in rb for k in range(len(scales)) for c in range(2)]
        loop = [v for r in rl for v in r]
        row = dict(case=case, pulses=len(pulses), ntime_total=int(sum(len(p[0]) for p in pulses)), scales=len(scales), nx=len(x),
                   ny=len(y), workgroups=len(pulses) * len(scales) * -(-len(x) * len(y) // 256), ms_batch=ms_b, ms_loop=ms_l,
                   speedup=ms_l / ms_b, max_abs_diff=max(float(np.abs(p - q).max()) for p, q in zip(flat, loop)),
                   bit_identical=all(np.array_equal(p, q) for p, q in zip(flat, loop)))
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    with open(os.path.join(ROOT, "tests", "golden", "epse.json")) as fh:
        meta = json.load(fh)["dzepse"]
    with np.load(os.path.join(ROOT, "tests", "golden", "epse.npz")) as z:
        six = [(z["dzepse/%s/rf" % n].ravel(), lobe_gradient(z["dzepse/%s/gx" % n], v["ngx"], v["tgx"])) for n, v in meta.items()]
    run("epse6", six, np.linspace(-4, 4, 128), np.linspace(-1000, 1000, 128), [0.8, 0.9, 1.0, 1.1, 1.2])

    gx = np.sin(np.pi * (np.arange(64) + 0.5) / 64)
    specs = [(math.pi, gx, 4.0 + 0.05 * k, 0.5, 16, 0.3, 0.01, 0.01, "pm") for k in range(64)]
    g = lobe_gradient(gx, 16, 0.5)
    run("epse64", [(rf.ravel(), g) for rf in mbfir.dzepse_batch(specs, ctx=ctx)], np.linspace(-4, 4, 64), np.linspace(-1000, 1000, 64),
        [0.9, 1.0, 1.1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
