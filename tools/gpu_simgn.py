"""Cost of the fused least-squares products (mbfir.abr2_gn_batch, mbfir.abr2_lsq_batch) against the shipped two-call paths they
replace, for the pulse of examples/spiral2d_gauss_newton.py: dz2d(8, 1, 4, 512, 1, 2) at 90 degrees on 128 x 128 points at 3
transmit-gain scales (192 forward workgroups), profile 'ex'.  Timed:
    gn_fused   one abr2_gn_batch product, one direction
    gn_pair    abr2_jvp_batch, the chain rule dM = 2 (conj(da) b + conj(a) db) and the seed in NumPy, abr2_vjp_batch
    lsq_fused  one abr2_lsq_batch call
    lsq_pair   abr2_batch, the residual and the seed in NumPy, abr2_vjp_batch
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the four alternate, minimum and
median of --reps each.  One JSON line.

    python tools/gpu_simgn.py [--reps 20]
    python tools/gpu_simgn.py --rocprof DIR [--reps 20]

The second form runs the first as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters in that run) and adds the
mean kernel times of the sweeps and folds from the trace to the JSON line.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_abr2_batch", "k_abr2_jvp_batch", "k_abr2_vjp_batch", "k_abr_vjp_fold", "k_abr2_gn_batch", "k_abr2_lsq_batch",
           "k_abr_gn_fold")


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    rf = rf * np.pi / 2
    x, sc = np.linspace(-8, 8, 128), (0.9, 1.0, 1.1)
    r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
    disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)
    target = np.stack([np.where(disc, np.sin(s * np.pi / 2) + 0j, 0.0) for s in sc])
    w = np.broadcast_to((disc | ring).astype(np.float64), target.shape)
    rng = np.random.default_rng(0)
    v = rng.standard_normal(len(rf)) + 1j * rng.standard_normal(len(rf))
    kw = dict(scales=sc, ctx=ctx)

    def gn_fused():
        return mbfir.abr2_gn_batch([(rf, g)], x, x, [v], [w], **kw)[0]

    def gn_pair():
        ((a, b), (da, db)), = mbfir.abr2_jvp_batch([(rf, g)], x, x, [v], **kw)
        c = w * 2 * (np.conj(da) * b + np.conj(a) * db)
        return mbfir.abr2_vjp_batch([(rf, g)], x, x, [(2 * b * np.conj(c), 2 * a * c)], **kw)[0]

    def lsq_fused():
        return mbfir.abr2_lsq_batch([(rf, g)], x, x, [target], [w], **kw)[0]

    def lsq_pair():
        (a, b), = mbfir.abr2_batch([(rf, g)], x, x, **kw)
        res = 2 * np.conj(a) * b - target
        c = w * res
        grad, = mbfir.abr2_vjp_batch([(rf, g)], x, x, [(2 * b * np.conj(c), 2 * a * c)], **kw)
        return 0.5 * float(np.sum(w * np.abs(res) ** 2)), grad
    runs = (("gn_fused", gn_fused), ("gn_pair", gn_pair), ("lsq_fused", lsq_fused), ("lsq_pair", lsq_pair))
    out = {name: f() for name, f in runs}
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t0 = time.perf_counter()
            f()
            t[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_simgn", samples=len(rf), nx=128, ny=128, scales=len(sc), forward_workgroups=3 * 64, reps=reps)
    for name, _ in runs:
        row["ms_" + name] = min(t[name])
        row["ms_" + name + "_median"] = float(np.median(t[name]))
    row["speedup_gn"] = row["ms_gn_pair"] / row["ms_gn_fused"]
    row["speedup_lsq"] = row["ms_lsq_pair"] / row["ms_lsq_fused"]
    # the two paths compute the same thing: largest difference relative to the largest entry
    row["gn_fused_vs_pair"] = float(np.abs(out["gn_fused"] - out["gn_pair"]).max() / np.abs(out["gn_pair"]).max())
    row["lsq_grad_fused_vs_pair"] = float(np.abs(out["lsq_fused"][1] - out["lsq_pair"][1]).max() / np.abs(out["lsq_pair"][1]).max())
    row["lsq_loss_fused_vs_pair"] = abs(out["lsq_fused"][0] - out["lsq_pair"][0]) / out["lsq_pair"][0]
    return row


def kernel_means(d):
    """mean microseconds per launch of every simulator kernel of the run, from the trace's SQLite database (rocprofv3's default
    output).  k_abr2_vjp_batch and k_abr_vjp_fold run in both pairs; their means are over both."""
    import sqlite3
    hits = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    if not hits:
        return None
    agg = {}
    for name, start, end in sqlite3.connect(hits[0]).cursor().execute("select name, start, end from kernels order by start"):
        key = next((k for k in sorted(KERNELS, key=len, reverse=True) if k in name), None)
        if key is None:
            continue
        c, t = agg.get(key, (0, 0.0))
        agg[key] = (c + 1, t + (end - start) / 1e3)
    return {k: dict(launches=c, mean_us=t / c) for k, (c, t) in agg.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps)))
        return
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "simgn", "--", sys.executable,
           os.path.abspath(__file__), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = km = kernel_means(a.rocprof)
    if km and all(k in km for k in ("k_abr2_jvp_batch", "k_abr2_vjp_batch", "k_abr2_gn_batch", "k_abr2_lsq_batch", "k_abr2_batch")):
        row["kernel_ratio_gn"] = km["k_abr2_gn_batch"]["mean_us"] / (km["k_abr2_jvp_batch"]["mean_us"] + km["k_abr2_vjp_batch"]["mean_us"])
        row["kernel_ratio_lsq"] = km["k_abr2_lsq_batch"]["mean_us"] / (km["k_abr2_batch"]["mean_us"] + km["k_abr2_vjp_batch"]["mean_us"])
    print(json.dumps(row))


if __name__ == "__main__":
    main()
