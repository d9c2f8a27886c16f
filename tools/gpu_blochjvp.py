"""Cost of the Bloch simulator's tangent (mbfir.bloch_jvp_batch) against the forward call it differentiates (mbfir.bloch_batch, mode 0)
on the same inputs, tools/gpu_blochgrad.py's case: a 600-sample, 26 ms H-1 pulse at T1 = 1 s, T2 = 40 ms on 2048 frequencies x 8
positions at 3 transmit-gain scales (192 forward workgroups), at K = 1, BJVP_K and 2 BJVP_K directions in b1 and m0.  Times are warm
host clocks around calls that end in a stream synchronise (transfers included); the calls alternate, the minimum and the median of
--reps each.  Central differences of the same K directions would cost 2 K forward calls.  One JSON line.

    python tools/gpu_blochjvp.py [--reps 20] [--dirs K ...]
    python tools/gpu_blochjvp.py --rocprof DIR [--reps 20]

The second form runs the first once per K as a child under `rocprofv3 --kernel-trace --stats -d DIR/K<K>` (no counters in those
runs) and adds the mean kernel times of k_bloch_batch and k_bloch_jvp_batch from each trace to the JSON line.
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
KERNELS = ("k_bloch_batch", "k_bloch_jvp_batch")


def measure(reps, dirs):
    import mbfir
    ctx = mbfir.get_context()
    G = mbfir.bloch_jvp_group()
    dirs = dirs or [1, G, 2 * G]
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    kmax = max(dirs)
    v = (rng.standard_normal((kmax, n)) + 1j * rng.standard_normal((kmax, n))) * np.abs(b1).max()
    dm0 = tuple(rng.standard_normal((3, kmax, nf, npos)))

    def fwd():
        return mbfir.bloch_batch(pulses, df, dp, scales=sc, ctx=ctx)

    def jvp(k):
        return lambda: mbfir.bloch_jvp_batch(pulses, df, dp, [v[:k]], scales=sc, tangents_m0=[tuple(d[:k] for d in dm0)], ctx=ctx)
    calls = [("forward", fwd)] + [("jvp_%d" % k, jvp(k)) for k in dirs]
    for _, fn in calls:
        fn()
    acc = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            acc[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochjvp", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps,
               group=G, dirs=dirs)
    for name, t in acc.items():
        row["ms_" + name] = min(t)
        row["ms_%s_median" % name] = float(np.median(t))
    for k in dirs:
        row["ratio_%d" % k] = row["ms_jvp_%d" % k] / row["ms_forward"]
    return row


def kernel_means(d):
    """mean microseconds per launch of KERNELS from the trace's SQLite database (rocprofv3's default output)"""
    import sqlite3
    hits = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    if not hits:
        return None
    agg = {}
    for name, start, end in sqlite3.connect(hits[0]).cursor().execute("select name, start, end from kernels"):
        for k in KERNELS:
            if k + "(" in name or k + "<" in name or name.endswith(k):
                c, t = agg.get(k, (0, 0.0))
                agg[k] = (c + 1, t + (end - start) / 1e3)
    return {k: dict(launches=c, mean_us=t / c) for k, (c, t) in agg.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dirs", type=int, nargs="+", help="the direction counts to time (default: 1, BJVP_K, 2 BJVP_K)")
    ap.add_argument("--rocprof", metavar="DIR", help="run once per K under rocprofv3 --kernel-trace --stats, output in DIR/K<K>")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps, a.dirs)))
        return
    # the traced programs are fresh children: this process never opens the GPU (the group size is a host-only call)
    import mbfir
    G = mbfir.bloch_jvp_group()
    out = dict(tool="gpu_blochjvp", traced=True, group=G, kernels={})      # host clocks under the tracer are not end-to-end figures
    for k in a.dirs or [1, G, 2 * G]:
        d = os.path.join(a.rocprof, "K%d" % k)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "blochjvp", "--", sys.executable, os.path.abspath(__file__),
               "--reps", str(a.reps), "--dirs", str(k)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
        km = kernel_means(d)
        out["kernels"][str(k)] = km
        if km and all(n in km for n in KERNELS):
            out["kernel_ratio_%d" % k] = km["k_bloch_jvp_batch"]["mean_us"] / km["k_bloch_batch"]["mean_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
