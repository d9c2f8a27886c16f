"""Cost of the Bloch simulator's adjoint (mbfir.bloch_vjp_batch) against the forward call it differentiates (mbfir.bloch_batch, mode
0) on the same inputs: a 600-sample, 26 ms H-1 pulse at T1 = 1 s, T2 = 40 ms on 2048 frequencies x 8 positions at 3 transmit-gain
scales (192 workgroups).  Times are warm host clocks around calls that end in a stream synchronise (transfers included); the two
calls alternate, the minimum and the median of --reps each.  One JSON line.

    python tools/gpu_blochgrad.py [--reps 20]
    python tools/gpu_blochgrad.py --rocprof DIR [--reps 20]

The second form runs the first as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters in that run) and adds the
mean kernel times of k_bloch_batch, k_bloch_vjp_batch and k_bloch_vjp_fold from the trace to the JSON line.
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
KERNELS = ("k_bloch_batch", "k_bloch_vjp_batch", "k_bloch_vjp_fold")


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    cot = [tuple(rng.standard_normal((3, len(sc), nf, npos)))]

    def fwd():
        return mbfir.bloch_batch(pulses, df, dp, scales=sc, ctx=ctx)

    def adj():
        return mbfir.bloch_vjp_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def adjm():
        return mbfir.bloch_vjp_batch(pulses, df, dp, cot, scales=sc, grad_m0=True, ctx=ctx)
    fwd()
    adj()
    adjm()
    tf, ta, tm = [], [], []
    for _ in range(reps):
        for fn, acc in ((fwd, tf), (adj, ta), (adjm, tm)):
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    return dict(tool="gpu_blochgrad", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps,
                ms_forward=min(tf), ms_vjp=min(ta), ms_vjp_m0=min(tm), ratio=min(ta) / min(tf), ratio_m0=min(tm) / min(tf),
                ms_forward_median=float(np.median(tf)), ms_vjp_median=float(np.median(ta)), ms_vjp_m0_median=float(np.median(tm)))


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
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps)))
        return
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochgrad", "--", sys.executable,
           os.path.abspath(__file__), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = kernel_means(a.rocprof)
    if row["kernels"] and all(k in row["kernels"] for k in KERNELS):
        km = row["kernels"]
        row["kernel_ratio"] = (km["k_bloch_vjp_batch"]["mean_us"] + km["k_bloch_vjp_fold"]["mean_us"]) / km["k_bloch_batch"]["mean_us"]
    print(json.dumps(row))


if __name__ == "__main__":
    main()
