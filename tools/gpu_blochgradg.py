"""Cost of the Bloch simulator's adjoint in b1, gr and df (mbfir.bloch_vjp_gr_batch) against its adjoint in b1 alone
(mbfir.bloch_vjp_batch) on the case of tools/gpu_blochgrad.py: a 600-sample, 26 ms H-1 pulse at T1 = 1 s, T2 = 40 ms on 2048
frequencies x 8 positions at 3 transmit-gain scales (192 workgroups).  Times are warm host clocks around calls that end in a stream
synchronise (transfers included); the calls alternate, the minimum and the median of --reps each.  One JSON line.

    python tools/gpu_blochgradg.py [--reps 20]
    python tools/gpu_blochgradg.py --rocprof DIR [--reps 20]

The second form runs the first as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters and nothing else traced in
that run) and adds the mean kernel times of both calls' sweep and fold kernels from the trace to the JSON line.
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
KERNELS = ("k_bloch_vjp_batch", "k_bloch_vjp_fold", "k_bloch_vjp_gr_batch<false>", "k_bloch_vjp_gr_batch<true>", "k_bloch_vjp_gr_fold")


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    cot = [tuple(rng.standard_normal((3, len(sc), nf, npos)))]

    def adj():
        return mbfir.bloch_vjp_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def adjg():
        return mbfir.bloch_vjp_gr_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def adjgd():
        return mbfir.bloch_vjp_gr_batch(pulses, df, dp, cot, scales=sc, grad_df=True, ctx=ctx)
    adj()
    adjg()
    adjgd()
    ta, tg, td = [], [], []
    for _ in range(reps):
        for fn, acc in ((adj, ta), (adjg, tg), (adjgd, td)):
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    return dict(tool="gpu_blochgradg", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps,
                ms_vjp=min(ta), ms_vjp_gr=min(tg), ms_vjp_gr_df=min(td), ratio=min(tg) / min(ta), ratio_df=min(td) / min(ta),
                ms_vjp_median=float(np.median(ta)), ms_vjp_gr_median=float(np.median(tg)), ms_vjp_gr_df_median=float(np.median(td)))


def kernel_means(d):
    """mean microseconds per launch of KERNELS from the trace's SQLite database (rocprofv3's default output)"""
    import sqlite3
    hits = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    if not hits:
        return None
    agg, seen = {}, set()
    for name, start, end in sqlite3.connect(hits[0]).cursor().execute("select name, start, end from kernels"):
        seen.add(name[:120])
        for k in KERNELS:
            if k + "(" in name or name.endswith(k):
                c, t = agg.get(k, (0, 0.0))
                agg[k] = (c + 1, t + (end - start) / 1e3)
    out = {k: dict(launches=c, mean_us=t / c) for k, (c, t) in agg.items()}
    if not all(k in agg for k in KERNELS):                  # say what the trace did hold
        out["names"] = sorted(seen)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps)))
        return
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochgradg", "--", sys.executable,
           os.path.abspath(__file__), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = km = kernel_means(a.rocprof)
    if km and all(k in km for k in KERNELS):
        old = km["k_bloch_vjp_batch"]["mean_us"] + km["k_bloch_vjp_fold"]["mean_us"]
        row["kernel_ratio"] = (km["k_bloch_vjp_gr_batch<false>"]["mean_us"] + km["k_bloch_vjp_gr_fold"]["mean_us"]) / old
        row["kernel_ratio_df"] = (km["k_bloch_vjp_gr_batch<true>"]["mean_us"] + km["k_bloch_vjp_gr_fold"]["mean_us"]) / old
    print(json.dumps(row))


if __name__ == "__main__":
    main()
