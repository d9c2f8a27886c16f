"""Cost of the fused least-squares products of the Bloch simulator's steady state (mbfir.bloch_ss_lsq_batch, mbfir.bloch_ss_gn_batch)
against the two-call paths of the same build that they replace, on the timing case of tools/gpu_blochss.py: a 600-sample, 26 ms H-1
period at T1 = 1 s, T2 = 40 ms on 2048 frequencies x 8 positions at 3 transmit-gain scales (192 workgroups).  Timed:
    lsq:        bloch_ss_lsq_batch                                  against  bloch_batch(mode=1), the NumPy residual, bloch_ss_vjp_batch
    gn (K = 1): bloch_ss_gn_batch                                   against  bloch_ss_jvp_batch, the NumPy weights, bloch_ss_vjp_batch
Times are warm host clocks around calls that end in a stream synchronise (transfers and the NumPy between the two calls included);
the calls alternate, the minimum and the median of --reps each.  One JSON line.

    python tools/gpu_blochssgn.py [--reps 20]
    python tools/gpu_blochssgn.py --rocprof DIR [--reps 20]

The second form runs the four device paths (each kernel then occurs in one configuration) as a child under `rocprofv3 --kernel-trace
--stats -d DIR` (no counters in that run) and adds the mean kernel times from the trace to the JSON line.
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
KERNELS = ("k_bloch_batch", "k_bloch_vjp_fold", "k_bloch_gn_fold", "k_bloch_ss_vjp_batch", "k_bloch_ss_jvp_batch", "k_bloch_ss_lsq_batch",
           "k_bloch_ss_gn_batch")


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    w = rng.uniform(0, 1, (3, len(sc), nf, npos))
    w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
    w, t = [tuple(w)], [tuple(rng.uniform(-1, 1, (3, len(sc), nf, npos)))]
    v = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(b1).max()]

    def lsq():
        return mbfir.bloch_ss_lsq_batch(pulses, df, dp, t, w, scales=sc, ctx=ctx)[0]

    def lsq2():
        m, = mbfir.bloch_batch(pulses, df, dp, scales=sc, mode=1, ctx=ctx)
        r = [m[c] - t[0][c] for c in range(3)]
        L = 0.5 * float(sum((w[0][c] * r[c] * r[c]).sum() for c in range(3)))
        return L, mbfir.bloch_ss_vjp_batch(pulses, df, dp, [tuple(w[0][c] * r[c] for c in range(3))], scales=sc, ctx=ctx)[0]

    def gn():
        return mbfir.bloch_ss_gn_batch(pulses, df, dp, v, w, scales=sc, ctx=ctx)[0]

    def gn2():
        (_, dm), = mbfir.bloch_ss_jvp_batch(pulses, df, dp, v, scales=sc, ctx=ctx)
        return mbfir.bloch_ss_vjp_batch(pulses, df, dp, [tuple(w[0][c] * dm[c] for c in range(3))], scales=sc, ctx=ctx)[0]
    calls = dict(lsq=lsq, lsq_two_calls=lsq2, gn=gn, gn_two_calls=gn2)
    for fn in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochssgn", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps)
    for k, ts in acc.items():
        row["ms_" + k] = min(ts)
        row["ms_" + k + "_median"] = float(np.median(ts))
    (La, ga), (Lb, gb), ha, hb = lsq(), lsq2(), gn(), gn2()
    row["lsq_two_calls_over_fused"] = row["ms_lsq_two_calls"] / row["ms_lsq"]
    row["gn_two_calls_over_fused"] = row["ms_gn_two_calls"] / row["ms_gn"]
    row["lsq_vs_two_calls_rel"] = max(abs(La - Lb) / abs(Lb), float(np.abs(ga - gb).max() / np.abs(gb).max()))
    row["gn_vs_two_calls_rel"] = float(np.abs(ha - hb).max() / np.abs(hb).max())
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
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps)))
        return
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochssgn", "--", sys.executable, os.path.abspath(__file__),
           "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = kernel_means(a.rocprof)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
