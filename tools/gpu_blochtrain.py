"""Cost of the pulse train (mbfir.bloch_train_batch) against the shipped way to get the same numbers: bloch_batch(mode=2) on the
waveform tiled ntr times on the host, picking the echo samples.  Two workloads:
    batch64: 64 periods of 64 samples (63 of 10 us and a dead time) x 64 repetitions on 85 frequencies x 1 position, alternating
             phase with an alpha/2 first repetition, C-13 (T1 30 s, T2 2 s), meq = 1 (the only one mode 2 knows);
    long:    one period of 600 samples (2 ms of pulse in a period of 6 ms) x 256 repetitions on 2048 x 8 = 16384 points.
The tiled call of `long` records 600 x 256 states of 16384 points, 60 GB in three planes, twice over on the host (the call's staging
and its result); it is therefore run over the points in chunks of --tiled-chunk (a caller with finite memory has to do the same) and
the chunks' times are added up.  Times are warm host clocks around calls that end in a stream synchronise (transfers included); the
calls alternate, the minimum and the median of --reps each (--tiled-reps for the tiled call, which is slow).  One JSON line per
workload.

    python tools/gpu_blochtrain.py [--workload batch64|long] [--reps 10] [--tiled-reps 3] [--tiled-chunk 2048]
    python tools/gpu_blochtrain.py --rocprof DIR --workload batch64 [--reps 10]

The second form runs the same calls (for `long`, one chunk of the tiled call) as a child under `rocprofv3 --kernel-trace --stats -d DIR`
(no counters in that run) and adds the mean kernel times from the trace to the JSON line.
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
KERNELS = ("k_bloch_train_prop", "k_bloch_train_run", "k_bloch_batch")


def workload(name):
    import mbfir
    rng = np.random.default_rng(0)
    gamma = mbfir.GAMMA_C13
    if name == "batch64":
        P, n, ntr, nf, npos = 64, 64, 64, 85, 1
        tp = np.append(np.full(n - 1, 1e-5), 6e-3 - (n - 1) * 1e-5)
    else:
        P, n, ntr, nf, npos = 1, 600, 256, 2048, 8
        tp = np.append(np.full(n - 1, 2e-3 / (n - 1)), 4e-3)
    pulses = []
    for q in range(P):
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * ((0.3 + 0.01 * q) / (gamma * tp[:-1].sum()))
        b1[-1] = 0.0
        gr = np.append(rng.uniform(0.5, 1.5, n - 1) * 0.05, 0.0)
        pulses.append((b1, gr, tp, 30.0, 2.0, "C-13"))
    df, dp = np.linspace(-100, 100, nf), np.linspace(-2, 2, npos) if npos > 1 else np.zeros(1)
    phases, gains = np.pi * np.arange(ntr), np.append(0.5, np.ones(ntr - 1))
    return dict(name=name, pulses=pulses, df=df, dp=dp, ntr=ntr, n=n, phases=phases, gains=gains, echo=n // 2)


def measure(W, reps, tiled_reps, chunk, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    pulses, df, dp, ntr, n, echo = W["pulses"], W["df"], W["dp"], W["ntr"], W["n"], W["echo"]
    tiles = [(np.concatenate([g * np.exp(1j * p) * b1 for p, g in zip(W["phases"], W["gains"])]), np.tile(gr, ntr), np.tile(tp, ntr),
              t1, t2, nuc) for b1, gr, tp, t1, t2, nuc in pulses]
    nf, npos = len(df), len(dp)
    fchunk = max(1, min(nf, chunk // npos))
    fsl = [slice(a, min(a + fchunk, nf)) for a in range(0, nf, fchunk)]
    if kernels_only:
        fsl = fsl[:1]

    def train():
        return mbfir.bloch_train_batch(pulses, df, dp, ntr, phases=W["phases"], gains=W["gains"], echo=echo, ctx=ctx)

    def tiled():
        out = []
        for sl in fsl:                                                   # the echo samples of every repetition: (S, nf, npos, ntr)
            res = mbfir.bloch_batch(tiles, df[sl], dp, mode=2, ctx=ctx)
            out.append([tuple(np.ascontiguousarray(v[..., echo - 1::n]) for v in tri) for tri in res])      # the recording is freed
        return out
    calls = dict(train=(train, reps), tiled=(tiled, tiled_reps))
    for fn, _ in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for r in range(max(reps, tiled_reps)):
        for k, (fn, cnt) in calls.items():
            if r < cnt:
                t0 = time.perf_counter()
                fn()
                acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrain", workload=W["name"], periods=len(pulses), samples=n, repetitions=ntr, nf=nf, npos=npos,
               reps=reps, tiled_reps=tiled_reps, tiled_point_chunks=len(fsl), tiled_samples=n * ntr,
               tiled_recorded_gb=3 * 8 * len(pulses) * nf * npos * n * ntr / 1e9,
               train_recorded_gb=3 * 8 * len(pulses) * nf * npos * ntr / 1e9)
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not kernels_only:
        a, b = train(), tiled()
        err = 0.0
        for q in range(len(pulses)):
            for c in range(3):
                w = np.concatenate([blk[q][c] for blk in b], 1)          # along the frequencies
                err = max(err, float(np.abs(a[q][c] - np.moveaxis(w, -1, 1)).max()))
        row["tiled_over_train"] = row["ms_tiled"] / row["ms_train"]
        row["train_vs_tiled_abs"] = err
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
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tiled-reps", type=int, default=3)
    ap.add_argument("--tiled-chunk", type=int, default=2048, help="points per tiled call")
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    ap.add_argument("--kernels-only", action="store_true", help="only what the traced run reports")
    a = ap.parse_args()
    names = a.workload or ["batch64", "long"]
    if not a.rocprof:
        for name in names:
            print(json.dumps(measure(workload(name), a.reps, min(a.reps, a.tiled_reps), a.tiled_chunk, a.kernels_only)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochtrain", "--", sys.executable,
           os.path.abspath(__file__), "--workload", names[0], "--reps", str(a.reps), "--tiled-reps", str(a.tiled_reps),
           "--tiled-chunk", str(a.tiled_chunk), "--kernels-only"]
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
