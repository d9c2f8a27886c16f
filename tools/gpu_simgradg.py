"""Cost of the simulators' adjoint with respect to rf and the gradient waveform (mbfir.abr2_vjp_rfg_batch) against the rf adjoint
(mbfir.abr2_vjp_batch), for the pulse, grid and scales of tools/gpu_simgrad.py: dz2d(8, 1, 4, 512, 1, 2) at 90 degrees on 128 x 128
points at 3 transmit-gain scales (192 workgroups).  Times are warm host clocks around calls that end in a stream synchronise
(transfers included); the two calls alternate, the minimum of --reps each.  One JSON line.

    python tools/gpu_simgradg.py [--reps 20]
    python tools/gpu_simgradg.py --rocprof DIR [--reps 20]

The second form runs the first as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters in that run) and adds the
mean kernel times of k_abr2_vjp_batch, k_abr_vjp_fold, k_abr2_vjp_rfg_batch and k_abr_vjp_rfg_fold from the trace to the JSON line.
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
KERNELS = ("k_abr2_vjp_batch", "k_abr_vjp_fold", "k_abr2_vjp_rfg_batch", "k_abr_vjp_rfg_fold")


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    pulses, x, sc = [(rf * np.pi / 2, g)], np.linspace(-8, 8, 128), (0.9, 1.0, 1.1)
    rng = np.random.default_rng(0)
    cot = [tuple(rng.standard_normal((3, 128, 128)) + 1j * rng.standard_normal((3, 128, 128)) for _ in range(2))]

    def adj():
        return mbfir.abr2_vjp_batch(pulses, x, x, cot, scales=sc, ctx=ctx)

    def adjg():
        return mbfir.abr2_vjp_rfg_batch(pulses, x, x, cot, scales=sc, ctx=ctx)
    adj()
    adjg()
    ta, tg = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        adj()
        ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        adjg()
        tg.append((time.perf_counter() - t0) * 1e3)
    return dict(tool="gpu_simgradg", samples=len(rf), nx=128, ny=128, scales=len(sc), workgroups=3 * 64, reps=reps,
                ms_vjp=min(ta), ms_vjp_rfg=min(tg), ratio=min(tg) / min(ta), ms_vjp_median=float(np.median(ta)),
                ms_vjp_rfg_median=float(np.median(tg)))


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
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "simgradg", "--", sys.executable,
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
        row["kernel_ratio"] = ((km["k_abr2_vjp_rfg_batch"]["mean_us"] + km["k_abr_vjp_rfg_fold"]["mean_us"])
                               / (km["k_abr2_vjp_batch"]["mean_us"] + km["k_abr_vjp_fold"]["mean_us"]))
    print(json.dumps(row))


if __name__ == "__main__":
    main()
