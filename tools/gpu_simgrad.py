"""Cost of the simulators' adjoint (mbfir.abr2_vjp_batch) against the forward call it differentiates (mbfir.abr2_batch), for the
pulse of examples/spiral2d_refine.py: dz2d(8, 1, 4, 512, 1, 2) at 90 degrees on 128 x 128 points at 3 transmit-gain scales (192
workgroups).  Times are warm host clocks around calls that end in a stream synchronise (transfers included); forward and adjoint
alternate, the minimum of --reps each.  One JSON line.

    python tools/gpu_simgrad.py [--reps 20]
    python tools/gpu_simgrad.py --rocprof DIR [--reps 20]

The second form runs the first as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters in that run) and adds the
mean kernel times of k_abr2_batch, k_abr2_vjp_batch and k_abr_vjp_fold from the trace to the JSON line.
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
KERNELS = ("k_abr2_batch", "k_abr2_vjp_batch", "k_abr_vjp_fold")


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    pulses, x, sc = [(rf * np.pi / 2, g)], np.linspace(-8, 8, 128), (0.9, 1.0, 1.1)
    rng = np.random.default_rng(0)
    cot = [tuple(rng.standard_normal((3, 128, 128)) + 1j * rng.standard_normal((3, 128, 128)) for _ in range(2))]

    def fwd():
        return mbfir.abr2_batch(pulses, x, x, scales=sc, ctx=ctx)

    def adj():
        return mbfir.abr2_vjp_batch(pulses, x, x, cot, scales=sc, ctx=ctx)
    fwd()
    adj()
    tf, ta = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fwd()
        tf.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        adj()
        ta.append((time.perf_counter() - t0) * 1e3)
    return dict(tool="gpu_simgrad", samples=len(rf), nx=128, ny=128, scales=len(sc), workgroups=3 * 64, reps=reps,
                ms_forward=min(tf), ms_vjp=min(ta), ratio=min(ta) / min(tf), ms_forward_median=float(np.median(tf)),
                ms_vjp_median=float(np.median(ta)))


def kernel_means(d):
    """mean microseconds per launch of KERNELS from the trace's SQLite database (rocprofv3's default output)"""
    import sqlite3
    hits = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    if not hits:
        return None
    agg = {}
    for name, start, end in sqlite3.connect(hits[0]).cursor().execute("select name, start, end from kernels"):
        for k in KERNELS:
            if k + "(" in name or name.endswith(k):
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
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "simgrad", "--", sys.executable,
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
        row["kernel_ratio"] = (km["k_abr2_vjp_batch"]["mean_us"] + km["k_abr_vjp_fold"]["mean_us"]) / km["k_abr2_batch"]["mean_us"]
    print(json.dumps(row))


if __name__ == "__main__":
    main()
