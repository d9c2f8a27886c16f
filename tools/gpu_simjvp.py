"""Cost of the simulators' tangent (mbfir.abr2_jvp_batch) against the forward call it differentiates (mbfir.abr2_batch) and against
what central differences cost, for the pulse of examples/spiral2d_refine.py: dz2d(8, 1, 4, 512, 1, 2) at 90 degrees on 128 x 128
points at 3 transmit-gain scales (192 forward workgroups).  Timed: abr2_batch; abr2_jvp_batch with K = 1 direction; abr2_jvp_batch
with K = JVP_K directions (one full group per workgroup); and 2 K forward calls, the price of central differences along K
directions.  Times are warm host clocks around calls that end in a stream synchronise (transfers included); the four alternate,
minimum and median of --reps each.  One JSON line.

    python tools/gpu_simjvp.py [--reps 20]
    python tools/gpu_simjvp.py --rocprof DIR [--reps 20]

The second form runs the first as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters in that run) and adds the
mean kernel times of k_abr2_batch and k_abr2_jvp_batch (its K = 1 and K = JVP_K launches apart) from the trace to the JSON line.
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


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    K = mbfir.jvp_group()
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    rf = rf * np.pi / 2
    x, sc = np.linspace(-8, 8, 128), (0.9, 1.0, 1.1)
    rng = np.random.default_rng(0)
    v = rng.standard_normal((K, len(rf))) + 1j * rng.standard_normal((K, len(rf)))
    h = 1e-6

    def fwd():
        return mbfir.abr2_batch([(rf, g)], x, x, scales=sc, ctx=ctx)

    def jvp1():
        return mbfir.abr2_jvp_batch([(rf, g)], x, x, [v[:1]], scales=sc, ctx=ctx)

    def jvpk():
        return mbfir.abr2_jvp_batch([(rf, g)], x, x, [v], scales=sc, ctx=ctx)

    def central():
        return [mbfir.abr2_batch([(rf + s * h * v[k], g)], x, x, scales=sc, ctx=ctx) for k in range(K) for s in (1, -1)]
    runs = (("forward", fwd), ("jvp_1", jvp1), ("jvp_k", jvpk), ("central_2k_forwards", central))
    for _, f in runs:
        f()
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t0 = time.perf_counter()
            f()
            t[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_simjvp", samples=len(rf), nx=128, ny=128, scales=len(sc), forward_workgroups=3 * 64, jvp_k=K, reps=reps)
    for name, _ in runs:
        row["ms_" + name] = min(t[name])
        row["ms_" + name + "_median"] = float(np.median(t[name]))
    f0 = row["ms_forward"]
    row["ratio_jvp_1"] = row["ms_jvp_1"] / f0                              # one direction, in forward calls
    row["ratio_jvp_k_per_direction"] = row["ms_jvp_k"] / K / f0            # K directions, per direction
    row["ratio_central_per_direction"] = row["ms_central_2k_forwards"] / K / f0
    return row


def kernel_means(d):
    """mean microseconds per launch of k_abr2_batch and of k_abr2_jvp_batch from the trace's SQLite database (rocprofv3's default
    output).  The K = 1 and the K = JVP_K launches have the same grid (one direction group) and alternate, K = 1 first, so they
    are told apart by their order."""
    import sqlite3
    hits = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    if not hits:
        return None
    agg, order = {}, 0
    for name, start, end in sqlite3.connect(hits[0]).cursor().execute("select name, start, end from kernels order by start"):
        if "k_abr2_jvp_batch" in name:
            key = "k_abr2_jvp_batch_1" if order % 2 == 0 else "k_abr2_jvp_batch_k"
            order += 1
        elif "k_abr2_batch" in name:
            key = "k_abr2_batch"
        else:
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
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "simjvp", "--", sys.executable,
           os.path.abspath(__file__), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = km = kernel_means(a.rocprof)
    if km and all(k in km for k in ("k_abr2_batch", "k_abr2_jvp_batch_1", "k_abr2_jvp_batch_k")):
        f0 = km["k_abr2_batch"]["mean_us"]
        row["kernel_ratio_jvp_1"] = km["k_abr2_jvp_batch_1"]["mean_us"] / f0
        row["kernel_ratio_jvp_k_per_direction"] = km["k_abr2_jvp_batch_k"]["mean_us"] / row["jvp_k"] / f0
    print(json.dumps(row))


if __name__ == "__main__":
    main()
