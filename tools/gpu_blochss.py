"""Cost of the derivatives of the Bloch simulator's steady state (mbfir.bloch_ss_vjp_batch, mbfir.bloch_ss_jvp_batch) against the
shipped calls on the same inputs: the timing case of tools/gpu_blochgrad.py, a 600-sample, 26 ms H-1 period at T1 = 1 s, T2 = 40 ms
on 2048 frequencies x 8 positions at 3 transmit-gain scales (192 workgroups).  Timed: bloch_batch(mode=1); bloch_vjp_batch (the
transient adjoint); the composition of shipped calls that yields the steady state's gradient (bloch_batch(mode=1), then per scale --
one m0 serves every scale of a transient call -- a tripled batch of grad_m0 adjoints with unit cotangents for A, NumPy 3 x 3 solves
and the adjoint from M: seven calls); bloch_ss_vjp_batch; bloch_ss_jvp_batch at K = 1 and K = 8.  Times are warm host clocks around
calls that end in a stream synchronise (transfers included); the calls alternate, the minimum and the median of --reps each.  One
JSON line.

    python tools/gpu_blochss.py [--reps 20]
    python tools/gpu_blochss.py --rocprof DIR [--reps 20]

The second form runs the kernels' share of the first (bloch_batch(mode=1), bloch_vjp_batch, bloch_ss_vjp_batch and bloch_ss_jvp_batch
at K = 8; each kernel then occurs in one configuration) as a child under `rocprofv3 --kernel-trace --stats -d DIR` (no counters in
that run) and adds the mean kernel times from the trace to the JSON line.
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
KERNELS = ("k_bloch_batch", "k_bloch_vjp_batch", "k_bloch_vjp_fold", "k_bloch_ss_vjp_batch", "k_bloch_ss_jvp_batch")


def measure(reps, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulse = (b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")
    pulses = [pulse]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    cot = [tuple(rng.standard_normal((3, len(sc), nf, npos)))]
    v = (rng.standard_normal((8, n)) + 1j * rng.standard_normal((8, n))) * np.abs(b1).max()
    unit = [tuple(np.full((1, nf, npos), 1.0 if c == i else 0.0) for c in range(3)) for i in range(3)]

    def fwd():
        return mbfir.bloch_batch(pulses, df, dp, scales=sc, mode=1, ctx=ctx)

    def adj():
        return mbfir.bloch_vjp_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def comp():
        (Mx, My, Mz), = fwd()
        g = 0
        for si, s in enumerate(sc):
            M = (Mx[si], My[si], Mz[si])
            rows = mbfir.bloch_vjp_batch(pulses * 3, df, dp, unit, scales=(s,), m0=M, grad_m0=True, ctx=ctx)
            A = np.stack([np.stack([rows[i][1][j][0] for j in range(3)], -1) for i in range(3)], -2)
            c = np.stack([cot[0][i][si] for i in range(3)], -1)[..., None]
            lam = np.linalg.solve(np.swapaxes(np.eye(3) - A, -1, -2), c)[..., 0]
            g = g + mbfir.bloch_vjp_batch(pulses, df, dp, [tuple(lam[None, ..., i] for i in range(3))], scales=(s,), m0=M, ctx=ctx)[0]
        return [g]

    def ssadj():
        return mbfir.bloch_ss_vjp_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def ssjvp1():
        return mbfir.bloch_ss_jvp_batch(pulses, df, dp, [v[0]], scales=sc, ctx=ctx)

    def ssjvp8():
        return mbfir.bloch_ss_jvp_batch(pulses, df, dp, [v], scales=sc, ctx=ctx)
    calls = dict(forward_ss=fwd, vjp=adj, ss_vjp=ssadj, ss_jvp_8=ssjvp8)
    if not kernels_only:
        calls.update(composition=comp, ss_jvp_1=ssjvp1)
    for fn in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochss", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps)
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not kernels_only:
        gc, gf = comp()[0], ssadj()[0]
        row["composition_over_fused"] = row["ms_composition"] / row["ms_ss_vjp"]
        row["fused_vs_composition_rel"] = float(np.abs(gc - gf).max() / np.abs(gf).max())
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
    ap.add_argument("--kernels-only", action="store_true", help="only the calls whose kernels the traced run reports")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps, a.kernels_only)))
        return
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochss", "--", sys.executable,
           os.path.abspath(__file__), "--reps", str(a.reps), "--kernels-only"]
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
