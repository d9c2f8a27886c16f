"""Cost of the steady state's adjoint in b1, gr and df (mbfir.bloch_ss_vjp_gr_batch) against its adjoint in b1 alone
(mbfir.bloch_ss_vjp_batch) and against the composition of shipped calls that yields the same gradients, on the timing case of
tools/gpu_blochss.py: a 600-sample, 26 ms H-1 period at T1 = 1 s, T2 = 40 ms on 2048 frequencies x 8 positions at 3 transmit-gain
scales (192 workgroups).  The composition, per scale (one m0 serves every scale of a transient call): bloch_batch(mode=1), a
tripled batch of grad_m0 adjoints with unit cotangents for the rows of A, NumPy 3 x 3 solves for lambda, and
bloch_vjp_gr_batch(grad_df=True) from M: nine calls.  Times are warm host clocks around calls that end in a stream synchronise
(transfers included); the three fused calls alternate, the minimum and the median of --reps each.  The composition runs in a loop of
its own after them: alternated with the others, the call that followed it took 19 ms in the median on an MI355X (its minimum was
unchanged; the cause was not looked into), which says nothing about that call.  One JSON line.

    python tools/gpu_blochssg.py [--reps 20]
    python tools/gpu_blochssg.py --rocprof DIR [--reps 20]

The second form runs the three fused calls of the first (each kernel then occurs in one configuration) as a child under `rocprofv3
--kernel-trace --stats -d DIR` (no counters and nothing else traced in that run) and adds the mean kernel times from the trace to
the JSON line.
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
KERNELS = ("k_bloch_ss_vjp_batch", "k_bloch_vjp_fold", "k_bloch_ss_vjp_gr_batch<false>", "k_bloch_ss_vjp_gr_batch<true>",
           "k_bloch_vjp_gr_fold")


def measure(reps, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    cot = [tuple(rng.standard_normal((3, len(sc), nf, npos)))]
    unit = [tuple(np.full((1, nf, npos), 1.0 if c == i else 0.0) for c in range(3)) for i in range(3)]

    def ssadj():
        return mbfir.bloch_ss_vjp_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def ssg():
        return mbfir.bloch_ss_vjp_gr_batch(pulses, df, dp, cot, scales=sc, ctx=ctx)

    def ssgd():
        return mbfir.bloch_ss_vjp_gr_batch(pulses, df, dp, cot, scales=sc, grad_df=True, ctx=ctx)

    def comp():
        g, gg, gd = 0, 0, []
        for si, s in enumerate(sc):
            (Mx, My, Mz), = mbfir.bloch_batch(pulses, df, dp, scales=(s,), mode=1, ctx=ctx)
            M = (Mx[0], My[0], Mz[0])
            rows = mbfir.bloch_vjp_batch(pulses * 3, df, dp, unit, scales=(s,), m0=M, grad_m0=True, ctx=ctx)
            A = np.stack([np.stack([rows[i][1][j][0] for j in range(3)], -1) for i in range(3)], -2)
            c = np.stack([cot[0][i][si] for i in range(3)], -1)[..., None]
            lam = np.linalg.solve(np.swapaxes(np.eye(3) - A, -1, -2), c)[..., 0]
            r, = mbfir.bloch_vjp_gr_batch(pulses, df, dp, [tuple(lam[None, ..., i] for i in range(3))], scales=(s,), m0=M,
                                          grad_df=True, ctx=ctx)
            g, gg = g + r[0], gg + r[1]
            gd.append(r[2][0])
        return [(g, gg, np.stack(gd))]
    calls = dict(ss_vjp=ssadj, ss_vjp_gr=ssg, ss_vjp_gr_df=ssgd)
    for fn in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    if not kernels_only:                                    # in a loop of its own (the module's docstring says why)
        comp()
        acc["composition"] = []
        for _ in range(reps):
            t0 = time.perf_counter()
            comp()
            acc["composition"].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochssg", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps)
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    row["ratio"] = row["ms_ss_vjp_gr"] / row["ms_ss_vjp"]
    row["ratio_df"] = row["ms_ss_vjp_gr_df"] / row["ms_ss_vjp"]
    if not kernels_only:
        (cg, cgg, cgd), (fg, fgg, fgd) = comp()[0], ssgd()[0]
        row["composition_over_fused"] = row["ms_composition"] / row["ms_ss_vjp_gr_df"]
        row["fused_vs_composition_rel_gr"] = float(np.abs(cgg - fgg).max() / np.abs(fgg).max())
        row["fused_vs_composition_rel_df"] = float(np.abs(cgd - fgd).max() / np.abs(fgd).max())
    return row


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
    ap.add_argument("--kernels-only", action="store_true", help="only the fused calls, whose kernels the traced run reports")
    a = ap.parse_args()
    if not a.rocprof:
        print(json.dumps(measure(a.reps, a.kernels_only)))
        return
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochssg", "--", sys.executable,
           os.path.abspath(__file__), "--reps", str(a.reps), "--kernels-only"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = km = kernel_means(a.rocprof)
    if km and all(k in km for k in KERNELS):
        old = km["k_bloch_ss_vjp_batch"]["mean_us"] + km["k_bloch_vjp_fold"]["mean_us"]
        row["kernel_ratio"] = (km["k_bloch_ss_vjp_gr_batch<false>"]["mean_us"] + km["k_bloch_vjp_gr_fold"]["mean_us"]) / old
        row["kernel_ratio_df"] = (km["k_bloch_ss_vjp_gr_batch<true>"]["mean_us"] + km["k_bloch_vjp_gr_fold"]["mean_us"]) / old
    print(json.dumps(row))


if __name__ == "__main__":
    main()
