"""Cost of the train's adjoint in b1, gr and df (mbfir.bloch_train_vjp_gr_batch) on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
The calls are timed alternating, the minimum and the median of --reps each (--tiled-reps for the tiled call and the central
difference), with a cotangent of the final state only, the one loss every call can express:
    gr:         the new call;
    gr_df:      the new call with grad_df=True;
    b1:         the shipped mbfir.bloch_train_vjp_batch (the parent's code) on the same inputs;
    tiled:      the shipped mbfir.bloch_vjp_gr_batch on the waveform tiled ntr times on the host, its grad_gr rows summed over the
                repetitions on the host (inside the timed region: it is part of getting the same numbers);
    fd_pair:    the two mbfir.bloch_train_batch calls of a central difference in one gr entry; the whole gradient by central
                differences is `samples` such pairs per axis (reported as ms_fd_all, extrapolated, not run).
The difference of the new call's grad_gr and grad_df from the tiled call's is reported relative to the largest entry.  Times are
warm host clocks around calls that end in a stream synchronise (transfers included).  One JSON line per workload.

    python tools/gpu_blochtrainvjpg.py [--workload batch64|long] [--reps 10] [--tiled-reps 3]
    python tools/gpu_blochtrainvjpg.py --rocprof DIR --workload batch64 [--reps 10]

The second form runs the same calls as a child under `rocprofv3 --kernel-trace --stats -d DIR` (nothing else traced, no counters in
that run) and adds the mean kernel times from the trace to the JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_blochtrain as fwd  # noqa: E402

fwd.KERNELS = ("k_bloch_train_prop_vjp_gr<false>", "k_bloch_train_prop_vjp_gr<true>", "k_bloch_train_vjp_gr_fold",
               "k_bloch_train_vjp_df_fold", "k_bloch_train_prop_vjp", "k_bloch_train_run_vjp", "k_bloch_train_vjp_fold",
               "k_bloch_train_prop", "k_bloch_train_run", "k_bloch_vjp_gr_batch<true>", "k_bloch_vjp_gr_fold")


def measure(W, reps, tiled_reps, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(1)
    pulses, df, dp, ntr, n, echo = W["pulses"], W["df"], W["dp"], W["ntr"], W["n"], W["echo"]
    ph, gn = W["phases"], W["gains"]
    nf, npos, P = len(df), len(dp), len(pulses)
    tiles = [(np.concatenate([g * np.exp(1j * p) * b1 for p, g in zip(ph, gn)]), np.tile(gr, ntr), np.tile(tp, ntr), t1, t2, nuc)
             for b1, gr, tp, t1, t2, nuc in pulses]
    cf = [tuple(rng.standard_normal((3, 1, nf, npos))) for _ in range(P)]
    kw = dict(phases=ph, gains=gn, echo=echo, ctx=ctx)
    h = np.zeros(n)
    h[n // 3] = 1e-6
    moved = [[(b1, gr + s * h, tp, t1, t2, nuc) for b1, gr, tp, t1, t2, nuc in pulses] for s in (1, -1)]

    def gr():
        return mbfir.bloch_train_vjp_gr_batch(pulses, df, dp, ntr, None, cot_final=cf, **kw)

    def gr_df():
        return mbfir.bloch_train_vjp_gr_batch(pulses, df, dp, ntr, None, cot_final=cf, grad_df=True, **kw)

    def b1():
        return mbfir.bloch_train_vjp_batch(pulses, df, dp, ntr, None, cot_final=cf, **kw)

    def tiled():
        return [(g.reshape(ntr, n, 3).sum(0), d) for _, g, d in mbfir.bloch_vjp_gr_batch(tiles, df, dp, cf, grad_df=True, ctx=ctx)]

    def fd_pair():
        return [mbfir.bloch_train_batch(m, df, dp, ntr, final=True, **kw) for m in moved]
    calls = dict(gr=(gr, reps), gr_df=(gr_df, reps), b1=(b1, reps), tiled=(tiled, tiled_reps), fd_pair=(fd_pair, tiled_reps))
    for fn, _ in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for r in range(max(reps, tiled_reps)):
        for k, (fn, cnt) in calls.items():
            if r < cnt:
                t0 = time.perf_counter()
                fn()
                acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainvjpg", workload=W["name"], periods=P, samples=n, repetitions=ntr, nf=nf, npos=npos, reps=reps,
               tiled_reps=tiled_reps, tiled_samples=n * ntr)
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not kernels_only:
        a, b = gr_df(), tiled()
        row["ms_fd_all"] = row["ms_fd_pair"] * n
        row["gr_over_b1"] = row["ms_gr"] / row["ms_b1"]
        row["gr_df_over_b1"] = row["ms_gr_df"] / row["ms_b1"]
        row["tiled_over_gr_df"] = row["ms_tiled"] / row["ms_gr_df"]
        row["fd_all_over_gr"] = row["ms_fd_all"] / row["ms_gr"]
        # batch64 has the one position 0: both gr gradients are exact zeros there, and the difference is reported as it is
        row["gr_vs_tiled_rel"] = max(float(np.abs(u[1] - v[0]).max() / max(np.abs(v[0]).max(), 1e-300)) for u, v in zip(a, b))
        row["df_vs_tiled_rel"] = max(float(np.abs(u[2] - v[1]).max() / np.abs(v[1]).max()) for u, v in zip(a, b))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tiled-reps", type=int, default=3)
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    ap.add_argument("--kernels-only", action="store_true", help="only what the traced run reports")
    a = ap.parse_args()
    names = a.workload or ["batch64", "long"]
    if not a.rocprof:
        for name in names:
            print(json.dumps(measure(fwd.workload(name), a.reps, min(a.reps, a.tiled_reps), a.kernels_only)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochtrainvjpg", "--", sys.executable,
           os.path.abspath(__file__), "--workload", names[0], "--reps", str(a.reps), "--tiled-reps", str(a.tiled_reps), "--kernels-only"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = fwd.kernel_means(a.rocprof)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
