"""Cost of the train's fused least-squares and Gauss-Newton products (mbfir.bloch_train_lsq_batch, mbfir.bloch_train_gn_batch, DESIGN
section 8ab) against the shipped two-call paths, on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
The calls are timed alternating, the minimum and the median of --reps each:
    lsq_full, lsq_bcast: the fused loss and gradient with echo-sized planes, and with point-sized planes used at every repetition;
    lsq_two:             mbfir.bloch_train_batch, a NumPy residual and loss over the echoes, mbfir.bloch_train_vjp_batch;
    gn_1, gn_4:          the fused products at 1 and 4 directions (broadcast weights);
    gn_two_1, gn_two_4:  mbfir.bloch_train_jvp_batch, NumPy weights, mbfir.bloch_train_vjp_batch once per direction.
The fused results are compared with the two-call ones relative to the largest entry.  Times are warm host clocks around calls that
end in a stream synchronise (transfers included).  One JSON line per workload.

    python tools/gpu_blochtraingn.py [--workload batch64|long] [--reps 5]
    python tools/gpu_blochtraingn.py --rocprof DIR --workload batch64 [--reps 5]

The second form runs lsq_bcast, gn_4 and lsq_two as a child under `rocprofv3 --kernel-trace --stats -d DIR` (nothing else traced, no
counters in that run) and adds the mean kernel times from the trace to the JSON line.
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

fwd.KERNELS = ("k_bloch_train_run_lsq", "k_bloch_train_run_gn", "k_bloch_train_gn_fold", "k_bloch_train_prop_vjp",
               "k_bloch_train_prop_jvp", "k_bloch_train_prop", "k_bloch_train_run_vjp", "k_bloch_train_run_jvp", "k_bloch_train_run",
               "k_bloch_train_vjp_fold")


def measure(W, reps, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(2)
    pulses, df, dp, ntr, n, echo = W["pulses"], W["df"], W["dp"], W["ntr"], W["n"], W["echo"]
    P, nf, npos = len(pulses), len(df), len(dp)
    rw = np.append(np.zeros(8), np.ones(ntr - 8))                       # the first echoes of the transient left out
    wb = [tuple(rng.uniform(0, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    tb = [tuple(rng.uniform(-1, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    rep = lambda tri: tuple(np.ascontiguousarray(np.broadcast_to(v[:, None], (1, ntr, nf, npos))) for v in tri)
    wf, tf = [rep(t) for t in wb], [rep(t) for t in tb]
    vs = [(rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))) * np.abs(p[0]).max() for p in pulses]
    kw = dict(phases=W["phases"], gains=W["gains"], echo=echo, demod=True, ctx=ctx)
    r4 = rw[None, :, None, None]

    def lsq_full():
        return mbfir.bloch_train_lsq_batch(pulses, df, dp, ntr, tf, wf, rep_weights=rw, **kw)

    def lsq_bcast():
        return mbfir.bloch_train_lsq_batch(pulses, df, dp, ntr, tb, wb, rep_weights=rw, **kw)

    def lsq_two():
        E = mbfir.bloch_train_batch(pulses, df, dp, ntr, **kw)
        res = [[e[i] - tb[q][i][:, None] for i in range(3)] for q, e in enumerate(E)]
        L = [0.5 * sum(float((r4 * wb[q][i][:, None] * r[i] ** 2).sum()) for i in range(3)) for q, r in enumerate(res)]
        ce = [tuple(r4 * wb[q][i][:, None] * r[i] for i in range(3)) for q, r in enumerate(res)]
        return list(zip(L, mbfir.bloch_train_vjp_batch(pulses, df, dp, ntr, ce, **kw)))

    def gn(K):
        return mbfir.bloch_train_gn_batch(pulses, df, dp, ntr, [v[:K] for v in vs], wb, rep_weights=rw, **kw)

    def gn_two(K):
        dE = mbfir.bloch_train_jvp_batch(pulses, df, dp, ntr, [v[:K] for v in vs], **kw)
        out = []
        for k in range(K):
            ce = [tuple(r4 * wb[q][i][:, None] * dE[q][i][k] for i in range(3)) for q in range(P)]
            out.append(mbfir.bloch_train_vjp_batch(pulses, df, dp, ntr, ce, **kw))
        return [np.stack([out[k][q] for k in range(K)]) for q in range(P)]
    calls = dict(lsq_full=lsq_full, lsq_bcast=lsq_bcast, lsq_two=lsq_two, gn_1=lambda: gn(1), gn_4=lambda: gn(4),
                 gn_two_1=lambda: gn_two(1), gn_two_4=lambda: gn_two(4))
    if kernels_only:              # a kernel's mean is over one configuration
        calls = {k: calls[k] for k in ("lsq_bcast", "gn_4", "lsq_two")}
    for fn in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtraingn", workload=W["name"], periods=P, samples=n, repetitions=ntr, nf=nf, npos=npos, reps=reps,
               echo_mb_per_plane_triple=3 * 8e-6 * P * ntr * nf * npos)
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not kernels_only:
        a, b, c = lsq_full(), lsq_bcast(), lsq_two()
        h, h2 = gn(4), gn_two(4)
        row["two_over_lsq_full"] = row["ms_lsq_two"] / row["ms_lsq_full"]
        row["two_over_lsq_bcast"] = row["ms_lsq_two"] / row["ms_lsq_bcast"]
        row["two_over_gn_1"] = row["ms_gn_two_1"] / row["ms_gn_1"]
        row["two_over_gn_4"] = row["ms_gn_two_4"] / row["ms_gn_4"]
        row["bcast_is_full"] = all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
        row["lsq_vs_two_rel"] = max(float(np.abs(x[1] - y[1]).max() / np.abs(y[1]).max()) for x, y in zip(b, c))
        row["loss_vs_two_rel"] = max(abs(x[0] - y[0]) / y[0] for x, y in zip(b, c))
        row["gn_vs_two_rel"] = max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(h, h2))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    ap.add_argument("--kernels-only", action="store_true", help="only what the traced run reports")
    a = ap.parse_args()
    names = a.workload or ["batch64", "long"]
    if not a.rocprof:
        for name in names:
            print(json.dumps(measure(fwd.workload(name), a.reps, a.kernels_only)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    # the traced program is a fresh child: this process never opens the GPU
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochtraingn", "--", sys.executable,
           os.path.abspath(__file__), "--workload", names[0], "--reps", str(a.reps), "--kernels-only"]
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
