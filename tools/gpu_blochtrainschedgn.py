"""Cost of the fused least-squares and Gauss-Newton products of the train's schedule (mbfir.bloch_train_lsq_sched_batch,
mbfir.bloch_train_gn_sched_batch) against the shipped two-call paths, on the two workloads of
tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
The calls are timed alternating, the minimum and the median of --reps each:
    lsq_full, lsq_bcast: the fused loss and schedule gradient with echo-sized planes, and with point-sized planes used at every
                         repetition;
    lsq_two:             mbfir.bloch_train_batch, a NumPy residual and loss over the echoes, mbfir.bloch_train_vjp_sched_batch;
    gn_1, gn_8:          the fused products at 1 and 8 directions (broadcast weights);
    gn_two_1, gn_two_8:  mbfir.bloch_train_jvp_sched_batch, NumPy weights, mbfir.bloch_train_vjp_sched_batch once per direction;
    gn_dense:            the 2 ntr unit directions, the dense normal matrix, in --dense-chunks calls of 2 ntr / chunks directions each
                         (1 unless the checkpoints of 2 ntr directions do not fit the device; the JSON line says how many);
    gn_two_dense:        the two-call path on the first --dense-two directions of them, timed once and scaled to 2 ntr directions
                         (the path is one pair of calls per direction, so its cost is linear in them; the JSON line says how many
                         were timed).
The fused results are compared with the two-call ones relative to the largest entry.  Times are warm host clocks around calls that
end in a stream synchronise (transfers included).  One JSON line per workload.

    timeout -k 10 600 python tools/gpu_blochtrainschedgn.py --workload batch64 --reps 5 && \\
    timeout -k 10 900 python tools/gpu_blochtrainschedgn.py --workload long --reps 5 && \\
    timeout -k 10 600 python tools/gpu_blochtrainschedgn.py --rocprof DIR --workload long --reps 5

Every step that opens the GPU runs under its own time limit and the steps are chained with &&, so that a step that fails or hangs
ends the chain.  The last form runs lsq_bcast, gn_8 and lsq_two as a fresh child under `timeout -k 10 <limit> rocprofv3 --kernel-trace
--stats -d DIR` (nothing else traced, no counters in that run; --limit sets the child's own limit) and adds the mean kernel times
from the trace to the JSON line.
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

fwd.KERNELS = ("k_bloch_train_run_sched_lsq", "k_bloch_train_run_sched_gn", "k_bloch_train_sched_gn_fold", "k_bloch_train_run_sched_jvp",
               "k_bloch_train_run_sched", "k_bloch_train_sched_fold", "k_bloch_train_prop_dgain", "k_bloch_train_prop", "k_bloch_train_run")


def measure(W, reps, kernels_only, dense_chunks, dense_two):
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
    dgs, dps = [rng.standard_normal((8, ntr)) for _ in range(P)], [rng.standard_normal((8, ntr)) for _ in range(P)]
    eye, zero = np.eye(ntr), np.zeros((ntr, ntr))
    ug, up = np.concatenate([eye, zero]), np.concatenate([zero, eye])
    kw = dict(phases=W["phases"], gains=W["gains"], echo=echo, demod=True, ctx=ctx)
    r4 = rw[None, :, None, None]

    def lsq_full():
        return mbfir.bloch_train_lsq_sched_batch(pulses, df, dp, ntr, tf, wf, rep_weights=rw, **kw)

    def lsq_bcast():
        return mbfir.bloch_train_lsq_sched_batch(pulses, df, dp, ntr, tb, wb, rep_weights=rw, **kw)

    def lsq_two():
        E = mbfir.bloch_train_batch(pulses, df, dp, ntr, **kw)
        res = [[e[i] - tb[q][i][:, None] for i in range(3)] for q, e in enumerate(E)]
        L = [0.5 * sum(float((r4 * wb[q][i][:, None] * r[i] ** 2).sum()) for i in range(3)) for q, r in enumerate(res)]
        ce = [tuple(r4 * wb[q][i][:, None] * r[i] for i in range(3)) for q, r in enumerate(res)]
        return [(l,) + g for l, g in zip(L, mbfir.bloch_train_vjp_sched_batch(pulses, df, dp, ntr, ce, **kw))]

    def gn_at(dg, dph):
        return mbfir.bloch_train_gn_sched_batch(pulses, df, dp, ntr, wb, tangents_gains=dg, tangents_phases=dph, rep_weights=rw, **kw)

    def gn(K):
        return gn_at([v[:K] for v in dgs], [v[:K] for v in dps])

    def gn_two_at(dg, dph):
        """the two-call path along the directions dg[q], dph[q] ((K, ntr) each): per pulse (Hg (K, ntr), Hp (K, ntr))"""
        dE = mbfir.bloch_train_jvp_sched_batch(pulses, df, dp, ntr, tangents_gains=dg, tangents_phases=dph, **kw)
        out = []
        for k in range(dg[0].shape[0]):
            ce = [tuple(r4 * wb[q][i][:, None] * dE[q][i][k] for i in range(3)) for q in range(P)]
            out.append(mbfir.bloch_train_vjp_sched_batch(pulses, df, dp, ntr, ce, **kw))
        return [(np.stack([o[q][0] for o in out]), np.stack([o[q][1] for o in out])) for q in range(P)]

    def gn_two(K):
        return gn_two_at([v[:K] for v in dgs], [v[:K] for v in dps])

    def gn_dense():
        step = (2 * ntr + dense_chunks - 1) // dense_chunks
        parts = [gn_at([ug[a:a + step]] * P, [up[a:a + step]] * P) for a in range(0, 2 * ntr, step)]
        return [np.concatenate([np.concatenate([p[q][0], p[q][1]], 1) for p in parts]) for q in range(P)]
    calls = dict(lsq_full=lsq_full, lsq_bcast=lsq_bcast, lsq_two=lsq_two, gn_1=lambda: gn(1), gn_8=lambda: gn(8),
                 gn_two_1=lambda: gn_two(1), gn_two_8=lambda: gn_two(8), gn_dense=gn_dense)
    if kernels_only:              # a kernel's mean is over one configuration
        calls = {k: calls[k] for k in ("lsq_bcast", "gn_8", "lsq_two")}
    for fn in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainschedgn", workload=W["name"], periods=P, samples=n, repetitions=ntr, nf=nf, npos=npos, reps=reps,
               echo_mb_per_plane_triple=3 * 8e-6 * P * ntr * nf * npos)
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not kernels_only:
        a, b, c = lsq_full(), lsq_bcast(), lsq_two()
        h, h2 = gn(8), gn_two(8)
        K2 = min(dense_two, 2 * ntr)
        t0 = time.perf_counter()
        d2 = gn_two_at([ug[:K2]] * P, [up[:K2]] * P)
        row["ms_gn_two_dense"] = (time.perf_counter() - t0) * 1e3 * (2 * ntr) / K2
        row["gn_two_dense_directions_timed"], row["dense_directions"], row["dense_chunks"] = K2, 2 * ntr, dense_chunks
        H = gn_dense()
        row["two_over_lsq_full"] = row["ms_lsq_two"] / row["ms_lsq_full"]
        row["two_over_lsq_bcast"] = row["ms_lsq_two"] / row["ms_lsq_bcast"]
        row["two_over_gn_1"] = row["ms_gn_two_1"] / row["ms_gn_1"]
        row["two_over_gn_8"] = row["ms_gn_two_8"] / row["ms_gn_8"]
        row["two_over_gn_dense"] = row["ms_gn_two_dense"] / row["ms_gn_dense"]
        same = lambda x, y: x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
        row["bcast_is_full"] = all(same(x, y) for x, y in zip(a, b))
        rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
        row["lsq_vs_two_rel"] = max(max(rel(x[1], y[1]), rel(x[2], y[2])) for x, y in zip(b, c))
        row["loss_vs_two_rel"] = max(abs(x[0] - y[0]) / y[0] for x, y in zip(b, c))
        row["gn_vs_two_rel"] = max(max(rel(x[0], y[0]), rel(x[1], y[1])) for x, y in zip(h, h2))
        row["dense_vs_two_rel"] = max(rel(Hq[:K2], np.concatenate([y[0], y[1]], 1)) for Hq, y in zip(H, d2))
        row["dense_asymmetry_rel"] = max(float(np.abs(Hq - Hq.T).max() / np.abs(Hq).max()) for Hq in H)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-chunks", type=int, default=1, help="calls the 2 ntr unit directions are spread over")
    ap.add_argument("--dense-two", type=int, default=8, help="directions of the dense set the two-call path is timed on")
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR")
    ap.add_argument("--limit", type=int, default=540, help="seconds the traced child may take (timeout -k 10)")
    ap.add_argument("--kernels-only", action="store_true", help="only what the traced run reports")
    a = ap.parse_args()
    names = a.workload or ["batch64", "long"]
    if not a.rocprof:
        for name in names:
            print(json.dumps(measure(fwd.workload(name), a.reps, a.kernels_only, a.dense_chunks, a.dense_two)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    # the traced program is a fresh child under its own time limit: this process never opens the GPU
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochtrainschedgn", "--",
           sys.executable, os.path.abspath(__file__), "--workload", names[0], "--reps", str(a.reps), "--kernels-only"]
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
