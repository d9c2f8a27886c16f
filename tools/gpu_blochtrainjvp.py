"""Cost of the train's tangent (mbfir.bloch_train_jvp_batch) on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
The calls are timed alternating, the minimum and the median of --reps each (--tiled-reps for the tiled call):
    jvp_1, jvp_k:     the new call with the tangent echoes, at ndir = 1 and at ndir = k, the larger of the two kernels' group sizes;
    fd_1, fd_k:       what it replaces, the central difference: two mbfir.bloch_train_batch calls per direction (the quotient is
                      not formed: only the calls are timed);
    jvp_final:        the new call with echoes=False, final=True at ndir = 1;
    tiled_final:      the shipped mbfir.bloch_jvp_batch on the waveform tiled ntr times on the host with the direction tiled as
                      gains[k] e^{+i phi_k} v, the one tangent both calls can express;
and, for scale, `forward`: mbfir.bloch_train_batch with the echoes.  The difference of the two final tangents is reported relative
to the largest entry.  Times are warm host clocks around calls that end in a stream synchronise (transfers included).  One JSON line
per workload.

    python tools/gpu_blochtrainjvp.py [--workload batch64|long] [--reps 10] [--tiled-reps 3]
    python tools/gpu_blochtrainjvp.py --rocprof DIR --workload batch64 [--reps 10]

The second form runs jvp_k, tiled_final and forward as a child under `rocprofv3 --kernel-trace --stats -d DIR` (nothing else traced,
no counters in that run) and adds the mean kernel times from the trace to the JSON line: the new kernels at ndir = k, the forward
kernels on the periods themselves.
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

fwd.KERNELS = ("k_bloch_train_prop_jvp", "k_bloch_train_run_jvp", "k_bloch_train_prop", "k_bloch_train_run", "k_bloch_jvp_batch")


def measure(W, reps, tiled_reps, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(1)
    pulses, df, dp, ntr, n, echo = W["pulses"], W["df"], W["dp"], W["ntr"], W["n"], W["echo"]
    ph, gn = W["phases"], W["gains"]
    P, K = len(pulses), max(mbfir.bloch_train_jvp_group())
    tile = lambda b: np.concatenate([g * np.exp(1j * p) * b for p, g in zip(ph, gn)])
    tiles = [(tile(b1), np.tile(gr, ntr), np.tile(tp, ntr), t1, t2, nuc) for b1, gr, tp, t1, t2, nuc in pulses]
    vs = [(rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * np.abs(p[0]).max() for p in pulses]
    v1, vt = [v[0] for v in vs], [tile(v[0]) for v in vs]
    h = 1e-5 / max(float(np.abs(v).max()) for v in vs) * max(float(np.abs(p[0]).max()) for p in pulses)
    moved = {k: [(p[0] + s * h * v[j],) + p[1:] for p, v in zip(pulses, vs) for j in range(k) for s in (1, -1)] for k in (1, K)}
    kw = dict(phases=ph, gains=gn, echo=echo, ctx=ctx)

    def jvp_1():
        return mbfir.bloch_train_jvp_batch(pulses, df, dp, ntr, v1, **kw)

    def jvp_k():
        return mbfir.bloch_train_jvp_batch(pulses, df, dp, ntr, vs, **kw)

    def fd_1():
        return mbfir.bloch_train_batch(moved[1], df, dp, ntr, **kw)

    def fd_k():
        return mbfir.bloch_train_batch(moved[K], df, dp, ntr, **kw)

    def jvp_final():
        return mbfir.bloch_train_jvp_batch(pulses, df, dp, ntr, v1, echoes=False, final=True, **kw)

    def tiled_final():
        return [t for _, t in mbfir.bloch_jvp_batch(tiles, df, dp, vt, ctx=ctx)]

    def forward():
        return mbfir.bloch_train_batch(pulses, df, dp, ntr, **kw)
    calls = dict(jvp_1=(jvp_1, reps), jvp_k=(jvp_k, reps), fd_1=(fd_1, reps), fd_k=(fd_k, reps), jvp_final=(jvp_final, reps),
                 tiled_final=(tiled_final, tiled_reps), forward=(forward, reps))
    if kernels_only:              # a kernel's mean is over one configuration: ndir = k, and the forward kernels on the periods themselves
        calls = {k: calls[k] for k in ("jvp_k", "tiled_final", "forward")}
    for fn, _ in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for r in range(max(reps, tiled_reps)):
        for k, (fn, cnt) in calls.items():
            if r < cnt:
                t0 = time.perf_counter()
                fn()
                acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainjvp", workload=W["name"], periods=P, samples=n, repetitions=ntr, nf=len(df), npos=len(dp), reps=reps,
               tiled_reps=tiled_reps, tiled_samples=n * ntr, k=K, groups=list(mbfir.bloch_train_jvp_group()))
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not kernels_only:
        a, b = jvp_final(), tiled_final()
        row["fd_over_jvp_1"] = row["ms_fd_1"] / row["ms_jvp_1"]
        row["fd_over_jvp_k"] = row["ms_fd_k"] / row["ms_jvp_k"]
        row["jvp_k_over_jvp_1"] = row["ms_jvp_k"] / row["ms_jvp_1"]
        row["jvp_1_over_forward"] = row["ms_jvp_1"] / row["ms_forward"]
        row["tiled_over_train"] = row["ms_tiled_final"] / row["ms_jvp_final"]
        row["train_vs_tiled_rel"] = max(float(np.abs(u - v).max() / np.abs(v).max()) for x, y in zip(a, b) for u, v in zip(x, y))
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
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochtrainjvp", "--", sys.executable,
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
