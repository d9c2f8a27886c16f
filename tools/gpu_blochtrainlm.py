"""Cost of one tried Levenberg-Marquardt step of the pulse train solved on the device (mbfir.bloch_train_lm_step_batch)
against the host loop of mbfir.refine_bloch_train_batch that it replaces, at cg = 8 and rtol = 0 (every iteration runs), on the two
workloads of tools/gpu_blochtrain.py with broadcast targets and weights:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
Timed per workload:
    device   one bloch_train_lm_step_batch call with targets: one upload, the propagator and the adjoint's checkpoints once, 8 rounds,
             the trial, one download
    host     the same step as the host solver takes it: 8 bloch_train_gn_batch calls with the CG arithmetic in NumPy, then 1
             bloch_train_lsq_batch call
    gn, lsq  one bloch_train_gn_batch call and one bloch_train_lsq_batch call alone, to say where the host solver's time goes
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the four alternate, minimum and median
of --reps each.  One JSON line per workload.

    python tools/gpu_blochtrainlm.py [--workload batch64|long] [--reps 5]
    python tools/gpu_blochtrainlm.py --rocprof DIR --workload batch64 [--reps 3]

The second form runs device and gn as a child under `rocprofv3 --kernel-trace --stats -d DIR` (nothing else traced, no counters in
that run) and adds the mean kernel times from the trace to the JSON line: k_bloch_train_lm_pvjp beside the shipped
k_bloch_train_prop_vjp and k_bloch_train_lm_prep beside k_bloch_train_prop say what hoisting the checkpoints out of the rounds buys.
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

CG = 8
fwd.KERNELS = ("k_bloch_train_lm_prep", "k_bloch_train_lm_jvp", "k_bloch_train_lm_run", "k_bloch_train_lm_pvjp", "k_bloch_train_lm_step",
               "k_bloch_train_run_lsq", "k_bloch_train_run_gn", "k_bloch_train_gn_fold", "k_bloch_train_prop_vjp",
               "k_bloch_train_prop_jvp", "k_bloch_train_prop", "k_lm_init", "k_bloch_lm_trial")


def _dot(u, v):
    return float((np.conj(u) * v).real.sum())


def measure(W, reps, kernels_only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(2)
    pulses, df, dp, ntr = W["pulses"], W["df"], W["dp"], W["ntr"]
    P, nf, npos = len(pulses), len(df), len(dp)
    rw = np.append(np.zeros(8), np.ones(ntr - 8))                       # the first echoes of the transient left out
    wb = [tuple(rng.uniform(0, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    tb = [tuple(rng.uniform(-1, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    kw = dict(rep_weights=rw, phases=W["phases"], gains=W["gains"], echo=W["echo"], demod=True, ctx=ctx)
    b = [-g for _, g in mbfir.bloch_train_lsq_batch(pulses, df, dp, ntr, tb, wb, **kw)]
    mu = [1e-3 * _dot(v, h) / _dot(v, v) for v, h in zip(b, mbfir.bloch_train_gn_batch(pulses, df, dp, ntr, b, wb, **kw))]

    def device():
        return [d for d, _ in mbfir.bloch_train_lm_step_batch(pulses, df, dp, ntr, b, wb, mu, targets=tb, cg=CG, rtol=0.0, **kw)]

    def host():                                                   # refine_bloch_train_batch's host solver, one tried step
        R = range(P)
        d = [np.zeros_like(v) for v in b]
        r = [v.copy() for v in b]
        p = [v.copy() for v in b]
        rr = [_dot(v, v) for v in r]
        for _ in range(CG):
            for q, hp in zip(R, mbfir.bloch_train_gn_batch(pulses, df, dp, ntr, p, wb, **kw)):
                ap = hp + mu[q] * p[q]
                alpha = rr[q] / _dot(p[q], ap)
                d[q], r[q] = d[q] + alpha * p[q], r[q] - alpha * ap
                rr[q], old = _dot(r[q], r[q]), rr[q]
                p[q] = r[q] + (rr[q] / old) * p[q]
        mbfir.bloch_train_lsq_batch([(pulses[q][0] + d[q],) + tuple(pulses[q][1:]) for q in R], df, dp, ntr, tb, wb, **kw)
        return d

    def gn():
        mbfir.bloch_train_gn_batch(pulses, df, dp, ntr, b, wb, **kw)

    def lsq():
        mbfir.bloch_train_lsq_batch(pulses, df, dp, ntr, tb, wb, **kw)
    runs = (("device", device), ("gn", gn)) if kernels_only else (("device", device), ("host", host), ("gn", gn), ("lsq", lsq))
    out = {name: f() for name, f in runs}
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t0 = time.perf_counter()
            f()
            t[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainlm", workload=W["name"], periods=P, samples=W["n"], repetitions=ntr, nf=nf, npos=npos, cg=CG, reps=reps)
    for name, _ in runs:
        row["ms_" + name] = min(t[name])
        row["ms_" + name + "_median"] = float(np.median(t[name]))
    if not kernels_only:
        row["speedup"] = row["ms_host"] / row["ms_device"]
        row["host_spread"] = row["ms_host_median"] / row["ms_host"]
        row["step_device_vs_host"] = max(float(np.abs(u - v).max() / np.abs(v).max()) for u, v in zip(out["device"], out["host"]))
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
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "blochtrainlm", "--", sys.executable,
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
