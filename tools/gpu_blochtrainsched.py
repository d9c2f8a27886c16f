"""Cost of the train's adjoint in its schedule (mbfir.bloch_train_vjp_sched_batch) on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
Calls timed, alternating, the minimum and the median of --reps each (--fd-reps for the central difference, which is slow):
    sched_final: the new call (gains and phases) with a cotangent of the final state only;
    vjp_final:   the shipped mbfir.bloch_train_vjp_batch (b1) on the same inputs;
    fd_final:    the batched central difference of the same loss: per period 2 ntr perturbed trains per variable (gains, phases), one
                 repetition moved at a time, all of them in one mbfir.bloch_train_batch call (final=True; it returns the echoes too, as
                 it always does), and the loss and the quotients on the host (inside the timed region: they are part of getting
                 the same numbers).  --fd-chunk bounds the perturbed repetitions per call (`long` returns 100 MB of echoes per
                 train: a caller with finite memory has to do the same); the chunks' times are added up;
    sched_all, vjp_all: the two adjoints with cotangents on every echo and on the final state.
The largest difference between the new call and the central difference is reported relative to the largest entry.  Times are warm
host clocks around calls that end in a stream synchronise (transfers included).  One JSON line per workload.

    python tools/gpu_blochtrainsched.py [--workload batch64|long] [--reps 10] [--fd-reps 2] [--fd-chunk 64]
    python tools/gpu_blochtrainsched.py --workload long --fd-reps 1 --fd-chunk 8          # 32 trains, 3.2 GB of echoes, per call
    python tools/gpu_blochtrainsched.py --rocprof DIR --workload batch64 [--reps 10]

The second form runs each of sched_final, vjp_final and fd_final in a child of its own under `rocprofv3 --kernel-trace --stats -d
DIR/<call>` (nothing else traced, no counters in that run) and adds, per call, the kernel time summed over its launches and divided
by the number of calls, and the mean per kernel.
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

fwd.KERNELS = ("k_bloch_train_prop_dgain", "k_bloch_train_run_sched", "k_bloch_train_sched_fold", "k_bloch_train_prop_vjp",
               "k_bloch_train_run_vjp", "k_bloch_train_vjp_fold", "k_bloch_train_prop", "k_bloch_train_run")
TRACED = ("sched_final", "vjp_final", "fd_final")
FD_ANGLE = 1e-5


def measure(W, reps, fd_reps, fd_chunk, only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(1)
    pulses, df, dp, ntr, echo = W["pulses"], W["df"], W["dp"], W["ntr"], W["echo"]
    ph, gn = W["phases"], W["gains"]
    nf, npos, P = len(df), len(dp), len(pulses)
    cf = [tuple(rng.standard_normal((3, 1, nf, npos))) for _ in range(P)]
    ce = [tuple(rng.standard_normal((3, 1, ntr, nf, npos))) for _ in range(P)]
    kw = dict(phases=ph, gains=gn, echo=echo, ctx=ctx)
    # a repetition turns by FD_ANGLE more or less: the step of tests/blochtrainsched_ref.py
    hg = [FD_ANGLE / (mbfir.GAMMA_C13 * (np.abs(p[0]) * p[2]).sum()) for p in pulses]

    def sched_final():
        return mbfir.bloch_train_vjp_sched_batch(pulses, df, dp, ntr, None, cot_final=cf, **kw)

    def vjp_final():
        return mbfir.bloch_train_vjp_batch(pulses, df, dp, ntr, None, cot_final=cf, **kw)

    def fd_final():
        gg, gp = np.zeros((P, ntr)), np.zeros((P, ntr))
        for k0 in range(0, ntr, fd_chunk):
            ks = range(k0, min(k0 + fd_chunk, ntr))
            moved, gains, phases = [], [], []
            for q, p in enumerate(pulses):
                for k in ks:
                    e = np.zeros(ntr)
                    e[k] = 1.0
                    moved += [p] * 4
                    gains += [gn + hg[q] * e, gn - hg[q] * e, gn, gn]
                    phases += [ph, ph, ph + FD_ANGLE * e, ph - FD_ANGLE * e]
            res = mbfir.bloch_train_batch(moved, df, dp, ntr, phases=phases, gains=gains, echo=echo, final=True, ctx=ctx)
            i = 0
            for q in range(P):
                for k in ks:
                    L = [sum(float((c * f).sum()) for c, f in zip(cf[q], res[i + j][1])) for j in range(4)]
                    gg[q, k], gp[q, k] = (L[0] - L[1]) / (2 * hg[q]), (L[2] - L[3]) / (2 * FD_ANGLE)
                    i += 4
        return gg, gp

    def sched_all():
        return mbfir.bloch_train_vjp_sched_batch(pulses, df, dp, ntr, ce, cot_final=cf, **kw)

    def vjp_all():
        return mbfir.bloch_train_vjp_batch(pulses, df, dp, ntr, ce, cot_final=cf, **kw)
    calls = dict(sched_final=(sched_final, reps), vjp_final=(vjp_final, reps), fd_final=(fd_final, fd_reps), sched_all=(sched_all, reps),
                 vjp_all=(vjp_all, reps))
    if only:
        calls = {only: calls[only]}
    for k, (fn, _) in calls.items():
        if k != "fd_final":                                             # the difference is many calls: its first warms the rest
            fn()
    acc, last = {k: [] for k in calls}, {}
    for r in range(max(c for _, c in calls.values())):
        for k, (fn, cnt) in calls.items():
            if r < cnt:
                t0 = time.perf_counter()
                last[k] = fn()
                acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainsched", workload=W["name"], periods=P, samples=W["n"], repetitions=ntr, nf=nf, npos=npos, reps=reps,
               fd_reps=fd_reps, fd_chunk=fd_chunk, fd_trains=4 * ntr * P, calls={k: c + (k != "fd_final") for k, (_, c) in calls.items()})
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not only:
        a, (fg, fp) = last["sched_final"], last["fd_final"]
        row["fd_over_sched"] = row["ms_fd_final"] / row["ms_sched_final"]
        row["vjp_over_sched_final"] = row["ms_vjp_final"] / row["ms_sched_final"]
        row["vjp_over_sched_all"] = row["ms_vjp_all"] / row["ms_sched_all"]
        row["sched_vs_fd_rel_gains"] = max(float(np.abs(u[0] - v).max() / np.abs(v).max()) for u, v in zip(a, fg))
        row["sched_vs_fd_rel_phases"] = max(float(np.abs(u[1] - v).max() / np.abs(v).max()) for u, v in zip(a, fp))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fd-reps", type=int, default=2)
    ap.add_argument("--fd-chunk", type=int, default=64, help="perturbed repetitions per bloch_train_batch call of the difference")
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR/<call>")
    ap.add_argument("--only", choices=TRACED + ("sched_all", "vjp_all"), help="time this call alone (what a traced child runs)")
    a = ap.parse_args()
    names = a.workload or ["batch64", "long"]
    if not a.rocprof:
        for name in names:
            print(json.dumps(measure(fwd.workload(name), a.reps, min(a.reps, a.fd_reps), a.fd_chunk, a.only)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    out = dict(tool="gpu_blochtrainsched", workload=names[0], traced=True, kernel_ms_per_call={}, kernels={})
    for call in TRACED:                                     # each traced program is a fresh child: this process never opens the GPU
        d = os.path.join(a.rocprof, call)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "blochtrainsched", "--", sys.executable, os.path.abspath(__file__),
               "--workload", names[0], "--reps", str(a.reps), "--fd-reps", str(a.fd_reps), "--fd-chunk", str(a.fd_chunk), "--only", call]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
        row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        means = fwd.kernel_means(d) or {}
        out["kernels"][call] = means
        out["kernel_ms_per_call"][call] = sum(v["launches"] * v["mean_us"] for v in means.values()) / 1e3 / row["calls"][call]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
