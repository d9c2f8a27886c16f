"""Cost of the schedule's Levenberg-Marquardt step evaluated and solved on the device (mbfir.bloch_train_lm_step_sched_batch,
mbfir.refine_bloch_train_sched_lm_batch) against the host path, on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points,
each with two schedules: 'two', the shipped one (gains 0.5, 1, 1, ...: two distinct gains), and 'ramp', ntr distinct gains on a smooth
ramp, which is what a refinement sees after its first accepted step on the gains.  Timed alternating, the minimum and the median of
--reps each, warm host clocks around calls that end in a stream synchronise (transfers included):
    fused:        one bloch_train_lm_step_sched_batch call with targets at cg = --cg (b = -g on the device);
    gn_lsq:       bloch_train_gn_sched_batch with the n = 2 ntr unit directions plus bloch_train_lsq_sched_batch: what the host solver
                  pays per accepted iterate on the device;
    host_k, device_k: refine_bloch_train_sched_lm_batch with solver='host' / 'device' at iters = 1 and 3; an accepted iterate is
                  (iters 3 - iters 1) / 2 (the JSON line has the refused steps: the figure is an iterate's only where none was).
One JSON line per (workload, schedule).

    timeout -k 10 600 python tools/gpu_blochtrainschedlm.py --workload batch64 --reps 3 && \\
    timeout -k 10 900 python tools/gpu_blochtrainschedlm.py --workload long --reps 3 && \\
    timeout -k 10 900 python tools/gpu_blochtrainschedlm.py --rocprof DIR --what counts --workload batch64 && \\
    timeout -k 10 900 python tools/gpu_blochtrainschedlm.py --rocprof DIR2 --what sweeps --workload long

Every step that opens the GPU runs under its own time limit and the steps are chained with &&.  --rocprof runs fresh children under
`timeout -k 10 <limit> rocprofv3 --kernel-trace --stats` (nothing else traced, no counters): 'counts' one child per (solver, iters in
1, 3) on the ramp schedule and reports the launches of k_bloch_train_prop and k_bloch_train_prop_dgain per accepted iterate; 'sweeps'
one child that repeats the fused call on the ramp schedule and reports the mean kernel times."""
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

fwd.KERNELS = ("k_bloch_train_lm_sched_init", "k_bloch_train_lm_sched_run", "k_bloch_train_lm_sched_step", "k_bloch_train_run_sched_lsq",
               "k_bloch_train_run_sched_gn", "k_bloch_train_sched_gn_fold", "k_bloch_train_prop_dgain", "k_bloch_train_prop")


def setup(W, schedule):
    rng = np.random.default_rng(2)
    P, nf, npos, ntr = len(W["pulses"]), len(W["df"]), len(W["dp"]), W["ntr"]
    rw = np.append(np.zeros(8), np.ones(ntr - 8))                       # the first echoes of the transient left out
    wb = [tuple(rng.uniform(0, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    tb = [tuple(rng.uniform(-1, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    gains = W["gains"] if schedule == "two" else np.linspace(0.5, 1.0, ntr)
    return rw, wb, tb, gains


def measure(W, schedule, reps, cg, parts):
    import mbfir
    ctx = mbfir.get_context()
    pulses, df, dp, ntr = W["pulses"], W["df"], W["dp"], W["ntr"]
    P = len(pulses)
    rw, wb, tb, gains = setup(W, schedule)
    kw = dict(phases=W["phases"], gains=gains, echo=W["echo"], demod=True, ctx=ctx)
    eye, zero = np.eye(ntr), np.zeros((ntr, ntr))
    ug, up = [np.concatenate([eye, zero])] * P, [np.concatenate([zero, eye])] * P
    last = {}

    def fused():
        return mbfir.bloch_train_lm_step_sched_batch(pulses, df, dp, ntr, wb, 1.0, targets=tb, rep_weights=rw, cg=cg, rtol=0.0, **kw)

    def gn_lsq():
        mbfir.bloch_train_gn_sched_batch(pulses, df, dp, ntr, wb, tangents_gains=ug, tangents_phases=up, rep_weights=rw, **kw)
        return mbfir.bloch_train_lsq_sched_batch(pulses, df, dp, ntr, tb, wb, rep_weights=rw, **kw)

    def refine(solver, iters):
        def run():
            last[solver, iters] = mbfir.refine_bloch_train_sched_lm_batch(pulses, df, dp, ntr, tb, wb, rep_weights=rw, iters=iters,
                                                                          solver=solver, cg=cg, **kw)[1]
        return run
    calls = dict(fused=fused, gn_lsq=gn_lsq)
    for solver in ("host", "device"):
        for iters in (1, 3):
            calls["%s_%d" % (solver, iters)] = refine(solver, iters)
    calls = {k: v for k, v in calls.items() if k in parts}
    for fn in calls.values():
        fn()
    acc = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainschedlm", workload=W["name"], schedule=schedule, distinct_gains=len(np.unique(gains)), periods=P,
               samples=W["n"], repetitions=ntr, nf=len(df), npos=len(dp), reps=reps, cg=cg)
    for k, t in acc.items():
        if t:
            row["ms_" + k] = min(t)
            row["ms_" + k + "_median"] = float(np.median(t))
    for (solver, iters), infos in last.items():
        row["%s_%d_run" % (solver, iters)] = dict(refused=[i["refused"] for i in infos][:4], steps=[len(i["losses"]) - 1 for i in infos][:4],
                                                  calls=infos[0]["calls"], losses=infos[0]["losses"])
    if "ms_fused" in row and "ms_gn_lsq" in row:
        row["gn_lsq_over_fused"] = row["ms_gn_lsq"] / row["ms_fused"]
    for solver in ("host", "device"):
        if "ms_%s_3" % solver in row and "ms_%s_1" % solver in row:
            row["ms_%s_iterate" % solver] = (row["ms_%s_3" % solver] - row["ms_%s_1" % solver]) / 2
            row["ms_%s_iterate_median" % solver] = (row["ms_%s_3_median" % solver] - row["ms_%s_1_median" % solver]) / 2
    if "ms_host_iterate" in row and "ms_device_iterate" in row:
        row["host_over_device_iterate"] = row["ms_host_iterate"] / row["ms_device_iterate"]
    return row


def traced(d, limit, args):
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "blochtrainschedlm", "--",
           sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    row["traced"] = True                                    # host clocks under the tracer are not end-to-end figures
    row["kernels"] = fwd.kernel_means(d)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--schedule", choices=("two", "ramp"), action="append")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cg", type=int, default=8)
    ap.add_argument("--parts", default="fused,gn_lsq,host_1,host_3,device_1,device_3", help="which calls to time, comma separated")
    ap.add_argument("--rocprof", metavar="DIR", help="run children under rocprofv3 --kernel-trace --stats, output under DIR")
    ap.add_argument("--what", choices=("counts", "sweeps"), default="counts")
    ap.add_argument("--limit", type=int, default=300, help="seconds a traced child may take (timeout -k 10)")
    a = ap.parse_args()
    names, scheds, parts = a.workload or ["batch64", "long"], a.schedule or ["two", "ramp"], a.parts.split(",")
    if not a.rocprof:
        for name in names:
            for s in scheds:
                print(json.dumps(measure(fwd.workload(name), s, a.reps, a.cg, parts)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    # the traced programs are fresh children under their own time limits: this process never opens the GPU
    base = ["--workload", names[0], "--schedule", "ramp", "--cg", str(a.cg)]
    if a.what == "sweeps":
        print(json.dumps(traced(a.rocprof, a.limit, base + ["--reps", str(a.reps), "--parts", "fused"])))
        return
    out = dict(tool="gpu_blochtrainschedlm", what="counts", workload=names[0], schedule="ramp")
    for solver in ("host", "device"):
        n = {}
        for iters in (1, 3):
            row = traced(os.path.join(a.rocprof, "%s_%d" % (solver, iters)), a.limit, base + ["--reps", "0", "--parts", "%s_%d" % (solver, iters)])
            n[iters] = {k: v["launches"] for k, v in (row["kernels"] or {}).items()}
            out["%s_%d_run" % (solver, iters)] = row.get("%s_%d_run" % (solver, iters))
            out["%s_%d_launches" % (solver, iters)] = n[iters]
        for k in ("k_bloch_train_prop", "k_bloch_train_prop_dgain"):
            out["%s_%s_per_iterate" % (solver, k)] = (n[3].get(k, 0) - n[1].get(k, 0)) / 2
    print(json.dumps(out))


if __name__ == "__main__":
    main()
