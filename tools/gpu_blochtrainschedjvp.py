"""Cost of the train's tangent in its schedule (mbfir.bloch_train_jvp_sched_batch) on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
Calls timed, alternating, the minimum and the median of --reps each (--fd-reps for the central differences, which are slow):
    jvp_k1, jvp_k8: the new call with 1 and with 8 dense directions (gains and phases), tangent echoes wanted;
    jac_final:      the new call with the 2 ntr unit directions, echoes=False, final=True: the whole Jacobian of the final state (on
                    `long` the tangent echoes of 512 directions would be about 50 GB and are not asked for);
    fd_k1, fd_k8:   the central difference that jvp_k1 / jvp_k8 replace: two perturbed trains per direction and period, all of them in
                    one mbfir.bloch_train_batch call, and the quotient on the host (inside the timed region: it is part of getting
                    the same numbers);
    adj_final:      one mbfir.bloch_train_vjp_sched_batch call with a cotangent of the final state, as context: a final-state loss
                    needs one such call per row, the Jacobian has 3 x points rows and 2 ntr columns.
The largest difference between jvp_k1 and fd_k1 is reported relative to the largest entry.  Times are warm host clocks around calls
that end in a stream synchronise (transfers included).  One JSON line per workload.

    python tools/gpu_blochtrainschedjvp.py [--workload batch64|long] [--reps 5] [--fd-reps 2]
    python tools/gpu_blochtrainschedjvp.py --rocprof DIR --workload batch64 [--reps 5]

The second form runs each of jvp_k1, jvp_k8 and jac_final in a child of its own under `rocprofv3 --kernel-trace --stats -d
DIR/<call>` (nothing else traced, no counters in that run) and adds, per call, the kernel time summed over its launches and divided
by the number of calls, the same per direction, and the mean per kernel.
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

fwd.KERNELS = ("k_bloch_train_run_sched_jvp", "k_bloch_train_prop_dgain", "k_bloch_train_prop", "k_bloch_train_run")
TRACED = ("jvp_k1", "jvp_k8", "jac_final")
FD_ANGLE = 1e-5


def measure(W, reps, fd_reps, only):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(1)
    pulses, df, dp, ntr, echo = W["pulses"], W["df"], W["dp"], W["ntr"], W["echo"]
    ph, gn = W["phases"], W["gains"]
    nf, npos, P = len(df), len(dp), len(pulses)
    dg, dph = rng.standard_normal((P, 8, ntr)), rng.standard_normal((P, 8, ntr))
    cf = [tuple(rng.standard_normal((3, 1, nf, npos))) for _ in range(P)]
    kw = dict(phases=ph, gains=gn, echo=echo, ctx=ctx)
    # no repetition turns by more than FD_ANGLE: the step of tests/blochtrainschedjvp_ref.py
    theta = [mbfir.GAMMA_C13 * (np.abs(p[0]) * p[2]).sum() for p in pulses]
    h = [[FD_ANGLE / float((np.abs(dg[q, k]) * theta[q] + np.abs(dph[q, k])).max()) for k in range(8)] for q in range(P)]

    def jvp(K):
        return mbfir.bloch_train_jvp_sched_batch(pulses, df, dp, ntr, tangents_gains=list(dg[:, :K]), tangents_phases=list(dph[:, :K]),
                                                 **kw)

    def jac_final():
        return mbfir.bloch_train_jacobian_sched_batch(pulses, df, dp, ntr, echoes=False, final=True, **kw)

    def fd(K):
        moved, gains, phases = [], [], []
        for q, p in enumerate(pulses):
            for k in range(K):
                moved += [p] * 2
                gains += [gn + h[q][k] * dg[q, k], gn - h[q][k] * dg[q, k]]
                phases += [ph + h[q][k] * dph[q, k], ph - h[q][k] * dph[q, k]]
        res = mbfir.bloch_train_batch(moved, df, dp, ntr, phases=phases, gains=gains, echo=echo, ctx=ctx)
        out = []
        for q in range(P):
            rows = [tuple((a - b) / (2 * h[q][k]) for a, b in zip(res[2 * (q * K + k)], res[2 * (q * K + k) + 1])) for k in range(K)]
            out.append(tuple(np.stack([r[i] for r in rows]) for i in range(3)))
        return out

    def adj_final():
        return mbfir.bloch_train_vjp_sched_batch(pulses, df, dp, ntr, None, cot_final=cf, **kw)
    calls = dict(jvp_k1=(lambda: jvp(1), reps), jvp_k8=(lambda: jvp(8), reps), jac_final=(jac_final, reps), fd_k1=(lambda: fd(1), fd_reps),
                 fd_k8=(lambda: fd(8), fd_reps), adj_final=(adj_final, reps))
    if only:
        calls = {only: calls[only]}
    for fn, _ in calls.values():
        fn()
    acc, last = {k: [] for k in calls}, {}
    for r in range(max(c for _, c in calls.values())):
        for k, (fn, cnt) in calls.items():
            if r < cnt:
                t0 = time.perf_counter()
                last[k] = fn()
                acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochtrainschedjvp", workload=W["name"], periods=P, samples=W["n"], repetitions=ntr, nf=nf, npos=npos, reps=reps,
               fd_reps=fd_reps, group=mbfir.bloch_train_sched_jvp_group(), directions=dict(jvp_k1=1, jvp_k8=8, jac_final=2 * ntr),
               calls={k: c + 1 for k, (_, c) in calls.items()})
    for k, t in acc.items():
        row["ms_" + k] = min(t)
        row["ms_" + k + "_median"] = float(np.median(t))
    if not only:
        row["fd_over_jvp_k1"] = row["ms_fd_k1"] / row["ms_jvp_k1"]
        row["fd_over_jvp_k8"] = row["ms_fd_k8"] / row["ms_jvp_k8"]
        row["ms_jac_final_per_direction"] = row["ms_jac_final"] / (2 * ntr)
        row["ms_adj_final_times_ntr"] = row["ms_adj_final"] * ntr
        row["jvp_vs_fd_rel"] = max(float(np.abs(a - b).max() / np.abs(b).max())
                                   for u, v in zip(last["jvp_k1"], last["fd_k1"]) for a, b in zip(u, v))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("batch64", "long"), action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fd-reps", type=int, default=2)
    ap.add_argument("--rocprof", metavar="DIR", help="run under rocprofv3 --kernel-trace --stats, output in DIR/<call>")
    ap.add_argument("--only", choices=TRACED + ("fd_k1", "fd_k8", "adj_final"), help="time this call alone (what a traced child runs)")
    a = ap.parse_args()
    names = a.workload or ["batch64", "long"]
    if not a.rocprof:
        for name in names:
            print(json.dumps(measure(fwd.workload(name), a.reps, min(a.reps, a.fd_reps), a.only)), flush=True)
        return
    if len(names) != 1:
        raise SystemExit("--rocprof takes one --workload: a kernel's mean is then over one configuration")
    out = dict(tool="gpu_blochtrainschedjvp", workload=names[0], traced=True, kernel_ms_per_call={}, kernel_ms_per_direction={}, kernels={})
    for call in TRACED:                                     # each traced program is a fresh child: this process never opens the GPU
        d = os.path.join(a.rocprof, call)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "blochtrainschedjvp", "--", sys.executable,
               os.path.abspath(__file__), "--workload", names[0], "--reps", str(a.reps), "--only", call]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
        row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        means = fwd.kernel_means(d) or {}
        out["kernels"][call] = means
        out["kernel_ms_per_call"][call] = sum(v["launches"] * v["mean_us"] for v in means.values()) / 1e3 / row["calls"][call]
        out["kernel_ms_per_direction"][call] = out["kernel_ms_per_call"][call] / row["directions"][call]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
