"""Cost of the fused least-squares products of the Bloch simulator (mbfir.bloch_lsq_batch, mbfir.bloch_gn_batch at K = 1) against the
two-call paths of the same build that they replace, on the case of tools/gpu_blochgrad.py: a 600-sample, 26 ms H-1 pulse at T1 = 1 s,
T2 = 40 ms on 2048 frequencies x 8 positions at 3 transmit-gain scales (192 workgroups).
    lsq       against  bloch_batch + the NumPy residual and loss + bloch_vjp_batch
    gn, K = 1 against  bloch_jvp_batch + the NumPy weights + bloch_vjp_batch
Times are warm host clocks around calls that end in a stream synchronise (transfers and the NumPy work between the calls included);
the four alternate, the minimum and the median of --reps each.  One JSON line.

    python tools/gpu_blochgn.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(reps):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(0)
    n, dur, nf, npos, sc = 600, 26e-3, 2048, 8, (0.9, 1.0, 1.1)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (2.0 / (mbfir.GAMMA_H1 * dur))
    pulses = [(b1, rng.uniform(0.5, 1.5, n) * 0.01, dur / n, 1.0, 40e-3, "H-1")]
    df, dp = np.linspace(-1000, 1000, nf), np.linspace(-2, 2, npos)
    w = tuple(rng.uniform(0, 1, (3, len(sc), nf, npos)))
    t = tuple(rng.uniform(-1, 1, (3, len(sc), nf, npos)))
    v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(b1).max()

    def lsq():
        return mbfir.bloch_lsq_batch(pulses, df, dp, [t], [w], scales=sc, ctx=ctx)[0]

    def lsq2():
        m, = mbfir.bloch_batch(pulses, df, dp, scales=sc, ctx=ctx)
        r = [m[c] - t[c] for c in range(3)]
        L = 0.5 * sum(float((w[c] * r[c] * r[c]).sum()) for c in range(3))
        g, = mbfir.bloch_vjp_batch(pulses, df, dp, [tuple(w[c] * r[c] for c in range(3))], scales=sc, ctx=ctx)
        return L, g

    def gn():
        return mbfir.bloch_gn_batch(pulses, df, dp, [v], [w], scales=sc, ctx=ctx)[0]

    def gn2():
        (_, dm), = mbfir.bloch_jvp_batch(pulses, df, dp, [v], scales=sc, ctx=ctx)
        return mbfir.bloch_vjp_batch(pulses, df, dp, [tuple(w[c] * dm[c] for c in range(3))], scales=sc, ctx=ctx)[0]
    fns = (("lsq", lsq), ("lsq_two_calls", lsq2), ("gn", gn), ("gn_two_calls", gn2))
    first = {k: f() for k, f in fns}
    agree = dict(loss=abs(first["lsq"][0] - first["lsq_two_calls"][0]) / abs(first["lsq_two_calls"][0]),
                 grad=float(np.abs(first["lsq"][1] - first["lsq_two_calls"][1]).max() / np.abs(first["lsq_two_calls"][1]).max()),
                 gn=float(np.abs(first["gn"] - first["gn_two_calls"]).max() / np.abs(first["gn_two_calls"]).max()))
    acc = {k: [] for k, _ in fns}
    for _ in range(reps):
        for k, f in fns:
            t0 = time.perf_counter()
            f()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(tool="gpu_blochgn", samples=n, nf=nf, npos=npos, scales=len(sc), workgroups=len(sc) * nf * npos // 256, reps=reps,
               relative_difference=agree)
    for k, _ in fns:
        row["ms_" + k] = min(acc[k])
        row["ms_" + k + "_median"] = float(np.median(acc[k]))
    row["speedup_lsq"] = row["ms_lsq_two_calls"] / row["ms_lsq"]
    row["speedup_gn"] = row["ms_gn_two_calls"] / row["ms_gn"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    print(json.dumps(measure(ap.parse_args().reps)))


if __name__ == "__main__":
    main()
