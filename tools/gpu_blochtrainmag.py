"""Cost of the magnitude fits of the pulse train (magnitude=True on mbfir.bloch_train_lsq_batch, bloch_train_gn_batch,
bloch_train_lm_step_batch, their _sched twins and the train refiners) on the two workloads of tools/gpu_blochtrain.py:
    batch64: 64 periods of 64 samples x 64 repetitions on 85 frequencies x 1 position;
    long:    one period of 600 samples x 256 repetitions on 2048 x 8 = 16384 points.
Point-sized planes used at every repetition (the broadcast form), the first 8 echoes left out, demodulated echoes.  Three comparisons
per workload and chain (b1: the period's samples; sched: the gains and phases), all in one session:
    twins:   each magnitude call against its component twin (same staging, same launches: the difference is the walk kernel's)
    routes:  the fused magnitude lsq and gn (K = 1) against the shipped two-call paths they replace: the forward call or the tangent,
             the NumPy seed over the echoes, then the adjoint; the component twins run in the same rotation, so that what a fused
             call pays for coming after a two-call path (echo-sized transfers and arrays) shows on both: the magnitude call
             follows the route in the rotation, or with --twin-first the component twin does
    solvers: one Levenberg-Marquardt iterate of the refiner with magnitude=True, solver="device" against solver="host"
Times are warm host clocks around calls that end in a stream synchronise (transfers and the NumPy between the calls included); the
calls of a comparison alternate; the minimum, the median and the spread (max - min) / min of --reps each.  One JSON line per workload
and chain.

    timeout -k 10 600 python tools/gpu_blochtrainmag.py --workload batch64 --reps 10 && \\
    timeout -k 10 900 python tools/gpu_blochtrainmag.py --workload long --reps 10
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_blochtrain as fwd  # noqa: E402


def clock(fns, reps):
    for _, f in fns:
        f()
    acc = {k: [] for k, _ in fns}
    for _ in range(reps):
        for k, f in fns:
            t0 = time.perf_counter()
            f()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(ms=min(v), median=float(np.median(v)), spread=(max(v) - min(v)) / min(v)) for k, v in acc.items()}


def direction(ex, ey):
    rho = np.sqrt(ex * ex + ey * ey)
    safe = np.where(rho > 0, rho, 1.0)
    return rho, np.where(rho > 0, ex / safe, 0.0), np.where(rho > 0, ey / safe, 0.0)


def measure(W, chain, reps, twin_first=False):
    import mbfir
    ctx = mbfir.get_context()
    rng = np.random.default_rng(3)
    pulses, df, dp, ntr, n = W["pulses"], W["df"], W["dp"], W["ntr"], W["n"]
    P, nf, npos = len(pulses), len(df), len(dp)
    rw = np.append(np.zeros(8), np.ones(ntr - 8))
    r4 = rw[None, :, None, None]
    w3 = [tuple(rng.uniform(0, 1, (1, nf, npos)) for _ in range(3)) for _ in range(P)]
    w2 = [(w[0], w[2]) for w in w3]
    t2 = [(rng.uniform(0, 1, (1, nf, npos)), rng.uniform(-1, 1, (1, nf, npos))) for _ in range(P)]
    t3 = [(t[0], t[0], t[1]) for t in t2]
    kw = dict(phases=W["phases"], gains=W["gains"], echo=W["echo"], demod=True, ctx=ctx)
    fkw = dict(kw, rep_weights=rw)
    mu = [1e-3] * P
    mag = dict(magnitude=True)
    if chain == "b1":
        v = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(p[0]).max() for p in pulses]
        lsq = lambda t, w, **m: mbfir.bloch_train_lsq_batch(pulses, df, dp, ntr, t, w, **fkw, **m)
        gn = lambda w, **m: mbfir.bloch_train_gn_batch(pulses, df, dp, ntr, v, w, **fkw, **m)
        lm = lambda t, w, **m: mbfir.bloch_train_lm_step_batch(pulses, df, dp, ntr, v, w, mu, targets=t, cg=4, rtol=0.0, **fkw, **m)
        jvp = lambda: mbfir.bloch_train_jvp_batch(pulses, df, dp, ntr, v, **kw)
        vjp = lambda ce: mbfir.bloch_train_vjp_batch(pulses, df, dp, ntr, ce, **kw)
        refine = lambda solver: mbfir.refine_bloch_train_lm_batch(pulses, df, dp, ntr, t2, w2, solver=solver, iters=1, cg=4, **fkw, **mag)
    else:
        dg, dph = [rng.standard_normal(ntr) for _ in range(P)], [rng.standard_normal(ntr) for _ in range(P)]
        lsq = lambda t, w, **m: mbfir.bloch_train_lsq_sched_batch(pulses, df, dp, ntr, t, w, **fkw, **m)
        gn = lambda w, **m: mbfir.bloch_train_gn_sched_batch(pulses, df, dp, ntr, w, tangents_gains=dg, tangents_phases=dph, **fkw, **m)
        lm = lambda t, w, **m: mbfir.bloch_train_lm_step_sched_batch(pulses, df, dp, ntr, w, mu, targets=t, cg=4, rtol=0.0, **fkw, **m)
        jvp = lambda: mbfir.bloch_train_jvp_sched_batch(pulses, df, dp, ntr, tangents_gains=dg, tangents_phases=dph, **kw)
        vjp = lambda ce: mbfir.bloch_train_vjp_sched_batch(pulses, df, dp, ntr, ce, **kw)
        refine = lambda solver: mbfir.refine_bloch_train_sched_lm_batch(pulses, df, dp, ntr, t2, w2, solver=solver, iters=1, cg=2 * ntr,
                                                                        **fkw, **mag)

    def lsq_route():
        seeds, L = [], []
        for e, t, w in zip(mbfir.bloch_train_batch(pulses, df, dp, ntr, **kw), t2, w2):
            rho, ux, uy = direction(e[0], e[1])
            r, rz = rho - t[0][:, None], e[2] - t[1][:, None]
            a, b = r4 * w[0][:, None], r4 * w[1][:, None]
            L.append(0.5 * float((a * r * r).sum() + (b * rz * rz).sum()))
            seeds.append((a * r * ux, a * r * uy, b * rz))
        return L, vjp(seeds)

    def gn_route():
        E = mbfir.bloch_train_batch(pulses, df, dp, ntr, **kw)
        seeds = []
        for e, de, w in zip(E, jvp(), w2):
            _, ux, uy = direction(e[0], e[1])
            d = [x[0] if x.ndim == 5 else x for x in de]                                      # one direction
            a = ux * d[0] + uy * d[1]
            seeds.append((r4 * w[0][:, None] * a * ux, r4 * w[0][:, None] * a * uy, r4 * w[1][:, None] * d[2]))
        return vjp(seeds)
    row = dict(tool="gpu_blochtrainmag", workload=W["name"], chain=chain, pulses=P, samples=n, ntr=ntr, points=nf * npos, reps=reps)
    row["twins"] = clock((("lsq_mag", lambda: lsq(t2, w2, **mag)), ("lsq", lambda: lsq(t3, w3)),
                          ("gn_mag", lambda: gn(w2, **mag)), ("gn", lambda: gn(w3)),
                          ("lm_mag", lambda: lm(t2, w2, **mag)), ("lm", lambda: lm(t3, w3))), reps)
    routes = [("lsq_mag", lambda: lsq(t2, w2, **mag)), ("lsq", lambda: lsq(t3, w3)), ("lsq_route", lsq_route),
              ("gn_mag", lambda: gn(w2, **mag)), ("gn", lambda: gn(w3)), ("gn_route", gn_route)]
    if twin_first:                                                        # the component twin is the call that follows a route
        routes = [routes[k] for k in (1, 0, 2, 4, 3, 5)]
    row["routes"] = clock(routes, reps)
    row["twin_first"] = twin_first
    row["solvers"] = clock((("device", lambda: refine("device")), ("host", lambda: refine("host"))), max(3, reps // 3))
    a, (Lb, gb) = lsq(t2, w2, **mag)[0], (lambda r: (r[0][0], r[1][0]))(lsq_route())
    ga, gb = np.concatenate([np.ravel(x) for x in a[1:]]), np.concatenate([np.ravel(x) for x in (gb if isinstance(gb, tuple) else (gb,))])
    row["lsq_vs_route_rel"] = max(abs(a[0] - Lb) / abs(Lb), float(np.abs(ga - gb).max() / np.abs(gb).max()))
    ha, hb = gn(w2, **mag)[0], gn_route()[0]
    ha, hb = [np.concatenate([np.ravel(x) for x in (h if isinstance(h, tuple) else (h,))]) for h in (ha, hb)]
    row["gn_vs_route_rel"] = float(np.abs(ha - hb).max() / np.abs(hb).max())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workload", choices=("batch64", "long", "both"), default="both")
    ap.add_argument("--chain", choices=("b1", "sched", "both"), default="both")
    ap.add_argument("--twin-first", action="store_true", help="routes: the component twin, not the magnitude call, follows a route")
    a = ap.parse_args()
    for name in (("batch64", "long") if a.workload == "both" else (a.workload,)):
        W = fwd.workload(name)
        for chain in (("b1", "sched") if a.chain == "both" else (a.chain,)):
            print(json.dumps(measure(W, chain, a.reps, a.twin_first)), flush=True)


if __name__ == "__main__":
    main()
