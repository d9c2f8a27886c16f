"""Batched device simulators against loops of single-pulse calls: one JSON line.
  sim_rf_scale  the two pulses of examples/specsat_minripple_c13.py at its five transmit gains: one sim_rf_scale_batch call against
                two sim_rf_scale calls (ten bloch calls)
  schedule      the 80-pulse flyback schedule of tools/gpu_ssmb_batch.py on the x x df grid of tests/test_ssmb_gpu.py (7 points per
                band x 241 positions): one bloch_batch call against 80 bloch calls
  abr           256 dzrf_batch pulses x 5 scales x 4000 points: one abr_batch call against 1280 abrm calls
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the minimum of --reps.

    python tools/gpu_sim_batch.py [--reps 3]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mbfir  # noqa: E402

SCALES = [0.8, 0.9, 1.0, 1.1, 1.2]


def best(fn, reps):
    fn()                                                   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), out


def trap(n, ramp, amp):
    t = np.full(n, float(amp))
    t[:ramp] = amp * (np.arange(ramp) + 0.5) / ramp
    t[n - ramp:] = t[:ramp][::-1]
    return t


def compare(batch, loop):
    """largest |batch - loop| over matching arrays, and whether they are bit-identical"""
    worst, same = 0.0, True
    for b, s in zip(batch, loop):
        worst = max(worst, float(np.abs(np.asarray(b) - np.asarray(s)).max()))
        same = same and np.array_equal(b, s)
    return worst, same


def specsat_pulses():
    """the two pulses of examples/specsat_minripple_c13.py: the multiband ap pulse and dzrf's 'sat' 'max' pulse (Gauss)"""
    B0, n, T, FA, d1, d2, gamma = 3.0, 150, 10.0, 90.0, 0.05, 1e-3, 1.0705
    cf = mbfir.spec.spectrum_c13(B0)[[2, 1]]
    mb_cf = list((cf - cf[0]) * 1e-3)
    dt = T / n
    if abs(dt / 4e-3 - round(dt / 4e-3)) > 1e-9:
        dt = 4e-3 * math.floor(dt / 4e-3)
        T = n * dt
    rf, _, rf_spec, _ = mbfir.dzrf_mb(n, dt, mb_cf, [0.05, 0.05], [FA, 0], [d1, d2], "sat", "ap_minstopripple_cvx", "C-13", 0, 1,
                                      1e-3, 0)
    rf2 = mbfir.dzrf(n, T * 0.25, "sat", "max", d1, 0.5 * d2)
    rf2 = mbfir.rfscaleg(rf2 * (FA * math.pi / 180) / np.sum(rf2), T, gamma)
    return [rf, rf2], dt, np.asarray(rf_spec["f"]) * (1 / dt) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = mbfir.get_context()
    out = {"tool": "gpu_sim_batch", "cases": []}

    def emit(row):
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    pulses, dt, f = specsat_pulses()
    ms_b, rb = best(lambda: mbfir.sim_rf_scale_batch(pulses, dt, SCALES, "C-13", f=f, ctx=ctx), a.reps)
    ms_l, rl = best(lambda: [mbfir.sim_rf_scale(p, dt, SCALES, "C-13", f=f, ctx=ctx) for p in pulses], a.reps)
    d, same = compare([v for r in rb for v in r[1:]], [v for r in rl for v in r[1:]])
    emit(dict(case="sim_rf_scale", pulses=len(pulses), ntime=[len(p) for p in pulses], scales=len(SCALES), nf=2048, ms_batch=ms_b,
              ms_loop=ms_l, speedup=ms_l / ms_b, max_abs_diff=d, bit_identical=same))

    cs = mbfir.spec.spectrum_c13(3.0) * 1e-3
    bands = [cs[4], cs[0], cs[2], cs[1]]                   # bicarbonate, pyruvate, alanine, lactate (kHz)
    base = dict(gx=trap(80, 16, 4.0), dt=0.004, ngx=25, mb_cf=bands, mb_range=[0.06] * 4, mb_ripple=[0.01] * 4,
                gfb=-trap(40, 8, 8.0))
    specs = [dict(base, mb_FA=[fa if i == t else 0 for i in range(4)]) for t in range(4) for fa in range(2, 42, 2)]
    designs = [d for d in mbfir.dzss_mb_batch(specs, ctx=ctx) if d[2]["status"] == "Solved"]
    fr = np.concatenate([np.linspace(c - 0.03, c + 0.03, 7) for c in bands]) * 1e3       # Hz (tests/test_ssmb_cpu.py physics_grids)
    x = np.linspace(-3, 3, 241) * designs[0][2]["thk"]                                  # cm; every pulse of the schedule: one thk
    sp = [(rf, g, 0.004e-3, 1e6, 1e6, "C-13") for rf, g, _ in designs]
    ms_b, rb = best(lambda: mbfir.bloch_batch(sp, fr, x, ctx=ctx), a.reps)
    ms_l, rl = best(lambda: [mbfir.bloch(*p[:5], fr, x, ctx=ctx) for p in sp], a.reps)
    d, same = compare([v[0] for r in rb for v in r], [v for r in rl for v in r])
    emit(dict(case="schedule", pulses=len(sp), ntime=len(sp[0][0]), nf=len(fr), npos=len(x),
              same_thk=bool(all(abs(i["thk"] - designs[0][2]["thk"]) < 1e-12 for _, _, i in designs)), ms_batch=ms_b, ms_loop=ms_l,
              speedup=ms_l / ms_b, max_abs_diff=d, bit_identical=same))

    specs = [(int(n), float(tb), "ex", "ls", 0.01, 0.01) for n, tb in zip(np.resize([64, 128, 200, 256, 400, 512], 256),
                                                                          np.resize([2.0, 4.0, 6.0, 8.0], 256))]
    rfs = mbfir.dzrf_batch(specs, ctx=ctx)
    xa = np.linspace(-10, 10, 4000)
    ms_b, rb = best(lambda: mbfir.abr_batch(rfs, xa, scales=SCALES, ctx=ctx), a.reps)
    ms_l, rl = best(lambda: [mbfir.abrm(rf * s, xa, ctx=ctx) for rf in rfs for s in SCALES], a.reps)
    d, same = compare([ab[c][k] for ab in rb for k in range(len(SCALES)) for c in range(2)], [v for r in rl for v in r])
    emit(dict(case="abr", pulses=len(rfs), ntime_total=int(sum(len(r) for r in rfs)), scales=len(SCALES), nx=len(xa), ms_batch=ms_b,
              ms_loop=ms_l, speedup=ms_l / ms_b, max_abs_diff=d, bit_identical=same))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
