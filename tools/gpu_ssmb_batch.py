"""Multiband spectral-spatial designer timing: one JSON line.
  schedule     a flip-angle schedule of C-13 metabolite-specific flyback excitations at 3 T (4 target metabolites x 20 flip angles =
               80 pulses, the other bands at 0 degrees): dzss_mb_batch against a loop of dzss_mb over the same specs
  slr2d        the 2D inverse SLR of those 80 pulses: one mbfir.slr2d_batch call against the host-FFT middle stage of dzepse_batch
               (b2rf_batch of the rows, a Python loop of per-column FFTs, b2rf_batch of the columns)
Times are warm host clocks around calls that end in a stream synchronise (transfers included); the minimum of --reps.

    python tools/gpu_ssmb_batch.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mbfir  # noqa: E402


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


def host_fft_slr2d(R, ctx):
    """dzepse_batch's way: one b2rf_batch over every row, the middle stage per column on the host, one b2rf_batch over the columns."""
    count, m, n = R.shape
    rn1 = mbfir.b2rf_batch(R.reshape(count * m, n), ctx=ctx).reshape(count, m, n)
    p2 = np.empty((count, n, m), dtype=np.complex128)
    for c in range(count):
        for j in range(n):
            th = rn1[c, :, j]
            s = np.sin(np.abs(th) / 2) * np.exp(-1j * np.angle(th))
            p2[c, j] = (mbfir.fftcp(s, 2 * m) / (2 * m))[m // 2:m // 2 + m]
    rf2 = mbfir.b2rf_batch(p2.reshape(count * n, m), ctx=ctx).reshape(count, n, m)
    return np.conj(rf2).transpose(0, 2, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = mbfir.get_context()
    out = {"tool": "gpu_ssmb_batch", "cases": []}

    def emit(row):
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    cs = mbfir.spec.spectrum_c13(3.0) * 1e-3
    bands = [cs[4], cs[0], cs[2], cs[1]]                   # bicarbonate, pyruvate, alanine, lactate (kHz)
    base = dict(gx=trap(80, 16, 4.0), dt=0.004, ngx=25, mb_cf=bands, mb_range=[0.06] * 4, mb_ripple=[0.01] * 4,
                gfb=-trap(40, 8, 8.0))
    specs = [dict(base, mb_FA=[fa if i == t else 0 for i in range(4)]) for t in range(4) for fa in range(2, 42, 2)]
    ms_b, rb = best(lambda: mbfir.dzss_mb_batch(specs, ctx=ctx), a.reps)
    ms_s, rs = best(lambda: [mbfir.dzss_mb(**s, ctx=ctx) for s in specs], 1)
    ms_1, _ = best(lambda: mbfir.dzss_mb(**specs[0], ctx=ctx), a.reps)
    emit(dict(case="schedule", pulses=len(specs), lgx=80, ngx=25, solved=sum(r[2]["status"] == "Solved" for r in rb),
              ms_batch=ms_b, ms_single_calls=ms_s, ms_single=ms_1, speedup=ms_s / ms_b,
              bit_identical=all(np.array_equal(p[0], q[0]) for p, q in zip(rb, rs))))

    R = np.stack([np.outer(np.conj(info["pwx"]), info["beta"]) for _, _, info in rb if info["status"] == "Solved"])
    ms_d, rd = best(lambda: mbfir.slr2d_batch(R, ctx=ctx), a.reps)
    ms_h, rh = best(lambda: host_fft_slr2d(R, ctx), a.reps)
    emit(dict(case="slr2d", count=len(R), m=R.shape[1], n=R.shape[2], ms_device=ms_d, ms_host_fft_middle=ms_h, speedup=ms_h / ms_d,
              max_rel_diff=float(np.abs(rd - rh).max() / np.abs(rh).max())))
    for m, n, count in ((128, 32, 256), (512, 64, 64), (2048, 16, 8)):
        rng = np.random.default_rng(m + n)
        X = (rng.standard_normal((count, m, n)) + 1j * rng.standard_normal((count, m, n))) * 0.5 / np.sqrt(n)
        ms_d, rd = best(lambda: mbfir.slr2d_batch(X, ctx=ctx), a.reps)
        ms_h, rh = best(lambda: host_fft_slr2d(X, ctx), 1)
        emit(dict(case="slr2d", count=count, m=m, n=n, ms_device=ms_d, ms_host_fft_middle=ms_h, speedup=ms_h / ms_d,
                  max_rel_diff=float(np.abs(rd - rh).max() / np.abs(rh).max())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
