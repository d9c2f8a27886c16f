"""Device root-flip search timing (mbfir.flip_search, RF criterion): one JSON line.
Three candidate sets -- n = 48 with 2^18 candidates (golden qp_modelA48 at max|B| = 0.99, all 18 pass-band zeros), n = 64 with
2^14 (golden lin_real64 at 0.99), n = 512 with 4096 explicit masks (synthetic, 40 flip factors, npoly rule at 0.7) -- each timed warm as a host
clock around the call (which ends in a stream synchronise; it includes the transfers and the twiddle setup): device ms,
candidates per second, the winning peak.  --host adds the time of the vectorised NumPy chain (b2a.m + ab2rf.m) over the same
set and its winning peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mbfir  # noqa: E402
from mbfir.flipzero import _flip, _poly  # noqa: E402


def cases():
    from test_flipsearch_gpu import all_masks, golden, split
    out = []
    for name, nz in (("qp_modelA48", 18), ("lin_real64", 14)):
        h = golden(name, 0.99)
        c0, zp = split(h)
        assert len(zp) == nz
        out.append(dict(case="%s_n%d_all%d" % (name, len(h), 2 ** nz), c0=c0, zp=zp, masks=None, target=np.sum(h),
                        host_masks=lambda nz=nz: all_masks(nz)))
    rng = np.random.default_rng(7)
    n, nz = 512, 40                                               # the large-n case of tests/test_flipsearch_gpu.py
    t = np.arange(n - nz) - (n - nz - 1) / 2
    c0 = (np.sinc(t / 8) * np.hamming(n - nz)).astype(np.complex128)
    zp = rng.uniform(0.85, 0.95, nz) * np.exp(2j * np.pi * (np.arange(nz) + rng.uniform(0, 1, nz)) / nz)
    m = (rng.random((nz, 4096)) < 0.5).astype(int)
    out.append(dict(case="synthetic_n512_masks4096", c0=c0, zp=zp, masks=m, bsf=0.7, host_masks=lambda m=m: m))
    return out


def host_time(c):
    from test_flipsearch_gpu import host_rf_peaks
    mask = c["host_masks"]()
    t0 = time.perf_counter()
    zsel = np.where(mask == 1, _flip(c["zp"])[:, None], c["zp"][:, None])
    best = np.inf
    for lo in range(0, mask.shape[1], 4096):                      # chunks keep the host memory bounded
        coef = np.zeros((min(4096, mask.shape[1] - lo), len(c["c0"]) + len(c["zp"])), dtype=np.complex128)
        coef[:, :len(c["c0"])] = c["c0"]
        deg = len(c["c0"]) - 1
        for j in range(len(c["zp"])):
            coef[:, 1:deg + 2] -= zsel[j, lo:lo + len(coef)][:, None] * coef[:, :deg + 1]
            deg += 1
        if "bsf" in c:                                            # npoly rule
            coef *= (c["bsf"] / np.abs(np.fft.fft(coef, 1 << int(np.ceil(np.log2(coef.shape[1]))), axis=1)).max(axis=1))[:, None]
        else:
            coef *= (c["target"] / np.sum(coef, axis=1))[:, None]
        best = min(best, float(host_rf_peaks(coef).min()))
    return time.perf_counter() - t0, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="also time the vectorised NumPy chain on the host")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = mbfir.Context(0)
    res = []
    for c in cases():
        kw = dict(masks=c["masks"], criterion="rf", ctx=ctx)
        kw.update(dict(bsf=c["bsf"]) if "bsf" in c else dict(target=c["target"]))
        b, best, _ = mbfir.flip_search(c["c0"], c["zp"], _flip(c["zp"]), return_peaks=True, **kw)      # warm-up
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, best, pk = mbfir.flip_search(c["c0"], c["zp"], _flip(c["zp"]), return_peaks=True, **kw)
            ts.append(time.perf_counter() - t0)
        ncand = len(pk)
        r = dict(case=c["case"], n=len(c["c0"]) + len(c["zp"]), candidates=ncand, device_ms=1e3 * min(ts),
                 candidates_per_s=ncand / min(ts), peak=float(pk[best]))
        if a.host:
            th, hb = host_time(c)
            r.update(host_numpy_s=th, host_peak=hb)
        res.append(r)
    ctx.close()
    print(json.dumps(dict(tool="gpu_flip_search", measured=True, cases=res)))


if __name__ == "__main__":
    main()
