"""Writes tests/golden/specfact_cases.npz: the conic solutions x the tap extraction is tested on (tests/specfact_ref.py,
tests/test_specfactstages_*.py).  Runs on the CPU from the package's own oracle; python tests/golden/make_specfact_cases.py

    B/<name>        the oracle's solution x (2n - 1 reals) of a fir_ap_cvx design: test_fuzz_gpu.make_case seeds 4, 16, 28 and 2324 (the
                    seed VERDICT item 1(c) names: device and oracle taps 1e-5 apart at identical conic solutions), and the headline
                    design's x as tests/golden/c3_golden.json holds it (n = 512, not solved again)
    C/<name>/<t>    the same x with x[0] shifted, in long double, so that the sample of smallest |real hpf| on the lp grid sits at
                    t max|hpf|: t = 1e-6, 1e-9, 1e-12, 1e-15 and 0 (the rounding level of x[0])

The padded spectrum of such a solution crosses zero between the design grid's points (min real hpf about -1e-4 max|hpf|), so how
deep the lp grid's troughs of |hpf| come out is an accident of where its samples fall; (C) takes the accident out.
The conditions the tests rely on are checked here and asserted again by tests/test_specfactstages_cpu.py."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import specfact_ref as sr                     # noqa: E402
from oracle import designers                  # noqa: E402
from test_fuzz_gpu import make_case           # noqa: E402

SEEDS = (4, 16, 28, 2324)


def main():
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    out = {}
    for seed in SEEDS:
        which, args = make_case(seed)
        assert which == "fir_ap_cvx"
        h, status, info = designers.fir_ap_cvx(*args, info=True)
        assert status == "Solved", seed
        n = args[0]
        out["B/seed%d" % seed] = np.asarray(info["x"][:2 * n - 1], dtype=np.float64)
    with open(os.path.join(HERE, "c3_golden.json")) as fh:
        c3 = json.load(fh)["c3_ap_512_16384"]
    out["B/headline"] = np.asarray(c3["x"][:2 * c3["n"] - 1], dtype=np.float64)
    for k in [k for k in out if k.startswith("B/")]:
        x = out[k]
        n = (len(x) + 1) // 2
        for t in sr.T_LEVELS:
            out["C/%s/%g" % (k[2:], t)] = sr.touch(x, n, t)
    loose = 0
    for k, x in sorted(out.items()):
        n = (len(x) + 1) // 2
        sp, base = sr.spread(0, x, n)
        hmax = float(np.abs(base["h"]).max())
        hpf = base["hpf"][0].real
        print("%-24s n %4d  min|re hpf| / max %.2e  min re hpf / max %+.2e  spread / max|h| %.2e" % (
            k, n, float(np.abs(hpf).min() / np.abs(hpf).max()), float(hpf.min() / np.abs(hpf).max()), sp[0] / hmax))
        if k.startswith("C/") and float(k.rsplit("/", 1)[1]) >= 1e-6:
            assert sp[0] <= 1e-9 * hmax, k
        loose += k.startswith("C/") and sp[0] >= 1e-5 * hmax
    assert loose >= 1
    np.savez_compressed(os.path.join(HERE, "specfact_cases.npz"), **out)


if __name__ == "__main__":
    main()
