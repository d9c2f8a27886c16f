"""NumPy restatement of the Levenberg-Marquardt step that mbfir.bloch_lm_step_batch solves on the device (helper of
tests/test_blochlm_cpu.py and tests/test_blochlm_gpu.py; not collected): tests/simlm_ref.py's cg_solve, imported, on the operator
of tests/blochgn_ref.py, and blochgn_ref.lsq for the trial.  It also holds the cases of the two test files, drawn through
blochgrad_ref.batch and blochgn_ref.cases so that the shapes are the ones the sweeps of the shipped products are already held at."""
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lmref = _load("simlm_ref")
gnref = _load("blochgn_ref")
cg_solve, STATUS = lmref.cg_solve, lmref.STATUS
SCALES = gnref.SCALES                      # 1, 0, 0.9


def step(pulse, df, pos, b, weights, mu, scales, m0=None, cg=8, rtol=1e-6, target=None):
    """One pulse of bloch_lm_step_batch on blochgn_ref: (d, info), info with 'loss' and 'grad' at b1 + d when a target is given."""
    d, info = cg_solve(lambda p: gnref.gn(pulse, df, pos, p, weights, scales, m0), b, mu, cg, rtol)
    if target is not None:
        info["loss"], info["grad"] = gnref.lsq((np.asarray(pulse[0], dtype=np.complex128) + d,) + tuple(pulse[1:]), df, pos, target,
                                               weights, scales, m0)
    return d, info


def dot(u, v):
    return float((np.conj(u) * v).real.sum())


NCASE = 7


def cases(shared):
    """The first seven pulses of blochgn_ref.cases(shared, 1): 1, 7, 8, 9, 255, 256 and 257 samples (around the checkpoint group of 8
    and the step kernel's stride of 256), a scalar interval on the even ones and a per-sample vector on the odd ones, one b1 sample
    exactly zero, a third of the weights zero, at the scales 1, 0, 0.9.  shared: the 3 x 5 grid for every pulse and m0 = None;
    else the grids 1 x 1, 3 x 5, 1 x 257, 3 x 200 per pulse and a random m0 per pulse.  Changed here: the 256-sample pulse has T2 a
    twentieth of its duration, and the 255-sample pulse has weights on mz alone.  Returns (pulses, dfs, dps, m0s or None, targets,
    weights)."""
    pulses, dfs, dps, m0s, tgs, wts, _ = gnref.cases(shared, 1)
    pulses, dfs, dps, m0s, tgs, wts = (list(v[:NCASE]) for v in (pulses, dfs, dps, m0s, tgs, wts))
    q = 5
    b1, gr, tp, t1, _, nuc = pulses[q]
    pulses[q] = (b1, gr, tp, t1, float(np.sum(gnref.intervals(pulses[q]))) / 20, nuc)
    wts[4] = (0.0, 0.0, wts[4][2])
    return pulses, dfs, dps, (None if shared else m0s), tgs, wts


# ---- the batch of 17 of the GPU test's independence check; tests/test_blochlm_cpu.py checks on the reference that its pulses do
# not all stop together --------------------------------------------------------------------------------------------------------
SC17, CG17, RTOL17 = (0.9,), 4, 1e-2          # one scale: the cases above cover the scale list


def batch17():
    """17 pulses of 1 to 300 samples, 256 and 257 among them, on their own grids of (1 + q % 3) x (3 + 2 q) points (the 257-sample
    pulse: 3 x 100, two chunks), T2 from 3 to 19 ms, random m0, weights a third of which are zero: (pulses, dfs, dps, m0s, targets,
    weights).  The grids are small because tests/test_blochlm_cpu.py runs the whole batch on the NumPy reference."""
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 300, 17)]
    lengths[3], lengths[11] = 256, 257
    pulses, dfs, dps, m0s, wts, tgs = [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (gnref.GAMMA_H1 * n * dt)
        tp = dt if q % 2 == 0 else dt * (1.0 + 0.2 * (-1.0) ** np.arange(n))
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, tp, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 100 if q == 11 else 3 + 2 * q
        dfs.append(gnref._grid(nf, 150.0))
        dps.append(gnref._grid(npos, 3.0))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        w = rng.uniform(0, 1, (3, len(SC17), nf, npos))
        w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
        w[2, 0, 0, 0] = 1.0
        wts.append(tuple(w))
        tgs.append(tuple(rng.uniform(-1, 1, (3, len(SC17), nf, npos))))
    return pulses, dfs, dps, m0s, tgs, wts


def rhs_and_mu(lsq, gn):
    """b = -gradient and mu = 1e-3 times the Rayleigh quotient of H at b (refine_bloch_batch's first mu) from the results of an lsq
    call and of a gn call on those b: lsq() -> [(L, g)], gn(bs) -> [H b]"""
    bs = [-g for _, g in lsq()]
    mus = [1e-3 * dot(b, h) / dot(b, b) for b, h in zip(bs, gn(bs))]
    return bs, mus
