"""NumPy restatement of the Levenberg-Marquardt step that mbfir.bloch_ss_lm_step_batch solves on the device (helper of
tests/test_blochsslm_cpu.py and tests/test_blochsslm_gpu.py; not collected): tests/simlm_ref.py's cg_solve, imported, on the operator
of tests/blochssgn_ref.py, and blochssgn_ref.lsq for the trial.  It also holds the cases of the two test files, drawn through
blochssgn_ref.cases and blochlm_ref.batch17 so that the shapes are the ones the shipped products and the transient step are held at."""
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
gnref = _load("blochssgn_ref")
blochlm = _load("blochlm_ref")
cg_solve, STATUS = lmref.cg_solve, lmref.STATUS
SCALES = gnref.SCALES                      # 1, 0, 0.9


def step(pulse, df, pos, b, weights, mu, scales, cg=8, rtol=1e-6, target=None):
    """One period of bloch_ss_lm_step_batch on blochssgn_ref: (d, info), info with 'loss' and 'grad' at b1 + d when a target is given."""
    d, info = cg_solve(lambda p: gnref.gn(pulse, df, pos, p, weights, scales), b, mu, cg, rtol)
    if target is not None:
        info["loss"], info["grad"] = gnref.lsq((np.asarray(pulse[0], dtype=np.complex128) + d,) + tuple(pulse[1:]), df, pos, target,
                                               weights, scales)
    return d, info


def dot(u, v):
    return float((np.conj(u) * v).real.sum())


NCASE = 7


def cases(shared):
    """The first seven periods of blochssgn_ref.cases(shared, 1): 1, 7, 8, 9, 255, 256 and 257 samples (around the checkpoint group
    of 8, the staged tile and the step kernel's stride of 256) on the grids 1 x 1, 3 x 5, 1 x 257 (a second chunk with one live
    thread) and 3 x 200 per pulse, or the shared 3 x 5 grid, at the scales 1, 0, 0.9, a third of the weights zero.  Changed here: the
    255-sample period has weights on mz alone (on its own 1 x 1 grid the draw leaves it weight zero at the scales 1 and 0.9: a
    period whose gradient and Gauss-Newton operator are exact zeros).  Returns (pulses, dfs, dps, targets, weights)."""
    pulses, dfs, dps, tgs, wts, _ = gnref.cases(shared, 1)
    pulses, dfs, dps, tgs, wts = (list(v[:NCASE]) for v in (pulses, dfs, dps, tgs, wts))
    wts[4] = (0.0, 0.0, wts[4][2])
    return pulses, dfs, dps, tgs, wts


# ---- the batch of 17 of the GPU test's independence check; tests/test_blochsslm_cpu.py checks on the reference that its periods do
# not all stop together --------------------------------------------------------------------------------------------------------
SC17, CG17, RTOL17 = (0.9,), 4, 1e-2          # one scale: the cases above cover the scale list


def batch17():
    """blochlm_ref.batch17()'s pulses, grids, targets and weights, each pulse taken as one period; there is no m0:
    (pulses, dfs, dps, targets, weights)"""
    pulses, dfs, dps, _, tgs, wts = blochlm.batch17()
    return pulses, dfs, dps, tgs, wts


def rhs_and_mu(lsq, gn):
    """b = -gradient and mu = 1e-3 times the Rayleigh quotient of H at b (refine_bloch_ss_batch's first mu) from the results of an
    lsq call and of a gn call on those b: lsq() -> [(L, g)], gn(bs) -> [H b]"""
    bs = [-g for _, g in lsq()]
    mus = [1e-3 * dot(b, h) / dot(b, b) for b, h in zip(bs, gn(bs))]
    return bs, mus
