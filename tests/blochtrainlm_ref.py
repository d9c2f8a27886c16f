"""NumPy restatement of the Levenberg-Marquardt step that mbfir.bloch_train_lm_step_batch solves on the device (helper of
tests/test_blochtrainlm_cpu.py and tests/test_blochtrainlm_gpu.py; not collected): tests/simlm_ref.py's cg_solve, imported, on the
operator blochtraingn_ref.gn, and blochtraingn_ref.lsq for the trial.  The cases are blochtraingn_ref.cases() and small(), used as
they are; batch17() builds the batch of the GPU test's independence check from small()-sized periods."""
import functools
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
gnref = _load("blochtraingn_ref")
tr, vjp = gnref.tr, gnref.vjp
cg_solve, STATUS = lmref.cg_solve, lmref.STATUS
PER_PULSE = ("pulses", "dfs", "dps", "ntr", "phases", "gains", "echo", "m0", "w", "t", "wf", "tf", "ce", "cf")


def dot(u, v):
    return float((np.conj(u) * v).real.sum())


def sub(c, idx):
    """the pulses idx of a case as a case"""
    d = dict(c)
    for k in PER_PULSE:
        if k in c:
            d[k] = [c[k][q] for q in idx]
    d["rw"] = None if c["rw"] is None else [c["rw"][q] for q in idx]
    return d


def moved(c, q, d):
    """the case with b1 + d as the period of pulse q"""
    out = dict(c)
    out["pulses"] = list(c["pulses"])
    p = c["pulses"][q]
    out["pulses"][q] = (np.asarray(p[0], dtype=np.complex128) + d,) + tuple(p[1:])
    return out


def gn(c, q, v, dtype=np.float64):
    """H v of pulse q along one direction v (ntime,), complex128"""
    return np.asarray(gnref.gn(c, q, np.asarray(v), dtype)[0], dtype=np.complex128)


def lsq(c, q, dtype=np.float64):
    """(L, g) of pulse q"""
    L, g, _ = gnref.lsq(c, q, dtype)
    return float(L), np.asarray(g, dtype=np.complex128)


def step(c, q, b, mu, cg=8, rtol=1e-6, trial=False, dtype=np.float64):
    """Pulse q of bloch_train_lm_step_batch on blochtraingn_ref: (d, info), info with 'loss' and 'grad' at b1 + d with trial."""
    d, info = cg_solve(lambda p: gn(c, q, p, dtype), b, mu, cg, rtol)
    if trial:
        info["loss"], info["grad"] = lsq(moved(c, q, d), q, dtype)
    return d, info


def rhs_and_mu(lsq_res, gn_fn):
    """b = -gradient and mu = 1e-3 times the Rayleigh quotient of H at b (the refinement's first mu) from the results of an lsq
    call, [(L, g, ...)], and a gn call on those b: gn_fn(bs) -> [H b]"""
    bs = [-np.asarray(r[1]) for r in lsq_res]
    mus = [1e-3 * dot(b, h) / dot(b, b) for b, h in zip(bs, gn_fn(bs))]
    return bs, mus


# ---- the batch of 17 of the GPU test's independence check; tests/test_blochtrainlm_cpu.py checks on the float64 reference that its
# pulses do not all stop at the same iteration ---------------------------------------------------------------------------------------
CG17, RTOL17 = 4, 1e-2
NTR17 = (1, 2, 3, 5, 7, 8, 9, 12, 4, 6, 10, 3, 9, 2, 5, 8, 7)


@functools.lru_cache(maxsize=None)
def batch17():
    """17 periods of small()'s size (9 samples with a gradient, 3 x 2 points, one scale), each its own draw, trains of 1 to 12
    repetitions at up to three gains and quadratic phases, echo after 4 samples, an echo term in the broadcast form and a final term,
    rep_weights given, demod.  A blochtraingn_ref case."""
    rng = np.random.default_rng(1717)
    f3, p2 = tr._grid(3, 60.0), np.array([[-1.0], [0.7]])
    c = dict(pulses=[], dfs=[], dps=[], ntr=list(NTR17), phases=[], gains=[], echo=[], m0=[], scales=(1.0,), cot="both", demod=True,
             meq=1.0, bcast=True, w=[], t=[], wf=[], tf=[], rw=[], ce=[], cf=[])
    for n in NTR17:
        c["pulses"].append(tr._period(rng, 9, *tr.C13, float(rng.uniform(0.3, 0.9)), 4e-3, True))
        c["dfs"].append(f3)
        c["dps"].append(p2)
        c["phases"].append(0.5 * np.deg2rad(117.0) * np.arange(n) * (np.arange(n) + 1))
        c["gains"].append(np.array([0.5, 0.75, 1.0])[np.arange(n) % 3])
        c["echo"].append(4)
        c["m0"].append(tr._m0(rng, 3, 2))
        c["w"].append(tuple(gnref._weights(rng, (3, 1, 3, 2))))
        c["t"].append(tuple(rng.uniform(-1.0, 1.0, (3, 1, 3, 2))))
        c["wf"].append(tuple(gnref._weights(rng, (3, 1, 3, 2))))
        c["tf"].append(tuple(rng.uniform(-1.0, 1.0, (3, 1, 3, 2))))
        c["rw"].append(rng.uniform(0.5, 1.5, n))
        c["ce"].append(None)
        c["cf"].append(None)
    return c
