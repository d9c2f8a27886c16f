"""NumPy restatement of the Levenberg-Marquardt step of a pulse train's schedule that mbfir.bloch_train_lm_step_sched_batch evaluates
and solves on the device, and of the refinement mbfir.refine_bloch_train_sched_lm_batch builds on it (helper of
tests/test_blochtrainschedlm_cpu.py and tests/test_blochtrainschedlm_gpu.py; not collected): tests/simlm_ref.py's cg_solve, imported,
on the operator blochtrainschedgn_ref.gn restricted to the varied halves, and blochtrainschedgn_ref.lsq for the evaluation.  A
schedule's vector (dg, dp) is carried as the complex array dg + i dp, so that cg_solve's inner product Re sum conj(u) v is the one
over the double2 pairs; a half that does not vary is an exact zero in it.

The cases are blochtrainsched_ref.cases() and small(), dressed as blochtrainschedgn_ref dresses them, and one more, 'stride': a
one-sample period, one frequency, one position, ntr = 257 at 257 distinct gains and quadratic phases, an echo term in the full form
and a final term.  It is the smallest shape that reaches the step kernel's second stride of 256 repetitions and the run kernel's
second staged chunk of the repetition table."""
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
gnref = _load("blochtrainschedgn_ref")
sched, gnr, tr = gnref.sched, gnref.gnr, gnref.tr
cg_solve, STATUS = lmref.cg_solve, lmref.STATUS
PER_PULSE = ("pulses", "dfs", "dps", "ntr", "phases", "gains", "echo", "m0", "w", "t", "wf", "tf", "ce", "cf")
VARIES = (("gains", "phases"), ("gains",), ("phases",))


def dot(u, v):
    return float((np.conj(u) * v).real.sum())


@functools.lru_cache(maxsize=None)
def stride():
    rng = np.random.default_rng(53)
    n = 257
    c = dict(pulses=[tr._period(rng, 1, *tr.H1, 0.4, 1e-3, False)], dfs=[np.array([35.0])], dps=[np.array([[0.6]])], ntr=[n],
             phases=[0.5 * np.deg2rad(117.0) * np.arange(n) * (np.arange(n) + 1)], gains=[np.linspace(0.5, 1.0, n)], echo=[1],
             m0=[tr._m0(rng, 1, 1)], scales=(1.0,), cot="both", demod=False, meq=1.0, ce=[None], cf=[None])
    return gnr._dress(c, "stride", rng)


def names():
    return list(gnref.cases()) + ["small", "stride"]


def case_of(name):
    return stride() if name == "stride" else gnref.case_of(name)


def sub(c, idx):
    """the pulses idx of a case as a case"""
    d = dict(c)
    for k in PER_PULSE:
        if k in c:
            d[k] = [c[k][q] for q in idx]
    d["rw"] = None if c["rw"] is None else [c["rw"][q] for q in idx]
    return d


def flags(vary):
    return "gains" in vary, "phases" in vary


def mask(v, vary):
    """the complex form with the half that does not vary set to an exact zero"""
    vg, vp = flags(vary)
    v = np.asarray(v, dtype=np.complex128)
    return (v.real if vg else 0.0) + 1j * (v.imag if vp else np.zeros(v.shape))


def gn(c, q, v, vary=VARIES[0], dtype=np.float64):
    """H v of pulse q along one direction v = dg + i dp (ntr,), restricted to the varied halves"""
    vg, vp = flags(vary)
    v = np.asarray(v, dtype=np.complex128)
    hg, hp = gnref.gn(c, q, v.real if vg else None, v.imag if vp else None, dtype)
    out = np.zeros(c["ntr"][q], dtype=np.complex128)
    if vg:
        out += np.asarray(hg[0], dtype=np.float64)
    if vp:
        out += 1j * np.asarray(hp[0], dtype=np.float64)
    return out


def lsq(c, q, vary=VARIES[0], dtype=np.float64):
    """(L, g) of pulse q, g = gg + i gp restricted to the varied halves"""
    L, gg, gp, _ = gnref.lsq(c, q, dtype)
    return float(L), mask(np.asarray(gg, dtype=np.float64) + 1j * np.asarray(gp, dtype=np.float64), vary)


def dense(c, q, vary=VARIES[0], dtype=np.float64):
    """H restricted to the varied halves in the real form [gains; phases] (2 ntr, 2 ntr), zero rows and columns where nothing varies"""
    vg, vp = flags(vary)
    n = c["ntr"][q]
    H = np.asarray(gnref.dense(c, q, dtype), dtype=np.float64)
    on = np.r_[np.full(n, vg), np.full(n, vp)]
    return H * on[:, None] * on[None, :]


def realform(v):
    return np.concatenate([v.real, v.imag])


def moved(c, q, x):
    """the case with the schedule of pulse q replaced by x = gains + i phases"""
    return gnref.moved(c, q, x.real, x.imag)


def schedule(c, q):
    return np.asarray(c["gains"][q], dtype=np.float64) + 1j * np.asarray(c["phases"][q], dtype=np.float64)


def step(c, q, b, mu, cg=8, rtol=1e-6, vary=VARIES[0], op=None):
    """Pulse q of a solve-only bloch_train_lm_step_sched_batch on blochtrainschedgn_ref (or on op): (d, info)"""
    return cg_solve(op or (lambda p: gn(c, q, p, vary)), mask(b, vary), mu, cg, rtol)


def eval_and_solve(c, q, mu, cg=8, rtol=1e-6, vary=VARIES[0], b=None):
    """The fused call: L and g at the case's schedule, then the solve at b (None: -g); (d, info) with 'loss' and 'grad'"""
    L, g = lsq(c, q, vary)
    d, info = step(c, q, -g if b is None else b, mu, cg, rtol, vary)
    info["loss"], info["grad"] = L, g
    return d, info


def rhs_and_mu(grads, gn_fn):
    """b = -gradient and mu = 1e-3 times the Rayleigh quotient of H at b (the refinement's first mu); gn_fn(bs) -> [H b]"""
    bs = [-np.asarray(g) for g in grads]
    mus = [1e-3 * dot(b, h) / dot(b, b) for b, h in zip(bs, gn_fn(bs))]
    return bs, mus


# ---- the refinement of one pulse, restated: the loop of mbfir.refine._lm_loop with mu0 given ------------------------------------
def _loop(x, L, g, mu, iters, take):
    """take(x, g, mu) -> (trial, L, g, broke); returns the iterates, the losses, the count of refused steps"""
    xs, Ls, refused, done = [x], [L], 0, 0
    while done < iters and dot(g, g) != 0.0 and mu <= 1e12:
        trial, Lt, gt, broke = take(x, g, mu)
        if Lt < L and not broke:
            x, L, g, mu = trial, Lt, gt, mu / 3
            xs.append(x)
            Ls.append(L)
            done += 1
        else:
            mu *= 4
            refused += 1
    return xs, Ls, refused


def refine_plain(c, q, mu0, iters, cg, rtol=1e-6, vary=VARIES[0]):
    """solve at x, then evaluate at x + d: two sets of sweeps per iterate"""
    def take(x, g, mu):
        d, info = step(moved(c, q, x), q, -g, mu, cg, rtol, vary)
        if info["status"] == "breakdown":
            return x, np.inf, g, True
        return (x + d,) + lsq(moved(c, q, x + d), q, vary) + (False,)
    x = schedule(c, q)
    return _loop(x, *lsq(c, q, vary), mu0, iters, take)


def refine_speculative(c, q, mu0, iters, cg, rtol=1e-6, vary=VARIES[0]):
    """the loop of refine_bloch_train_sched_lm_batch(solver='device'): the call that evaluates a trial solves the next step at mu / 3;
    returns refine_plain's values and the number of fused calls"""
    held, calls = {}, [0]

    def take(x, g, mu):
        if held.get("at") is not x or held["mu"] != mu:
            calls[0] += 1
            d, info = step(moved(c, q, x), q, -g, mu, cg, rtol, vary)
            held.update(at=x, mu=mu, d=d, broke=info["status"] == "breakdown")
        if held["broke"]:
            return x, np.inf, g, True
        trial = x + held["d"]
        calls[0] += 1
        d, info = eval_and_solve(moved(c, q, trial), q, mu / 3, cg, rtol, vary)
        held.update(at=trial, mu=mu / 3, d=d, broke=info["status"] == "breakdown")
        return trial, info["loss"], info["grad"], False
    x = schedule(c, q)
    return _loop(x, *lsq(c, q, vary), mu0, iters, take) + (calls[0],)


# ---- the batch of 17 of the GPU test's independence check -----------------------------------------------------------------------
CG17, RTOL17 = 4, 1e-2
NTR17 = (1, 2, 3, 5, 7, 8, 9, 12, 4, 6, 10, 3, 9, 2, 5, 8, 7)


@functools.lru_cache(maxsize=None)
def batch17():
    """17 periods of small()'s size (9 samples with a gradient, 3 x 2 points, one scale), each its own draw, trains of 1 to 12
    repetitions at up to three gains and quadratic phases, echo after 4 samples, an echo term in the broadcast form and a final term,
    rep_weights given, demod"""
    rng = np.random.default_rng(1718)
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
        c["w"].append(tuple(gnr._weights(rng, (3, 1, 3, 2))))
        c["t"].append(tuple(rng.uniform(-1.0, 1.0, (3, 1, 3, 2))))
        c["wf"].append(tuple(gnr._weights(rng, (3, 1, 3, 2))))
        c["tf"].append(tuple(rng.uniform(-1.0, 1.0, (3, 1, 3, 2))))
        c["rw"].append(rng.uniform(0.5, 1.5, n))
        c["ce"].append(None)
        c["cf"].append(None)
    return c


def refine_dense(c, q, iters, vary=VARIES[0], mu0=None, lsq_fn=None, dense_fn=None):
    """The loop of mbfir.refine_bloch_train_sched_batch (solver 'host') for one pulse: H formed once per accepted iterate,
    symmetrised, (H + mu I) d = -g solved by a dense Cholesky factorisation on the varied halves.  lsq_fn(x) -> (L, g) and
    dense_fn(x) -> H in the real form restricted to the varied halves (n, n): the reference's by default, the device's when the
    caller passes them.  Returns (iterates, losses, refused)."""
    vg, vp = flags(vary)
    ntr = c["ntr"][q]
    on = np.r_[np.full(ntr, vg), np.full(ntr, vp)]
    lsq_fn = lsq_fn or (lambda x: lsq(moved(c, q, x), q, vary))
    dense_fn = dense_fn or (lambda x: dense(moved(c, q, x), q, vary)[np.ix_(on, on)])
    pack = lambda v: realform(v)[on]

    def unpack(r):
        full_ = np.zeros(2 * ntr)
        full_[on] = r
        return full_[:ntr] + 1j * full_[ntr:]

    held = {}

    def take(x, g, mu):
        if held.get("at") is not x:
            H = dense_fn(x)
            held.update(at=x, H=(H + H.T) / 2)
        n = held["H"].shape[0]
        try:
            ch = np.linalg.cholesky(held["H"] + mu * np.eye(n))
        except np.linalg.LinAlgError:
            return x, np.inf, g, True
        trial = x + unpack(np.linalg.solve(ch.T, np.linalg.solve(ch, -pack(g))))
        return (trial,) + tuple(lsq_fn(trial)) + (False,)

    x = schedule(c, q)
    L, g = lsq_fn(x)
    if mu0 is None:
        H = dense_fn(x)
        mu0 = 1e-3 * float(pack(g) @ (H @ pack(g))) / dot(g, g)
    return _loop(x, L, g, mu0, iters, take)
