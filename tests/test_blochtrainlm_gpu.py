"""The Levenberg-Marquardt step of the pulse train solved on the device (mbfir.bloch_train_lm_step_batch: k_lm_init, the shipped
k_bloch_train_prop, k_bloch_train_lm_prep, the rounds of k_bloch_train_lm_jvp, k_bloch_train_lm_run, k_bloch_train_lm_pvjp and
k_bloch_train_lm_step, and for the trial k_bloch_lm_trial with the shipped kernels of bloch_train_lsq_batch on the trial rows) and
mbfir.refine_bloch_train_lm_batch on it.  The cases are blochtraingn_ref.cases() and small(), as they are.  No case has an exactly
zero gradient or operator (the CPU test holds that on the reference), so none is given another right-hand side.

Exact, without a tolerance: the trial's loss and gradient are bloch_train_lsq_batch's at b1 + d; the first iteration follows from
one shipped bloch_train_gn_batch product and the step kernel's arithmetic restated in NumPy (this is what holds the checkpoints
hoisted into k_bloch_train_lm_prep and the bodies shared through sim_dev.h to the bits of the shipped product); a pulse's outputs do
not depend on the batch, its order or a repeated call.  Against the dense solve on small(): the project's 1e-4 max|d|.  Against the
recurrence of tests/simlm_ref.py (cg_solve) run on the shipped bloch_train_gn_batch as the operator: ncg and status equal, and for
d, rr and gg the bounds that tests/test_blochlm_gpu.py derives in its docstring, the perturbation measured on code that is not under
test (the same recurrence on blochtraingn_ref.gn in float64 against the recurrence on the device product):
    |d - d_ref| <= max(100 max over the case's cg of |d_ref(blochtraingn_ref) - d_ref(device gn)|, 1e-13 max|d_ref|)
    |rr - rr_ref| <= 2 sqrt(rr_ref) dr + dr^2 + 2e-13 sqrt(rr_ref gg) + 1e-26 gg,   dr = (trace(H) + mu) sqrt(2n) (the bound on d)
gg is within 1e-14 relative.  DESIGN 8ac has the figures measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainlm_ref", os.path.join(ROOT, "tests", "blochtrainlm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
ref = lmref.gnref
_dot = lmref.dot
NAMES = list(ref.cases()) + ["small"]
PAIRS = [(name, q) for name in NAMES for q in range(len(ref.case_of(name)["pulses"]))]


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _opt(v):
    return None if v[0] is None else list(v)


def _kw(c):
    return dict(phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"], m0=_opt(c["m0"]),
                meq=c["meq"], demod=c["demod"], rep_weights=None if c["rw"] is None else list(c["rw"]), weights_final=_opt(c["wf"]))


def _lsq(c, pulses=None):
    df, dp = _grids(c)
    return mbfir.bloch_train_lsq_batch(c["pulses"] if pulses is None else pulses, df, dp, list(c["ntr"]), _opt(c["t"]), _opt(c["w"]),
                                       targets_final=_opt(c["tf"]), **_kw(c))


def _gn(c, vs):
    df, dp = _grids(c)
    return mbfir.bloch_train_gn_batch(c["pulses"], df, dp, list(c["ntr"]), list(vs), _opt(c["w"]), **_kw(c))


def _lm(c, bs, mus, trial=True, targets=None, targets_final=None, **over):
    df, dp = _grids(c)
    kw = _kw(c)
    kw.update(over)
    if trial:
        kw.update(targets=_opt(c["t"]) if targets is None else targets, targets_final=_opt(c["tf"]) if targets_final is None else targets_final)
    return mbfir.bloch_train_lm_step_batch(c["pulses"], df, dp, list(c["ntr"]), list(bs), _opt(c["w"]), list(mus), **kw)


def _moved(p, d):
    return (p[0] + d,) + tuple(p[1:])


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case with, per pulse, b = -gradient at b1 and mu = 1e-3 times the Rayleigh quotient of H at b, from the shipped device
    calls: (case, bs, mus, the lsq results at b1)"""
    c = ref.case_of(name)
    at_b1 = _lsq(c)
    bs, mus = lmref.rhs_and_mu(at_b1, lambda v: _gn(c, v))
    assert all(_dot(b, b) > 0 for b in bs) and all(m > 0 for m in mus), name
    return c, bs, mus, at_b1


def _one(name, q):
    c, bs, mus, _ = _case(name)
    return lmref.sub(c, [q]), [bs[q]], [mus[q]]


def _same(a, b):
    """every output of a pulse, bit for bit"""
    (da, ia), (db, ib) = a, b
    keys = set(ia) & set(ib)
    assert {"ncg", "rr", "gg", "status"} <= keys
    return np.array_equal(da, db) and all(np.array_equal(ia[k], ib[k]) for k in keys)


@pytest.mark.parametrize("name", NAMES)
def test_idle_call_and_trial_are_the_shipped_lsq_call(name):
    """rtol = 1e300: nothing runs, d = 0 and the loss and gradient are bloch_train_lsq_batch's at b1; cg in (0, 3) at rtol = 0: they
    are bloch_train_lsq_batch's at b1 + d with the returned d, bit for bit.  Solve-only returns the same d and state.  On the
    full-form cases, with the targets set to bloch_train_batch's own echoes and final state at b1 + d, the loss is 0.0 and the
    gradient exact zeros."""
    c, bs, mus, at_b1 = _case(name)
    df, dp = _grids(c)
    for (d, i), (L, g), b in zip(_lm(c, bs, mus, rtol=1e300), at_b1, bs):
        assert np.array_equal(d, np.zeros_like(d)) and i["ncg"] == 0 and i["status"] == "rtol"
        assert i["loss"] == L and np.array_equal(i["grad"], g)
        assert i["rr"] == i["gg"] and abs(i["gg"] - _dot(b, b)) <= 1e-14 * _dot(b, b)
    for cg in (0, 3):
        got = _lm(c, bs, mus, cg=cg, rtol=0.0)
        moved = [_moved(p, d) for p, (d, _) in zip(c["pulses"], got)]
        want = _lsq(c, moved)
        solve = _lm(c, bs, mus, trial=False, cg=cg, rtol=0.0)
        for (d, i), (L, g), (d0, i0) in zip(got, want, solve):
            n = len(d)
            # rtol = 0 stops a pulse before the cap only at a residual of exact zeros
            assert (i["ncg"] == cg and i["status"] == "cg") or (0 < i["ncg"] < cg and i["rr"] == 0.0 and i["status"] == "rtol"), (n, cg)
            assert cg == 0 or np.abs(d).max() > 0
            assert i["loss"] == L and np.array_equal(i["grad"], g), (n, cg)
            assert "loss" not in i0 and "grad" not in i0 and _same((d, i), (d0, i0)), (n, cg)
        if not c["bcast"]:
            there = mbfir.bloch_train_batch(moved, df, dp, list(c["ntr"]), final=True, phases=list(c["phases"]), gains=list(c["gains"]),
                                            echo=list(c["echo"]), scales=c["scales"], m0=_opt(c["m0"]), meq=c["meq"], demod=c["demod"])
            te = None if c["w"][0] is None else [e for e, _ in there]
            tf = None if c["wf"][0] is None else [f for _, f in there]
            df_, dp_ = _grids(c)
            kw = dict(_kw(c), targets=te, targets_final=tf, cg=cg, rtol=0.0)
            at_rest = mbfir.bloch_train_lm_step_batch(c["pulses"], df_, dp_, list(c["ntr"]), bs, _opt(c["w"]), mus, **kw)
            for (d, _), (dz, iz) in zip(got, at_rest):
                assert np.array_equal(dz, d) and iz["loss"] == 0.0 and np.array_equal(iz["grad"], np.zeros(len(d))), (len(d), cg)


def _device_sum(v):
    """the step kernel's sum of one real per sample: thread t adds samples t, t + 256, ... in order, then the fixed tree over 256"""
    part = np.zeros(256)
    for t in range(min(256, len(v))):
        for m in range(t, len(v), 256):
            part[t] = part[t] + v[m]
    o = 128
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return float(part[0])


def _device_dot(u, v):
    return _device_sum(u.real * v.real + u.imag * v.imag)


@pytest.mark.parametrize("name", NAMES)
def test_first_iteration_has_the_bits_of_the_shipped_product(name):
    """cg = 1, rtol = 0: H p of a running pulse is bloch_train_gn_batch's on p = b, bit for bit, so gg, rr and d follow exactly from
    one shipped product and the step kernel's arithmetic restated in NumPy (every product and sum rounded once, the sums in the
    kernel's order).  The shipped product sweeps the period forwards inside k_bloch_train_prop_vjp; the step reads the checkpoints
    that k_bloch_train_lm_prep left."""
    c, bs, mus, _ = _case(name)
    got = _lm(c, bs, mus, trial=False, cg=1, rtol=0.0)
    for (d, i), b, hb, mu in zip(got, bs, _gn(c, bs), mus):
        gg = _device_dot(b, b)
        ap = hb + mu * b
        alpha = gg / _device_dot(b, ap)
        r = b + (-alpha) * ap
        assert i["gg"] == gg and i["ncg"] == 1, len(b)
        assert np.array_equal(d, 0.0 + alpha * b), len(b)
        assert i["rr"] == _device_dot(r, r), len(b)


def test_outputs_have_the_same_bits_alone_in_17_reversed_and_repeated():
    c = lmref.batch17()
    every = list(range(17))
    bs, mus = lmref.rhs_and_mu(_lsq(c), lambda v: _gn(c, v))

    def lm(idx, trial=True):
        return _lm(lmref.sub(c, idx), [bs[q] for q in idx], [mus[q] for q in idx], trial=trial, cg=lmref.CG17, rtol=lmref.RTOL17)

    full, again, rev, bare = lm(every), lm(every), lm(every[::-1])[::-1], lm(every, trial=False)
    print("iterations per pulse %s" % [i["ncg"] for _, i in full])
    for q in every:
        assert _same(full[q], again[q]) and _same(full[q], rev[q]) and _same(full[q], bare[q]), q
        assert "loss" in full[q][1] and "loss" not in bare[q][1]
        alone, = lm([q])
        assert _same(alone, full[q]), q
    assert len(set(i["ncg"] for _, i in full)) > 1                   # the pulses of the batch do not all stop together


@pytest.mark.parametrize("name", ["batch", "shared", "groups"])
def test_a_pulse_of_the_cases_alone_has_its_bits_in_the_batch(name):
    c, bs, mus, _ = _case(name)
    full = _lm(c, bs, mus, cg=3, rtol=1e-3)
    for q in range(len(c["pulses"])):
        c1, b, m = _one(name, q)
        alone, = _lm(c1, b, m, cg=3, rtol=1e-3)
        assert _same(alone, full[q]), q


def _realform(v):
    return np.concatenate([v.real, v.imag])


def _dense_h(c1, n):
    """H of one pulse from 2n shipped gn products, real form"""
    cols, = _gn(c1, [np.concatenate([np.eye(n), 1j * np.eye(n)])])
    return np.stack([_realform(col) for col in cols], axis=1)


def test_step_is_the_dense_solve_on_small():
    """H from 2n = 18 shipped gn products, mu = 1e-2 trace(H) / 2n, cg = 4n, rtol = 1e-16: within 1e-4 of max|d|"""
    c1, b, _ = _one("small", 0)
    n = len(b[0])
    assert n == 9
    H = _dense_h(c1, n)
    assert np.trace(H) > 0
    mu = 1e-2 * np.trace(H) / (2 * n)
    want = np.linalg.solve(H + mu * np.eye(2 * n), _realform(b[0]))
    (d, i), = _lm(c1, b, [mu], trial=False, cg=4 * n, rtol=1e-16)
    err = np.abs(_realform(d) - want).max() / np.abs(want).max()
    print("step against the dense solve %.3g after %d iterations (%s), condition number %.0f"
          % (err, i["ncg"], i["status"], np.linalg.cond(H + mu * np.eye(2 * n))))
    assert err <= 1e-4


@pytest.mark.parametrize("name,q", PAIRS)
def test_step_is_the_recurrence_on_the_shipped_operator(name, q):
    """cg in 1, 2, 3, 8 with rtol = 0 (the module's docstring has the bounds); one pulse per case.  Of these the caps below 2n, the
    number of real unknowns: in exact arithmetic the residual is zero after 2n iterations at the latest, so from there on the
    recurrence runs on rounding noise, and whether rr is an exact zero (status 'rtol' at rtol = 0, and the pulse stops) or 1e-30 of
    gg (status 'cg', and it goes on) is not a property of the step.  The one-sample periods are held at cg = 1."""
    c1, (b,), (mu,) = _one(name, q)
    CGS = tuple(cg for cg in (1, 2, 3, 8) if cg < 2 * len(b))
    assert CGS[0] == 1
    got = {cg: _lm(c1, [b], [mu], trial=False, cg=cg, rtol=0.0)[0] for cg in CGS}

    @functools.lru_cache(maxsize=None)
    def shipped_of(key):
        return _gn(c1, [np.frombuffer(key, dtype=complex)])[0]

    @functools.lru_cache(maxsize=None)
    def numpy_of(key):
        return lmref.gn(c1, 0, np.frombuffer(key, dtype=complex))

    def shipped(v):                                                  # the runs with a smaller cg repeat the first products of cg = 8
        return shipped_of(v.tobytes())

    def numpy(v):
        return numpy_of(v.tobytes())

    on_dev = {cg: lmref.cg_solve(shipped, b, mu, cg, 0.0) for cg in CGS}
    on_ref = {cg: lmref.cg_solve(numpy, b, mu, cg, 0.0) for cg in CGS}
    scale = max(np.abs(on_dev[cg][0]).max() for cg in CGS)
    spread = max(np.abs(on_dev[cg][0] - on_ref[cg][0]).max() for cg in CGS)
    bound = max(100 * spread, 1e-13 * scale)
    n = len(b)
    trace = float(np.trace(_dense_h(c1, n)))
    dr = (trace + mu) * np.sqrt(2 * n) * bound
    for cg in CGS:
        (d, i), (d0, i0) = got[cg], on_dev[cg]
        err = float(np.abs(d - d0).max())
        rr_spread = abs(on_ref[cg][1]["rr"] - i0["rr"])
        rr_bound = 2 * np.sqrt(i0["rr"]) * dr + dr * dr + 2e-13 * np.sqrt(i0["rr"] * i0["gg"]) + 1e-26 * i0["gg"]
        rr_err = abs(i["rr"] - i0["rr"])
        print("%s pulse %d n %d cg %d: |d - recurrence| %.3g, the two references apart %.3g, bound %.3g, share %.3g (max|d| %.3g); "
              "rr %.6g, |rr - recurrence| %.3g, references apart %.3g, bound %.3g, share %.3g; ncg %d (%d)"
              % (name, q, n, cg, err, spread, bound, err / bound if bound else 0.0, scale, i0["rr"], rr_err, rr_spread, rr_bound,
                 rr_err / rr_bound if rr_bound else 0.0, i["ncg"], i0["ncg"]))
        assert i["ncg"] == i0["ncg"] and i["status"] == i0["status"], cg
        assert abs(i["gg"] - i0["gg"]) <= 1e-14 * i0["gg"], cg
        assert err <= bound, cg
        assert rr_err <= rr_bound, cg


@pytest.mark.parametrize("name,q", [(name, q) for name, q in PAIRS if len(ref.case_of(name)["pulses"][q][0]) == 1])
def test_one_sample_periods_past_exact_convergence(name, q):
    """The caps the recurrence test leaves out, cg = 2, 3, 8 >= 2n on the one-sample periods: in exact arithmetic the residual is
    zero after two iterations.  d is held to the recurrence on the shipped product at cg = 2 with the recurrence test's bound, plus
    what later iterations can still move it by; the status and ncg are the recurrence's, or the device's residual is below 1e-28 gg
    (it reaches an exact zero where NumPy's complex products leave 1e-30 gg); a pulse that stopped at an exact zero has the d of
    cg = 2 whatever the cap."""
    c1, (b,), (mu,) = _one(name, q)
    assert len(b) == 1
    shipped = lambda v: _gn(c1, [v])[0]
    numpy = lambda v: lmref.gn(c1, 0, v)
    d2, i2 = lmref.cg_solve(shipped, b, mu, 2, 0.0)
    bound = max(100 * np.abs(d2 - lmref.cg_solve(numpy, b, mu, 2, 0.0)[0]).max(), 1e-13 * np.abs(d2).max())
    got = {cg: _lm(c1, [b], [mu], trial=False, cg=cg, rtol=0.0)[0] for cg in (2, 3, 8)}
    for cg, (d, i) in got.items():
        d0, i0 = lmref.cg_solve(shipped, b, mu, cg, 0.0)
        print("%s pulse %d cg %d: ncg %d (%d), status %s (%s), rr / gg %.3g (%.3g), |d - d(cg = 2)| %.3g, bound %.3g"
              % (name, q, cg, i["ncg"], i0["ncg"], i["status"], i0["status"], i["rr"] / i["gg"], i0["rr"] / i0["gg"],
                 np.abs(d - d2).max(), bound))
        assert 2 <= i["ncg"] <= cg and abs(i["gg"] - i0["gg"]) <= 1e-14 * i0["gg"]
        assert (i["status"] == i0["status"] and i["ncg"] == i0["ncg"]) or i["rr"] <= 1e-28 * i["gg"]
        # iterations past the second solve (H + mu I) delta = r for the residual left, and H >= 0: |delta| <= |r| / mu
        slack = np.sqrt(max(got[2][1]["rr"], i2["rr"])) / mu
        assert np.abs(d - d2).max() <= bound + slack
        if i["status"] == "rtol":
            assert i["rr"] == 0.0 and np.array_equal(d, got[2][0])


@pytest.mark.parametrize("name", ["small", "batch", "allgains"])
def test_breakdown_and_a_vanishing_operator(name):
    """All-zero weights and mu = 0: <p, (H + mu) p> = 0, status 'breakdown', d = 0, ncg = 0.  scales = (0.0,) with mu > 0: the fold's
    factor makes H an exact zero, so d = rhs / mu after one iteration."""
    c, bs, mus, _ = _case(name)
    P = len(c["pulses"])
    nil = (0.0, 0.0, 0.0)
    unweighted = dict(c, w=[None if w is None else nil for w in c["w"]], wf=[None if w is None else nil for w in c["wf"]])
    for d, i in _lm(unweighted, bs, [0.0] * P):
        assert i["status"] == "breakdown" and i["ncg"] == 0 and np.array_equal(d, np.zeros_like(d))
        assert i["loss"] == 0.0 and np.array_equal(i["grad"], np.zeros_like(d))

    def first_scale(tri):
        return None if tri is None else tuple(np.asarray(x)[:1] for x in tri)

    s0 = dict(c, scales=(0.0,), w=[first_scale(t) for t in c["w"]], t=[first_scale(t) for t in c["t"]],
              wf=[first_scale(t) for t in c["wf"]], tf=[first_scale(t) for t in c["tf"]])
    for (d, i), b, m in zip(_lm(s0, bs, mus, trial=False), bs, mus):
        # alpha = <b, b> / <b, mu b>: two sums of n positive terms, each term rounded twice at the most, one division, and one more
        # rounding each in alpha b and b / mu: (2 n + 8) u relative, and the residual b - alpha (mu b) is of that order
        tol = (2 * len(b) + 8) * 1.2e-16
        assert i["ncg"] == 1 and i["status"] == "rtol" and i["rr"] <= (2 * tol) ** 2 * i["gg"]
        assert np.abs(d - b / m).max() <= tol * np.abs(b / m).max()
    for d, i in _lm(c, [np.zeros_like(b) for b in bs], mus, trial=False):
        assert i["status"] == "rtol" and i["ncg"] == 0 and i["rr"] == 0.0 and i["gg"] == 0.0
        assert np.array_equal(d, np.zeros_like(d)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()


def _raw_tables(ntr, gains, phi, echo, meq):
    uq, gi = np.unique(gains, return_inverse=True)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([echo], dtype=np.int32), np.array([meq])]
    ip, lp, ptr = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp)), mbfir._ptr
    return tab, [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8])]


def test_outputs_are_written_in_full_and_nowhere_else():
    """The raw call with NaN sentinels: every entry of the wanted outputs is written, the 16 entries after them are not, the loss
    and gradient of a solve-only call are left alone, and the bits are the Python call's"""
    c, bs, mus, _ = _case("allgains")
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0]
    n, S, O = len(p[0]), 2, 2 * 6
    wf = tuple(np.full((S, 3, 2), 0.5 + i) for i in range(3))
    tf = tuple(np.full((S, 3, 2), 0.1 * i) for i in range(3))
    d = dict(c, wf=[wf], tf=[tf])
    (dw, iw), = _lm(d, bs, mus, cg=2, rtol=0.0)
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    A = mbfir._BlochArgs("raw", [p], df, dp, c["scales"])
    keep, targs = _raw_tables(ntr, c["gains"][0], c["phases"][0], c["echo"][0], c["meq"])
    m0 = A.m0_planes(c["m0"][0], np.array([0, O]), [1])
    flat = lambda tri: [np.ascontiguousarray(np.ravel(v)) for v in tri]
    w, t, wfp, tfp = flat(c["w"][0]), flat(c["t"][0]), flat(wf), flat(tf)
    b = [np.ascontiguousarray(bs[0].real), np.ascontiguousarray(bs[0].imag)]
    mu = np.array([mus[0]])
    for trial in (True, False):
        dr, di, gr, gi = (np.full(n + 16, np.nan) for _ in range(4))
        rr, gg, loss = (np.full(1 + 16, np.nan) for _ in range(3))
        ncg, status = (np.full(1 + 16, -7, dtype=np.int32) for _ in range(2))
        ip = lambda a: a.ctypes.data_as(mbfir._ip)
        rc = lib.mbfir_bloch_train_lm_step_batch(ctx._h, *A.head, *targs, int(c["demod"]), *[ptr(a) for a in m0], 0, *[ptr(a) for a in w],
                                                 None, *[ptr(a) for a in wfp], ptr(b[0]), ptr(b[1]), ptr(mu), 2, 0.0,
                                                 *[ptr(a) if trial else None for a in t + tfp], ptr(dr), ptr(di), ip(ncg), ptr(rr), ptr(gg),
                                                 ip(status), ptr(loss), ptr(gr), ptr(gi))
        assert rc == 0, ctx.last_error()
        assert np.array_equal(dr[:n] + 1j * di[:n], dw) and np.all(np.isnan(dr[n:])) and np.all(np.isnan(di[n:]))
        assert ncg[0] == iw["ncg"] == 2 and status[0] == 1 and np.all(ncg[1:] == -7) and np.all(status[1:] == -7)
        assert rr[0] == iw["rr"] and gg[0] == iw["gg"] and np.all(np.isnan(rr[1:])) and np.all(np.isnan(gg[1:]))
        if trial:
            assert loss[0] == iw["loss"] and np.all(np.isnan(loss[1:]))
            assert np.array_equal(gr[:n] + 1j * gi[:n], iw["grad"]) and np.all(np.isnan(gr[n:])) and np.all(np.isnan(gi[n:]))
        else:
            assert np.all(np.isnan(loss)) and np.all(np.isnan(gr)) and np.all(np.isnan(gi))


def test_errors_through_the_raw_call_in_their_order():
    """every MBFIR_E_ARG case with its message: the train's and the gn checks first, then a null array of the step's own, mu, cg,
    rtol, then the targets; a good call before and after"""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    who = "bloch_train_lm_step_batch:"
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    neg, nan, inf = np.r_[one[:5], -1.0, one[:58]], np.r_[one[:5], np.nan, one[:58]], np.r_[np.inf, one[:63]]
    rneg = np.r_[1.0, -1.0, one[:62]]
    mneg, mnan = np.r_[-1.0, one[:63]], np.r_[np.nan, one[:63]]      # one pulse: mu[0] is the one that is read
    o = [np.zeros(64) for _ in range(7)]
    k = [np.zeros(4, dtype=np.int32) for _ in range(2)]
    N3 = (None,) * 3

    def opt(a, f=p):
        return f(a) if a is not None else None

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, ntr=I(4), roff=L(0, 4),
             echo=I(2), ebcast=0, w=(one,) * 3, rw=None, wf=(one,) * 3, b=(d, d), mu=one, cg=2, rtol=1e-6, t=(d,) * 3, tf=(d,) * 3,
             out=(o[4], o[5], o[6]), first=None):
        res = [p(o[0]), p(o[1]), ip(k[0]), p(o[2]), p(o[3]), ip(k[1])] + [opt(a) for a in out]
        if first is not None:
            res[first] = None
        return lib.mbfir_bloch_train_lm_step_batch(
            ctx._h, npulse, lp(toff), p(d), p(d), None, None, None, lp(tsoff), p(d), p(one), p(one), p(one), nfgrid, lp(foff), p(d), npgrid,
            lp(poff), p(d), None, None, nscale, p(one), opt(ntr, ip), lp(roff), p(one), p(np.zeros(64)), ip(I(0, 1, 1, 0)), lp(L(0, 2)),
            p(np.array([0.5, 1.0])), opt(echo, ip), p(one), 0, None, None, None, ebcast, *[opt(a) for a in w], opt(rw),
            *[opt(a) for a in wf], *[opt(a) for a in b], opt(mu), cg, rtol, *[opt(a) for a in t], *[opt(a) for a in tf], *res)

    cases = ((dict(npulse=0), "no pulses"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
             (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(ebcast=2), "ebcast must be 0 or 1"),
             (dict(w=(one, None, one)), "the echo weights are given together"), (dict(wf=(None, one, one)), "the final weights are given together"),
             (dict(w=N3, wf=N3, t=N3, tf=N3), "neither an echo term nor a final term"),
             (dict(w=(one, neg, one)), "a weight is negative"), (dict(wf=(nan, one, one)), "a weight is negative or not finite"),
             (dict(rw=rneg), "a repetition weight is negative or not finite"),
             (dict(b=(None, d)), "required array is null"), (dict(b=(d, None)), "required array is null"),
             (dict(mu=None), "required array is null"), (dict(first=0), "required array is null"), (dict(first=2), "required array is null"),
             (dict(first=5), "required array is null"), (dict(out=(None, o[5], o[6])), "required array is null"),
             (dict(out=(o[4], o[5], None)), "required array is null"),
             (dict(t=(None, d, None), tf=N3, out=(None, None, None)), "required array is null"),
             (dict(mu=mneg), "mu is negative or not finite"), (dict(mu=mnan), "mu is negative or not finite"),
             (dict(mu=inf), "mu is negative or not finite"), (dict(cg=-1), "cg must be at least 0"),
             (dict(rtol=-1e-300), "rtol is negative or not a number"), (dict(rtol=float("nan")), "rtol is negative or not a number"),
             (dict(t=(None, d, d)), "tx, ty and tz are given together"), (dict(t=(d, d, None)), "tx, ty and tz are given together"),
             (dict(tf=(d, None, d)), "tfx, tfy and tfz are given together"),
             (dict(w=N3, tf=(d,) * 3), "a target is given for a term that has no weights"),
             (dict(wf=N3, t=(d,) * 3), "a target is given for a term that has no weights"),
             (dict(t=N3), "a term that has weights has no target"), (dict(tf=N3), "a term that has weights has no target"),
             # the order: each check hides the later ones
             (dict(ebcast=2, cg=-1), "ebcast"), (dict(w=(one, neg, one), b=(None, d)), "a weight is negative"),
             (dict(mu=None, t=(None, d, d)), "required array is null"), (dict(t=(d, None, d), mu=mneg), "mu is negative"),
             (dict(mu=mneg, cg=-1, rtol=-1.0), "mu is negative"), (dict(cg=-1, rtol=-1.0), "cg must be"),
             (dict(rtol=-1.0, t=(None, d, d)), "rtol is negative"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0
    assert call(t=N3, tf=N3, out=(None, None, None)) == 0                  # solve only
    assert call(w=N3, t=N3) == 0 and call(wf=N3, tf=N3) == 0 and call(ebcast=1, rw=one) == 0
    assert call(cg=0) == 0 and call(rtol=float("inf")) == 0 and call(mu=np.zeros(4)) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    kw = dict(phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2)
    tri = (1.0, 1.0, 1.0)
    tg = tuple(np.full((1, 4, 2, 3), 1e-5) for _ in range(3))
    tgf = tuple(np.full((1, 2, 3), 1e-5) for _ in range(3))
    (dw, iw), = mbfir.bloch_train_lm_step_batch([pulse], d[:2], d[:3], 4, [d[:3] * (1 + 1j)], [tri], 1.0, targets=[tg], targets_final=[tgf],
                                                weights_final=[tri], cg=2, **kw)
    assert call() == 0
    assert np.array_equal(o[0][:3] + 1j * o[1][:3], dw) and k[0][0] == iw["ncg"] and o[2][0] == iw["rr"] and o[3][0] == iw["gg"]
    assert o[4][0] == iw["loss"] and np.array_equal(o[5][:3] + 1j * o[6][:3], iw["grad"])


def test_refine_on_the_device_solver():
    """tests/test_blochtraingn_gpu.py's refine case: the 9-sample period, 3 x 2 points, 9 repetitions, three gains, two outer
    iterations.  The accepted losses fall, 'calls' counts the steps under 'lm', a pulse alone has its bits in a batch of three, and
    solver='host' is refine_bloch_train_batch."""
    c = ref.small()
    p = c["pulses"][0]
    rng = np.random.default_rng(5)
    ntr, gains = 9, np.tile([0.5, 0.75, 1.0], 3)
    pulses = [(p[0] * s,) + tuple(p[1:]) for s in (1.0, 0.9, 1.1)]
    w = (np.ones((3, 2)), np.ones((3, 2)), 0.5)
    tg = tuple(rng.uniform(-0.5, 0.5, (3, 2)) for _ in range(3))
    rw = np.r_[0.0, 0.0, np.ones(7)]
    kw = dict(rep_weights=rw, phases=np.pi, gains=gains, echo=c["echo"][0], m0=c["m0"][0], demod=True, iters=2, cg=4)
    args = (c["dfs"][0], c["dps"][0], ntr)
    b1s, infos = mbfir.refine_bloch_train_lm_batch(pulses, *args, [tg] * 3, [w] * 3, solver="device", **kw)
    for q in range(3):
        L = infos[q]["losses"]
        print("pulse %d: losses %s, refused %d, calls %s" % (q, ["%.6g" % v for v in L], infos[q]["refused"], infos[q]["calls"]))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
        cc = infos[q]["calls"]
        assert set(cc) == {"lsq", "gn", "lm"} and cc["lsq"] == 1 and cc["gn"] == 1 and cc["lm"] == len(L) - 1 + infos[q]["refused"]
        (b1,), (info,) = mbfir.refine_bloch_train_lm_batch([pulses[q]], *args, [tg], [w], solver="device", **kw)
        assert np.array_equal(b1, b1s[q]) and info == infos[q]
        (Lend, _), = mbfir.bloch_train_lsq_batch([(b1s[q],) + tuple(p[1:])], c["dfs"][0], c["dps"][0], ntr, [tg], [w], rep_weights=rw,
                                                 phases=np.pi, gains=gains, echo=c["echo"][0], m0=c["m0"][0], demod=True)
        assert Lend == L[-1]
    new = mbfir.refine_bloch_train_lm_batch(pulses, *args, [tg] * 3, [w] * 3, solver="host", **kw)
    old = mbfir.refine_bloch_train_batch(pulses, *args, [tg] * 3, [w] * 3, **kw)
    for q in range(3):
        assert np.array_equal(new[0][q], old[0][q]) and new[1][q] == old[1][q] and set(new[1][q]["calls"]) == {"lsq", "gn"}
