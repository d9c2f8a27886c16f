"""The Levenberg-Marquardt step of the pulse train's schedule evaluated and solved on the device
(mbfir.bloch_train_lm_step_sched_batch: the shipped k_bloch_train_prop, k_bloch_train_prop_dgain, k_bloch_train_run_sched_lsq and
k_bloch_train_sched_gn_fold, then k_bloch_train_lm_sched_init and the rounds of k_bloch_train_lm_sched_run and
k_bloch_train_lm_sched_step) and mbfir.refine_bloch_train_sched_lm_batch on it, following tests/test_blochtrainlm_gpu.py's plan.  The
cases are blochtrainsched_ref.cases() and small() as blochtrainschedgn_ref dresses them, and 'stride' (one sample, one point, ntr =
257: the step kernel's second stride and the run kernel's second staged chunk).  No case has an exactly zero gradient or operator
(tests/test_blochtrainschedlm_cpu.py holds that on the reference), so none is given another right-hand side.  A schedule's vector
is carried as dg + i dp.

Exact, without a tolerance: the loss and gradient are bloch_train_lsq_sched_batch's at the call's schedule; cg = 0 is that call and
d = 0; the first iteration follows from one shipped bloch_train_gn_sched_batch product at K = 1 and the step kernel's arithmetic
restated in NumPy (this holds the body moved into sim_dev.h to the bits of the shipped product); d from the device's own -g is d
from a solve-only call given -g; a pulse's outputs do not depend on the batch, its order or a repeated call; with vary=("phases",)
the outputs follow from the shipped phases-only product, which never launches the period's tangent, and the gains' outputs are not
there; outputs are written in full and nowhere else.  Against the dense solve on small(): the project's 1e-4 max|d|.  Against the
recurrence of tests/simlm_ref.py (cg_solve) run on the shipped bloch_train_gn_sched_batch as the operator: ncg and status equal, and
for d, rr and gg the bounds that tests/test_blochlm_gpu.py derives in its docstring, the perturbation measured on code that is not
under test (the same recurrence on blochtrainschedgn_ref.gn in float64 against the recurrence on the device product):
    |d - d_ref| <= max(100 max over the case's cg of |d_ref(blochtrainschedgn_ref) - d_ref(device gn)|, 1e-13 max|d_ref|)
    |rr - rr_ref| <= 2 sqrt(rr_ref) dr + dr^2 + 2e-13 sqrt(rr_ref gg) + 1e-26 gg,   dr = (trace(H) + mu) sqrt(2 ntr) (the bound on d)
gg is within 1e-14 relative.  DESIGN 8ag has the figures measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainschedlm_ref", os.path.join(ROOT, "tests", "blochtrainschedlm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
_dot = lmref.dot
NAMES = lmref.names()
PAIRS = [(name, q) for name in NAMES for q in range(len(lmref.case_of(name)["pulses"]))]
BOTH, GAINS, PHASES = lmref.VARIES


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _opt(v):
    return None if v[0] is None else list(v)


def _kw(c):
    return dict(phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"], m0=_opt(c["m0"]),
                meq=c["meq"], demod=c["demod"], rep_weights=None if c["rw"] is None else list(c["rw"]), weights_final=_opt(c["wf"]))


def _cx(a, b):
    """two halves, either None -> a + i b"""
    n = len(a if a is not None else b)
    return (np.zeros(n) if a is None else a) + 1j * (np.zeros(n) if b is None else b)


def _halves(v, vary):
    return (np.ascontiguousarray(v.real) if "gains" in vary else None, np.ascontiguousarray(v.imag) if "phases" in vary else None)


def _lsq(c, vary=BOTH):
    """the shipped call: [(L, g)], g = gg + i gp with zeros for a half not asked for"""
    df, dp = _grids(c)
    res = mbfir.bloch_train_lsq_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["t"]), _opt(c["w"]), targets_final=_opt(c["tf"]),
                                            grad_gains="gains" in vary, grad_phases="phases" in vary, **_kw(c))
    return [(L, _cx(gg, gp)) for L, gg, gp in res]


def _gn(c, vs, vary=BOTH):
    """the shipped product at K = 1 along vs[q] = dg + i dp, only the varied halves given and asked for"""
    df, dp = _grids(c)
    hv = [_halves(np.asarray(v), vary) for v in vs]
    res = mbfir.bloch_train_gn_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["w"]),
                                           tangents_gains=[h[0] for h in hv] if "gains" in vary else None,
                                           tangents_phases=[h[1] for h in hv] if "phases" in vary else None,
                                           prod_gains="gains" in vary, prod_phases="phases" in vary, **_kw(c))
    return [_cx(a, b) for a, b in res]


def _lm(c, mus, bs=None, vary=BOTH, evaluate=True, **over):
    """the call under test: [(d, info)] with d = dg + i dp and, with evaluate, info['grad'] = gg + i gp"""
    df, dp = _grids(c)
    kw = _kw(c)
    kw.update(over)
    if evaluate:
        kw.update(targets=_opt(c["t"]), targets_final=_opt(c["tf"]))
    res = mbfir.bloch_train_lm_step_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["w"]), list(mus), vary=vary,
                                                b=None if bs is None else [_halves(b, vary) for b in bs], **kw)
    out = []
    for dg, dph, info in res:
        assert (dg is None) == ("gains" not in vary) and (dph is None) == ("phases" not in vary)
        info = dict(info)
        if "loss" in info:
            assert (info["grad_gains"] is None) == (dg is None) and (info["grad_phases"] is None) == (dph is None)
            info["grad"] = _cx(info.pop("grad_gains"), info.pop("grad_phases"))
        out.append((_cx(dg, dph), info))
    return out


@functools.lru_cache(maxsize=None)
def _case(name, vary=BOTH):
    """the case with, per pulse, b = -gradient at its schedule and mu = 1e-3 times the Rayleigh quotient of H at b, from the shipped
    device calls: (case, bs, mus, the lsq results)"""
    c = lmref.case_of(name)
    at = _lsq(c, vary)
    bs, mus = lmref.rhs_and_mu([g for _, g in at], lambda v: _gn(c, v, vary))
    assert all(_dot(b, b) > 0 for b in bs) and all(m > 0 for m in mus), name
    return c, bs, mus, at


def _one(name, q, vary=BOTH):
    c, bs, mus, _ = _case(name, vary)
    return lmref.sub(c, [q]), [bs[q]], [mus[q]]


def _same(a, b):
    """every output of a pulse, bit for bit"""
    (da, ia), (db, ib) = a, b
    keys = set(ia) & set(ib)
    assert {"ncg", "rr", "gg", "status"} <= keys
    return np.array_equal(da, db) and all(np.array_equal(ia[k], ib[k]) for k in keys)


@pytest.mark.parametrize("vary", lmref.VARIES)
@pytest.mark.parametrize("name", NAMES)
def test_evaluation_is_the_shipped_lsq_call_and_the_devices_own_rhs_is_minus_g(name, vary):
    """L and g are bloch_train_lsq_sched_batch's whatever the solve does; cg = 0 is that call and nothing more (d = 0, ncg = 0);
    rtol = 1e300 leaves every pulse idle; d from b = None (the device's -g) is d from a solve-only call given -g, state included;
    a given b does not change L and g."""
    c, bs, mus, at = _case(name, vary)
    for cg, rtol in ((0, 0.0), (3, 0.0), (3, 1e300)):
        got = _lm(c, mus, vary=vary, cg=cg, rtol=rtol)
        solve = _lm(c, mus, bs, vary=vary, evaluate=False, cg=cg, rtol=rtol)
        given = _lm(c, mus, [2.0 * b for b in bs], vary=vary, cg=cg, rtol=rtol)
        for (d, i), (L, g), (d0, i0), (_, i2), b in zip(got, at, solve, given, bs):
            assert i["loss"] == L and np.array_equal(i["grad"], g), (cg, rtol)
            assert i2["loss"] == L and np.array_equal(i2["grad"], g), (cg, rtol)
            assert "loss" not in i0 and _same((d, i), (d0, i0)), (cg, rtol)
            assert abs(i["gg"] - _dot(b, b)) <= 1e-14 * _dot(b, b)
            if cg == 0 or rtol > 1:
                assert np.array_equal(d, np.zeros_like(d)) and i["ncg"] == 0 and i["rr"] == i["gg"]
                assert i["status"] == ("rtol" if rtol > 1 else "cg")
            else:
                assert (i["ncg"] == cg and i["status"] == "cg") or (0 < i["ncg"] < cg and i["rr"] == 0.0 and i["status"] == "rtol")
                assert np.abs(d).max() > 0
            if vary == GAINS:
                assert not d.imag.any()
            if vary == PHASES:
                assert not d.real.any()


def _device_sum(v):
    """the step kernel's sum of one real per repetition: thread t adds repetitions t, t + 256, ... in order, then the fixed tree"""
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


@pytest.mark.parametrize("vary", lmref.VARIES)
@pytest.mark.parametrize("name", NAMES)
def test_first_iteration_has_the_bits_of_the_shipped_product(name, vary):
    """cg = 1, rtol = 0: H p of a running pulse is bloch_train_gn_sched_batch's on p = b, bit for bit, so gg, rr and d follow exactly
    from one shipped product and the step kernel's arithmetic restated in NumPy (every product and sum rounded once, the sums in
    the kernel's order).  With vary = ("phases",) the shipped product is the one that never launches the period's tangent."""
    c, bs, mus, _ = _case(name, vary)
    got = _lm(c, mus, bs, vary=vary, evaluate=False, cg=1, rtol=0.0)
    for (d, i), b, hb, mu in zip(got, bs, _gn(c, bs, vary), mus):
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
    bs, mus = lmref.rhs_and_mu([g for _, g in _lsq(c)], lambda v: _gn(c, v))

    def lm(idx, evaluate=True):
        return _lm(lmref.sub(c, idx), [mus[q] for q in idx], None if evaluate else [bs[q] for q in idx], evaluate=evaluate, cg=lmref.CG17,
                   rtol=lmref.RTOL17)

    full, again, rev, bare = lm(every), lm(every), lm(every[::-1])[::-1], lm(every, evaluate=False)
    print("iterations per pulse %s" % [i["ncg"] for _, i in full])
    for q in every:
        assert _same(full[q], again[q]) and _same(full[q], rev[q]) and _same(full[q], bare[q]), q
        assert "loss" in full[q][1] and "loss" not in bare[q][1]
        alone, = lm([q])
        assert _same(alone, full[q]) and alone[1]["loss"] == full[q][1]["loss"], q
    assert len(set(i["ncg"] for _, i in full)) > 1                   # the pulses of the batch do not all stop together


@pytest.mark.parametrize("name", ["batch", "shared", "groups"])
def test_a_pulse_of_the_cases_alone_has_its_bits_in_the_batch(name):
    c, bs, mus, _ = _case(name)
    full = _lm(c, mus, cg=3, rtol=1e-3)
    for q in range(len(c["pulses"])):
        c1, _, m = _one(name, q)
        alone, = _lm(c1, m, cg=3, rtol=1e-3)
        assert _same(alone, full[q]), q


def _dense_h(c1, vary=BOTH):
    """H of one pulse on the varied halves from shipped gn products, real form [gains; phases] of the varied halves"""
    n = c1["ntr"][0]
    _, _, H = mbfir.bloch_train_normal_sched_batch(c1["pulses"], c1["dfs"][0], c1["dps"][0], n, _opt(c1["t"]), _opt(c1["w"]), vary=vary,
                                                   targets_final=_opt(c1["tf"]), **_kw(c1))[0]
    return H


def _pack(v, vary):
    return np.concatenate([h for h in _halves(v, vary) if h is not None])


@pytest.mark.parametrize("vary", lmref.VARIES)
def test_step_is_the_dense_solve_on_small(vary):
    """H from the shipped gn products, mu = 1e-2 trace(H) / n, cg = 4 n, rtol = 1e-16: within 1e-4 of max|d|"""
    c1, b, _ = _one("small", 0, vary)
    H = _dense_h(c1, vary)
    n = H.shape[0]
    assert n == c1["ntr"][0] * len(vary) and np.trace(H) > 0
    mu = 1e-2 * np.trace(H) / n
    want = np.linalg.solve(H + mu * np.eye(n), _pack(b[0], vary))
    (d, i), = _lm(c1, [mu], b, vary=vary, evaluate=False, cg=4 * n, rtol=1e-16)
    err = np.abs(_pack(d, vary) - want).max() / np.abs(want).max()
    print("%s: step against the dense solve %.3g after %d iterations (%s), condition number %.0f"
          % (vary, err, i["ncg"], i["status"], np.linalg.cond(H + mu * np.eye(n))))
    assert err <= 1e-4


def _recurrences(c1, b, mu, caps):
    """cg_solve at every cap on the shipped product and on the float64 reference, the products of a smaller cap shared"""
    @functools.lru_cache(maxsize=None)
    def shipped_of(key):
        return _gn(c1, [np.frombuffer(key, dtype=complex)])[0]

    @functools.lru_cache(maxsize=None)
    def numpy_of(key):
        return lmref.gn(c1, 0, np.frombuffer(key, dtype=complex))

    shipped, numpy = (lambda v: shipped_of(v.tobytes())), (lambda v: numpy_of(v.tobytes()))
    return ({cg: lmref.cg_solve(shipped, b, mu, cg, 0.0) for cg in caps}, {cg: lmref.cg_solve(numpy, b, mu, cg, 0.0) for cg in caps})


@pytest.mark.parametrize("name,q", PAIRS)
def test_step_is_the_recurrence_on_the_shipped_operator(name, q):
    """cg in 1, 2, 3, 8 with rtol = 0 (the module's docstring has the bounds); one pulse per case.  Of these the caps below 2 ntr, the
    number of real unknowns: in exact arithmetic the residual is zero after 2 ntr iterations at the latest, so from there on the
    recurrence runs on rounding noise.  The single repetition is held at cg = 1."""
    c1, (b,), (mu,) = _one(name, q)
    n = len(b)
    CGS = tuple(cg for cg in (1, 2, 3, 8) if cg < 2 * n)
    assert CGS[0] == 1
    got = {cg: _lm(c1, [mu], [b], evaluate=False, cg=cg, rtol=0.0)[0] for cg in CGS}
    on_dev, on_ref = _recurrences(c1, b, mu, CGS)
    scale = max(np.abs(on_dev[cg][0]).max() for cg in CGS)
    spread = max(np.abs(on_dev[cg][0] - on_ref[cg][0]).max() for cg in CGS)
    bound = max(100 * spread, 1e-13 * scale)
    trace = float(np.trace(_dense_h(c1)))
    dr = (trace + mu) * np.sqrt(2 * n) * bound
    for cg in CGS:
        (d, i), (d0, i0) = got[cg], on_dev[cg]
        err = float(np.abs(d - d0).max())
        rr_spread = abs(on_ref[cg][1]["rr"] - i0["rr"])
        rr_bound = 2 * np.sqrt(i0["rr"]) * dr + dr * dr + 2e-13 * np.sqrt(i0["rr"] * i0["gg"]) + 1e-26 * i0["gg"]
        rr_err = abs(i["rr"] - i0["rr"])
        print("%s pulse %d ntr %d cg %d: |d - recurrence| %.3g, the two references apart %.3g, bound %.3g, share %.3g (max|d| %.3g); "
              "rr %.6g, |rr - recurrence| %.3g, references apart %.3g, bound %.3g, share %.3g; ncg %d (%d)"
              % (name, q, n, cg, err, spread, bound, err / bound if bound else 0.0, scale, i0["rr"], rr_err, rr_spread, rr_bound,
                 rr_err / rr_bound if rr_bound else 0.0, i["ncg"], i0["ncg"]))
        assert i["ncg"] == i0["ncg"] and i["status"] == i0["status"], cg
        assert abs(i["gg"] - i0["gg"]) <= 1e-14 * i0["gg"], cg
        assert err <= bound, cg
        assert rr_err <= rr_bound, cg


@pytest.mark.parametrize("name,q", [(name, q) for name, q in PAIRS if 2 * lmref.case_of(name)["ntr"][q] <= 8])
def test_short_trains_past_exact_convergence(name, q):
    """The caps the recurrence test leaves out, those of 2, 3, 8 that are >= 2 ntr = n0, on every train of at most four repetitions
    (the one-sample periods 'one', 'hard' and the third pulse of 'shared' among them): in exact arithmetic the residual is zero
    after n0 iterations.  d is held to the recurrence on the shipped product at cg = n0 with the recurrence
    test's bound, plus what later iterations can still move it by; the status and ncg are the recurrence's, or the device's residual
    is below 1e-28 gg; a pulse that stopped at an exact zero has the d of cg = n0 whatever the cap."""
    c1, (b,), (mu,) = _one(name, q)
    n0 = 2 * len(b)
    caps = [n0] + [cg for cg in (2, 3, 8) if cg > n0]
    shipped = lambda v: _gn(c1, [v])[0]
    numpy = lambda v: lmref.gn(c1, 0, v)
    d2, i2 = lmref.cg_solve(shipped, b, mu, n0, 0.0)
    bound = max(100 * np.abs(d2 - lmref.cg_solve(numpy, b, mu, n0, 0.0)[0]).max(), 1e-13 * np.abs(d2).max())
    got = {cg: _lm(c1, [mu], [b], evaluate=False, cg=cg, rtol=0.0)[0] for cg in caps}
    for cg, (d, i) in got.items():
        d0, i0 = lmref.cg_solve(shipped, b, mu, cg, 0.0)
        print("%s pulse %d cg %d: ncg %d (%d), status %s (%s), rr / gg %.3g (%.3g), |d - d(cg = %d)| %.3g, bound %.3g"
              % (name, q, cg, i["ncg"], i0["ncg"], i["status"], i0["status"], i["rr"] / i["gg"], i0["rr"] / i0["gg"], n0,
                 np.abs(d - d2).max(), bound))
        assert 1 <= i["ncg"] <= cg and abs(i["gg"] - i0["gg"]) <= 1e-14 * i0["gg"]
        assert (i["status"] == i0["status"] and i["ncg"] == i0["ncg"]) or i["rr"] <= 1e-28 * i["gg"]
        # iterations past exact convergence solve (H + mu I) delta = r for the residual left, and H >= 0: |delta| <= |r| / mu
        slack = np.sqrt(max(got[n0][1]["rr"], i2["rr"])) / mu
        assert np.abs(d - d2).max() <= bound + slack
        if i["status"] == "rtol":
            assert i["rr"] == 0.0


@pytest.mark.parametrize("name", ["small", "batch", "allgains", "stride"])
def test_breakdown_and_a_vanishing_operator(name):
    """All-zero weights and mu = 0: <p, (H + mu) p> = 0, status 'breakdown', d = 0, ncg = 0.  scales = (0.0,) with mu > 0: without RF
    neither a gain nor a phase moves anything, H vanishes (to the rounding of a commutator squared), so d = b / mu after one round."""
    c, bs, mus, _ = _case(name)
    P = len(c["pulses"])
    nil = (0.0, 0.0, 0.0)
    unweighted = dict(c, w=[None if w is None else nil for w in c["w"]], wf=[None if w is None else nil for w in c["wf"]])
    for d, i in _lm(unweighted, [0.0] * P, bs):
        assert i["status"] == "breakdown" and i["ncg"] == 0 and np.array_equal(d, np.zeros_like(d))
        assert i["loss"] == 0.0 and np.array_equal(i["grad"], np.zeros_like(d))

    def first_scale(tri):
        return None if tri is None else tuple(np.asarray(x)[:1] for x in tri)

    s0 = dict(c, scales=(0.0,), w=[first_scale(t) for t in c["w"]], t=[first_scale(t) for t in c["t"]],
              wf=[first_scale(t) for t in c["wf"]], tf=[first_scale(t) for t in c["tf"]])
    for (d, i), b, m in zip(_lm(s0, mus, bs, evaluate=False), bs, mus):
        # alpha = <b, b> / <b, mu b>: two sums of 2 ntr positive terms, each term rounded twice at the most, one division, and one
        # more rounding each in alpha b and b / mu: (4 ntr + 8) u relative, and the residual b - alpha (mu b) is of that order
        tol = (4 * len(b) + 8) * 1.2e-16
        assert i["ncg"] == 1 and i["status"] == "rtol" and i["rr"] <= (2 * tol) ** 2 * i["gg"]
        assert np.abs(d - b / m).max() <= tol * np.abs(b / m).max()
    for d, i in _lm(c, mus, [np.zeros_like(b) for b in bs], evaluate=False):
        assert i["status"] == "rtol" and i["ncg"] == 0 and i["rr"] == 0.0 and i["gg"] == 0.0
        assert np.array_equal(d, np.zeros_like(d)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()


def _raw_tables(ntr, gains, phi, echo, meq):
    uq, gi = np.unique(gains, return_inverse=True)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([echo], dtype=np.int32), np.array([meq])]
    ip, lp, ptr = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp)), mbfir._ptr
    return tab, [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8])]


@pytest.mark.parametrize("name", ["allgains", "stride"])
def test_outputs_are_written_in_full_and_nowhere_else(name):
    """The raw call with NaN sentinels, for every vary and with and without targets: every entry of the wanted outputs is written,
    the 16 entries after them are not, the loss and gradient of a solve-only call and the arrays of a half that does not vary (which
    the call is not given) are left alone, and the bits are the Python call's"""
    c = lmref.case_of(name)
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0]
    S, npt = len(c["scales"]), len(c["dfs"][0]) * len(c["dps"][0])
    O = S * npt
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    A = mbfir._BlochArgs("raw", [p], df, dp, c["scales"])
    keep, targs = _raw_tables(ntr, c["gains"][0], c["phases"][0], c["echo"][0], c["meq"])
    m0 = A.m0_planes(c["m0"][0], np.array([0, O]), [1])
    flat = lambda tri: [None] * 3 if tri is None else [np.ascontiguousarray(np.ravel(v)) for v in tri]
    w, t, wfp, tfp = flat(c["w"][0]), flat(c["t"][0]), flat(c["wf"][0]), flat(c["tf"][0])
    opt = lambda a: None if a is None else ptr(a)
    rw = None if c["rw"] is None else np.ascontiguousarray(c["rw"][0])
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    for vary in lmref.VARIES:
        _, bs, mus, _ = _case(name, vary)
        vg, vp = lmref.flags(vary)
        mu = np.array([mus[0]])
        for evaluate in (True, False):
            (dw, iw), = _lm(c, mus, None if evaluate else bs, vary=vary, evaluate=evaluate, cg=2, rtol=0.0)
            b = _halves(bs[0], vary)
            dg, dph, gg_, gp_ = (np.full(ntr + 16, np.nan) for _ in range(4))
            rr, gg, loss = (np.full(1 + 16, np.nan) for _ in range(3))
            ncg, status = (np.full(1 + 16, -7, dtype=np.int32) for _ in range(2))
            rc = lib.mbfir_bloch_train_lm_step_sched_batch(
                ctx._h, *A.head, *targs, int(c["demod"]), *[ptr(a) for a in m0], 0, *[opt(a) for a in w],
                *[opt(a) if evaluate else None for a in t], opt(rw), *[opt(a) for a in wfp],
                *[opt(a) if evaluate else None for a in tfp], *[None if evaluate or h is None else ptr(h) for h in b], ptr(mu), 2, 0.0,
                ptr(dg) if vg else None, ptr(dph) if vp else None, ip(ncg), ptr(rr), ptr(gg), ip(status),
                ptr(loss) if evaluate else None, ptr(gg_) if evaluate and vg else None, ptr(gp_) if evaluate and vp else None)
            assert rc == 0, ctx.last_error()
            for arr, want, on in ((dg, dw.real, vg), (dph, dw.imag, vp)):
                assert (np.array_equal(arr[:ntr], want) and np.all(np.isnan(arr[ntr:]))) if on else np.all(np.isnan(arr))
            assert ncg[0] == iw["ncg"] == 2 and status[0] == 1 and np.all(ncg[1:] == -7) and np.all(status[1:] == -7)
            assert rr[0] == iw["rr"] and gg[0] == iw["gg"] and np.all(np.isnan(rr[1:])) and np.all(np.isnan(gg[1:]))
            if evaluate:
                assert loss[0] == iw["loss"] and np.all(np.isnan(loss[1:]))
                for arr, want, on in ((gg_, iw["grad"].real, vg), (gp_, iw["grad"].imag, vp)):
                    assert (np.array_equal(arr[:ntr], want) and np.all(np.isnan(arr[ntr:]))) if on else np.all(np.isnan(arr))
            else:
                assert np.all(np.isnan(loss)) and np.all(np.isnan(gg_)) and np.all(np.isnan(gp_))


def test_errors_through_the_raw_call_in_their_order():
    """every MBFIR_E_ARG case with its message: the train's checks (sizes that overflow among them) and those the lsq and gn calls of
    the schedule share first, then a null array of the step's own, mu, cg, rtol, then the halves, the targets and the right-hand
    side; a good call before and after.  The sizes: the train's echo entries, the train's workgroups, and a case that passes the
    train's checks and trips bloch_train_sched_gn_check on the checkpoints of two states where those of one state would fit (what
    the run kernel writes; the shipped lsq call checks one).  bloch_lm_check's bound on roff (2^52 repetitions, a sum of ints) is
    out of reach of a call whose tables must exist."""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    who = "bloch_train_lm_step_sched_batch:"
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
    N2, N3 = (None,) * 2, (None,) * 3
    big = 2 ** 31 - 1
    long_tab = (np.ones(2 ** 19), np.zeros(2 ** 19), np.zeros(2 ** 19, dtype=np.int32), L(0, 1), np.array([1.0]))

    def opt(a, f=p):
        return f(a) if a is not None else None

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, ntr=I(4), roff=L(0, 4),
             echo=I(2), ebcast=0, w=(one,) * 3, rw=None, wf=(one,) * 3, b=N2, mu=one, cg=2, rtol=1e-6, t=(d,) * 3, tf=(d,) * 3,
             dd=(o[0], o[1]), out=(o[4], o[5], o[6]), first=None, h=ctx._h,
             tables=(one, np.zeros(64), I(0, 1, 1, 0), L(0, 2), np.array([0.5, 1.0]))):
        res = [ip(k[0]), p(o[2]), p(o[3]), ip(k[1])]
        if first is not None:
            res[first] = None
        return lib.mbfir_bloch_train_lm_step_sched_batch(
            h, npulse, lp(toff), p(d), p(d), None, None, None, lp(tsoff), p(d), p(one), p(one), p(one), nfgrid, lp(foff), p(d), npgrid,
            lp(poff), p(d), None, None, nscale, p(one), opt(ntr, ip), lp(roff), p(tables[0]), p(tables[1]), ip(tables[2]), lp(tables[3]),
            p(tables[4]), opt(echo, ip), p(one), 0, None, None, None, ebcast, *[opt(a) for a in w], *[opt(a) for a in t],
            opt(rw), *[opt(a) for a in wf], *[opt(a) for a in tf], *[opt(a) for a in b], opt(mu), cg, rtol, *[opt(a) for a in dd], *res,
            *[opt(a) for a in out])

    cases = ((dict(npulse=0), "no pulses"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
             (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(ebcast=2), "ebcast must be 0 or 1"),
             (dict(w=(one, None, one)), "the echo weights are given together"), (dict(wf=(None, one, one)), "the final weights are given together"),
             (dict(w=N3, wf=N3, t=N3, tf=N3, b=(d, d)), "neither an echo term nor a final term"),
             # 2^30 points x 2^31 - 1 repetitions: the echo entries pass 2^56 in the train's own check, before a table is read;
             # 2^40 points: 2^32 workgroups
             (dict(ntr=I(big), roff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
             (dict(foff=L(0, 2 ** 20), poff=L(0, 2 ** 20)), "overflows"),
             (dict(dd=N2, out=(o[4], None, None)), "neither the gains nor the phases vary"),
             # one point, 2^30 scales, 2^19 repetitions at one gain: the train's own checks pass (2^49 echo entries, 2^30 workgroups)
             # and read the tables, which are as long as ntr says; the checkpoints of two states per group of 8 repetitions are
             # 2^30 x 2^16 x 1536 doubles, past 2^56, where those of one state are not; no plane is read before
             (dict(foff=L(0, 1), poff=L(0, 1), nscale=2 ** 30, ntr=I(2 ** 19), roff=L(0, 2 ** 19), tables=long_tab), "overflows"),
             (dict(w=(one, neg, one)), "a weight is negative"), (dict(wf=(nan, one, one)), "a weight is negative or not finite"),
             (dict(rw=rneg), "a repetition weight is negative or not finite"),
             (dict(mu=None), "required array is null"), (dict(first=0), "required array is null"), (dict(first=1), "required array is null"),
             (dict(first=2), "required array is null"), (dict(first=3), "required array is null"),
             (dict(out=(None, o[5], o[6])), "required array is null"), (dict(out=(o[4], None, o[6])), "required array is null"),
             (dict(out=(o[4], o[5], None)), "required array is null"),
             (dict(t=(None, d, None), tf=N3, out=N3), "required array is null"),
             (dict(mu=mneg), "mu is negative or not finite"), (dict(mu=mnan), "mu is negative or not finite"),
             (dict(mu=inf), "mu is negative or not finite"), (dict(cg=-1), "cg must be at least 0"),
             (dict(rtol=-1e-300), "rtol is negative or not a number"), (dict(rtol=float("nan")), "rtol is negative or not a number"),
             (dict(dd=(None, o[1]), out=(o[4], o[5], o[6])), "for a half that does not vary"),
             (dict(dd=(o[0], None), out=(o[4], o[5], o[6])), "for a half that does not vary"),
             (dict(dd=(None, o[1]), out=(o[4], None, o[6]), b=(d, d)), "for a half that does not vary"),
             (dict(dd=(o[0], None), out=(o[4], o[5], None), b=(d, d)), "for a half that does not vary"),
             (dict(t=(None, d, d)), "tx, ty and tz are given together"), (dict(t=(d, d, None)), "tx, ty and tz are given together"),
             (dict(tf=(d, None, d)), "tfx, tfy and tfz are given together"),
             (dict(w=N3, tf=(d,) * 3), "a target is given for a term that has no weights"),
             (dict(wf=N3, t=(d,) * 3), "a target is given for a term that has no weights"),
             (dict(t=N3), "a term that has weights has no target"), (dict(tf=N3), "a term that has weights has no target"),
             (dict(b=(d, None)), "for every half that varies or not at all"), (dict(b=(None, d)), "for every half that varies or not at all"),
             (dict(t=N3, tf=N3, out=N3), "neither targets nor a right-hand side"),
             # the order: each check hides the later ones
             (dict(foff=L(0, 2 ** 20), poff=L(0, 2 ** 20), ebcast=2, w=(one, neg, one)), "overflows"),
             (dict(ntr=I(big), roff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15), dd=N2, mu=None), "overflows"),
             (dict(foff=L(0, 1), poff=L(0, 1), nscale=2 ** 30, ntr=I(2 ** 19), roff=L(0, 2 ** 19), tables=long_tab, ebcast=2), "ebcast"),
             (dict(foff=L(0, 1), poff=L(0, 1), nscale=2 ** 30, ntr=I(2 ** 19), roff=L(0, 2 ** 19), tables=long_tab, mu=None), "overflows"),
             (dict(ebcast=2, cg=-1), "ebcast"), (dict(w=(one, neg, one), mu=None), "a weight is negative"),
             (dict(mu=None, t=(None, d, d)), "required array is null"), (dict(t=(d, None, d), mu=mneg), "mu is negative"),
             (dict(mu=mneg, cg=-1, rtol=-1.0), "mu is negative"), (dict(cg=-1, rtol=-1.0), "cg must be"),
             (dict(rtol=-1.0, t=(None, d, d)), "rtol is negative"), (dict(t=(None, d, d), b=(d, None)), "tx, ty and tz"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
    assert call(h=None) == mbfir.E_ARG
    assert call() == 0
    assert call(t=N3, tf=N3, out=N3, b=(d, d)) == 0                        # solve only
    assert call(b=(d, d)) == 0                                             # b given, still evaluated
    assert call(w=N3, t=N3) == 0 and call(wf=N3, tf=N3) == 0 and call(ebcast=1, rw=one) == 0
    assert call(dd=(o[0], None), out=(o[4], o[5], None)) == 0 and call(dd=(None, o[1]), out=(o[4], None, o[6])) == 0
    assert call(dd=(None, o[1]), out=N3, t=N3, tf=N3, b=(None, d)) == 0
    assert call(cg=0) == 0 and call(rtol=float("inf")) == 0 and call(mu=np.zeros(4)) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    kw = dict(phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2)
    tri = (1.0, 1.0, 1.0)
    tg = tuple(np.full((1, 4, 2, 3), 1e-5) for _ in range(3))
    tgf = tuple(np.full((1, 2, 3), 1e-5) for _ in range(3))
    (dgw, dpw, iw), = mbfir.bloch_train_lm_step_sched_batch([pulse], d[:2], d[:3], 4, [tri], 1.0, targets=[tg], targets_final=[tgf],
                                                           weights_final=[tri], cg=2, **kw)
    assert call() == 0
    assert np.array_equal(o[0][:4], dgw) and np.array_equal(o[1][:4], dpw) and k[0][0] == iw["ncg"] and o[2][0] == iw["rr"]
    assert o[3][0] == iw["gg"] and o[4][0] == iw["loss"] and np.array_equal(o[5][:4], iw["grad_gains"])
    assert np.array_equal(o[6][:4], iw["grad_phases"])


def _refine_case():
    """tests/test_blochtrainschedgn_gpu.py's refine shape: the 9-sample period, 3 x 2 points, 9 repetitions, three gains, three pulses;
    also as a case of the reference (point-sized planes, the broadcast form)"""
    c0 = lmref.gnref.small()
    p = c0["pulses"][0]
    rng = np.random.default_rng(5)
    ntr, gains = 9, np.tile([0.5, 0.75, 1.0], 3)
    pulses = [(p[0] * s,) + tuple(p[1:]) for s in (1.0, 0.9, 1.1)]
    w = (np.ones((3, 2)), np.ones((3, 2)), 0.5)
    tg = tuple(rng.uniform(-0.5, 0.5, (3, 2)) for _ in range(3))
    rw = np.r_[0.0, 0.0, np.ones(7)]
    kw = dict(rep_weights=rw, phases=np.pi, gains=gains, echo=c0["echo"][0], m0=c0["m0"][0], demod=True)
    args = (c0["dfs"][0], c0["dps"][0], ntr)
    plane = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (1, 3, 2)).copy()
    case = dict(pulses=pulses, dfs=[c0["dfs"][0]] * 3, dps=[c0["dps"][0]] * 3, ntr=[ntr] * 3, phases=[np.pi * np.arange(ntr)] * 3,
                gains=[gains] * 3, echo=[c0["echo"][0]] * 3, m0=[c0["m0"][0]] * 3, scales=(1.0,), cot="echo", demod=True, meq=1.0,
                bcast=True, w=[tuple(plane(v) for v in w)] * 3, t=[tuple(plane(v) for v in tg)] * 3, wf=[None] * 3, tf=[None] * 3,
                rw=[rw] * 3, ce=[None] * 3, cf=[None] * 3)
    return pulses, args, tg, w, kw, case


def test_refine_host_is_the_shipped_refinement():
    pulses, args, tg, w, kw, _ = _refine_case()
    for vary in (BOTH, GAINS):
        new = mbfir.refine_bloch_train_sched_lm_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, solver="host", **kw)
        old = mbfir.refine_bloch_train_sched_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, **kw)
        for q in range(3):
            assert np.array_equal(new[0][q][0], old[0][q][0]) and np.array_equal(new[0][q][1], old[0][q][1])
            assert new[1][q] == old[1][q] and set(new[1][q]["calls"]) == {"lsq", "gn"}


@pytest.mark.parametrize("vary", [BOTH, GAINS])
def test_refine_on_the_device_solver(vary):
    """solver='device' at cg = 4 n, two outer iterations: the losses fall, as many steps are accepted as by the host solver, a pulse
    alone has its bits in the batch of three, 'calls' counts at most two fused calls per step taken and one more than the steps when
    nothing was refused, and the final loss is the host solver's within a margin measured on code not under test: the host loop
    (dense Cholesky) on the float64 reference's H and gradient against the same loop on the device's, times 100.  The CG tolerance is
    set to rtol = 1e-24, so that the step is the solve and not its first digits.  Measured on one MI355X: |L - L host| is at most
    2.8e-13 at L = 9.26 (both halves, pulse 1) against its margin of 3.6e-13, 0.79 of it; the other five (pulse, vary) pairs take at
    most 0.10 of margins of 3.6e-13 to 1.2e-12; every run accepts two steps, refuses none and takes three fused calls."""
    pulses, args, tg, w, kw, case = _refine_case()
    n = 9 * len(vary)
    host_s, host_i = mbfir.refine_bloch_train_sched_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, **kw)
    sch, infos = mbfir.refine_bloch_train_sched_lm_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, solver="device", cg=4 * n,
                                                         rtol=1e-24, **kw)
    for q in range(3):
        L, Lh = infos[q]["losses"], host_i[q]["losses"]
        _, Lr, _ = lmref.refine_dense(case, q, 2, vary)
        margin = 100 * abs(Lr[-1] - Lh[-1])
        cc, steps = infos[q]["calls"], len(L) - 1 + infos[q]["refused"]
        print("%s pulse %d: losses %s (host %s, reference loop %s), refused %d (host %d), calls %s; |L - L host| %.3g, margin %.3g, share %.3g"
              % (vary, q, ["%.9g" % v for v in L], ["%.9g" % v for v in Lh], ["%.9g" % v for v in Lr], infos[q]["refused"],
                 host_i[q]["refused"], cc, abs(L[-1] - Lh[-1]), margin, abs(L[-1] - Lh[-1]) / margin if margin else np.inf))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
        assert len(L) == len(Lh) and len(Lr) == len(Lh), q
        assert sch[q][0].shape == sch[q][1].shape == (9,)
        if vary == GAINS:
            assert np.array_equal(sch[q][1], np.pi * np.arange(9))
        assert set(cc) == {"lsq", "gn", "lm"} and cc["lsq"] == 1 and cc["gn"] == 1
        assert cc["lm"] <= 2 * steps and (infos[q]["refused"] > 0 or cc["lm"] == steps + 1), (q, cc)
        (one,), (info,) = mbfir.refine_bloch_train_sched_lm_batch([pulses[q]], *args, [tg], [w], vary=vary, iters=2, solver="device",
                                                                  cg=4 * n, rtol=1e-24, **kw)
        assert np.array_equal(one[0], sch[q][0]) and np.array_equal(one[1], sch[q][1]) and info == infos[q]
        assert abs(L[-1] - Lh[-1]) <= margin, (q, L[-1], Lh[-1], margin)
