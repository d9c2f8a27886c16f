"""The Levenberg-Marquardt step of the pulse train solved on the device, without one: the NumPy recurrence
(tests/blochtrainlm_ref.py) against the dense solve on the small cases; mbfir.refine_bloch_train_lm_batch(solver="device") with the
device step stubbed by the reference against solver="host" on the reference, bit for bit, and solver="host" against
refine_bloch_train_batch; the argument errors that mbfir.bloch_train_lm_step_batch raises before any device work; the C symbol; and
the conditions on the inputs of tests/test_blochtrainlm_gpu.py: that no case has an exactly zero gradient or operator, and that the
pulses of its batch of 17 do not all stop at the same iteration.

The float64 figure of the first step: the reference recurrence run to convergence (cg = 4n, rtol = 1e-30) differs from the dense
solve of (H + mu I) d = -g, H from 2n reference products and mu = trace(H) / 2n, by at most 7.9e-16 of max|d| on small(), groups and
allgains (8ab's analogue through the host loop was 8.8e-16); the test asserts 1e-12."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainlm_ref", os.path.join(ROOT, "tests", "blochtrainlm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
ref = lmref.gnref
# what every test of this file is about, taken at import: without the step and its driver none of them means anything, the ones on
# the reference and on the inputs of the GPU tests included
STEP, DRIVER = mbfir.bloch_train_lm_step_batch, mbfir.refine_bloch_train_lm_batch


def _realform(v):
    return np.concatenate([np.real(v), np.imag(v)], -1)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "groups", "allgains"])
def test_reference_first_step_is_the_dense_levenberg_marquardt_step(name):
    c = ref.case_of(name)
    worst = 0.0
    for q in range(len(c["pulses"])):
        n = len(c["pulses"][q][0])
        H = _realform(ref.gn(c, q, np.concatenate([np.eye(n), 1j * np.eye(n)]).astype(complex), np.float64)).T
        L0, g = lmref.lsq(c, q)
        mu = float(np.trace(H)) / (2 * n)
        want = np.linalg.solve((H + H.T) / 2 + mu * np.eye(2 * n), -_realform(g))
        d, info = lmref.step(c, q, -g, mu, cg=4 * n, rtol=1e-30, trial=True)
        err = np.abs(_realform(d) - want).max() / np.abs(want).max()
        worst = max(worst, err)
        print("%s pulse %d: reference step against the dense solve %.3g after %d iterations (%s)" % (name, q, err, info["ncg"], info["status"]))
        assert info["status"] in ("rtol", "cg") and 1 <= info["ncg"] <= 4 * n and info["gg"] == lmref.dot(g, g)
        L, grad = lmref.lsq(lmref.moved(c, q, d), q)
        assert info["loss"] == L and np.array_equal(info["grad"], grad) and L < L0
    assert worst <= 1e-12


def test_zero_right_hand_side_zero_cap_and_zero_weights():
    c = ref.small()
    n = len(c["pulses"][0][0])
    d, info = lmref.step(c, 0, np.zeros(n, dtype=complex), 0.1)
    assert info["ncg"] == 0 and info["status"] == "rtol" and info["rr"] == 0.0 and info["gg"] == 0.0
    assert np.array_equal(d, np.zeros(n)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()
    b = np.ones(n) + 0j
    d, info = lmref.step(c, 0, b, 0.1, cg=0)
    assert np.array_equal(d, np.zeros(n)) and info["ncg"] == 0 and info["status"] == "cg" and info["rr"] == info["gg"] == float(n)
    zero = tuple(np.zeros_like(v) for v in c["w"][0])
    zf = tuple(np.zeros_like(v) for v in c["wf"][0])
    d, info = lmref.step(dict(c, w=[zero], wf=[zf]), 0, b, 0.0)                 # H = 0 and mu = 0: <p, A p> = 0
    assert np.array_equal(d, np.zeros(n)) and info["ncg"] == 0 and info["status"] == "breakdown"


def test_no_case_has_an_exactly_zero_gradient_or_operator():
    """what tests/test_blochtrainlm_gpu.py relies on when it takes b = -g and mu from the Rayleigh quotient for every case"""
    for name in list(ref.cases()) + ["small"]:
        c = ref.case_of(name)
        for q in range(len(c["pulses"])):
            _, g = lmref.lsq(c, q)
            assert lmref.dot(g, g) > 0 and lmref.dot(g, lmref.gn(c, q, g)) > 0, (name, q)


def test_the_pulses_of_the_batch_of_17_do_not_all_stop_together():
    """The condition on the inputs that tests/test_blochtrainlm_gpu.py asserts of its batch of 17, here on the float64 reference, at
    that test's cg and rtol"""
    c = lmref.batch17()
    every = range(17)
    assert len(c["pulses"]) == 17 and all(len(p[0]) == 9 for p in c["pulses"]) and len(set(c["ntr"])) > 5 and c["scales"] == (1.0,)
    assert all(len(c["dfs"][q]) == 3 and len(c["dps"][q]) == 2 for q in every)
    bs, mus = lmref.rhs_and_mu([lmref.lsq(c, q) for q in every], lambda v: [lmref.gn(c, q, v[q]) for q in every])
    ncg = [lmref.step(c, q, bs[q], mus[q], lmref.CG17, lmref.RTOL17)[1]["ncg"] for q in every]
    print("iterations per pulse on the reference:", ncg)
    assert len(set(ncg)) > 1


# ---- declarations, bindings, errors ------------------------------------------------------------------------------------------------
def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    m = re.search(r"\bint\s+mbfir_bloch_train_lm_step_batch\s*\(([^;]*)\)\s*;", hdr)
    sym = mbfir.SYMBOLS["mbfir_bloch_train_lm_step_batch"][1]
    assert m and len(m.group(1).split(",")) == 64 and len(sym) == 64
    gn, lm = mbfir.SYMBOLS["mbfir_bloch_train_gn_batch"][1], mbfir.SYMBOLS["mbfir_bloch_lm_step_batch"][1]
    assert sym[:44] == gn[:44]                                        # mbfir_bloch_train_gn_batch's head through wfx, wfy, wfz
    assert sym[44:49] == lm[29:34]                                    # b_re, b_im, mu, cg, rtol
    assert sym[49:55] == [mbfir._dp] * 6                              # tx, ty, tz, tfx, tfy, tfz
    assert sym[55:] == lm[37:]                                        # the outputs of mbfir_bloch_lm_step_batch
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names[44:55] == ["b_re", "b_im", "mu", "cg", "rtol", "tx", "ty", "tz", "tfx", "tfy", "tfz"]
    assert names[55:] == ["d_re", "d_im", "ncg", "rr", "gg", "status", "loss", "g_re", "g_im"]
    assert getattr(mbfir.load_library(), "mbfir_bloch_train_lm_step_batch") is not None
    assert callable(mbfir.bloch_train_lm_step_batch) and callable(mbfir.refine_bloch_train_lm_batch)
    a, b = inspect.signature(mbfir.refine_bloch_train_lm_batch), inspect.signature(mbfir.refine_bloch_train_batch)
    assert list(a.parameters) == list(b.parameters)
    par = list(inspect.signature(mbfir.bloch_train_lm_step_batch).parameters)
    assert par[:7] == ["pulses", "df", "dp", "ntr", "rhs", "weights", "mu"] and {"targets", "targets_final", "cg", "rtol"} <= set(par)
    csrc = os.path.join(ROOT, "multiband-rf-pulse-design_amd", "csrc")
    assert "blochtrainlm.o" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "blochtrainlm.hip")).read()
    for k in ("k_bloch_train_lm_prep", "k_bloch_train_lm_step", "bloch_train_prop_jvp_body", "bloch_train_run_gn_body",
              "bloch_train_prop_vjp_forward", "bloch_train_prop_vjp_backward", "lm_init_launch", "bloch_lm_trial_launch", "lm_block_sum",
              "lm_redot", "lm_axpy", "lm_goes_on"):
        assert k in src, k
    assert "atomic" not in src.replace("No atomics", "")
    assert "Deterministic" in mbfir.bloch_train_lm_step_batch.__doc__


def test_c_call_refuses_a_null_context():
    args = [None] + [0 if a in (ctypes.c_int, ctypes.c_double) else None for a in mbfir.SYMBOLS["mbfir_bloch_train_lm_step_batch"][1][1:]]
    assert mbfir.load_library().mbfir_bloch_train_lm_step_batch(*args) == mbfir.E_ARG


class _NoDevice:
    """Stands for the library: any call is device work that must not have been reached"""

    def __getattr__(self, name):
        raise AssertionError("the library call %s was reached" % name)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(mbfir, "load_library", lambda: _NoDevice())
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: (_ for _ in ()).throw(AssertionError("a context was asked for")))
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    b, one = np.ones(4, dtype=complex), (1.0, 1.0, 1.0)
    who = "bloch_train_lm_step_batch: "

    def call(pl, n, w=[one], rhs=None, mu=0.1, **kw):
        return mbfir.bloch_train_lm_step_batch(pl, df, dp, n, [b] * len(pl) if rhs is None else rhs, w, mu, **kw)

    with pytest.raises(ValueError, match=who + "no pulses"):
        call([], 4, [])
    with pytest.raises(ValueError, match=who + "the scale list is empty"):
        call([p], 4, scales=())
    with pytest.raises(ValueError, match=who + "ntr of pulse 0 must be at least 1"):
        call([p], 0)
    with pytest.raises(ValueError, match=who + r"echo of pulse 0 must lie in \[0, ntime\]"):
        call([p], 4, echo=5)
    with pytest.raises(ValueError, match=who + "a gain is not finite"):
        call([p], 4, gains=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match=who + "meq of pulse 0 is not finite"):
        call([p], 4, meq=np.nan)
    with pytest.raises(ValueError, match=who + "neither an echo term nor a final term is given"):
        call([p], 4, None)
    with pytest.raises(ValueError, match=who + "targets are given for an echo term that has no weights"):
        call([p], 4, None, weights_final=[one], targets=[one], targets_final=[one])
    with pytest.raises(ValueError, match=who + "targets_final are given for a final term that has no weights"):
        call([p], 4, targets=[one], targets_final=[one])
    with pytest.raises(ValueError, match=who + "with targets, every term that has weights needs its own"):
        call([p], 4, weights_final=[one], targets=[one])
    with pytest.raises(ValueError, match=who + "with targets, every term that has weights needs its own"):
        call([p], 4, weights_final=[one], targets_final=[one])
    with pytest.raises(ValueError, match=who + "2 right-hand sides for 1 pulses"):
        call([p], 4, rhs=[b, b])
    with pytest.raises(ValueError, match=who + r"the right-hand side of pulse 0 has shape \(3,\), not \(4,\)"):
        call([p], 4, rhs=[b[:3]])
    for bad in (-1e-300, np.nan, np.inf, [0.1, -1.0]):
        with pytest.raises(ValueError, match=who + "a damping mu is negative or not finite"):
            call([p, p], 4, [one, one], mu=bad)
    with pytest.raises(ValueError, match=who + "mu must be a number or one number per pulse"):
        call([p], 4, mu=[0.1, 0.2])
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match=who + "cg must be an integer, at least 0"):
            call([p], 4, cg=bad)
    for bad in (-1e-300, np.nan):
        with pytest.raises(ValueError, match=who + "rtol is negative or not a number"):
            call([p], 4, rtol=bad)
    with pytest.raises(ValueError, match=who + "2 weight triples for 1 pulses"):
        call([p], 4, [one, one])
    with pytest.raises(ValueError, match=who + "the weights of pulse 0 must be a triple"):
        call([p], 4, [(1.0, 1.0)])
    with pytest.raises(ValueError, match=who + r"a weight of pulse 0 has shape \(2, 5\)"):
        call([p], 4, [(np.ones((2, 5)), 1.0, 1.0)])
    with pytest.raises(ValueError, match=who + "a weight of pulse 0 is negative or not finite"):
        call([p], 4, [(-1.0, 1.0, 1.0)])
    with pytest.raises(ValueError, match=who + "a weight of pulse 0 is negative or not finite"):
        call([p], 4, weights_final=[(np.nan, 1.0, 1.0)])
    with pytest.raises(ValueError, match=who + "2 target triples for 1 pulses"):
        call([p], 4, targets=[one, one])
    with pytest.raises(ValueError, match=who + r"a target of pulse 0 has shape \(1, 3, 3, 5\)"):
        call([p], 4, targets=[(np.ones((1, 3, 3, 5)), 1.0, 1.0)])
    with pytest.raises(ValueError, match=who + "a repetition weight is negative or not finite"):
        call([p], 4, rep_weights=np.array([1.0, -1.0, 1.0, 1.0]))
    who = "refine_bloch_train_lm_batch: "
    with pytest.raises(ValueError, match=who + "solver must be 'host' or 'device', not 'gpu'"):
        mbfir.refine_bloch_train_lm_batch([p], df, dp, 4, [one], [one], solver="gpu")
    with pytest.raises(ValueError, match=who + "no pulses"):
        mbfir.refine_bloch_train_lm_batch([], df, dp, 4, [], [], solver="device")
    with pytest.raises(ValueError, match=who + "iters must be at least 0 and cg at least 1"):
        mbfir.refine_bloch_train_lm_batch([p], df, dp, 4, [one], [one], cg=0, solver="device")
    with pytest.raises(ValueError, match=who + "2 targets triples for 1 pulses"):
        mbfir.refine_bloch_train_lm_batch([p], df, dp, 4, [one, one], [one], solver="device")
    with pytest.raises(ValueError, match=who + "neither an echo term nor a final term is given"):
        mbfir.refine_bloch_train_lm_batch([p], df, dp, 4, None, None, solver="device")
    with pytest.raises(ValueError, match="refine_bloch_train_batch: the train has no device step") as e:
        mbfir.refine_bloch_train_batch([p], df, dp, 4, [one], [one], solver="device")
    assert "refine_bloch_train_lm_batch" in str(e.value)


# ---- refine_bloch_train_lm_batch on calls stubbed by the reference -------------------------------------------------------------------
@pytest.fixture
def on_reference(monkeypatch):
    """The three device wrappers of the train replaced by the reference; returns the log of the calls' names."""
    log = []

    def case(pulses, df, dp, ntr, q, weights, targets, kw):
        pick = lambda v: v[q] if isinstance(v, list) else v
        return dict(pulses=[pulses[q]], dfs=[df], dps=[dp], ntr=[pick(ntr)], phases=[pick(kw["phases"])], gains=[pick(kw["gains"])],
                    echo=[pick(kw["echo"])], m0=[kw["m0"]], scales=kw["scales"], meq=kw["meq"], demod=kw["demod"],
                    w=[weights[q]], t=[None if targets is None else targets[q]], wf=[None], tf=[None],
                    rw=None if kw["rep_weights"] is None else [pick(kw["rep_weights"])], ce=[None], cf=[None])

    def lsq(pulses, df, dp, ntr, targets, weights, *, targets_final=None, weights_final=None, ctx=None, **kw):
        assert targets_final is None and weights_final is None
        log.append("lsq")
        return [lmref.lsq(case(pulses, df, dp, ntr, q, weights, targets, kw), 0) for q in range(len(pulses))]

    def gn(pulses, df, dp, ntr, tangents, weights, *, weights_final=None, ctx=None, **kw):
        log.append("gn")
        return [lmref.gn(case(pulses, df, dp, ntr, q, weights, None, kw), 0, tangents[q]) for q in range(len(pulses))]

    def lm(pulses, df, dp, ntr, rhs, weights, mu, *, targets=None, targets_final=None, weights_final=None, cg=8, rtol=1e-6, ctx=None, **kw):
        assert targets_final is None and weights_final is None and targets is not None
        log.append("lm")
        mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (len(pulses),))
        return [lmref.step(case(pulses, df, dp, ntr, q, weights, targets, kw), 0, rhs[q], float(mu[q]), cg, rtol, trial=True)
                for q in range(len(pulses))]

    monkeypatch.setattr(mbfir, "bloch_train_lsq_batch", lsq)
    monkeypatch.setattr(mbfir, "bloch_train_gn_batch", gn)
    monkeypatch.setattr(mbfir, "bloch_train_lm_step_batch", lm, raising=False)
    return log


def _fit():
    c = ref.small()
    p = c["pulses"][0]
    pulses = [(p[0] * s,) + tuple(p[1:]) for s in (1.0, 0.9, 1.1)]
    kw = dict(rep_weights=c["rw"][0], phases=c["phases"][0], gains=c["gains"][0], echo=c["echo"][0], m0=c["m0"][0], meq=c["meq"])
    return c, pulses, [c["t"][0]] * 3, [c["w"][0]] * 3, kw


def _run(fn, idx, **over):
    c, pulses, tg, w, kw = _fit()
    kw = dict(kw, iters=3, cg=4)
    kw.update(over)
    return fn([pulses[q] for q in idx], c["dfs"][0], c["dps"][0], 3, [tg[q] for q in idx], [w[q] for q in idx], **kw)


def _same(a, b):
    (ra, ia), (rb, ib) = a, b
    assert len(ra) == len(rb)
    for u, v in zip(ra, rb):
        assert np.array_equal(u, v)
    for u, v in zip(ia, ib):
        assert u["losses"] == v["losses"] and u["mu"] == v["mu"] and u["status"] == v["status"] and u["refused"] == v["refused"]


def _counts_hold(infos):
    for i in infos:
        c = i["calls"]
        assert set(c) == {"lsq", "gn", "lm"}
        assert c["lm"] == (len(i["losses"]) - 1) + i["refused"] and c["gn"] <= 1 and c["lsq"] == 1


@pytest.mark.parametrize("q", [0, 1, 2])
def test_device_solver_on_the_reference_has_the_bits_of_the_host_solver(on_reference, q):
    host = _run(mbfir.refine_bloch_train_lm_batch, [q])
    assert "lm" not in on_reference and set(host[1][0]["calls"]) == {"lsq", "gn"}
    old = _run(mbfir.refine_bloch_train_batch, [q])
    _same(host, old)
    assert host[1] == old[1]                                                  # the whole infos, the 'calls' included
    del on_reference[:]
    dev = _run(mbfir.refine_bloch_train_lm_batch, [q], solver="device")
    _same(dev, host)
    _counts_hold(dev[1])
    assert len(dev[1][0]["losses"]) >= 2
    c = dev[1][0]["calls"]
    assert c["gn"] == 1                                                        # the Rayleigh quotient alone
    assert on_reference == ["lsq", "gn"] + ["lm"] * c["lm"]                    # what the loop called is what it counted


def test_device_solver_in_a_batch_of_three_and_reversed(on_reference):
    alone = [_run(mbfir.refine_bloch_train_lm_batch, [q], solver="device") for q in range(3)]
    for order in ([0, 1, 2], [2, 1, 0]):
        dev = _run(mbfir.refine_bloch_train_lm_batch, order, solver="device")
        _same(dev, _run(mbfir.refine_bloch_train_lm_batch, order))
        _same(dev, _run(mbfir.refine_bloch_train_batch, order))
        _counts_hold(dev[1])
        for k, q in enumerate(order):
            assert np.array_equal(dev[0][k], alone[q][0][0]) and dev[1][k] == alone[q][1][0]


def test_a_refused_step_is_the_host_solvers_refused_step(on_reference, monkeypatch):
    """The first trial step is refused by force (its loss reported as infinite): the host solver sees it in its second lsq call, the
    device solver in its first lm call."""
    honest_lsq, honest_lm, count = mbfir.bloch_train_lsq_batch, mbfir.bloch_train_lm_step_batch, [0, 0]

    def refusing_lsq(*a, **k):
        count[0] += 1
        res = honest_lsq(*a, **k)
        return [(np.inf, g) for _, g in res] if count[0] == 2 else res

    def refusing_lm(*a, **k):
        count[1] += 1
        res = honest_lm(*a, **k)
        return [(d, dict(i, loss=np.inf)) for d, i in res] if count[1] == 1 else res

    monkeypatch.setattr(mbfir, "bloch_train_lsq_batch", refusing_lsq)
    host = _run(mbfir.refine_bloch_train_lm_batch, [0], mu0=0.05)
    monkeypatch.setattr(mbfir, "bloch_train_lsq_batch", honest_lsq)
    monkeypatch.setattr(mbfir, "bloch_train_lm_step_batch", refusing_lm)
    dev = _run(mbfir.refine_bloch_train_lm_batch, [0], mu0=0.05, solver="device")
    assert host[1][0]["refused"] >= 1
    _same(dev, host)
    _counts_hold(dev[1])
    assert dev[1][0]["calls"]["gn"] == 0                                       # mu0 given: no Rayleigh quotient


def test_a_breakdown_is_a_refused_step(on_reference, monkeypatch):
    honest, count = mbfir.bloch_train_lm_step_batch, [0]

    def breaking(*a, **k):
        count[0] += 1
        res = honest(*a, **k)
        return [(d, dict(i, status="breakdown")) for d, i in res] if count[0] == 1 else res

    monkeypatch.setattr(mbfir, "bloch_train_lm_step_batch", breaking)
    (_,), (got,) = _run(mbfir.refine_bloch_train_lm_batch, [0], iters=2, mu0=0.05, solver="device")
    monkeypatch.setattr(mbfir, "bloch_train_lm_step_batch", honest)
    (_,), (want,) = _run(mbfir.refine_bloch_train_lm_batch, [0], iters=2, mu0=0.2, solver="device")
    assert got["refused"] == want["refused"] + 1 and got["losses"] == want["losses"] and got["mu"] == want["mu"]
