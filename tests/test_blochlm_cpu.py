"""The Levenberg-Marquardt step of the Bloch model solved on the device, without one: the NumPy recurrence (tests/blochlm_ref.py)
against the dense solve; refine_bloch_batch(solver="device") on the reference against solver="host" on the reference, bit for bit;
the argument errors that mbfir.bloch_lm_step_batch raises before any device work; the C symbol; and the condition on the inputs of
tests/test_blochlm_gpu.py's batch of 17, that its pulses do not all stop together."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochlm_ref", os.path.join(ROOT, "tests", "blochlm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
ref = lmref.gnref

N, RSC = 5, (0.9, 1.0, 1.1)


def _grid_of(v, k):
    return v[k] if isinstance(v, list) else v


def _m0_of(m0, k):
    return m0[k] if isinstance(m0, list) else m0


@pytest.fixture
def on_reference(monkeypatch):
    """The three device wrappers replaced by the reference; returns the log of the calls' names."""
    log = []

    def lsq(pulses, df, dp, targets, weights, *, scales=(1.0,), m0=None, ctx=None):
        log.append("lsq")
        return [tuple(ref.lsq(p, _grid_of(df, k), _grid_of(dp, k), t, w, scales, _m0_of(m0, k)))
                for k, (p, t, w) in enumerate(zip(pulses, targets, weights))]

    def gn(pulses, df, dp, tangents, weights, *, scales=(1.0,), m0=None, ctx=None):
        log.append("gn")
        return [ref.gn(p, _grid_of(df, k), _grid_of(dp, k), v, w, scales, _m0_of(m0, k))
                for k, (p, v, w) in enumerate(zip(pulses, tangents, weights))]

    def lm(pulses, df, dp, rhs, weights, mu, *, targets=None, cg=8, rtol=1e-6, scales=(1.0,), m0=None, ctx=None):
        log.append("lm")
        mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (len(pulses),))
        return [lmref.step(p, _grid_of(df, k), _grid_of(dp, k), b, w, float(mu[k]), scales, _m0_of(m0, k), cg, rtol,
                           None if targets is None else targets[k])
                for k, (p, b, w) in enumerate(zip(pulses, rhs, weights))]

    monkeypatch.setattr(mbfir, "bloch_lsq_batch", lsq)
    monkeypatch.setattr(mbfir, "bloch_gn_batch", gn)
    monkeypatch.setattr(mbfir, "bloch_lm_step_batch", lm)
    return log


def _problem(seed, t2_over_dur=2.0):
    """tests/test_blochgn_cpu.py's: a 5-sample pulse near 60 degrees on 3 x 3 points (n = 5, 9 points); the target is its own end
    point at gain 1, perturbed; weights with zeros, none on mx at all"""
    rng = np.random.default_rng(seed)
    dur, gamma = 2e-3, ref.GAMMA_H1
    b1 = (np.hanning(N + 2)[1:-1] + 0.1 * rng.standard_normal(N)) * (np.pi / 3 / (gamma * dur / N * np.hanning(N + 2).sum())) + 0j
    p = (b1, rng.uniform(0.5, 1.5, N) * 0.05, dur / N, 1.0, t2_over_dur * dur, "H-1")
    df, dp = ref._grid(3, 100.0), ref._grid(3, 2.0)
    m = ref.forward(*p[:5], df, dp, gamma, 1.0)
    t = (0.0, m[1] * (1 + 0.2 * rng.standard_normal((3, 3))), np.stack([m[2] + 0.1 * rng.standard_normal((3, 3)) for _ in RSC]))
    w = np.ones((3, 3))
    w[1, 1] = 0.0
    return p, df, dp, t, (0.0, w, np.stack([w] * 3))


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


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_device_solver_on_the_reference_has_the_bits_of_the_host_solver(on_reference, seed):
    p, df, dp, t, w = _problem(seed)
    kw = dict(scales=RSC, iters=3, cg=4)
    host = mbfir.refine_bloch_batch([p], df, dp, [t], [w], **kw)
    assert "lm" not in on_reference and set(host[1][0]["calls"]) == {"lsq", "gn"}
    again = mbfir.refine_bloch_batch([p], df, dp, [t], [w], solver="host", **kw)
    _same(again, host)
    assert again[1][0]["calls"] == host[1][0]["calls"]
    dev = mbfir.refine_bloch_batch([p], df, dp, [t], [w], solver="device", **kw)
    _same(dev, host)
    _counts_hold(dev[1])
    assert len(dev[1][0]["losses"]) >= 2
    assert dev[1][0]["calls"]["gn"] == 1                                       # the Rayleigh quotient alone


def test_device_solver_in_a_batch_of_three_and_reversed(on_reference):
    probs = [_problem(s) for s in (4, 5, 6)]
    df, dp = probs[0][1], probs[0][2]
    kw = dict(scales=RSC, iters=3, cg=4)
    rng = np.random.default_rng(12)
    m0 = [tuple(rng.uniform(-0.4, 0.4, (3, 3, 3))) for _ in probs]
    alone = [mbfir.refine_bloch_batch([p[0]], df, dp, [p[3]], [p[4]], m0=[m0[k]], **kw) for k, p in enumerate(probs)]
    for order in ((0, 1, 2), (2, 1, 0)):
        args = ([probs[q][0] for q in order], df, dp, [probs[q][3] for q in order], [probs[q][4] for q in order])
        dev = mbfir.refine_bloch_batch(*args, m0=[m0[q] for q in order], solver="device", **kw)
        _same(dev, mbfir.refine_bloch_batch(*args, m0=[m0[q] for q in order], **kw))
        _counts_hold(dev[1])
        for k, q in enumerate(order):
            assert np.array_equal(dev[0][k], alone[q][0][0])


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_a_refused_step_is_the_host_solvers_refused_step(on_reference, monkeypatch, seed):
    """The first trial step is refused by force (its loss reported as infinite): the host solver sees it in its second lsq call, the
    device solver in its first lm call."""
    p, df, dp, t, w = _problem(seed)
    kw = dict(scales=RSC, iters=3, cg=4, mu0=0.05)
    honest_lsq, honest_lm, count = mbfir.bloch_lsq_batch, mbfir.bloch_lm_step_batch, [0, 0]

    def refusing_lsq(*a, **k):
        count[0] += 1
        res = honest_lsq(*a, **k)
        return [(np.inf, g) for _, g in res] if count[0] == 2 else res

    def refusing_lm(*a, **k):
        count[1] += 1
        res = honest_lm(*a, **k)
        return [(d, dict(i, loss=np.inf)) for d, i in res] if count[1] == 1 else res

    monkeypatch.setattr(mbfir, "bloch_lsq_batch", refusing_lsq)
    host = mbfir.refine_bloch_batch([p], df, dp, [t], [w], **kw)
    monkeypatch.setattr(mbfir, "bloch_lsq_batch", honest_lsq)
    monkeypatch.setattr(mbfir, "bloch_lm_step_batch", refusing_lm)
    dev = mbfir.refine_bloch_batch([p], df, dp, [t], [w], solver="device", **kw)
    assert host[1][0]["refused"] >= 1
    _same(dev, host)
    _counts_hold(dev[1])
    assert dev[1][0]["calls"]["gn"] == 0                                       # mu0 given: no Rayleigh quotient


def test_a_breakdown_is_a_refused_step(on_reference, monkeypatch):
    p, df, dp, t, w = _problem(2)
    honest, count = mbfir.bloch_lm_step_batch, [0]

    def breaking(*a, **k):
        count[0] += 1
        res = honest(*a, **k)
        return [(d, dict(i, status="breakdown")) for d, i in res] if count[0] == 1 else res

    monkeypatch.setattr(mbfir, "bloch_lm_step_batch", breaking)
    (_,), (got,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=2, mu0=0.05, solver="device")
    monkeypatch.setattr(mbfir, "bloch_lm_step_batch", honest)
    (_,), (want,) = mbfir.refine_bloch_batch([p], df, dp, [t], [w], scales=RSC, iters=2, mu0=0.2, solver="device")
    assert got["refused"] == want["refused"] + 1 and got["losses"] == want["losses"] and got["mu"] == want["mu"]


def _realform(v):
    return np.concatenate([np.real(v), np.imag(v)], -1)


@pytest.mark.parametrize("t2_over_dur", [2.0, 1.0])
def test_reference_step_is_the_dense_levenberg_marquardt_step(t2_over_dur):
    """n = 5, 9 points, mu = 1e-2 trace(H) / 2n, cg = 4n, rtol = 1e-16: within 1e-4 of max|d|, the bound of
    test_first_step_is_the_dense_levenberg_marquardt_step; with T2 twice the pulse's duration and as short as the pulse"""
    p, df, dp, t, w = _problem(1, t2_over_dur)
    e = np.concatenate([np.eye(N), 1j * np.eye(N)])
    H = _realform(ref.gn(p, df, dp, e, w, RSC)).T
    _, g = ref.lsq(p, df, dp, t, w, RSC)
    mu = 1e-2 * np.trace(H) / (2 * N)
    want = np.linalg.solve(H + mu * np.eye(2 * N), -_realform(g))
    d, info = lmref.step(p, df, dp, -g, w, mu, RSC, None, cg=4 * N, rtol=1e-16, target=t)
    err = np.abs(_realform(d) - want).max() / np.abs(want).max()
    print("T2 / duration %g: reference step against the dense solve %.3g after %d iterations (%s)"
          % (t2_over_dur, err, info["ncg"], info["status"]))
    assert err <= 1e-4
    assert info["status"] in ("rtol", "cg") and 1 <= info["ncg"] <= 4 * N and info["gg"] == float((np.conj(g) * g).real.sum())
    L, grad = ref.lsq((p[0] + d,) + p[1:], df, dp, t, w, RSC)
    assert info["loss"] == L and np.array_equal(info["grad"], grad)


def test_zero_right_hand_side_zero_cap_and_zero_weights():
    p, df, dp, t, w = _problem(1)
    d, info = lmref.step(p, df, dp, np.zeros(N, dtype=complex), w, 0.1, RSC)
    assert info["ncg"] == 0 and info["status"] == "rtol" and info["rr"] == 0.0 and info["gg"] == 0.0
    assert np.array_equal(d, np.zeros(N)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()
    b = np.ones(N) + 0j
    d, info = lmref.step(p, df, dp, b, w, 0.1, RSC, cg=0)
    assert np.array_equal(d, np.zeros(N)) and info["ncg"] == 0 and info["status"] == "cg" and info["rr"] == info["gg"] == float(N)
    d, info = lmref.step(p, df, dp, b, (0.0, 0.0, 0.0), 0.0, RSC)                 # H = 0 and mu = 0: <p, A p> = 0
    assert np.array_equal(d, np.zeros(N)) and info["ncg"] == 0 and info["status"] == "breakdown"


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    b, z, one = np.ones(4, dtype=complex), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    fn, who = mbfir.bloch_lm_step_batch, "bloch_lm_step_batch"
    with pytest.raises(ValueError, match=who + ": no pulses"):
        fn([], df, dp, [], [], 0.1)
    with pytest.raises(ValueError, match="scale list is empty"):
        fn([p], df, dp, [b], [one], 0.1, scales=())
    with pytest.raises(ValueError, match="empty grid"):
        fn([p], np.zeros(0), dp, [b], [one], 0.1)
    with pytest.raises(ValueError, match="2 right-hand sides for 1 pulses"):
        fn([p], df, dp, [b, b], [one], 0.1)
    with pytest.raises(ValueError, match=r"right-hand side of pulse 0 has shape \(3,\), not \(4,\)"):
        fn([p], df, dp, [b[:3]], [one], 0.1)
    with pytest.raises(ValueError, match=r"right-hand side of pulse 0 has shape \(1, 4\)"):
        fn([p], df, dp, [b[None]], [one], 0.1)
    with pytest.raises(ValueError, match="2 weight triples for 1 pulses"):
        fn([p], df, dp, [b], [one, one], 0.1)
    with pytest.raises(ValueError, match="must be a triple"):
        fn([p], df, dp, [b], [(1.0, 1.0)], 0.1)
    with pytest.raises(ValueError, match="has shape"):
        fn([p], df, dp, [b], [(1.0, 1.0, np.ones((3, 4)))], 0.1)
    with pytest.raises(ValueError, match="negative or not finite"):
        fn([p], df, dp, [b], [(1.0, -1.0, 1.0)], 0.1)
    for bad in (-1e-300, np.nan, np.inf, [0.1, -1.0]):
        with pytest.raises(ValueError, match="mu is negative or not finite"):
            fn([p, p], df, dp, [b, b], [one, one], bad)
    with pytest.raises(ValueError, match="mu must be a number or one number per pulse"):
        fn([p], df, dp, [b], [one], [0.1, 0.2])
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="cg must be an integer, at least 0"):
            fn([p], df, dp, [b], [one], 0.1, cg=bad)
    for bad in (-1e-300, np.nan):
        with pytest.raises(ValueError, match="rtol is negative or not a number"):
            fn([p], df, dp, [b], [one], 0.1, rtol=bad)
    with pytest.raises(ValueError, match="2 target triples for 1 pulses"):
        fn([p], df, dp, [b], [one], 0.1, targets=[z, z])
    with pytest.raises(ValueError, match="must be a triple"):
        fn([p], df, dp, [b], [one], 0.1, targets=[np.zeros((3, 5))])
    with pytest.raises(ValueError, match="has shape"):
        fn([p], df, dp, [b], [one], 0.1, targets=[(0.0, 0.0, np.zeros(5))])
    with pytest.raises(ValueError, match="solver must be 'host' or 'device', not 'x'"):
        mbfir.refine_bloch_batch([p], df, dp, [z], [one], solver="x")
    with pytest.raises(ValueError, match="iters must be at least 0 and cg at least 1"):
        mbfir.refine_bloch_batch([p], df, dp, [z], [one], cg=0, solver="device")


def test_c_call_refuses_a_null_context():
    args = [None] + [0 if a in (ctypes.c_int, ctypes.c_double) else None for a in mbfir.SYMBOLS["mbfir_bloch_lm_step_batch"][1][1:]]
    assert mbfir.load_library().mbfir_bloch_lm_step_batch(*args) == mbfir.E_ARG


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    m = re.search(r"\bint\s+mbfir_bloch_lm_step_batch\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 46
    assert len(mbfir.SYMBOLS["mbfir_bloch_lm_step_batch"][1]) == 46
    assert getattr(mbfir.load_library(), "mbfir_bloch_lm_step_batch") is not None
    assert callable(mbfir.bloch_lm_step_batch)
    src = open(os.path.join(ROOT, "multiband-rf-pulse-design_amd", "csrc", "blochgn.hip")).read()
    for k in ("k_bloch_lm_sweep", "k_bloch_lm_step", "k_bloch_lm_trial"):
        assert k in src
    assert "atomic" not in src.replace("No atomics", "")


def test_the_pulses_of_the_batch_of_17_do_not_all_stop_together():
    """The condition on the inputs that tests/test_blochlm_gpu.py asserts of its batch of 17, here on the reference alone, at that
    test's cg and rtol"""
    pulses, dfs, dps, m0s, tgs, wts = lmref.batch17()
    every = range(17)
    bs, mus = lmref.rhs_and_mu(lambda: [ref.lsq(pulses[q], dfs[q], dps[q], tgs[q], wts[q], lmref.SC17, m0s[q]) for q in every],
                               lambda v: [ref.gn(pulses[q], dfs[q], dps[q], v[q], wts[q], lmref.SC17, m0s[q]) for q in every])
    ncg = [lmref.step(pulses[q], dfs[q], dps[q], bs[q], wts[q], mus[q], lmref.SC17, m0s[q], lmref.CG17, lmref.RTOL17)[1]["ncg"]
           for q in every]
    print("iterations per pulse on the reference:", ncg)
    assert len(set(ncg)) > 1
