"""The Levenberg-Marquardt step solved on the device, without one: the NumPy recurrence (tests/simlm_ref.py) against the dense solve;
refine_batch(solver="device") on the reference against solver="host" on the reference, bit for bit; the argument errors that
mbfir.abr_lm_step_batch / abr2_lm_step_batch raise before any device work; the C symbols."""
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("simlm_ref", os.path.join(ROOT, "tests", "simlm_ref.py"))
lmref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lmref)
ref = lmref.gnref

N, NX = 5, 9
RSC = (0.9, 1.0, 1.1)


def _split(p):
    return p if isinstance(p, tuple) else (p, None)


def _grid(v, k):
    return v[k] if isinstance(v, list) else v


@pytest.fixture
def on_reference(monkeypatch):
    """The six device wrappers replaced by the reference; returns the log of the calls' names."""
    log = []

    def lsq(pulses, x, *rest, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        y, targets, weights = (None,) + rest if len(rest) == 2 else rest
        log.append("lsq")
        return [ref.lsq(*_split(p), _grid(x, k), t, w, scales, profile, None if y is None else _grid(y, k), hard_pulse)
                for k, (p, t, w) in enumerate(zip(pulses, targets, weights))]

    def gn(pulses, x, *rest, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        y, tangents, weights = (None,) + rest if len(rest) == 2 else rest
        log.append("gn")
        return [ref.gn(*_split(p), _grid(x, k), v, w, scales, profile, None if y is None else _grid(y, k), hard_pulse)
                for k, (p, v, w) in enumerate(zip(pulses, tangents, weights))]

    def lm(pulses, x, *rest, targets=None, cg=8, rtol=1e-6, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
        y, rhs, weights, mu = (None,) + rest if len(rest) == 3 else rest
        log.append("lm")
        mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (len(pulses),))
        return [lmref.step(*_split(p), _grid(x, k), b, w, float(mu[k]), scales, profile, None if y is None else _grid(y, k),
                           hard_pulse, cg, rtol, None if targets is None else targets[k])
                for k, (p, b, w) in enumerate(zip(pulses, rhs, weights))]

    for name, fn in (("abr_lsq_batch", lsq), ("abr2_lsq_batch", lsq), ("abr_gn_batch", gn), ("abr2_gn_batch", gn),
                     ("abr_lm_step_batch", lm), ("abr2_lm_step_batch", lm)):
        monkeypatch.setattr(mbfir, name, fn)
    return log


def _problem(seed, kind="ex", hard=False):
    """tests/test_simgn_cpu.py's: a pulse near 60 degrees, its profile at gain 1 perturbed as the target, weights with zeros"""
    rng = np.random.default_rng(seed)
    rf = (np.hanning(N + 2)[1:-1] + 0.1 * rng.standard_normal(N)) * (np.pi / 3 / np.hanning(N + 2).sum()) + 0j
    x = np.linspace(-2, 2, NX)
    a, b = ref.forward(rf, None, x, None, hard)
    f = ref.profile(kind, a, b)
    t = np.stack([f * (1 + 0.2 * rng.standard_normal(NX)) for _ in RSC])
    w = np.ones((len(RSC), NX))
    w[:, 1] = 0.0
    return rf, x, t, w


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


@pytest.mark.parametrize("seed", [2, 3, 4, 5, 6])
def test_device_solver_on_the_reference_has_the_bits_of_the_host_solver(on_reference, seed):
    rf, x, t, w = _problem(seed)
    kw = dict(scales=RSC, iters=3, cg=4)
    host = mbfir.refine_batch([rf], x, [t], [w], **kw)
    assert "lm" not in on_reference and set(host[1][0]["calls"]) == {"lsq", "gn"}
    dev = mbfir.refine_batch([rf], x, [t], [w], solver="device", **kw)
    _same(dev, host)
    _counts_hold(dev[1])
    assert len(dev[1][0]["losses"]) >= 2
    assert dev[1][0]["calls"]["gn"] == 1                                       # the Rayleigh quotient alone


def test_device_solver_in_a_batch_and_in_two_dimensions(on_reference):
    probs = [_problem(s) for s in (2, 3, 4, 5, 6)]
    x = probs[0][1]
    kw = dict(scales=RSC, iters=3, cg=4)
    args = ([p[0] for p in probs], x, [p[2] for p in probs], [p[3] for p in probs])
    dev = mbfir.refine_batch(*args, solver="device", **kw)
    _same(dev, mbfir.refine_batch(*args, **kw))
    _counts_hold(dev[1])
    rng = np.random.default_rng(9)
    rf = [0.2 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) for _ in range(2)]
    g = np.full(N, 2 * np.pi / N) + 0.3j
    xs, ys = [np.linspace(-1, 1, 3), np.linspace(-2, 2, 4)], [np.linspace(-1, 1, 2), np.linspace(-1, 1, 2)]
    t = [np.zeros((1, 3, 2), dtype=complex), np.zeros((1, 4, 2), dtype=complex)]
    w = [np.ones((3, 2)), np.ones((4, 2))]
    dev = mbfir.refine_batch([(r, g) for r in rf], xs, ys, t, w, iters=2, solver="device")
    _same(dev, mbfir.refine_batch([(r, g) for r in rf], xs, ys, t, w, iters=2))
    _counts_hold(dev[1])


@pytest.mark.parametrize("seed", [2, 3, 4, 5, 6])
def test_a_refused_step_is_the_host_solvers_refused_step(on_reference, monkeypatch, seed):
    """The first trial step is refused by force (its loss reported as infinite), as in test_a_refused_step_changes_only_mu: the
    host solver sees it in its second lsq call, the device solver in its first lm call."""
    rf, x, t, w = _problem(seed)
    kw = dict(scales=RSC, iters=3, cg=4, mu0=0.05)
    honest_lsq, honest_lm, count = mbfir.abr_lsq_batch, mbfir.abr_lm_step_batch, [0, 0]

    def refusing_lsq(*a, **k):
        count[0] += 1
        res = honest_lsq(*a, **k)
        return [(np.inf, g) for _, g in res] if count[0] == 2 else res

    def refusing_lm(*a, **k):
        count[1] += 1
        res = honest_lm(*a, **k)
        return [(d, dict(i, loss=np.inf)) for d, i in res] if count[1] == 1 else res

    monkeypatch.setattr(mbfir, "abr_lsq_batch", refusing_lsq)
    host = mbfir.refine_batch([rf], x, [t], [w], **kw)
    monkeypatch.setattr(mbfir, "abr_lsq_batch", honest_lsq)
    monkeypatch.setattr(mbfir, "abr_lm_step_batch", refusing_lm)
    dev = mbfir.refine_batch([rf], x, [t], [w], solver="device", **kw)
    assert host[1][0]["refused"] >= 1
    _same(dev, host)
    _counts_hold(dev[1])
    assert dev[1][0]["calls"]["gn"] == 0                                       # mu0 given: no Rayleigh quotient


def test_a_breakdown_is_a_refused_step(on_reference, monkeypatch):
    rf, x, t, w = _problem(2)
    honest, count = mbfir.abr_lm_step_batch, [0]

    def breaking(*a, **k):
        count[0] += 1
        res = honest(*a, **k)
        return [(d, dict(i, status="breakdown")) for d, i in res] if count[0] == 1 else res

    monkeypatch.setattr(mbfir, "abr_lm_step_batch", breaking)
    (_,), (got,) = mbfir.refine_batch([rf], x, [t], [w], scales=RSC, iters=2, mu0=0.05, solver="device")
    monkeypatch.setattr(mbfir, "abr_lm_step_batch", honest)
    (_,), (want,) = mbfir.refine_batch([rf], x, [t], [w], scales=RSC, iters=2, mu0=0.2, solver="device")
    assert got["refused"] == want["refused"] + 1 and got["losses"] == want["losses"] and got["mu"] == want["mu"]


def _realform(v):
    return np.concatenate([v.real, v.imag])


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("hard", [False, True])
def test_reference_step_is_the_dense_levenberg_marquardt_step(kind, hard):
    """n = 5, nx = 9, mu = 1e-2 trace(H) / 2n, cg = 4n, rtol = 1e-16: within 1e-4 of max|d|, the bound of
    test_first_step_is_the_dense_levenberg_marquardt_step."""
    rf, x, t, w = _problem(1, kind, hard)
    cols = []
    for j in range(2 * N):
        e = np.zeros(N, dtype=complex)
        e[j % N] = 1.0 if j < N else 1j
        cols.append(_realform(ref.gn(rf, None, x, e, w, RSC, kind, None, hard)))
    H = np.stack(cols, axis=1)
    _, g = ref.lsq(rf, None, x, t, w, RSC, kind, None, hard)
    mu = 1e-2 * np.trace(H) / (2 * N)
    want = np.linalg.solve(H + mu * np.eye(2 * N), -_realform(g))
    d, info = lmref.step(rf, None, x, -g, w, mu, RSC, kind, None, hard, cg=4 * N, rtol=1e-16, target=t)
    err = np.abs(_realform(d) - want).max() / np.abs(want).max()
    print("%s hard %s: reference step against the dense solve %.3g after %d iterations (%s)" % (kind, hard, err, info["ncg"], info["status"]))
    assert err <= 1e-4
    assert info["status"] in ("rtol", "cg") and 1 <= info["ncg"] <= 4 * N and info["gg"] == float((np.conj(g) * g).real.sum())
    L, grad = ref.lsq(rf + d, None, x, t, w, RSC, kind, None, hard)
    assert info["loss"] == L and np.array_equal(info["grad"], grad)


def test_zero_right_hand_side_and_zero_cap():
    rf, x, t, w = _problem(1)
    d, info = lmref.step(rf, None, x, np.zeros(N, dtype=complex), w, 0.1, RSC)
    assert info["ncg"] == 0 and info["status"] == "rtol" and info["rr"] == 0.0 and info["gg"] == 0.0
    assert np.array_equal(d, np.zeros(N)) and not np.signbit(d.real).any() and not np.signbit(d.imag).any()
    b = np.ones(N) + 0j
    d, info = lmref.step(rf, None, x, b, w, 0.1, RSC, cg=0)
    assert np.array_equal(d, np.zeros(N)) and info["ncg"] == 0 and info["status"] == "cg" and info["rr"] == info["gg"] == float(N)
    d, info = lmref.step(rf, None, x, b, np.zeros_like(w), 0.0, RSC)               # H = 0 and mu = 0: <p, A p> = 0
    assert np.array_equal(d, np.zeros(N)) and info["ncg"] == 0 and info["status"] == "breakdown"


def test_argument_errors_come_before_any_device_work():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    rf, b = np.ones(4), np.ones(4, dtype=complex)
    t1, w1 = np.zeros((2, 5), dtype=complex), np.ones((2, 5))
    t2, w2 = np.zeros((2, 5, 3), dtype=complex), np.ones((2, 5, 3))
    sc = (1.0, 0.9)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr_lm_step_batch([], x, [], [], 0.1)
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr2_lm_step_batch([rf], x, y, [b], [w2], 0.1, scales=())
    with pytest.raises(ValueError, match="profile must be one of"):
        mbfir.abr_lm_step_batch([rf], x, [b], [w1], 0.1, scales=sc, profile="xy")
    with pytest.raises(ValueError, match="2 right-hand sides for 1 pulses"):
        mbfir.abr_lm_step_batch([rf], x, [b, b], [w1], 0.1, scales=sc)
    with pytest.raises(ValueError, match=r"right-hand side of pulse 0 has shape \(3,\), not \(4,\)"):
        mbfir.abr_lm_step_batch([rf], x, [b[:3]], [w1], 0.1, scales=sc)
    with pytest.raises(ValueError, match=r"right-hand side of pulse 0 has shape \(1, 4\)"):
        mbfir.abr2_lm_step_batch([rf], x, y, [b[None]], [w2], 0.1, scales=sc)
    with pytest.raises(ValueError, match=r"weights of pulse 0 have shape \(2, 4\)"):
        mbfir.abr_lm_step_batch([rf], x, [b], [w1[:, :4]], 0.1, scales=sc)
    with pytest.raises(ValueError, match="negative or not finite"):
        mbfir.abr_lm_step_batch([rf], x, [b], [-w1], 0.1, scales=sc)
    for bad in (-1e-300, np.nan, np.inf, [0.1, -1.0]):
        with pytest.raises(ValueError, match="mu is negative or not finite"):
            mbfir.abr_lm_step_batch([rf, rf], x, [b, b], [w1, w1], bad, scales=sc)
        with pytest.raises(ValueError, match="mu is negative or not finite"):
            mbfir.abr2_lm_step_batch([rf, rf], x, y, [b, b], [w2, w2], bad, scales=sc)
    with pytest.raises(ValueError, match="mu must be a number or one number per pulse"):
        mbfir.abr_lm_step_batch([rf], x, [b], [w1], [0.1, 0.2], scales=sc)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="cg must be an integer, at least 0"):
            mbfir.abr_lm_step_batch([rf], x, [b], [w1], 0.1, scales=sc, cg=bad)
    for bad in (-1e-300, np.nan):
        with pytest.raises(ValueError, match="rtol is negative or not a number"):
            mbfir.abr_lm_step_batch([rf], x, [b], [w1], 0.1, scales=sc, rtol=bad)
        with pytest.raises(ValueError, match="rtol is negative or not a number"):
            mbfir.abr2_lm_step_batch([rf], x, y, [b], [w2], 0.1, scales=sc, rtol=bad)
    with pytest.raises(ValueError, match=r"target of pulse 0 has shape \(5,\)"):
        mbfir.abr_lm_step_batch([rf], x, [b], [w1], 0.1, scales=sc, targets=[t1[0]])
    with pytest.raises(ValueError, match="2 targets for 1 pulses"):
        mbfir.abr2_lm_step_batch([rf], x, y, [b], [w2], 0.1, scales=sc, targets=[t2, t2])
    with pytest.raises(ValueError, match="'inv' is real"):
        mbfir.abr_lm_step_batch([rf], x, [b], [w1], 0.1, scales=sc, profile="inv", targets=[t1 + 1j])
    with pytest.raises(ValueError, match="'inv' is real"):
        mbfir.abr2_lm_step_batch([rf], x, y, [b], [w2], 0.1, scales=sc, profile="sat", targets=[t2 + 1j])
    with pytest.raises(ValueError, match="solver must be 'host' or 'device', not 'x'"):
        mbfir.refine_batch([rf], x, [t1], [w1], scales=sc, solver="x")


def test_c_calls_refuse_a_null_context():
    lib = mbfir.load_library()
    d = np.ones(8)
    k = np.zeros(2, dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    lp, p, ip = off.ctypes.data_as(mbfir._lp), mbfir._ptr(d), k.ctypes.data_as(mbfir._ip)
    tail = (p, p, p, 8, 1e-6, p, p, p, p, ip, p, p, ip, p, p, p)
    assert lib.mbfir_abr_lm_step_batch(None, 1, lp, p, p, None, 1, lp, p, 1, p, 0, 0, p, *tail) == mbfir.E_ARG
    assert lib.mbfir_abr2_lm_step_batch(None, 1, lp, p, p, None, None, 1, lp, p, 1, lp, p, 1, p, 0, 0, p, *tail) == mbfir.E_ARG


def test_lm_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym, nargs in (("mbfir_abr_lm_step_batch", 30), ("mbfir_abr2_lm_step_batch", 34)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert len(mbfir.SYMBOLS[sym][1]) == nargs
        assert getattr(mbfir.load_library(), sym) is not None
    for name in ("abr_lm_step_batch", "abr2_lm_step_batch"):
        assert callable(getattr(mbfir, name))
