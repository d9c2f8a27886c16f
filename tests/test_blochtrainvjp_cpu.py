"""The adjoint of the pulse train without a device: the NumPy reference of tests/blochtrainvjp_ref.py against itself (two independent
routes in long double, float64 against long double, central differences of the train in long double, the properties of dL/dm0 and
of echo = 0), the C ABI's declaration, binding and export, the Python-side argument errors before any device work, and
mbfir.torchsim.bloch_train on calls stubbed by the reference."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainvjp_ref", os.path.join(ROOT, "tests", "blochtrainvjp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
tr = ref.tr
LD = np.longdouble
CASES = list(ref.cases())
_structured = lambda *a, **k: ref.train_vjp(*a, **k)[:2]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(a).max())


@pytest.mark.parametrize("name", CASES)
def test_the_two_longdouble_routes_agree_and_the_opposite_sense_is_far_off(name):
    """The reversed tiled recursion and the structured route agree to about 1e-16 relative in G and in dL/dm0 (long double carries
    1e-19; a train of 257 repetitions loses two digits of it).  With the phase's sense reversed in the chain rule the tiled route is
    of the order of the gradient itself off wherever the phases are not multiples of pi."""
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        G, gm = ref.reference(name)[q]
        Gt, gmt = ref.run(ref.tiled_vjp, c, q, LD)
        assert _rel(G, Gt) <= 2e-16, (q, _rel(G, Gt))
        top = max(float(np.abs(v).max()) for v in gm)
        assert max(float(np.abs(a - b).max()) for a, b in zip(gm, gmt)) <= 2e-16 * top, q
        if np.abs(np.sin(c["phases"][q])).max() > 0.1 and len(c["pulses"][q][0]) > 1:
            Gw, _ = ref.run(ref.tiled_vjp, c, q, LD, sense=-1)
            assert _rel(G, Gw) > 0.1, (q, _rel(G, Gw))


def test_the_opposite_sense_is_checked_on_some_case():
    cs = ref.cases()
    assert sum(np.abs(np.sin(c["phases"][q])).max() > 0.1 and len(c["pulses"][q][0]) > 1 for c in cs.values()
               for q in range(len(c["pulses"]))) >= 4


@pytest.mark.parametrize("name", CASES)
def test_float64_is_within_a_hundredth_of_the_bounds(name):
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        G, gm = ref.reference(name)[q]
        G64, gm64 = ref.run(_structured, c, q, np.float64)
        sb = float((np.abs(G64 - G) / ref.bound_b1(c, q)).max())
        sm = max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(gm64, gm))
        print("%s pulse %d: float64 against long double, share of the b1 bound %.3g, of the m0 bound %.3g" % (name, q, sb, sm))
        assert sb <= 0.01 and sm <= 0.01, (q, sb, sm)


def test_the_cases_cover_the_edges():
    cs = ref.cases()
    assert set(tr.cases()) <= set(cs)
    ntr = {n for c in cs.values() for n in c["ntr"]}
    assert {1, 2, 7, 8, 9, 257} <= ntr
    assert any(len(c["dfs"][q]) * len(c["dps"][q]) == 65 for c in cs.values() for q in range(len(c["pulses"])))
    assert any(len(np.unique(c["gains"][q])) == c["ntr"][q] > 1 for c in cs.values() for q in range(len(c["pulses"])))
    assert {c["cot"] for c in cs.values()} == {"echo", "final", "both"}
    assert {c["demod"] for c in cs.values()} == {False, True} and {c["meq"] for c in cs.values()} == {0.0, 1.0}
    assert tr.cases()["c13_ramp"].keys() == {"pulses", "dfs", "dps", "ntr", "phases", "gains", "echo", "m0", "scales"}     # untouched


def _losses(c, b1=None, m0=None, dtype=LD):
    """The per-point loss of the small case through blochtrain_ref.train"""
    p = c["pulses"][0]
    p = p if b1 is None else (b1,) + p[1:]
    E, F = tr.train(p, c["dfs"][0], c["dps"][0], c["ntr"][0], c["phases"][0], c["gains"][0], c["echo"][0], c["scales"][0],
                    c["m0"][0] if m0 is None else m0, c["meq"], c["demod"], dtype)
    return ref.loss(c, 0, [E[None, :, i] for i in range(3)], [F[None, i] for i in range(3)])


def test_central_differences_of_the_train_in_longdouble():
    """9 samples, 3 repetitions, 6 points, in b1 and in m0; the step and the tolerance are blochtrainvjp_ref's FD_ANGLE, FD_M0 and
    FD_TOL, with the reason in its docstring"""
    c = ref.small()
    G, gm = ref.run(_structured, c, 0, LD)
    p = c["pulses"][0]
    sb, sm = ref.scale_b1(c, 0), ref.scale_m0(c, 0)[0]
    h = ref.FD_ANGLE / (tr.gamma_of(p[5]) * tr.intervals(p) * ref.amax_of(c, 0))
    worst = 0.0
    for t in range(len(p[0])):
        for unit in (1.0, 1j):
            d = np.zeros(len(p[0]), dtype=complex)
            d[t] = unit * h[t]
            fd = (_losses(c, p[0] + d).sum() - _losses(c, p[0] - d).sum()) / (2 * LD(h[t]))
            worst = max(worst, float(abs(fd - (G[t].real if unit == 1.0 else G[t].imag)) / sb[t]))
    print("central differences in b1: worst %.3g of the scale (FD_TOL %.0e)" % (worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL
    m0 = np.stack(c["m0"][0])
    for i in range(3):
        d = np.zeros_like(m0)
        d[i] = ref.FD_M0
        fd = (_losses(c, m0=tuple(m0 + d)) - _losses(c, m0=tuple(m0 - d))) / (2 * LD(ref.FD_M0))
        assert float((np.abs(fd - gm[i][0]) / sm).max()) <= ref.FD_TOL, i


def test_dldm0_has_the_same_bits_for_any_m0_and_any_meq():
    c = ref.cases()["groups"]
    rng = np.random.default_rng(3)
    other = tuple(rng.uniform(-1, 1, (3, 3, 2)))
    for q in range(3):
        base = ref.run(_structured, c, q, np.float64)[1]
        for kw in (dict(m0=other), dict(meq=1.0), dict(meq=0.37, m0=None)):
            got = ref.run(_structured, c, q, np.float64, **kw)[1]
            assert all(np.array_equal(a, b) for a, b in zip(base, got)), (q, kw)
        assert not np.array_equal(ref.run(_structured, c, q, np.float64, m0=other)[0], ref.run(_structured, c, q, np.float64)[0])


def test_echo_zero_reaches_b1_only_through_later_repetitions():
    """echo = 0: echo_k = m_k.  With one repetition the echo is m0 itself and the b1 gradient is exactly zero, with dL/dm0 the
    cotangent; with three repetitions the cotangent of the first echo does not reach b1, the others do."""
    c = dict(ref.small())
    c["echo"], c["cf"] = [0], [None]
    ce = c["ce"][0]
    one = dict(c, ntr=[1], phases=[c["phases"][0][:1]], gains=[c["gains"][0][:1]], ce=[tuple(v[:, :1] for v in ce)])
    for route in (_structured, ref.tiled_vjp):
        G, gm = ref.run(route, one, 0, np.float64)
        assert not G.any()
        # the structured route turns the cotangent by Z(+phi) and back: two rotations' rounding, 4 u of its 2-norm
        top = 4 * tr.U * np.sqrt(sum(v[:, 0] ** 2 for v in one["ce"][0]))
        assert all(np.all(np.abs(a - b[:, 0]) <= top) for a, b in zip(gm, one["ce"][0]))
    first = dict(c, ce=[tuple(np.concatenate([v[:, :1], np.zeros_like(v[:, 1:])], 1) for v in ce)])
    assert not ref.run(_structured, first, 0, np.float64)[0].any()
    assert ref.run(_structured, c, 0, np.float64)[0].all()


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    name = "mbfir_bloch_train_vjp_batch"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    # the train's arguments through demod and m0 (its own 19 less the six output planes), six cotangent planes, five gradient planes
    assert len(mbfir.SYMBOLS[name][1]) == len(mbfir.SYMBOLS["mbfir_bloch_train_batch"][1]) - 6 + 11
    assert getattr(mbfir.load_library(), name) is not None                       # the library exports it
    assert callable(mbfir.bloch_train_vjp_batch)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
    assert getattr(mbfir.load_library(), name)(*args) == mbfir.E_ARG             # a null context is refused before anything is read


class _NoDevice:
    """Stands for the library: any call is device work that must not have been reached"""

    def __getattr__(self, name):
        raise AssertionError("the library call %s was reached" % name)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(mbfir, "load_library", lambda: _NoDevice())
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: (_ for _ in ()).throw(AssertionError("a context was asked for")))
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    call = mbfir.bloch_train_vjp_batch
    e, f = np.zeros((1, 4, 3, 5)), np.zeros((1, 3, 5))
    E, F = [(e, e, e)], [(f, f, f)]
    who = "bloch_train_vjp_batch: "
    with pytest.raises(ValueError, match=who + "no pulses"):
        call([], df, dp, 4, [])
    with pytest.raises(ValueError, match=who + "the scale list is empty"):
        call([p], df, dp, 4, E, scales=())
    with pytest.raises(ValueError, match=who + "ntr of pulse 0 must be at least 1"):
        call([p], df, dp, 0, E)
    with pytest.raises(ValueError, match=who + "ntr must be an integer"):
        call([p], df, dp, 2.5, E)
    with pytest.raises(ValueError, match=who + r"echo of pulse 0 must lie in \[0, ntime\]"):
        call([p], df, dp, 4, E, echo=5)
    with pytest.raises(ValueError, match=who + "phases of pulse 0 has 3 entries for its 4 repetitions"):
        call([p], df, dp, 4, E, phases=np.zeros(3))
    with pytest.raises(ValueError, match=who + "a gain is not finite"):
        call([p], df, dp, 4, E, gains=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match=who + "a cosine or sine of the phase table is not finite"):
        call([p], df, dp, 4, E, phases=np.nan)
    with pytest.raises(ValueError, match=who + "2 values of meq for 1 pulses"):
        call([p], df, dp, 4, E, meq=[1.0, 0.0])
    with pytest.raises(ValueError, match=who + "meq of pulse 0 is not finite"):
        call([p], df, dp, 4, E, meq=np.nan)
    with pytest.raises(ValueError, match=who + "neither echo cotangents nor final cotangents are given"):
        call([p], df, dp, 4, None)
    with pytest.raises(ValueError, match=who + "2 echo cotangent triples for 1 pulses"):
        call([p], df, dp, 4, E * 2)
    with pytest.raises(ValueError, match=who + "2 final cotangent triples for 1 pulses"):
        call([p], df, dp, 4, None, cot_final=F * 2)
    with pytest.raises(ValueError, match=who + "the echo cotangent of pulse 0 must be a triple"):
        call([p], df, dp, 4, [(e, e)])
    with pytest.raises(ValueError, match=who + "the final cotangent of pulse 0 must be a triple"):
        call([p], df, dp, 4, E, cot_final=[f])
    with pytest.raises(ValueError, match=who + "the echo cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, [(e, e, e[:, :3])])
    with pytest.raises(ValueError, match=who + "the echo cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, F)                                                   # the final state's shape where the echoes' belongs
    with pytest.raises(ValueError, match=who + "the final cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, None, cot_final=E)
    with pytest.raises(ValueError, match=who + "the final cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, None, cot_final=F, scales=(1.0, 0.9))


def _stub_device_calls(monkeypatch, asked):
    """mbfir's two train calls replaced by the NumPy reference, so that torchsim's plumbing runs without a device"""
    def bloch_train_batch(pulses, df, dp, ntr, *, phases, gains, echo, scales, m0, meq, demod, final):
        res = [tr.train(pulses[0], df, dp, ntr, phases, gains, echo, s, m0, meq, demod) for s in scales]
        E = tuple(np.stack([e[:, i] for e, _ in res]) for i in range(3))
        F = tuple(np.stack([f[i] for _, f in res]) for i in range(3))
        return [(E, F) if final else E]

    def bloch_train_vjp_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_m0):
        asked.append(grad_m0)
        g, gm = ref.vjp_scaled(_structured, pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                               None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(g, gm) if grad_m0 else g]
    monkeypatch.setattr(mbfir, "bloch_train_batch", bloch_train_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_batch", bloch_train_vjp_batch, raising=False)


def test_torchsim_bloch_train_passes_gradcheck_on_stubbed_calls(monkeypatch):
    """gradcheck in b1, in m0 and in both, echoes alone and with the final state, demod off and on, on 6 samples, 4 repetitions and
    2 x 3 points; a backward that needs only b1 does not ask for dL/dm0; a forward-mode tangent raises NotImplementedError; torchsim.bloch is
    the function it was."""
    import torch
    asked = []
    bloch_before = mbfir.torchsim._bloch_function()
    _stub_device_calls(monkeypatch, asked)
    rng = np.random.default_rng(7)
    gamma, dt = tr.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 6) * 0.05
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 2, 3)), dtype=torch.float64, requires_grad=True)
    kw = dict(nucleus="H-1", phases=np.array([0.0, 2.0, -1.0, 0.5]), gains=np.array([0.5, 1.0, 1.0, 0.8]), echo=3, scales=(1.0, 0.8), meq=0.5)

    def f(b, m, final=False, demod=False):
        out = mbfir.torchsim.bloch_train(b, gr, dt, 1.0, 1e-3, df, dp, 4, m0=m, final=final, demod=demod, **kw)
        return out[0] + out[1] if final else out
    assert torch.autograd.gradcheck(lambda b: f(b, None), (b1,))
    assert torch.autograd.gradcheck(lambda b: f(b, None, True, True), (b1,))
    assert torch.autograd.gradcheck(lambda m: f(b1.detach(), m, True), (m0,))
    assert torch.autograd.gradcheck(lambda b, m: f(b, m, True), (b1, m0))
    assert torch.autograd.gradcheck(lambda b, m: f(b, m, False, True), (b1, m0))
    (mx, my, mz), (fx, fy, fz) = mbfir.torchsim.bloch_train(b1, gr, dt, 1.0, 1e-3, df, dp, 4, m0=m0.detach(), final=True, **kw)
    assert mx.dtype == torch.float64 and tuple(mx.shape) == (2, 4, 2, 3) and tuple(fz.shape) == (2, 2, 3)
    del asked[:]
    (mx * my + mz).sum().backward()
    assert asked == [False] and b1.grad is not None
    with pytest.raises(ValueError, match="complex128"):
        mbfir.torchsim.bloch_train(torch.ones(6), gr, dt, 1.0, 1e-3, df, dp, 4)
    with pytest.raises(ValueError, match="shape"):
        mbfir.torchsim.bloch_train(b1, gr, dt, 1.0, 1e-3, df, dp, 4, m0=torch.zeros(3, 6, dtype=torch.float64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: f(b, None), (b1.detach(),), (torch.ones_like(b1),))
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda m: f(b1.detach(), m), (m0.detach(),), (torch.ones_like(m0),))
    assert mbfir.torchsim._bloch_function() is bloch_before                      # torchsim.bloch keeps its classes
