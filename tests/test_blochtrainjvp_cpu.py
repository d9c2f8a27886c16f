"""The tangent of the pulse train without a device: the NumPy reference of tests/blochtrainjvp_ref.py against itself (two independent
routes in long double, float64 against long double, central differences of the train in long double, the adjoint identity against
tests/blochtrainvjp_ref.py, the exact zeros of scale 0 and of echo = 0), the C ABI's declaration, binding and export, the
Python-side argument errors before any device work, and mbfir.torchsim.bloch_train(forward_mode=True) on calls stubbed by the
references."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainjvp_ref", os.path.join(ROOT, "tests", "blochtrainjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
tr, vjp = ref.tr, ref.vjp
LD = np.longdouble
CASES = list(ref.cases())
K = 2


def _worst(got, want, scale):
    """The largest |got - want| / scale over the planes of (dE, dF); scale: (K, nf, npos)"""
    w = 0.0
    for g, r in zip(got[0], want[0]):
        w = max(w, float((np.abs(g - r) / scale[:, None, None]).max()))
    for g, r in zip(got[1], want[1]):
        w = max(w, float((np.abs(g - r) / scale[:, None]).max()))
    return w


def _checks_sense(c, q):
    return np.abs(np.sin(c["phases"][q])).max() > 0.1 and len(c["pulses"][q][0]) > 1


@pytest.mark.parametrize("name", CASES)
def test_the_two_longdouble_routes_agree_and_the_opposite_sense_is_far_off(name):
    """The tangent of the tiled recursion and the structured route agree to 2e-16 of the tangent's size, the order to which the
    adjoint's two routes agree (long double carries 1e-19; a train of 257 repetitions loses two digits of it).  With the direction
    tiled by e^{-i phi_k} the tiled route is of the order of the tangent itself off wherever the phases are not multiples of pi."""
    c = ref.cases()[name]
    vs, dms = ref.directions(name, K)
    for q in range(len(c["pulses"])):
        want = ref.reference(name, K)[q]
        got = ref.run(ref.tiled_jvp, c, q, vs[q], dms[q], LD)
        size = ref.size_jvp(c, q, vs[q], dms[q])
        assert _worst(got, want, size) <= 2e-16, (q, _worst(got, want, size))
        if _checks_sense(c, q):
            zero = tuple(np.zeros_like(d) for d in dms[q])
            a = ref.run(ref.train_jvp, c, q, vs[q], zero, LD)
            b = ref.run(ref.tiled_jvp, c, q, vs[q], zero, LD, sense=-1)
            top = max(float(np.abs(x).max()) for x in a[0] + a[1])
            off = max(float(np.abs(x - y).max()) for x, y in zip(a[0] + a[1], b[0] + b[1]))
            assert off > 0.1 * top, (q, off, top)


def test_the_opposite_sense_is_checked_on_some_case():
    cs = ref.cases()
    assert sum(_checks_sense(c, q) for c in cs.values() for q in range(len(c["pulses"]))) >= 4


@pytest.mark.parametrize("name", CASES)
def test_float64_is_within_a_hundredth_of_the_bound(name):
    c = ref.cases()[name]
    vs, dms = ref.directions(name, K)
    for q in range(len(c["pulses"])):
        want = ref.reference(name, K)[q]
        got = ref.run(ref.train_jvp, c, q, vs[q], dms[q], np.float64)
        share = _worst(got, want, ref.bound_jvp(c, q, vs[q], dms[q]))
        print("%s pulse %d: float64 against long double, share of the bound %.3g" % (name, q, share))
        assert share <= 0.01, (q, share)


def test_the_first_directions_do_not_depend_on_how_many_are_drawn():
    v2, d2 = ref.directions("groups", 2)
    v5, d5 = ref.directions("groups", 5)
    assert all(np.array_equal(a, b[:2]) for a, b in zip(v2, v5))
    assert all(np.array_equal(x, y[:2]) for a, b in zip(d2, d5) for x, y in zip(a, b))
    assert ref.cases() is vjp.cases()


def _train(c, b1=None, m0=None, dtype=LD):
    p = c["pulses"][0]
    p = p if b1 is None else (b1,) + p[1:]
    return tr.train(p, c["dfs"][0], c["dps"][0], c["ntr"][0], c["phases"][0], c["gains"][0], c["echo"][0], c["scales"][0],
                    c["m0"][0] if m0 is None else m0, c["meq"], c["demod"], dtype)


def test_central_differences_of_the_train_in_longdouble():
    """9 samples, 3 repetitions, 6 points, along v and along dm0; the steps and the tolerance are blochtrainjvp_ref's, with the
    reason in its docstring"""
    c = ref.small()
    vs, dms = ref.directions("small", K)
    p = c["pulses"][0]
    zero = tuple(np.zeros_like(d) for d in dms[0])
    dE, dF = ref.run(ref.train_jvp, c, 0, vs[0], zero, LD)
    scale = c["ntr"][0] * ref.drive(c, 0, vs[0])[:, None, None] * ref.mu_of(c, 0)
    worst = 0.0
    for k in range(K):
        h = ref.FD_ANGLE / ref.drive(c, 0, vs[0])[k]
        (Ep, Fp), (Em, Fm) = _train(c, p[0] + h * vs[0][k]), _train(c, p[0] - h * vs[0][k])
        fe, ff = (Ep - Em) / (2 * LD(h)), (Fp - Fm) / (2 * LD(h))
        for i in range(3):
            worst = max(worst, float((np.abs(fe[:, i] - dE[i][k, 0]) / scale[k]).max()), float((np.abs(ff[i] - dF[i][k, 0]) / scale[k]).max()))
    print("central differences along v: worst %.3g of the scale (FD_TOL %.0e)" % (worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL
    dE, dF = ref.run(ref.train_jvp, c, 0, np.zeros_like(vs[0]), dms[0], LD)
    m0 = np.stack(c["m0"][0])
    for k in range(K):
        d = np.stack([x[k] for x in dms[0]])
        sm = np.maximum(np.abs(d).sum(0), 1.0)
        (Ep, Fp), (Em, Fm) = _train(c, m0=tuple(m0 + ref.FD_M0 * d)), _train(c, m0=tuple(m0 - ref.FD_M0 * d))
        fe, ff = (Ep - Em) / (2 * LD(ref.FD_M0)), (Fp - Fm) / (2 * LD(ref.FD_M0))
        for i in range(3):
            assert float((np.abs(fe[:, i] - dE[i][k, 0]) / sm).max()) <= ref.FD_TOL
            assert float((np.abs(ff[i] - dF[i][k, 0]) / sm).max()) <= ref.FD_TOL


@pytest.mark.parametrize("name", ["groups", "p65", "allgains", "batch"])
def test_the_adjoint_identity_against_the_reference_of_the_adjoint(name):
    """sum ce . decho + sum cf . dm_N = Re sum conj(G) v + sum gm0 . dm_0 in float64, within the two sides' own bounds"""
    c = ref.cases()[name]
    vs, dms = ref.directions(name, 1)
    for q in range(len(c["pulses"])):
        G, gm = vjp.run(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], c, q, np.float64)
        dE, dF = ref.run(ref.train_jvp, c, q, vs[q], dms[q], np.float64)
        d0 = tuple(d[0] for d in dms[q])
        left = ref.pairing(c, q, [e[0] for e in dE], [f[0] for f in dF])
        right = float((np.conj(G) * vs[q][0]).real.sum()) + sum(float((g * d).sum()) for g, d in zip(gm, d0))
        tol = ref.identity_tol(c, q, vs[q][0], d0)
        assert abs(left - right) <= tol, (q, left, right, tol)
        assert abs(left) > 1e3 * tol                                              # the identity is not met by smallness


def test_scale_zero_and_echo_zero_give_exact_zeros():
    c = ref.cases()["groups"]
    vs, _ = ref.directions("groups", K)
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    _, tan = ref.prop_jvp(p, df, dp, 0.0, 4, vs[0])
    assert not any(np.any(x) for M in (tan[0], tan[2]) for row in M for x in row) and not any(np.any(x) for b in (tan[1], tan[3]) for x in b)
    _, tan = ref.prop_jvp(p, df, dp, 1.0, 0, vs[0])
    assert not any(np.any(x) for row in tan[2] for x in row) and not any(np.any(x) for x in tan[3])
    assert any(np.any(x) for row in tan[0] for x in row)
    prim, tan9 = ref.prop_jvp(p, df, dp, 1.0, 9, vs[0])                          # echo = ntime: the bits of (dA, dB)
    assert all(np.array_equal(a, b) for ra, rb in zip(tan9[0], tan9[2]) for a, b in zip(ra, rb))
    want = tr.prop(p, df, dp, 1.0, 9)
    assert all(np.allclose(a, b, rtol=0, atol=1e-14) for ra, rb in zip(prim[0], want[0]) for a, b in zip(ra, rb))


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    name = "mbfir_bloch_train_jvp_batch"
    assert re.search(r"\b%s\s*\(" % name, hdr) and re.search(r"\bmbfir_test_bloch_train_jvp_group\s*\(", hdr)
    assert len(mbfir.SYMBOLS[name][1]) == len(mbfir.SYMBOLS["mbfir_bloch_train_batch"][1]) + 12
    lib = mbfir.load_library()
    assert getattr(lib, name) is not None                                        # the library exports it
    assert callable(mbfir.bloch_train_jvp_batch)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
    assert getattr(lib, name)(*args) == mbfir.E_ARG                              # a null context is refused before anything is read
    g = mbfir.bloch_train_jvp_group()
    assert len(g) == 2 and all(k in (1, 2, 4, 8) for k in g)


class _NoDevice:
    """Stands for the library: any call is device work that must not have been reached"""

    def __getattr__(self, name):
        raise AssertionError("the library call %s was reached" % name)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(mbfir, "load_library", lambda: _NoDevice())
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: (_ for _ in ()).throw(AssertionError("a context was asked for")))
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    call = mbfir.bloch_train_jvp_batch
    v, d = np.ones(4, dtype=complex), np.zeros((3, 5))
    who = "bloch_train_jvp_batch: "
    with pytest.raises(ValueError, match=who + "no pulses"):
        call([], df, dp, 4, [])
    with pytest.raises(ValueError, match=who + "the scale list is empty"):
        call([p], df, dp, 4, [v], scales=())
    with pytest.raises(ValueError, match=who + "ntr of pulse 0 must be at least 1"):
        call([p], df, dp, 0, [v])
    with pytest.raises(ValueError, match=who + "ntr must be an integer"):
        call([p], df, dp, 2.5, [v])
    with pytest.raises(ValueError, match=who + r"echo of pulse 0 must lie in \[0, ntime\]"):
        call([p], df, dp, 4, [v], echo=5)
    with pytest.raises(ValueError, match=who + "phases of pulse 0 has 3 entries for its 4 repetitions"):
        call([p], df, dp, 4, [v], phases=np.zeros(3))
    with pytest.raises(ValueError, match=who + "a gain is not finite"):
        call([p], df, dp, 4, [v], gains=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match=who + "a cosine or sine of the phase table is not finite"):
        call([p], df, dp, 4, [v], phases=np.nan)
    with pytest.raises(ValueError, match=who + "2 values of meq for 1 pulses"):
        call([p], df, dp, 4, [v], meq=[1.0, 0.0])
    with pytest.raises(ValueError, match=who + "meq of pulse 0 is not finite"):
        call([p], df, dp, 4, [v], meq=np.nan)
    with pytest.raises(ValueError, match=who + "echoes=False requires final=True"):
        call([p], df, dp, 4, [v], echoes=False)
    with pytest.raises(ValueError, match=who + "2 tangents for 1 pulses"):
        call([p], df, dp, 4, [v, v])
    with pytest.raises(ValueError, match=who + r"the tangent of pulse 0 has shape \(3,\), not \(4,\) or \(K, 4\)"):
        call([p], df, dp, 4, [v[:3]])
    with pytest.raises(ValueError, match=who + "the tangent of pulse 1 has shape .* every pulse takes the same K"):
        call([p, p], df, dp, 4, [v, np.stack([v, v])])
    with pytest.raises(ValueError, match=who + "2 m0 tangent triples for 1 pulses"):
        call([p], df, dp, 4, [v], tangents_m0=[(d, d, d)] * 2)
    with pytest.raises(ValueError, match=who + "the m0 tangent of pulse 0 must be a triple"):
        call([p], df, dp, 4, [v], tangents_m0=[(d, d)])
    with pytest.raises(ValueError, match=who + "an m0 tangent of pulse 0 has shape"):
        call([p], df, dp, 4, [v], tangents_m0=[(d, d, d[:2])])
    with pytest.raises(ValueError, match=who + "an m0 tangent of pulse 0 has shape"):
        call([p], df, dp, 4, [np.stack([v, v])], tangents_m0=[(np.zeros((3, 3, 5)),) * 3])      # three m0 directions for K = 2


def _stub_device_calls(monkeypatch, asked):
    """mbfir's three train calls replaced by the NumPy references, so that torchsim's plumbing runs without a device"""
    def bloch_train_batch(pulses, df, dp, ntr, *, phases, gains, echo, scales, m0, meq, demod, final):
        res = [tr.train(pulses[0], df, dp, ntr, phases, gains, echo, s, m0, meq, demod) for s in scales]
        E = tuple(np.stack([e[:, i] for e, _ in res]) for i in range(3))
        F = tuple(np.stack([f[i] for _, f in res]) for i in range(3))
        return [(E, F) if final else E]

    def bloch_train_vjp_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_m0):
        g, gm = vjp.vjp_scaled(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                               None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(g, gm) if grad_m0 else g]

    def bloch_train_jvp_batch(pulses, df, dp, ntr, tangents, *, tangents_m0, phases, gains, echo, scales, m0, meq, demod, final):
        asked.append((tangents[0].ndim, tangents_m0 is not None, final))
        dE, dF = ref.jvp_scaled(ref.train_jvp, pulses[0], df, dp, ntr, phases, gains, echo, tangents[0],
                                None if tangents_m0 is None else tangents_m0[0], scales, m0, meq, demod, np.float64)
        dE, dF = tuple(e[0] for e in dE), tuple(f[0] for f in dF)                 # a 1-D tangent: no K axis
        return [(dE, dF) if final else dE]
    monkeypatch.setattr(mbfir, "bloch_train_batch", bloch_train_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_batch", bloch_train_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_train_jvp_batch", bloch_train_jvp_batch, raising=False)


def test_torchsim_bloch_train_forward_mode_on_stubbed_calls(monkeypatch):
    """gradcheck with check_forward_ad in b1, in m0 and in both, echoes alone and with the final state, on 4 samples, 3 repetitions
    and 1 x 2 points (8z's test has the larger problem for the backward); torch.func.jvp equals the
    reference; one bloch_train_jvp_batch call with one direction per tangent; the default still raises; torchsim.bloch is the
    function it was."""
    import torch
    asked = []
    bloch_before = mbfir.torchsim._bloch_function()
    _stub_device_calls(monkeypatch, asked)
    rng = np.random.default_rng(7)
    gamma, dt = tr.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(4) + 1j * rng.standard_normal(4)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 4) * 0.05
    df, dp = np.array([-100.0]), np.array([-1.0, 1.5])
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 1, 2)), dtype=torch.float64, requires_grad=True)
    kw = dict(nucleus="H-1", phases=np.array([0.0, 2.0, -1.0]), gains=np.array([0.5, 1.0, 0.8]), echo=3, scales=(1.0, 0.8), meq=0.5)

    def f(b, m, final=False, demod=False, forward_mode=True):
        out = mbfir.torchsim.bloch_train(b, gr, dt, 1.0, 1e-3, df, dp, 3, m0=m, final=final, demod=demod, forward_mode=forward_mode, **kw)
        return out[0] + out[1] if final else out
    # the backward is the parent class's (tests/test_blochtrainvjp_cpu.py): it is checked again on the first and the last only
    check = lambda fn, args, back=False: torch.autograd.gradcheck(fn, args, check_forward_ad=True, check_backward_ad=back)
    assert check(lambda b: f(b, None), (b1,), True)
    assert check(lambda b: f(b, None, True, True), (b1,))
    assert check(lambda m: f(b1.detach(), m), (m0,))
    assert check(lambda m: f(b1.detach(), m, True), (m0,))
    assert check(lambda b, m: f(b, m), (b1, m0))
    assert check(lambda b, m: f(b, m, True, True), (b1, m0), True)
    del asked[:]
    vb = torch.tensor(rng.standard_normal(4) + 1j * rng.standard_normal(4), dtype=torch.complex128) * abs(b0).max()
    vm = torch.tensor(rng.standard_normal((3, 1, 2)), dtype=torch.float64)
    out, tan = torch.func.jvp(lambda b, m: f(b, m, True), (b1.detach(), m0.detach()), (vb, vm))
    assert asked == [(1, True, True)]                                            # one call, one direction, both tangents
    pulse = (b0, gr, dt, 1.0, 1e-3, "H-1")
    dE, dF = ref.jvp_scaled(ref.train_jvp, pulse, df, dp, 3, kw["phases"], kw["gains"], 3, vb.numpy(), tuple(vm.numpy()), kw["scales"],
                            tuple(m0.detach().numpy()), 0.5, False, np.float64)
    assert len(tan) == 6 and tuple(tan[0].shape) == (2, 3, 1, 2) and tuple(tan[5].shape) == (2, 1, 2)
    assert all(np.array_equal(t.numpy(), w[0]) for t, w in zip(tan, dE + dF))
    del asked[:]
    _, tan = torch.func.jvp(lambda m: f(b1.detach(), m), (m0.detach(),), (vm,))  # m0 alone: the b1 direction is zero
    assert asked == [(1, True, False)]
    dE, _ = ref.jvp_scaled(ref.train_jvp, pulse, df, dp, 3, kw["phases"], kw["gains"], 3, np.zeros(4), tuple(vm.numpy()), kw["scales"],
                           tuple(m0.detach().numpy()), 0.5, False, np.float64)
    assert all(np.array_equal(t.numpy(), w[0]) for t, w in zip(tan, dE))
    with pytest.raises(NotImplementedError, match="forward-mode"):               # the default keeps its class
        torch.func.jvp(lambda b: f(b, None, forward_mode=False), (b1.detach(),), (torch.ones_like(b1),))
    assert mbfir.torchsim._bloch_function() is bloch_before                      # torchsim.bloch keeps its classes
