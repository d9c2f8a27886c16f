"""The adjoint of the pulse train in its schedule without a device: the NumPy reference of tests/blochtrainsched_ref.py against
itself (float64 against long double, the structured route against the contracted tiled adjoint, central differences of
blochtrain_ref.train one repetition at a time, the closed forms of the hard-pulse case, the two Euler identities with the b1 adjoint
and its dL/dm0), the C ABI's declaration, binding and export, the Python-side argument errors before any device work, and
mbfir.torchsim.bloch_train's backward in gains and phases on calls stubbed by the reference."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainsched_ref", os.path.join(ROOT, "tests", "blochtrainsched_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
vjp, tr = ref.vjp, ref.tr
LD = np.longdouble
CASES = list(ref.cases())


def test_the_cases_cover_the_kernels_edges():
    cs = ref.cases()
    assert {"repeat", "zerogain", "hard"} <= set(cs) and set(vjp.cases()) <= set(cs)
    every = [(c, q) for c in cs.values() for q in range(len(c["pulses"]))]
    assert {1, 7, 8, 9, 257} <= {c["ntr"][q] for c, q in every}
    assert {6, 65, 300} <= {len(c["dfs"][q]) * len(c["dps"][q]) for c, q in every}
    assert {1, 9, 257} <= {len(c["pulses"][q][0]) for c, q in every}
    assert {1, 3} <= {len(c["scales"]) for c in cs.values()}
    assert {True, False} == {c["demod"] for c in cs.values()} and {0.0, 1.0} == {c["meq"] for c in cs.values()}
    assert {"echo", "final", "both"} == {c["cot"] for c in cs.values()}
    assert any(c["echo"][q] == 0 for c, q in every) and any(c["echo"][q] == len(c["pulses"][q][0]) for c, q in every)
    assert any(0 < c["echo"][q] < len(c["pulses"][q][0]) for c, q in every)
    ng = [(len(np.unique(c["gains"][q])), c["ntr"][q]) for c, q in every]
    assert any(g == 1 and n > 1 for g, n in ng) and any(1 < g < n for g, n in ng) and any(g == n and n > 1 for g, n in ng)
    assert list(cs["repeat"]["gains"][0]) == [0.5, 0.5, 1.0, 0.5] and list(cs["zerogain"]["gains"][0]) == [1.0, 0.0, 0.7]


@pytest.mark.parametrize("name", CASES)
def test_float64_is_within_a_hundredth_of_the_bounds(name):
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        gg, gp, gm = ref.reference(name)[q]
        g64, p64, m64 = ref.run(ref.sched_vjp, c, q, np.float64)
        sg = float(np.abs(g64 - gg).max() / ref.bound_gains(c, q))
        sp = float(np.abs(p64 - gp).max() / ref.bound_phases(c, q))
        sm = max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(m64, gm))
        print("%s pulse %d: float64 against long double, share of the gains bound %.3g, of the phases bound %.3g, of the m0 bound %.3g"
              % (name, q, sg, sp, sm))
        assert np.isfinite(g64).all() and np.isfinite(p64).all()
        assert sg <= 0.01 and sp <= 0.01 and sm <= 0.01, (q, sg, sp, sm)


@pytest.mark.parametrize("name", CASES)
def test_the_two_longdouble_routes_agree(name):
    """The contracted tiled adjoint and the structured route agree far within the float64 bounds: to 1e-5 of them (long double
    carries 1e-19 where the bounds' constant is 1e-12; a train of 257 repetitions loses two digits of it)"""
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        gg, gp, gm = ref.reference(name)[q]
        tg, tp, tm = ref.run(ref.tiled_sched, c, q, LD)
        assert np.abs(tg - gg).max() <= 1e-5 * ref.bound_gains(c, q), (q, np.abs(tg - gg).max() / ref.bound_gains(c, q))
        assert np.abs(tp - gp).max() <= 1e-5 * ref.bound_phases(c, q), (q, np.abs(tp - gp).max() / ref.bound_phases(c, q))
        assert max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(tm, gm)) <= 1e-5, q


def _total_loss(c, q, gains, phases, dtype):
    r = [tr.train(c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], phases, gains, c["echo"][q], s, c["m0"][q], c["meq"], c["demod"],
                  dtype) for s in c["scales"]]
    E, F = np.stack([e for e, _ in r]), np.stack([f for _, f in r])
    return ref.loss(c, q, [E[:, :, i] for i in range(3)], [F[:, i] for i in range(3)]).sum()


@pytest.mark.parametrize("name", ref.FD_CASES)
@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_central_differences_of_the_train_one_repetition_at_a_time(name, dtype):
    c, q = ref.case(name), 0
    losses = [_total_loss(c, q, g, p, dtype) for g, p in ref.fd_schedules(c, q)]
    dg, dp = ref.fd_quotients(c, q, losses)
    gg, gp, _ = ref.reference(name)[q]
    sg, sp = float(np.abs(dg - gg).max() / ref.scale_gains(c, q)), float(np.abs(dp - gp).max() / ref.scale_phases(c, q))
    print("%s in %s: central differences off by %.3g of the gains scale and %.3g of the phases scale" % (name, np.dtype(dtype).name, sg, sp))
    assert sg <= ref.FD_TOL and sp <= ref.FD_TOL, (sg, sp)
    if dtype is LD:                                                      # the differences' own error, 1e-9 of the entry's size
        assert sg * c["ntr"][q] <= 1e-9 and sp * c["ntr"][q] <= 1e-9, (sg, sp)


def test_repeated_gains_have_one_entry_per_repetition():
    """The three repetitions at gain 0.5 of 'repeat' have three different derivatives, and none is their sum"""
    gg = np.asarray(ref.reference("repeat")[0][0], dtype=np.float64)
    same = gg[[0, 1, 3]]
    assert np.abs(np.diff(np.sort(same))).min() > 1e-3 * np.abs(same).max()
    assert np.abs(gg).min() > 0


def test_a_zero_gain_has_a_finite_nonzero_derivative():
    """Finite, and far above the rounding of its own bound: the entry is a derivative, not a zero that was left there"""
    c = ref.cases()["zerogain"]
    gg, gp, _ = ref.run(ref.sched_vjp, c, 0, np.float64)
    assert np.isfinite(gg).all() and np.isfinite(gp).all() and abs(gg[1]) > 1e6 * ref.bound_gains(c, 0)


def test_the_hard_pulse_case_has_its_closed_forms():
    c = ref.cases()["hard"]
    E, F = tr.train(c["pulses"][0], c["dfs"][0], c["dps"][0], 4, c["phases"][0], c["gains"][0], 1, 1.0, c["m0"][0], 0.0, False, LD)
    Th = ref.HARD_THETA * np.cumsum(c["gains"][0])
    assert np.abs(E[:, 1, 0, 0] - np.sin(Th)).max() <= 1e-14 and np.abs(E[:, 2, 0, 0] - np.cos(Th)).max() <= 1e-14
    assert abs(F[2, 0, 0] - np.cos(Th[-1])) <= 1e-14 and np.abs(E[:, 0]).max() <= 1e-14
    gg, gp = ref.hard_closed()
    for dtype, share in ((LD, 1e-3), (np.float64, 0.01)):
        rg, rp, _ = ref.run(ref.sched_vjp, c, 0, dtype)
        assert np.abs(rg - gg).max() <= share * ref.bound_gains(c, 0) and np.abs(rp - gp).max() <= share * ref.bound_phases(c, 0)


@pytest.mark.parametrize("name", CASES)
def test_the_euler_identities_and_dm0_against_the_b1_adjoint(name):
    """L is homogeneous in (gains, b1) jointly, and a common phase is a rotation of b1: sum_k gains[k] gg[k] = sum_t (Re b1 Re G + Im b1
    Im G) and, without demod, sum_k gp[k] = sum_t (-Im b1 Re G + Re b1 Im G), G from blochtrainvjp_ref.train_vjp; dL/dm0 is its dL/dm0"""
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        gg, gp, gm = ref.reference(name)[q]
        G, gmv = vjp.reference(name)[q] if name in vjp.cases() else vjp.run(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], c, q, LD)
        b1 = np.asarray(c["pulses"][q][0], dtype=np.complex128)
        lhs = (np.asarray(c["gains"][q], dtype=LD) * gg).sum()
        rhs = (b1.real.astype(LD) * G.real + b1.imag.astype(LD) * G.imag).sum()
        tol = 1e-5 * (np.abs(c["gains"][q]).sum() * ref.bound_gains(c, q) + (np.abs(b1) * vjp.bound_b1(c, q)).sum())
        assert abs(lhs - rhs) <= tol, (q, lhs, rhs, tol)
        if not c["demod"]:
            rhs = (-b1.imag.astype(LD) * G.real + b1.real.astype(LD) * G.imag).sum()
            tol = 1e-5 * (c["ntr"][q] * ref.bound_phases(c, q) + (np.abs(b1) * vjp.bound_b1(c, q)).sum())
            assert abs(gp.sum() - rhs) <= tol, (q, gp.sum(), rhs, tol)
        assert all(np.array_equal(a, b) for a, b in zip(gm, gmv)), q


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    name = "mbfir_bloch_train_vjp_sched_batch"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    # mbfir_bloch_train_vjp_batch's arguments with (ggain, gphi) in the place of (g_re, g_im)
    assert mbfir.SYMBOLS[name][1] == mbfir.SYMBOLS["mbfir_bloch_train_vjp_batch"][1]
    assert getattr(mbfir.load_library(), name) is not None                       # the library exports it
    assert callable(mbfir.bloch_train_vjp_sched_batch)
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
    call = mbfir.bloch_train_vjp_sched_batch
    e, f = np.zeros((1, 4, 3, 5)), np.zeros((1, 3, 5))
    E, F = [(e, e, e)], [(f, f, f)]
    who = "bloch_train_vjp_sched_batch: "
    with pytest.raises(ValueError, match=who + "no pulses"):
        call([], df, dp, 4, [])
    with pytest.raises(ValueError, match=who + "ntr of pulse 0 must be at least 1"):
        call([p], df, dp, 0, E)
    with pytest.raises(ValueError, match=who + r"echo of pulse 0 must lie in \[0, ntime\]"):
        call([p], df, dp, 4, E, echo=5)
    with pytest.raises(ValueError, match=who + "gains of pulse 0 has 3 entries for its 4 repetitions"):
        call([p], df, dp, 4, E, gains=np.ones(3))
    with pytest.raises(ValueError, match=who + "a gain is not finite"):
        call([p], df, dp, 4, E, gains=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match=who + "a cosine or sine of the phase table is not finite"):
        call([p], df, dp, 4, E, phases=np.nan)
    with pytest.raises(ValueError, match=who + "neither echo cotangents nor final cotangents are given"):
        call([p], df, dp, 4, None)
    with pytest.raises(ValueError, match=who + "neither the gradient in the gains nor the gradient in the phases is wanted"):
        call([p], df, dp, 4, E, grad_gains=False, grad_phases=False)
    with pytest.raises(ValueError, match=who + "2 echo cotangent triples for 1 pulses"):
        call([p], df, dp, 4, E * 2)
    with pytest.raises(ValueError, match=who + "the final cotangent of pulse 0 must be a triple"):
        call([p], df, dp, 4, E, cot_final=[f])
    with pytest.raises(ValueError, match=who + "the echo cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, F)
    with pytest.raises(ValueError, match=who + "the final cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, None, cot_final=F, scales=(1.0, 0.9))


def _stub_device_calls(monkeypatch, asked):
    """mbfir's three train calls replaced by the NumPy reference, so that torchsim's plumbing runs without a device"""
    def bloch_train_batch(pulses, df, dp, ntr, *, phases, gains, echo, scales, m0, meq, demod, final):
        res = [tr.train(pulses[0], df, dp, ntr, phases, gains, echo, s, m0, meq, demod) for s in scales]
        E = tuple(np.stack([e[:, i] for e, _ in res]) for i in range(3))
        F = tuple(np.stack([f[i] for _, f in res]) for i in range(3))
        return [(E, F) if final else E]

    def bloch_train_vjp_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_m0):
        asked.append(("b1", grad_m0))
        g, gm = vjp.vjp_scaled(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                               None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(g, gm) if grad_m0 else g]

    def bloch_train_vjp_sched_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_gains,
                                    grad_phases):
        asked.append(("sched", grad_gains, grad_phases))
        gg, gp, _ = ref.sched_scaled(ref.sched_vjp, pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                                     None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(gg if grad_gains else None, gp if grad_phases else None)]
    monkeypatch.setattr(mbfir, "bloch_train_batch", bloch_train_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_batch", bloch_train_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_sched_batch", bloch_train_vjp_sched_batch, raising=False)


def test_torchsim_bloch_train_differentiates_the_schedule_on_stubbed_calls(monkeypatch):
    """gradcheck in gains, in phases, in both and together with b1 and m0, echoes alone and with the final state, demod off and on;
    the backward asks each call only for what needs a gradient; array schedules take the path they took; a forward-mode tangent in
    the schedule raises NotImplementedError"""
    import torch
    asked = []
    _stub_device_calls(monkeypatch, asked)
    rng = np.random.default_rng(11)
    gamma, dt = tr.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 6) * 0.05
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 2, 3)), dtype=torch.float64, requires_grad=True)
    gains = torch.tensor([0.5, 1.0, 0.0, 0.5], dtype=torch.float64, requires_grad=True)
    phases = torch.tensor([0.0, 2.0, -1.0, 0.5], dtype=torch.float64, requires_grad=True)
    kw = dict(nucleus="H-1", echo=3, scales=(1.0, 0.8), meq=0.5)

    def f(b, m, g, p, final=False, demod=False):
        out = mbfir.torchsim.bloch_train(b, gr, dt, 1.0, 1e-3, df, dp, 4, m0=m, gains=g, phases=p, final=final, demod=demod, **kw)
        return out[0] + out[1] if final else out
    b1c, pc = b1.detach(), phases.detach().numpy()
    assert torch.autograd.gradcheck(lambda g: f(b1c, None, g, pc), (gains,))
    assert torch.autograd.gradcheck(lambda p: f(b1c, None, gains.detach(), p, True, True), (phases,))
    assert torch.autograd.gradcheck(lambda g, p: f(b1c, None, g, p, True), (gains, phases))
    assert torch.autograd.gradcheck(lambda b, m, g, p: f(b, m, g, p, True), (b1, m0, gains, phases))
    assert torch.autograd.gradcheck(lambda b, g: f(b, None, g, pc, False, True), (b1, gains))
    del asked[:]
    mx, my, mz = f(b1c, None, gains, pc)
    (mx * my + mz).sum().backward()
    assert asked == [("sched", True, False)] and gains.grad is not None and tuple(gains.grad.shape) == (4,)
    del asked[:]
    mx, my, mz = f(b1, None, gains, phases)
    (mx * my + mz).sum().backward()
    assert asked == [("sched", True, True), ("b1", False)] and phases.grad is not None
    del asked[:]
    mx, my, mz = f(b1, None, gains.detach().numpy(), pc)                          # arrays: the path before the schedule had a gradient
    (mx * my + mz).sum().backward()
    assert asked == [("b1", False)]
    with pytest.raises(ValueError, match="shape"):
        f(b1c, None, torch.ones(3, dtype=torch.float64, requires_grad=True), pc)
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda g: f(b1c, None, g, pc), (gains.detach(),), (torch.ones_like(gains),))
