"""The tangent of the pulse train in its schedule without a device: the NumPy reference of tests/blochtrainschedjvp_ref.py against
itself (float64 against long double, two independent routes in long double, the pairing with the adjoint of
tests/blochtrainsched_ref.py, central differences of the train in long double, the closed forms of the case 'hard'), the C ABI's
declaration, binding and export, the Python-side argument errors before any device work, and
mbfir.torchsim.bloch_train(forward_mode=True) with the schedule in the graph on calls stubbed by the references."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainschedjvp_ref", os.path.join(ROOT, "tests", "blochtrainschedjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
sched, jvp, vjp, tr = ref.sched, ref.jvp, ref.vjp, ref.tr
LD = np.longdouble
CASES = list(ref.cases()) + ["small"]
K = 3                                                                             # one direction of every kind


@pytest.mark.parametrize("name", CASES)
def test_float64_is_within_a_hundredth_of_the_bound(name):
    c = ref.case(name)
    for q in range(len(c["pulses"])):
        d = ref.directions(name, K)[q]
        got = ref.run(ref.sched_jvp, c, q, *d, np.float64)
        want = ref.reference(name, K)[q]
        share = ref.worst(got, want, ref.bound_jvp(c, q, *d))
        top = ref.worst(want, (tuple(0 * w for w in want[0]), tuple(0 * w for w in want[1])), ref.size_jvp(c, q, *d))
        print("%s pulse %d: float64 against long double, share of the bound %.3g; the tangent reaches %.3g of its size" % (name, q, share, top))
        assert share <= 0.01, (q, share)
        assert top <= 1.0, (q, top)                                               # size is the size of the tangent


@pytest.mark.parametrize("name", CASES)
def test_the_two_longdouble_routes_agree(name):
    """The tangent of the tiled sample-by-sample recursion and the structured route agree to 2e-16 of the tangent's size, the order to
    which blochtrainjvp_ref's two routes agree (long double carries 1e-19; a train of 257 repetitions loses two digits of it)"""
    c = ref.case(name)
    for q in range(len(c["pulses"])):
        d = ref.directions(name, K)[q]
        got = ref.run(ref.tiled_jvp, c, q, *d, LD)
        w = ref.worst(got, ref.reference(name, K)[q], ref.size_jvp(c, q, *d))
        print("%s pulse %d: tiled against structured in long double, %.3g of the size" % (name, q, w))
        assert w <= 2e-16, (q, w)


@pytest.mark.parametrize("name", CASES)
def test_the_pairing_with_the_adjoint_in_longdouble(name):
    """<cot, J d> = gg . dg + gp . dp + <dL/dm0, dm0> with blochtrainsched_ref.sched_vjp, to 1e-15 relative, for every kind of
    direction"""
    c = ref.case(name)
    for q in range(len(c["pulses"])):
        dg, dp, dm0 = ref.directions(name, K)[q]
        dE, dF = ref.reference(name, K)[q]
        gg, gp, gm = sched.reference(name)[q]
        for k in range(K):
            left = 0
            if c["ce"][q] is not None:
                left = left + sum((np.asarray(ck, dtype=LD) * e[k]).sum() for ck, e in zip(c["ce"][q], dE))
            if c["cf"][q] is not None:
                left = left + sum((np.asarray(ck, dtype=LD) * f[k]).sum() for ck, f in zip(c["cf"][q], dF))
            right = (gg * dg[k]).sum() + (gp * dp[k]).sum() + sum((g * d[k].astype(LD)[None]).sum() for g, d in zip(gm, dm0))
            rel = abs(left - right) / max(abs(left), abs(right))
            print("%s pulse %d direction %d: pairing off by %.3g relative" % (name, q, k, rel))
            assert rel <= 1e-15, (q, k, left, right)


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_central_differences_of_the_train_in_longdouble(name):
    """Along the dense direction; the step and the tolerance are blochtrainschedjvp_ref's, with the reason in its docstring"""
    c = ref.case(name)
    dgs, dps, dms = ref.directions(name, K)[0]
    dg, dp, dm0 = dgs[2], dps[2], tuple(x[2] for x in dms)                        # direction 2 is the dense one
    dE, dF = ref.reference(name, K)[0]
    h = ref.fd_step(c, 0, dg, dp)
    m0 = np.stack(c["m0"][0])
    d = np.stack(dm0)
    scale = c["ntr"][0] * ref.size_jvp(c, 0, dg[None], dp[None], tuple(x[None] for x in dm0))[0]
    worst = 0.0
    for si, s in enumerate(c["scales"]):
        def train(sign):
            return tr.train(c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0], c["phases"][0] + sign * h * dp,
                            c["gains"][0] + sign * h * dg, c["echo"][0], s, tuple(m0 + sign * h * d), c["meq"], c["demod"], LD)
        (Ep, Fp), (Em, Fm) = train(+1), train(-1)
        fe, ff = (Ep - Em) / (2 * LD(h)), (Fp - Fm) / (2 * LD(h))
        for i in range(3):
            worst = max(worst, float((np.abs(fe[:, i] - dE[i][2, si]) / scale).max()), float((np.abs(ff[i] - dF[i][2, si]) / scale).max()))
    print("%s: central differences along the dense direction, worst %.3g of ntr size (FD_TOL %.0e)" % (name, worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL


def test_the_case_hard_against_its_closed_forms():
    c = ref.cases()["hard"]
    N = c["ntr"][0]
    dE, dF = ref.jacobian("hard")[0]
    wE, wF = ref.hard_closed()
    bound = ref.bound_jvp(c, 0, *ref.unit_directions(N), None)                    # (2 N, 1, 1)
    for i in range(3):
        assert np.all(np.abs(dE[i][:, 0, :, 0, 0] - wE[:, :, i]) <= bound[:, 0]), i
        assert np.all(np.abs(dF[i][:, 0, 0, 0] - wF[:, i]) <= bound[:, 0, 0]), i
    assert np.abs(wE).max() > 0.1 and np.abs(wE[N:]).max() > 0.1                  # neither half is met by smallness


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    name = "mbfir_bloch_train_jvp_sched_batch"
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m and re.search(r"\bmbfir_test_bloch_train_sched_jvp_group\s*\(", hdr)
    # mbfir_bloch_train_jvp_batch's arguments with (dgain, dphi) in the place of (v_re, v_im)
    assert mbfir.SYMBOLS[name][1] == mbfir.SYMBOLS["mbfir_bloch_train_jvp_batch"][1]
    assert len(m.group(1).split(",")) == len(mbfir.SYMBOLS[name][1])
    src = open(os.path.join(ROOT, "multiband-rf-pulse-design_amd", "csrc", "api.cpp")).read()
    m = re.search(r"\bint\s+%s\s*\(([^{]*)\)\s*\{" % name, src)
    assert m and len(m.group(1).split(",")) == len(mbfir.SYMBOLS[name][1])
    lib = mbfir.load_library()
    assert getattr(lib, name) is not None                                        # the library exports it
    assert callable(mbfir.bloch_train_jvp_sched_batch) and callable(mbfir.bloch_train_jacobian_sched_batch)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
    assert getattr(lib, name)(*args) == mbfir.E_ARG                              # a null context is refused before anything is read
    assert mbfir.bloch_train_sched_jvp_group() in (1, 2, 4, 8)


class _NoDevice:
    """Stands for the library: any call is device work that must not have been reached"""

    def __getattr__(self, name):
        raise AssertionError("the library call %s was reached" % name)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(mbfir, "load_library", lambda: _NoDevice())
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: (_ for _ in ()).throw(AssertionError("a context was asked for")))
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    call = mbfir.bloch_train_jvp_sched_batch
    g, d = np.ones(4), np.zeros((3, 5))
    who = "bloch_train_jvp_sched_batch: "
    with pytest.raises(ValueError, match=who + "no pulses"):
        call([], df, dp, 4, tangents_gains=[])
    with pytest.raises(ValueError, match=who + "ntr of pulse 0 must be at least 1"):
        call([p], df, dp, 0, tangents_gains=[g])
    with pytest.raises(ValueError, match=who + "gains of pulse 0 has 3 entries for its 4 repetitions"):
        call([p], df, dp, 4, tangents_gains=[g], gains=np.ones(3))
    with pytest.raises(ValueError, match=who + "echoes=False requires final=True"):
        call([p], df, dp, 4, tangents_gains=[g], echoes=False)
    with pytest.raises(ValueError, match=who + "no direction is given"):
        call([p], df, dp, 4)
    with pytest.raises(ValueError, match=who + "2 gains tangents for 1 pulses"):
        call([p], df, dp, 4, tangents_gains=[g, g])
    with pytest.raises(ValueError, match=who + "the phases tangent of pulse 0 is complex"):
        call([p], df, dp, 4, tangents_phases=[g.astype(complex)])
    with pytest.raises(ValueError, match=who + r"the gains tangent of pulse 0 has shape \(3,\), not \(4,\) or \(K, 4\)"):
        call([p], df, dp, 4, tangents_gains=[g[:3]])
    with pytest.raises(ValueError, match=who + r"the phases tangent of pulse 0 has shape \(2, 3\), not \(4,\) or \(K, 4\)"):
        call([p], df, dp, 4, tangents_phases=[np.ones((2, 3))])
    with pytest.raises(ValueError, match=who + "the gains tangent of pulse 1 has shape .* every pulse takes the same K"):
        call([p, p], df, dp, 4, tangents_gains=[g, np.stack([g, g])])
    with pytest.raises(ValueError, match=who + "2 directions of the phases for 1 of the gains"):
        call([p], df, dp, 4, tangents_gains=[g], tangents_phases=[np.stack([g, g])])
    with pytest.raises(ValueError, match=who + "2 m0 tangent triples for 1 pulses"):
        call([p], df, dp, 4, tangents_gains=[g], tangents_m0=[(d, d, d)] * 2)
    with pytest.raises(ValueError, match=who + "an m0 tangent of pulse 0 has shape"):
        call([p], df, dp, 4, tangents_gains=[np.stack([g, g])], tangents_m0=[(np.zeros((3, 3, 5)),) * 3])
    jac = mbfir.bloch_train_jacobian_sched_batch
    with pytest.raises(ValueError, match="bloch_train_jacobian_sched_batch: the pulses of a call must share ntr"):
        jac([p, p], df, dp, [4, 3])
    with pytest.raises(ValueError, match="bloch_train_jacobian_sched_batch: tangents_gains is not an argument"):
        jac([p], df, dp, 4, tangents_gains=[g])


def _stub_device_calls(monkeypatch, asked):
    """mbfir's train calls replaced by the float64 references, so that torchsim's plumbing runs without a device"""
    def bloch_train_batch(pulses, df, dp, ntr, *, phases, gains, echo, scales, m0, meq, demod, final):
        res = [tr.train(pulses[0], df, dp, ntr, phases, gains, echo, s, m0, meq, demod) for s in scales]
        E = tuple(np.stack([e[:, i] for e, _ in res]) for i in range(3))
        F = tuple(np.stack([f[i] for _, f in res]) for i in range(3))
        return [(E, F) if final else E]

    def bloch_train_vjp_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_m0):
        g, gm = vjp.vjp_scaled(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                               None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(g, gm) if grad_m0 else g]

    def bloch_train_vjp_sched_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_gains,
                                    grad_phases):
        gg, gp, _ = sched.sched_scaled(sched.sched_vjp, pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                                       None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(gg if grad_gains else None, gp if grad_phases else None)]

    def bloch_train_jvp_batch(pulses, df, dp, ntr, tangents, *, tangents_m0, phases, gains, echo, scales, m0, meq, demod, final):
        asked.append(("b1", tangents_m0 is not None))
        dE, dF = jvp.jvp_scaled(jvp.train_jvp, pulses[0], df, dp, ntr, phases, gains, echo, tangents[0],
                                None if tangents_m0 is None else tangents_m0[0], scales, m0, meq, demod, np.float64)
        dE, dF = tuple(e[0] for e in dE), tuple(f[0] for f in dF)                 # a 1-D tangent: no K axis
        return [(dE, dF) if final else dE]

    def bloch_train_jvp_sched_batch(pulses, df, dp, ntr, *, tangents_gains, tangents_phases, tangents_m0, phases, gains, echo, scales,
                                    m0, meq, demod, final):
        asked.append(("sched", tangents_gains is not None, tangents_phases is not None, tangents_m0 is not None))
        assert all(t is None or t[0].ndim == 1 for t in (tangents_gains, tangents_phases))                  # one direction
        dE, dF = ref.jvp_scaled(ref.sched_jvp, pulses[0], df, dp, ntr, phases, gains, echo,
                                None if tangents_gains is None else tangents_gains[0],
                                None if tangents_phases is None else tangents_phases[0],
                                None if tangents_m0 is None else tuple(np.asarray(d)[None] for d in tangents_m0[0]), scales, m0, meq,
                                demod, np.float64)
        dE, dF = tuple(e[0] for e in dE), tuple(f[0] for f in dF)
        return [(dE, dF) if final else dE]
    monkeypatch.setattr(mbfir, "bloch_train_batch", bloch_train_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_batch", bloch_train_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_sched_batch", bloch_train_vjp_sched_batch)
    monkeypatch.setattr(mbfir, "bloch_train_jvp_batch", bloch_train_jvp_batch)
    monkeypatch.setattr(mbfir, "bloch_train_jvp_sched_batch", bloch_train_jvp_sched_batch, raising=False)


def test_torchsim_bloch_train_forward_mode_in_the_schedule_on_stubbed_calls(monkeypatch):
    """gradcheck with check_forward_ad in gains, in phases, in both and jointly with b1 and m0, echoes alone and with the final state,
    demod off and on, on 4 samples, 3 repetitions and 1 x 2 points; the jvp asks each call only for what has a tangent, m0's going to
    one call; forward_mode=False still raises"""
    import torch
    asked = []
    _stub_device_calls(monkeypatch, asked)
    rng = np.random.default_rng(13)
    gamma, dt = tr.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(4) + 1j * rng.standard_normal(4)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 4) * 0.05
    df, dp = np.array([-100.0]), np.array([-1.0, 1.5])
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 1, 2)), dtype=torch.float64, requires_grad=True)
    gains = torch.tensor([0.5, 0.0, 0.8], dtype=torch.float64, requires_grad=True)
    phases = torch.tensor([0.0, 2.0, -1.0], dtype=torch.float64, requires_grad=True)
    kw = dict(nucleus="H-1", echo=3, scales=(1.0, 0.8), meq=0.5)

    def f(b, m, g, p, final=False, demod=False, forward_mode=True):
        out = mbfir.torchsim.bloch_train(b, gr, dt, 1.0, 1e-3, df, dp, 3, m0=m, gains=g, phases=p, final=final, demod=demod,
                                         forward_mode=forward_mode, **kw)
        return out[0] + out[1] if final else out
    b1c, gc, pc = b1.detach(), gains.detach(), phases.detach()
    gcn, pcn = gc.numpy().copy(), pc.numpy().copy()                               # constants of the graph
    # the backward is the parent class's (tests/test_blochtrainsched_cpu.py): it is checked again on the first and the last only
    check = lambda fn, args, back=False: torch.autograd.gradcheck(fn, args, check_forward_ad=True, check_backward_ad=back)
    assert check(lambda g: f(b1c, None, g, pcn), (gains,), True)
    assert check(lambda p: f(b1c, None, gcn, p, True, True), (phases,))
    assert check(lambda g, p: f(b1c, None, g, p, True), (gains, phases))
    assert check(lambda g, p: f(b1c, None, g, p, False, True), (gains, phases))
    assert check(lambda b, g: f(b, None, g, pcn), (b1, gains))
    assert check(lambda b, m, g, p: f(b, m, g, p, True), (b1, m0, gains, phases))
    assert check(lambda b, m, g, p: f(b, m, g, p, True, True), (b1, m0, gains, phases), True)
    vg = torch.tensor(rng.standard_normal(3), dtype=torch.float64)
    vp = torch.tensor(rng.standard_normal(3), dtype=torch.float64)
    vb = torch.tensor(rng.standard_normal(4) + 1j * rng.standard_normal(4), dtype=torch.complex128) * abs(b0).max()
    vm = torch.tensor(rng.standard_normal((3, 1, 2)), dtype=torch.float64)
    pulse = (b0, gr, dt, 1.0, 1e-3, "H-1")
    m0h = tuple(m0.detach().numpy())
    del asked[:]
    _, tan = torch.func.jvp(lambda g: f(b1c, None, g, pcn), (gc,), (vg,))
    assert asked == [("sched", True, False, False)]
    dE, _ = ref.jvp_scaled(ref.sched_jvp, pulse, df, dp, 3, pcn, gcn, 3, vg.numpy(), None, None, kw["scales"], None, 0.5,
                           False, np.float64)
    assert len(tan) == 3 and tuple(tan[0].shape) == (2, 3, 1, 2) and all(np.array_equal(t.numpy(), w[0]) for t, w in zip(tan, dE))
    del asked[:]
    torch.func.jvp(lambda p: f(b1c, None, gc, p), (pc,), (vp,))                   # a tensor of gains without a tangent
    assert asked == [("sched", False, True, False)]
    del asked[:]
    with torch.autograd.forward_ad.dual_level():                                 # m0 alone has a tangent; the gains only require grad
        f(b1c, torch.autograd.forward_ad.make_dual(m0.detach(), vm), gains, pcn)
    assert asked == [("sched", False, False, True)]
    del asked[:]
    _, tan = torch.func.jvp(lambda b, m, g, p: f(b, m, g, p, True), (b1c, m0.detach(), gc, pc), (vb, vm, vg, vp))
    assert asked == [("sched", True, True, True), ("b1", False)]                 # m0's tangent goes to one call only
    dE, dF = ref.jvp_scaled(ref.sched_jvp, pulse, df, dp, 3, pcn, gcn, 3, vg.numpy(), vp.numpy(),
                            tuple(v[None] for v in vm.numpy()), kw["scales"], m0h, 0.5, False, np.float64)
    bE, bF = jvp.jvp_scaled(jvp.train_jvp, pulse, df, dp, 3, pcn, gcn, 3, vb.numpy(), None, kw["scales"], m0h, 0.5, False,
                            np.float64)
    assert len(tan) == 6 and all(np.array_equal(t.numpy(), a[0] + b[0]) for t, a, b in zip(tan, dE + dF, bE + bF))
    del asked[:]
    torch.func.jvp(lambda b, g: f(b, None, g, pcn), (b1c, gc), (vb, vg))
    assert asked == [("sched", True, False, False), ("b1", False)]
    with pytest.raises(NotImplementedError, match="forward-mode"):               # the default keeps its class
        torch.func.jvp(lambda g: f(b1c, None, g, pcn, forward_mode=False), (gc,), (vg,))
