"""The adjoint of the pulse train in b1, m0, the gradient waveform and the off-resonance without a device: the NumPy reference of
tests/blochtrainvjpg_ref.py against itself (two independent routes in long double, the b1 and m0 parts against
tests/blochtrainvjp_ref.py to the bit, central differences of the long-double train entry by entry, float64 against long double, the
scale sweep), the C ABI's declaration, binding and export, the Python-side argument errors before any device work, and
mbfir.torchsim.bloch_train on calls stubbed by the reference."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainvjpg_ref", os.path.join(ROOT, "tests", "blochtrainvjpg_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
vjp, tr = ref.vjp, ref.tr
LD = np.longdouble
CASES = list(ref.cases())


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(a).max())


@pytest.mark.parametrize("name", CASES)
def test_the_two_longdouble_routes_agree(name):
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        a, b = ref.reference(name, LD)[q], ref.run(ref.tiled_vjp_gr, c, q, LD)
        live = ref.bound_gr(c, q)[0] > 0                                           # the axes some position has
        eg, ed = _rel(a[1][:, live], b[1][:, live]), _rel(a[3], b[3])
        print("%s pulse %d: structured against tiled in long double, gr %.3g df %.3g relative" % (name, q, eg, ed))
        assert eg <= 1e-15 and ed <= 1e-15, (q, eg, ed)
        assert not a[1][:, ~live].any() and not b[1][:, ~live].any(), q


@pytest.mark.parametrize("name", CASES)
def test_the_b1_and_m0_parts_are_the_b1_adjoint_of_the_reference_to_the_bit(name):
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        got = ref.reference(name)[q]
        want = vjp.run(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], c, q, np.float64)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(u, v) for u, v in zip(got[2], want[1])), q


def test_central_differences_of_the_train_in_longdouble():
    """Every entry of gr moved by FD_GR and every entry of df by FD_DF on small(): within FD_TOL of the largest entry"""
    c = ref.small()
    G = ref.run(ref.train_vjp_gr, c, 0, LD)
    p = c["pulses"][0]
    gr = np.asarray(p[1], dtype=np.float64).reshape(len(p[0]), -1)
    df = np.asarray(c["dfs"][0], dtype=np.float64)
    worst = 0.0
    for t in range(gr.shape[0]):
        d = np.zeros_like(gr)
        d[t, 0] = ref.FD_GR
        fd = (ref.loss_of_train(c, 0, gr + d, df) - ref.loss_of_train(c, 0, gr - d, df)) / (2 * LD(ref.FD_GR))
        worst = max(worst, float(abs(fd - G[1][t, 0]) / np.abs(G[1]).max()))
    assert gr.shape[1] == 1 and not G[1][:, 1:].any()                              # no position has a y or z coordinate
    gd, worst_df = G[3].sum((0, 2)), 0.0
    for f in range(len(df)):
        d = np.zeros_like(df)
        d[f] = ref.FD_DF
        fd = (ref.loss_of_train(c, 0, gr, df + d) - ref.loss_of_train(c, 0, gr, df - d)) / (2 * LD(ref.FD_DF))
        worst_df = max(worst_df, float(abs(fd - gd[f]) / np.abs(gd).max()))
    print("central differences of the long-double train: gr %.3g of max|grad_gr|, df %.3g of max|grad_df| (FD_TOL %.0e)"
          % (worst, worst_df, ref.FD_TOL))
    assert worst <= ref.FD_TOL and worst_df <= ref.FD_TOL


@pytest.mark.parametrize("name", CASES)
def test_float64_is_within_a_hundredth_of_the_bounds(name):
    c = ref.cases()[name]
    for q in range(len(c["pulses"])):
        f, l = ref.reference(name)[q], ref.reference(name, LD)[q]
        bg, bd = ref.bound_gr(c, q), ref.bound_df(c, q)
        pos = bg > 0
        sg = float((np.abs(f[1] - l[1])[pos] / bg[pos]).max())
        sd = float((np.abs(f[3] - l[3]) / bd).max())
        sb = float((np.abs(f[0] - l[0]) / ref.bound_b1(c, q)).max())
        sm = max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(f[2], l[2]))
        print("%s pulse %d: float64 against long double, share of the bounds gr %.3g df %.3g b1 %.3g m0 %.3g" % (name, q, sg, sd, sb, sm))
        assert max(sg, sd, sb, sm) <= 0.01, (q, sg, sd, sb, sm)
        assert np.all(f[1][~pos] == 0.0) and np.all(l[1][~pos] == 0.0), q


def test_the_cases_cover_the_sub_groups_and_the_axes():
    c = ref.cases()["sub"]
    assert [len(p[0]) for p in c["pulses"]] == [2, 3, 4, 5] and [d.shape[1] for d in c["dps"]] == [3, 2, 1, 3]
    assert c["ntr"] == [3, 9, 8, 5] and c["echo"] == [1, 3, 0, 2] and c["scales"] == (1.0, 0.0, 0.9)
    assert all(len(np.unique(g)) == 3 for g in c["gains"])
    assert [int((ref.bound_gr(c, q)[0] > 0).sum()) for q in range(4)] == [3, 2, 1, 3]
    assert set(vjp.cases()) < set(ref.cases())


def test_the_scale_sweep_gr_has_no_amplitude_factor_scale_zero_has_no_b1_gradient_and_df_is_per_scale():
    c = ref.cases()["sub"]
    for q in range(4):
        args = (c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q])
        tail = (c["m0"][q], c["meq"], c["demod"], np.float64)
        G, gg, gm, gd = ref.reference("sub")[q]
        each = [ref.vjp_gr_scaled(ref.train_vjp_gr, *args, [v[k:k + 1] for v in c["ce"][q]], [v[k:k + 1] for v in c["cf"][q]], (s,), *tail)
                for k, s in enumerate(c["scales"])]
        assert not each[1][0].any() and each[1][1].any() and each[1][3].any()      # scale 0: no b1 gradient, gr and df live
        assert np.array_equal(gg, (each[0][1] + each[1][1]) + each[2][1])          # the plain sum: no factor scale x gain
        assert np.array_equal(G, (each[0][0] + each[1][0]) + each[2][0])
        for k in range(3):
            assert np.array_equal(gd[k], each[k][3][0]) and all(np.array_equal(a[k], b[0]) for a, b in zip(gm, each[k][2]))


def test_the_reference_prints_its_step_sweep():
    eg, ed = ref.fd_sweep()
    print("gr: " + "  ".join("h %.0e: %.3g" % kv for kv in eg.items()))
    print("df: " + "  ".join("h %.0e: %.3g" % kv for kv in ed.items()))
    assert min(eg, key=eg.get) == ref.FD_DIR_GR and min(ed, key=ed.get) == ref.FD_DIR_DF
    assert eg[ref.FD_DIR_GR] <= 1.5 * ref.FD_DIR_GR_MIN and ed[ref.FD_DIR_DF] <= 1.5 * ref.FD_DIR_DF_MIN


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    name = "mbfir_bloch_train_vjp_gr_batch"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    # mbfir_bloch_train_vjp_batch's arguments, then ggx, ggy, ggz and gdf
    assert len(mbfir.SYMBOLS[name][1]) == len(mbfir.SYMBOLS["mbfir_bloch_train_vjp_batch"][1]) + 4
    assert mbfir.SYMBOLS[name][1][:-4] == mbfir.SYMBOLS["mbfir_bloch_train_vjp_batch"][1]
    assert getattr(mbfir.load_library(), name) is not None                       # the library exports it
    assert callable(mbfir.bloch_train_vjp_gr_batch)
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
    call = mbfir.bloch_train_vjp_gr_batch
    e, f = np.zeros((1, 4, 3, 5)), np.zeros((1, 3, 5))
    E, F = [(e, e, e)], [(f, f, f)]
    who = "bloch_train_vjp_gr_batch: "
    with pytest.raises(ValueError, match=who + "no pulses"):
        call([], df, dp, 4, [])
    with pytest.raises(ValueError, match=who + "the scale list is empty"):
        call([p], df, dp, 4, E, scales=())
    with pytest.raises(ValueError, match=who + "pulse 0 has more than 3 gradient axes"):
        call([(np.ones(4), np.ones((4, 4)), 4e-6, 1.0, 1.0, "C-13")], df, dp, 4, E)
    with pytest.raises(ValueError, match=who + "ntr of pulse 0 must be at least 1"):
        call([p], df, dp, 0, E)
    with pytest.raises(ValueError, match=who + r"echo of pulse 0 must lie in \[0, ntime\]"):
        call([p], df, dp, 4, E, echo=5)
    with pytest.raises(ValueError, match=who + "phases of pulse 0 has 3 entries for its 4 repetitions"):
        call([p], df, dp, 4, E, phases=np.zeros(3))
    with pytest.raises(ValueError, match=who + "a gain is not finite"):
        call([p], df, dp, 4, E, gains=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match=who + "meq of pulse 0 is not finite"):
        call([p], df, dp, 4, E, meq=np.nan)
    with pytest.raises(ValueError, match=who + "neither echo cotangents nor final cotangents are given"):
        call([p], df, dp, 4, None, grad_df=True)
    with pytest.raises(ValueError, match=who + "2 echo cotangent triples for 1 pulses"):
        call([p], df, dp, 4, E * 2)
    with pytest.raises(ValueError, match=who + "the final cotangent of pulse 0 must be a triple"):
        call([p], df, dp, 4, E, cot_final=[f])
    with pytest.raises(ValueError, match=who + "the echo cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, F, grad_m0=True)
    with pytest.raises(ValueError, match=who + "the final cotangents of pulse 0 have shapes"):
        call([p], df, dp, 4, None, cot_final=F, scales=(1.0, 0.9))


def _stub_device_calls(monkeypatch, asked):
    """mbfir's three train calls replaced by the NumPy reference, so that torchsim's plumbing runs without a device; asked collects
    (call, keywords) of every adjoint call"""
    def bloch_train_batch(pulses, df, dp, ntr, *, phases, gains, echo, scales, m0, meq, demod, final):
        res = [tr.train(pulses[0], df, dp, ntr, phases, gains, echo, s, m0, meq, demod) for s in scales]
        E = tuple(np.stack([e[:, i] for e, _ in res]) for i in range(3))
        F = tuple(np.stack([f[i] for _, f in res]) for i in range(3))
        return [(E, F) if final else E]

    def bloch_train_vjp_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_m0):
        asked.append(("b1", dict(grad_m0=grad_m0)))
        g, gm = vjp.vjp_scaled(lambda *a, **k: vjp.train_vjp(*a, **k)[:2], pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                               None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(g, gm) if grad_m0 else g]

    def bloch_train_vjp_gr_batch(pulses, df, dp, ntr, cot, *, cot_final, phases, gains, echo, scales, m0, meq, demod, grad_m0, grad_df):
        asked.append(("gr", dict(grad_m0=grad_m0, grad_df=grad_df)))
        g, gg, gm, gd = ref.vjp_gr_scaled(ref.train_vjp_gr, pulses[0], df, dp, ntr, phases, gains, echo, cot[0],
                                          None if cot_final is None else cot_final[0], scales, m0, meq, demod, np.float64)
        return [(g, gg) + ((gm,) if grad_m0 else ()) + ((gd,) if grad_df else ())]
    monkeypatch.setattr(mbfir, "bloch_train_batch", bloch_train_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_batch", bloch_train_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_train_vjp_gr_batch", bloch_train_vjp_gr_batch, raising=False)


def test_torchsim_bloch_train_passes_gradcheck_in_gr_and_df_on_stubbed_calls(monkeypatch):
    """6 samples plus a dead time, 2 x 3 points, two scales, 3 repetitions at two gains: gradcheck in gr, in df and in (b1, gr, df, m0);
    a backward that needs only b1 makes the b1 call with its keywords; grad_df and grad_m0 are asked for only when needed; the
    ValueErrors and NotImplementedErrors"""
    import torch
    asked = []
    _stub_device_calls(monkeypatch, asked)
    rng = np.random.default_rng(11)
    gamma, dt = tr.GAMMA_H1, 1e-4
    b0 = np.append((rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt)), 0.0)
    g0 = np.append(rng.uniform(0.5, 1.5, (6, 2)) * 0.05, np.zeros((1, 2)), 0)
    tp = np.append(np.full(6, dt), 2e-3)
    d0, dp = np.array([-100.0, 30.0]), np.array([[-1.0, 0.5], [0.0, 0.0], [1.5, -0.7]])
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    gr = torch.tensor(g0, dtype=torch.float64, requires_grad=True)
    df = torch.tensor(d0, dtype=torch.float64, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 2, 3)), dtype=torch.float64, requires_grad=True)
    kw = dict(nucleus="H-1", phases=np.array([0.0, 2.0, -1.0]), gains=np.array([0.5, 1.0, 1.0]), echo=3, scales=(1.0, 0.8), meq=0.5)

    def f(b, g, d, m=None, final=False, demod=False):
        out = mbfir.torchsim.bloch_train(b, g, tp, 0.13, 0.03, d, dp, 3, m0=m, final=final, demod=demod, **kw)
        return out[0] + out[1] if final else out
    assert torch.autograd.gradcheck(lambda g: f(b1.detach(), g, d0), (gr,))
    assert torch.autograd.gradcheck(lambda d: f(b1.detach(), g0, d, None, True, True), (df,))
    assert torch.autograd.gradcheck(lambda b, g, d, m: f(b, g, d, m, True), (b1, gr, df, m0))
    g1 = torch.tensor(g0[:, 0], dtype=torch.float64, requires_grad=True)            # a 1-D gr: its gradient is cut to its shape
    sum(o.sum() for o in f(b1.detach(), g1, d0)).backward()
    g2 = torch.tensor(np.stack([g0[:, 0], np.zeros(7)], 1), dtype=torch.float64, requires_grad=True)
    sum(o.sum() for o in f(b1.detach(), g2, d0)).backward()
    assert g1.grad.shape == (7,) and np.array_equal(g1.grad.numpy(), g2.grad.numpy()[:, 0])
    # what each backward asks of the device
    del asked[:]
    sum(o.sum() for o in f(b1, gr.detach().requires_grad_(False), df)).backward()
    assert asked == [("gr", dict(grad_m0=False, grad_df=True))]
    del asked[:]
    sum(o.sum() for o in f(b1.detach(), gr, d0, m0)).backward()
    assert asked == [("gr", dict(grad_m0=True, grad_df=False))]
    del asked[:]
    tkw = (("phases", kw["phases"]), ("gains", kw["gains"]), ("echo", 3), ("scales", (1.0, 0.8)), ("meq", 0.5), ("demod", False))
    out = mbfir.torchsim._train_g_function().apply(b1, None, gr.detach(), d0, (tp, 0.13, 0.03, "H-1"), dp, 3, tkw, False)
    sum(o.sum() for o in out).backward()                                            # the new class where neither gr nor df needs one
    assert asked == [("b1", dict(grad_m0=False))]
    del asked[:]
    sum(o.sum() for o in f(b1, g0, d0)).backward()                                  # neither in the graph: the shipped class
    assert asked == [("b1", dict(grad_m0=False))]
    with pytest.raises(ValueError, match=r"a gr that requires grad must be a float64 tensor of shape \(n,\) or \(n, 1..3\)"):
        f(b1, torch.tensor(g0, dtype=torch.float32, requires_grad=True), d0)
    with pytest.raises(ValueError, match=r"a gr that requires grad must be a float64 tensor of shape \(n,\) or \(n, 1..3\)"):
        f(b1, torch.zeros(7, 4, dtype=torch.float64, requires_grad=True), d0)
    with pytest.raises(ValueError, match=r"a df that requires grad must be a float64 tensor of shape \(nf,\)"):
        f(b1, g0, torch.tensor(d0[None], dtype=torch.float64, requires_grad=True))
    for fm in (False, True):
        with pytest.raises(NotImplementedError, match="forward-mode"):
            torch.func.jvp(lambda g: mbfir.torchsim.bloch_train(b1.detach(), g, tp, 0.13, 0.03, d0, dp, 3, forward_mode=fm, **kw),
                           (gr.detach(),), (torch.ones_like(gr),))
        with pytest.raises(NotImplementedError, match="forward-mode"):
            torch.func.jvp(lambda d: mbfir.torchsim.bloch_train(b1.detach(), g0, tp, 0.13, 0.03, d, dp, 3, forward_mode=fm, **kw),
                           (df.detach(),), (torch.ones_like(df),))
    sched = dict(kw, gains=torch.tensor(kw["gains"], requires_grad=True))
    with pytest.raises(NotImplementedError, match="gains and the phases"):
        mbfir.torchsim.bloch_train(b1, gr, tp, 0.13, 0.03, d0, dp, 3, **sched)
    sched = dict(kw, phases=torch.tensor(kw["phases"], requires_grad=True))
    with pytest.raises(NotImplementedError, match="gains and the phases"):
        mbfir.torchsim.bloch_train(b1, g0, tp, 0.13, 0.03, df, dp, 3, **sched)
