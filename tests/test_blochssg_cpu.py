"""The NumPy reference of the steady state's adjoint in b1, gr and df (tests/blochssg_ref.py, no GPU): its b1 part and M against
tests/blochss_ref.py, its gr and df part against central differences of that file's long-double steady state, its float64 form
against its long-double one on the cases of tests/test_blochssg_gpu.py, the scale sweep, and the declaration, the binding, the
argument errors and the torch plumbing of mbfir.bloch_ss_vjp_gr_batch / mbfir.torchsim.bloch(steady_state=True), none of which needs
a device."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochssg_ref", os.path.join(ROOT, "tests", "blochssg_ref.py"))
refg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refg)
ref = refg.ss


@functools.lru_cache(maxsize=None)
def _case(shared):
    """The eight periods (and, on their own grids, the four short ones) with kappa and the float64 results"""
    pulses, dfs, dps, cots = ref.batch(shared)
    if not shared:
        pulses, dfs, dps, cots = [a + b for a, b in zip((pulses, dfs, dps, cots), refg.batch_sub())]
    ks = [ref.kappa(p, df, dp, ref.SCALES) for p, df, dp in zip(pulses, dfs, dps)]
    res = [refg.ss_vjp_gr_scaled(p, df, dp, c, ref.SCALES) for p, df, dp, c in zip(pulses, dfs, dps, cots)]
    return pulses, dfs, dps, cots, ks, res


def test_short_periods_span_t1_over_period_and_every_remainder():
    pulses, dfs, dps, cots = refg.batch_sub()
    assert [len(p[0]) for p in pulses] == [2, 3, 4, 5] and refg.batch_sub()[0] is pulses
    for q, p in enumerate(pulses):
        tr = float(ref.intervals(p).sum())
        assert 4.0 <= p[3] / tr <= 1000.0 * (1 + 1e-12), q
        assert (np.ndim(p[2]) == 1) == (q % 2 == 1) and (q % 2 == 0 or p[0][-1] == 0.0)
        assert cots[q][0].shape[1:] == refg.POINTS[(q + 1) % 4]


@pytest.mark.parametrize("shared", [False, True])
def test_reference_b1_part_and_steady_state_are_blochss_ref(shared):
    pulses, dfs, dps, cots, _, res = _case(shared)
    for q, (p, df, dp, cot, (g, _, _, M)) in enumerate(zip(pulses, dfs, dps, cots, res)):
        if q >= 8 or (len(p[0]) > 260 and shared):
            continue                                                    # the eight periods; the long ones once
        wg, wm = ref.ss_vjp_scaled(p, df, dp, cot, ref.SCALES)
        assert np.array_equal(g, wg) and all(np.array_equal(a, b) for a, b in zip(M, wm)), q


@pytest.mark.parametrize("q", [1, 3])
def test_reference_gr_and_df_are_the_central_differences_of_the_longdouble_steady_state(q):
    """Entry by entry on periods q = 1 (n = 7, kappa 30.5) and q = 3 (n = 9, kappa 5001) of batch(True), scales (1, 0, 0.9): h = 1e-6
    G/cm in gr against 1e-7 max(max|g|, 1), h = 1e-3 Hz in df against 1e-6 max|grad_df|.  Measured: gr 2.6e-11 and 9.0e-10 of
    max(max|g|, 1) = 2.35 and 18.2; df 5.7e-12 and 2.3e-10 of max|grad_df|"""
    pulses, dfs, dps, cots, ks, res = _case(True)
    pulse, df, dp, cot = pulses[q], dfs[q], dps[q], cots[q]
    b1, gr, tp, t1, t2, nucleus = pulse
    n = len(b1)
    gr3 = np.concatenate([gr, np.zeros((n, 3 - gr.shape[1]))], 1)       # an axis the pulse does not play: differentiated at zero
    c = [np.asarray(v, dtype=np.longdouble) for v in cot]

    def Lp(g, f):
        """per entry (S, nf, npos), in long double: df of one frequency row moves only that row's points"""
        M = ref.ss_scaled((b1, g, tp, t1, t2, nucleus), f, dp, ref.SCALES, np.longdouble)
        return c[0] * M[0] + c[1] * M[1] + c[2] * M[2]
    _, gg, gdf, _ = res[q]
    fd = np.zeros_like(gg)
    for t in range(n):
        for a in range(3):
            e = np.zeros_like(gr3)
            e[t, a] = 1e-6
            fd[t, a] = float((Lp(gr3 + e, df).sum() - Lp(gr3 - e, df).sum()) / np.longdouble(2e-6))
    fdf = ((Lp(gr3, df + 1e-3) - Lp(gr3, df - 1e-3)) / np.longdouble(2e-3)).astype(np.float64)
    eg, ed = float(np.abs(fd - gg).max()), float(np.abs(fdf - gdf).max())
    sg, sd = max(float(np.abs(gg).max()), 1.0), float(np.abs(gdf).max())
    print("q %d n %d kappa %.4g: gr |fd - ref| %.3g of max(max|g|, 1) = %.3g: %.3g; df |fd - ref| %.3g of max|grad_df| = %.3g: %.3g"
          % (q, n, ks[q], eg, sg, eg / sg, ed, sd, ed / sd))
    assert np.all(np.isfinite(gg)) and np.all(np.isfinite(gdf)) and np.abs(gg).max() > 0 and sd > 0
    assert eg <= 1e-7 * sg and ed <= 1e-6 * sd


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_is_the_longdouble_one_to_a_hundredth_of_each_bound(shared):
    """Measured worst shares (tests/blochssg_ref.py has them): b1 and M as tests/test_blochss_cpu.py; gr with the first power of
    kappa, df with the second.  The share df would have with the first power is printed beside it."""
    pulses, dfs, dps, cots, ks, res = _case(shared)
    worst = np.zeros(5)
    for q, (p, df, dp, cot, k, (g64, a64, d64, M64)) in enumerate(zip(pulses, dfs, dps, cots, ks, res)):
        gl, al, dl, Ml = refg.ss_vjp_gr_scaled(p, df, dp, cot, ref.SCALES, np.longdouble)
        sm = max(float(np.abs(a - b).max()) for a, b in zip(M64, Ml)) / refg.bound_m(k)
        sb = float((np.abs(g64 - gl).astype(np.float64) / refg.bound_b1(p, cot, ref.SCALES, k)).max())
        ea, ba = np.abs(a64 - al).astype(np.float64), refg.bound_gr(p, dp, cot, k)
        ed, bd = np.abs(d64 - dl).astype(np.float64), refg.bound_df(p, cot, k)
        pos = ba > 0
        sa, sd = float((ea[pos] / ba[pos]).max()) if pos.any() else 0.0, float((ed / bd).max())
        print("shared %s n %d points %s kappa %.4g: |f64 - ld| / bound: M %.3g, b1 %.3g, gr %.3g, df %.3g (first power of kappa: %.3g)"
              % (shared, len(p[0]), cot[0].shape[1:], k, sm, sb, sa, sd, sd * k))
        worst = np.maximum(worst, [sm, sb, sa, sd, sd * k])
        assert sm <= 0.01 and sb <= 0.01 and sa <= 0.01 and sd <= 0.01, q
        assert np.all(a64[~pos] == 0.0) and np.all(al[~pos] == 0.0), q                 # a zero bound: exactly zero
    print("shared %s worst shares: M %.3g, b1 %.3g, gr %.3g, df %.3g (first power of kappa: %.3g)" % ((shared,) + tuple(worst)))


def test_scale_sweep_carries_s_in_b1_and_not_in_gr():
    """At b1 = 0 the period does not depend on the scale: the gr and df gradients of every scale are then those of scale 1, while
    the b1 gradient of scale s is s times the one with respect to s b1; a sweep is the sum of its scales, grad_df is per scale, and
    the b1 gradient of scale 0 is exactly zero."""
    pulses, dfs, dps, cots, _, res = _case(True)
    pulse, df, dp, cot = pulses[3], dfs[3], dps[3], cots[3]
    w = [c[0] for c in cot]
    zp = (np.zeros_like(pulse[0]),) + pulse[1:]
    g1, a1, d1, _ = refg.ss_vjp_gr(zp, df, dp, 1.0, w)
    g3, a3, d3, _ = refg.ss_vjp_gr(zp, df, dp, 3.0, w)
    assert np.array_equal(a1, a3) and np.array_equal(d1, d3) and np.abs(g1).max() > 0
    assert np.allclose(g3, 3.0 * g1, rtol=1e-14, atol=0)
    g, a, d, M = res[3]
    parts = [refg.ss_vjp_gr(pulse, df, dp, s, [c[k] for c in cot]) for k, s in enumerate(ref.SCALES)]
    assert np.array_equal(a, parts[0][1] + parts[1][1] + parts[2][1]) and np.array_equal(g, parts[0][0] + parts[1][0] + parts[2][0])
    assert all(np.array_equal(d[k], parts[k][2]) for k in range(3)) and np.array_equal(parts[1][0], np.zeros(len(pulse[0])))
    assert all(np.array_equal(M[c][k], parts[k][3][c]) for c in range(3) for k in range(3))
    assert d.shape == (3,) + cot[0].shape[1:] and a.shape == (len(pulse[0]), 3) and a.dtype == np.float64


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_bloch_ss_vjp_gr_batch\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_bloch_ss_vjp_gr_batch"][1]) == len(mbfir.SYMBOLS["mbfir_bloch_ss_vjp_batch"][1]) + 4 == 35
    assert getattr(mbfir.load_library(), "mbfir_bloch_ss_vjp_gr_batch") is not None     # the library exports it
    assert callable(mbfir.bloch_ss_vjp_gr_batch)


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    c = np.zeros((1, 3, 5))
    call = mbfir.bloch_ss_vjp_gr_batch
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: no pulses"):
        call([], df, dp, [])
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: the scale list is empty"):
        call([p], df, dp, [(c, c, c)], scales=())
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: pulse 1 has no samples"):
        call([p, (np.zeros(0),) + p[1:]], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: pulse 0 has more than 3 gradient axes"):
        call([(p[0], np.zeros((4, 4))) + p[2:]], df, dp, [(c, c, c)])
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: 2 cotangent triples for 1 pulses"):
        call([p], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: the cotangent of pulse 0 must be a triple"):
        call([p], df, dp, [(c, c)])
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: the cotangents of pulse 0 have shapes"):
        call([p], df, dp, [(c, c, c[:, :, :4])], grad_df=True)
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: the cotangents of pulse 0 have shapes"):
        call([p], df, dp, [(c, c, c)], scales=(1.0, 0.9), steady=True)
    with pytest.raises(ValueError, match="bloch_ss_vjp_gr_batch: an empty grid"):
        call([p], np.zeros(0), dp, [(c, c, c)])
    with pytest.raises(TypeError):                                                        # no m0: the steady state does not depend on it
        call([p], df, dp, [(c, c, c)], m0=None)
    # the C call refuses a null context before it reads anything else (the checks that need a context, each with its message:
    # tests/test_blochssg_gpu.py)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS["mbfir_bloch_ss_vjp_gr_batch"][1][1:]]
    assert mbfir.load_library().mbfir_bloch_ss_vjp_gr_batch(*args) == mbfir.E_ARG


def _stub_device_calls(monkeypatch, calls):
    """mbfir's steady-state calls replaced by the NumPy references, so that torchsim's plumbing runs without a device; calls
    receives (name, keyword arguments) of every adjoint call"""
    def bloch_batch(pulses, df, dp, *, scales, mode):
        assert mode == 1
        return [ref.ss_scaled(pulses[0], df, dp, scales)]

    def bloch_ss_vjp_batch(pulses, df, dp, cot, **kw):
        calls.append(("b1", kw))
        return [ref.ss_vjp_scaled(pulses[0], df, dp, cot[0], kw["scales"])[0]]

    def bloch_ss_vjp_gr_batch(pulses, df, dp, cot, *, scales, grad_df):
        calls.append(("gr", dict(scales=scales, grad_df=grad_df)))
        g, gg, gd, _ = refg.ss_vjp_gr_scaled(pulses[0], df, dp, cot[0], scales)
        return [(g, gg) + ((gd,) if grad_df else ())]

    def bloch_ss_jvp_batch(pulses, df, dp, tangents, *, scales):
        calls.append(("jvp", dict(scales=scales)))
        assert np.ndim(tangents[0]) == 1                                                  # one direction, without the K axis
        M, tan = ref.ss_jvp(pulses[0], df, dp, tangents[0], scales)
        return [(M, tuple(t[0] for t in tan))]
    monkeypatch.setattr(mbfir, "bloch_batch", bloch_batch)
    monkeypatch.setattr(mbfir, "bloch_ss_vjp_batch", bloch_ss_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_ss_vjp_gr_batch", bloch_ss_vjp_gr_batch, raising=False)
    monkeypatch.setattr(mbfir, "bloch_ss_jvp_batch", bloch_ss_jvp_batch)


SC = (1.0, 0.8)


def _torch_case():
    """6 samples plus a dead time (a period of 2.6 ms at T1 = 0.13 s: T1 / period = 50), two gradient axes, 2 x 3 points"""
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(7) + 1j * rng.standard_normal(7)) * (0.5 / (gamma * dt))
    b0[-1] = 0.0
    g0 = rng.uniform(0.5, 1.5, (7, 2)) * 0.05
    g0[-1] = 0.0
    tp = np.append(np.full(6, dt), 2e-3)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    gr = torch.tensor(g0, dtype=torch.float64, requires_grad=True)
    df = torch.tensor([-100.0, 30.0], dtype=torch.float64, requires_grad=True)
    dp = np.array([[-1.0, 0.5], [0.0, 0.0], [1.5, -0.7]])
    return b1, gr, df, dp, tp


def _f(b, g, d, dp, tp, **kw):
    return mbfir.torchsim.bloch(b, g, tp, 0.13, 0.03, d, dp, nucleus="H-1", scales=SC, steady_state=True, **kw)


def test_torchsim_bloch_steady_state_passes_gradcheck_in_gr_and_df_on_stubbed_calls(monkeypatch):
    """gradcheck in gr (two axes, and one axis as a 1-D tensor), in df and in (b1, gr, df); gr's gradient has gr's shape, df's is
    summed over scales and positions; the forward is the steady state of the reference"""
    import torch
    calls = []
    _stub_device_calls(monkeypatch, calls)
    b1, gr, df, dp, tp = _torch_case()
    f = lambda b, g, d: _f(b, g, d, dp, tp)
    b0, g0, d0 = b1.detach(), gr.detach(), df.detach()
    assert torch.autograd.gradcheck(lambda g: f(b0, g, d0), (gr,))
    g1 = gr.detach()[:, 0].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda g: f(b0, g, d0), (g1,))
    assert torch.autograd.gradcheck(lambda d: f(b0, g0, d), (df,))
    assert torch.autograd.gradcheck(f, (b1, gr, df))
    assert calls and all(c[0] == "gr" for c in calls)
    mx, my, mz = f(b1, gr, df)
    want = ref.ss_scaled((b0.numpy(), g0.numpy(), tp, 0.13, 0.03, "H-1"), d0.numpy(), dp, SC)
    assert all(np.array_equal(o.detach().numpy(), w) for o, w in zip((mx, my, mz), want))
    (mx * my + mz).sum().backward()
    assert gr.grad.shape == gr.shape and df.grad.shape == df.shape and b1.grad.shape == b1.shape
    cot = (my.detach().numpy(), mx.detach().numpy(), np.ones_like(want[2]))
    _, gg, gd, _ = refg.ss_vjp_gr_scaled((b0.numpy(), g0.numpy(), tp, 0.13, 0.03, "H-1"), d0.numpy(), dp, cot, SC)
    assert np.array_equal(gr.grad.numpy(), gg[:, :2]) and np.array_equal(df.grad.numpy(), gd.sum(axis=(0, 2)))


def test_torchsim_bloch_steady_state_asks_only_for_what_is_needed(monkeypatch):
    calls = []
    _stub_device_calls(monkeypatch, calls)
    b1, gr, df, dp, tp = _torch_case()

    def run(b, g, d, **kw):
        del calls[:]
        mx, my, mz = _f(b, g, d, dp, tp, **kw)
        (mx * my + mz).sum().backward()
        return list(calls)
    g0, d0 = gr.detach(), df.detach()
    # only b1: today's call with today's keyword arguments, never the new one; tensors that do not require grad are constants
    for fm in (False, True):
        assert run(b1, g0.numpy(), d0.numpy(), forward_mode=fm) == [("b1", dict(scales=SC))]
        assert run(b1, g0, d0, forward_mode=fm) == [("b1", dict(scales=SC))]
    # gr and / or df: one call of the new function, grad_df only when needed
    assert run(b1, gr, d0) == [("gr", dict(scales=SC, grad_df=False))]
    assert run(b1, g0, df) == [("gr", dict(scales=SC, grad_df=True))]
    assert run(b1.detach(), gr, df, forward_mode=True) == [("gr", dict(scales=SC, grad_df=True))]
    # an output that the loss does not use has a zero cotangent, in both forward_mode settings
    for fm in (False, True):
        gr.grad = None
        _f(b1, gr, d0, dp, tp, forward_mode=fm)[0].sum().backward()
        one = np.ones((2, 2, 3))
        want = refg.ss_vjp_gr_scaled((b1.detach().numpy(), g0.numpy(), tp, 0.13, 0.03, "H-1"), d0.numpy(), dp,
                                     (one, 0 * one, 0 * one), SC)[1]
        assert np.array_equal(gr.grad.numpy(), want[:, :2])


def test_torchsim_bloch_steady_state_refuses_other_dtypes_shapes_and_forward_tangents(monkeypatch):
    import torch
    calls = []
    _stub_device_calls(monkeypatch, calls)
    b1, gr, df, dp, tp = _torch_case()
    f = lambda b, g, d, **kw: _f(b, g, d, dp, tp, **kw)
    with pytest.raises(ValueError, match="gr that requires grad must be a float64 tensor of shape"):
        f(b1, gr.detach().float().requires_grad_(True), df)
    with pytest.raises(ValueError, match="gr that requires grad must be a float64 tensor of shape"):
        f(b1, torch.zeros(7, 4, dtype=torch.float64, requires_grad=True), df)
    with pytest.raises(ValueError, match="df that requires grad must be a float64 tensor of shape"):
        f(b1, gr, df.detach().float().requires_grad_(True))
    with pytest.raises(ValueError, match="df that requires grad must be a float64 tensor of shape"):
        f(b1, gr, df.detach().reshape(2, 1).requires_grad_(True))
    with pytest.raises(ValueError, match="does not depend on m0"):
        f(b1, gr, df, m0=(0.0, 0.0, 1.0))
    b0, g0, d0 = b1.detach(), gr.detach(), df.detach()
    for fm in (False, True):
        with pytest.raises(NotImplementedError, match="forward-mode"):
            torch.func.jvp(lambda g: f(b0, g, d0, forward_mode=fm), (g0,), (torch.ones_like(g0),))
        with pytest.raises(NotImplementedError, match="forward-mode"):
            torch.func.jvp(lambda d: f(b0, g0, d, forward_mode=fm), (d0,), (torch.ones_like(d0),))
    # the b1 tangent with forward_mode stays one bloch_ss_jvp_batch call and equals the reference, gr and df being inputs of the graph
    v = np.random.default_rng(9).standard_normal(7) + 1j * np.random.default_rng(10).standard_normal(7)
    del calls[:]
    out, tan = torch.func.jvp(lambda b: f(b, gr, df, forward_mode=True), (b0,), (torch.tensor(v),))
    assert [c[0] for c in calls] == ["jvp"]
    wm, wt = ref.ss_jvp((b0.numpy(), g0.numpy(), tp, 0.13, 0.03, "H-1"), d0.numpy(), dp, v, SC)
    assert all(np.array_equal(o.detach().numpy(), w) for o, w in zip(out, wm))
    assert all(np.array_equal(t.detach().numpy(), w[0]) for t, w in zip(tan, wt))
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: f(b, gr, df), (b0,), (torch.tensor(v),))
