"""The NumPy reference of the Bloch adjoint in gr and df (tests/blochgradg_ref.py, no GPU): its b1 and m0 part against
tests/blochgrad_ref.py, its gr and df part against central differences of that file's forward, its float64 form against its
long-double one on the cases of tests/test_blochgradg_gpu.py, the scale sweep, and the declaration, the binding, the argument errors
and the torch plumbing of mbfir.bloch_vjp_gr_batch / mbfir.torchsim.bloch, none of which needs a device."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochgradg_ref", os.path.join(ROOT, "tests", "blochgradg_ref.py"))
refg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refg)
ref = refg.base


@functools.lru_cache(maxsize=None)
def _batch(shared):
    return ref.batch(shared)


def _small(t2):
    """9 samples, 3 gradient axes, 3 x 5 points with df = 0 and position 0 among them, sample 3 zero in b1 and gr, per-sample tp"""
    rng = np.random.default_rng(7)
    n, gamma = 9, ref.GAMMA_H1
    dt = (t2 / 3 / n if t2 < 10e-3 else 4e-4) * (1.0 + 0.2 * (-1.0) ** np.arange(n))
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.5 / (gamma * dt.sum()))
    gr = rng.uniform(0.5, 1.5, (n, 3)) * 0.1 * (4e-4 / dt.mean())
    b1[3], gr[3] = 0.0, 0.0
    df = ref._grid(3, 200.0)
    dp = np.stack([ref._grid(5, 2.0) * (1.0 - 0.3 * a) for a in range(3)], 1)
    m0 = tuple(rng.uniform(-0.5, 0.5, (3, 3, 5)))
    w = rng.standard_normal((3, 3, 5))
    return (b1, gr, dt, 1.0, t2, "H-1"), df, dp, m0, w, gamma


@pytest.mark.parametrize("shared", [False, True])
def test_reference_b1_and_m0_part_is_blochgrad_ref(shared):
    pulses, dfs, dps, m0s, cots = _batch(shared)
    for q, (p, df, dp, m0, cot) in enumerate(zip(pulses, dfs, dps, m0s, cots)):
        if len(p[0]) > 260 and shared:
            continue                                                    # the long pulses once
        g, _, gm, _ = refg.vjp_gr_scaled(p, df, dp, cot, ref.SCALES, m0)
        wg, wm = ref.vjp_scaled(p, df, dp, cot, ref.SCALES, m0)
        assert np.array_equal(g, wg) and all(np.array_equal(a, b) for a, b in zip(gm, wm)), q


@pytest.mark.parametrize("t2", [40e-3, 1e-3])
def test_reference_gr_and_df_are_the_central_differences_of_the_forward(t2):
    """Entry by entry: h = 1e-6 G/cm in gr against 1e-7 max(max|g|, 1), h = 1e-3 Hz in df against 1e-6 max|grad_df|.  The check
    case has a zero b1 and gr sample, so at df = 0 / position 0 the rotation angle of that sample is exactly 0."""
    pulse, df, dp, m0, w, gamma = _small(t2)
    b1, gr, dt, t1, _, _ = pulse

    def L(g, f):
        m = ref.forward(b1, g, dt, t1, t2, f, dp, gamma, 1.0, m0)
        return float(sum((w[c] * m[c]).sum() for c in range(3)))

    def Lp(g, f):
        """per point: df of one frequency row moves only that row's points"""
        m = ref.forward(b1, g, dt, t1, t2, f, dp, gamma, 1.0, m0)
        return sum(w[c] * m[c] for c in range(3))
    _, gg, _, gdf = refg.vjp_gr(b1, gr, dt, t1, t2, df, dp, gamma, 1.0, m0, tuple(w))
    fd = np.zeros_like(gg)
    for t in range(len(b1)):
        for a in range(3):
            e = np.zeros_like(gr)
            e[t, a] = 1e-6
            fd[t, a] = (L(gr + e, df) - L(gr - e, df)) / 2e-6
    fdf = (Lp(gr, df + 1e-3) - Lp(gr, df - 1e-3)) / 2e-3                # every point has its own df: shift them all at once
    eg, ed = float(np.abs(fd - gg).max()), float(np.abs(fdf - gdf).max())
    sg, sd = max(float(np.abs(gg).max()), 1.0), float(np.abs(gdf).max())
    print("T2 %.0e: gr |fd - ref| %.3g of max(max|g|, 1) = %.3g: %.3g; df |fd - ref| %.3g of max|grad_df| = %.3g: %.3g"
          % (t2, eg, sg, eg / sg, ed, sd, ed / sd))
    assert np.all(gg[3] != 0.0) and np.all(np.isfinite(gg)) and np.all(np.isfinite(gdf))        # phi = 0: the generator, not 0 or NaN
    assert eg <= 1e-7 * sg and ed <= 1e-6 * sd


@pytest.mark.parametrize("shared", [False, True])
def test_float64_reference_is_the_longdouble_one_to_a_hundredth_of_the_device_bounds(shared):
    pulses, dfs, dps, m0s, cots = _batch(shared)
    if not shared:
        extra = refg.batch_sub()
        pulses, dfs, dps, m0s, cots = [a + b for a, b in zip((pulses, dfs, dps, m0s, cots), extra)]
    for q, (p, df, dp, m0, cot) in enumerate(zip(pulses, dfs, dps, m0s, cots)):
        _, g64, _, d64 = refg.vjp_gr_scaled(p, df, dp, cot, ref.SCALES, m0)
        _, gld, _, dld = refg.vjp_gr_scaled(p, df, dp, cot, ref.SCALES, m0, dtype=np.longdouble)
        eg, bg = np.abs(g64 - gld).astype(np.float64), refg.bound_gr(p, dp, cot)
        ed, bd = np.abs(d64 - dld).astype(np.float64), refg.bound_df(p, cot)
        pos = bg > 0
        print("shared %s n %d points %s: gr |f64 - ld| / bound %.3g, df |f64 - ld| / bound %.3g"
              % (shared, len(p[0]), cot[0].shape[1:], (eg[pos] / bg[pos]).max() if pos.any() else 0.0, (ed / bd).max()))
        assert np.all(eg <= bg / 100) and np.all(ed <= bd / 100), q
        assert np.all(g64[~pos] == 0.0) and np.all(gld[~pos] == 0.0), q                # a zero bound: exactly zero


def test_scale_sweep_carries_s_in_b1_and_not_in_gr():
    """At b1 = 0 the forward does not depend on the scale: the gr and df gradients of every scale are then those of scale 1,
    while the b1 gradient of scale s is s times the one with respect to s b1; and a sweep is the sum of its scales."""
    pulse, df, dp, m0, w, gamma = _small(40e-3)
    b1, gr, dt, t1, t2, _ = pulse
    z = np.zeros_like(b1)
    g1, gg1, _, d1 = refg.vjp_gr(z, gr, dt, t1, t2, df, dp, gamma, 1.0, m0, tuple(w))
    g3, gg3, _, d3 = refg.vjp_gr(z, gr, dt, t1, t2, df, dp, gamma, 3.0, m0, tuple(w))
    assert np.array_equal(gg1, gg3) and np.array_equal(d1, d3) and np.abs(g1).max() > 0
    assert np.allclose(g3, 3.0 * g1, rtol=1e-14, atol=0)
    sc = (1.0, 0.0, 0.9)
    cot = tuple(np.stack([w[c]] * 3) for c in range(3))
    g, gg, gm, gd = refg.vjp_gr_scaled(pulse, df, dp, cot, sc, m0)
    parts = [refg.vjp_gr(b1, gr, dt, t1, t2, df, dp, gamma, s, m0, tuple(w)) for s in sc]
    assert np.array_equal(gg, parts[0][1] + parts[1][1] + parts[2][1]) and np.array_equal(g, parts[0][0] + parts[1][0] + parts[2][0])
    assert all(np.array_equal(gd[k], parts[k][3]) for k in range(3)) and np.array_equal(parts[1][0], np.zeros(len(b1)))
    assert np.abs(parts[1][1]).max() > 0                                # scale 0 still moves with gr: no factor s


def test_the_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_bloch_vjp_gr_batch\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_bloch_vjp_gr_batch"][1]) == len(mbfir.SYMBOLS["mbfir_bloch_vjp_batch"][1]) + 4 == 38
    assert getattr(mbfir.load_library(), "mbfir_bloch_vjp_gr_batch") is not None        # the library exports it
    assert callable(mbfir.bloch_vjp_gr_batch)


def test_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    c = np.zeros((1, 3, 5))
    with pytest.raises(ValueError, match="bloch_vjp_gr_batch: no pulses"):
        mbfir.bloch_vjp_gr_batch([], df, dp, [])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.bloch_vjp_gr_batch([p], df, dp, [(c, c, c)], scales=())
    with pytest.raises(ValueError, match="pulse 1 has no samples"):
        mbfir.bloch_vjp_gr_batch([p, (np.zeros(0),) + p[1:]], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="more than 3 gradient axes"):
        mbfir.bloch_vjp_gr_batch([(p[0], np.zeros((4, 4))) + p[2:]], df, dp, [(c, c, c)])
    with pytest.raises(ValueError, match="2 cotangent triples for 1 pulses"):
        mbfir.bloch_vjp_gr_batch([p], df, dp, [(c, c, c)] * 2)
    with pytest.raises(ValueError, match="triple"):
        mbfir.bloch_vjp_gr_batch([p], df, dp, [(c, c)])
    with pytest.raises(ValueError, match="shapes"):
        mbfir.bloch_vjp_gr_batch([p], df, dp, [(c, c, c[:, :, :4])], grad_df=True)
    with pytest.raises(ValueError, match="shapes"):
        mbfir.bloch_vjp_gr_batch([p], df, dp, [(c, c, c)], scales=(1.0, 0.9))
    with pytest.raises(ValueError, match="empty grid"):
        mbfir.bloch_vjp_gr_batch([p], np.zeros(0), dp, [(c, c, c)])
    # the C call refuses a null context before it reads anything else (the checks that need a context, each with its message:
    # tests/test_blochgradg_gpu.py)
    args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS["mbfir_bloch_vjp_gr_batch"][1][1:]]
    assert mbfir.load_library().mbfir_bloch_vjp_gr_batch(*args) == mbfir.E_ARG


def _stub_device_calls(monkeypatch, calls):
    """mbfir's three Bloch calls replaced by the NumPy references, so that torchsim's plumbing runs without a device; calls
    receives (name, grad_m0, grad_df) of every adjoint call"""
    def bloch_batch(pulses, df, dp, *, scales, m0):
        b1, gr, tp, t1, t2, nucleus = pulses[0]
        out = [ref.forward(b1, gr, tp, t1, t2, df, dp, ref.gamma_of(nucleus), s, m0) for s in scales]
        return [tuple(np.stack([o[c] for o in out]) for c in range(3))]

    def bloch_vjp_batch(pulses, df, dp, cot, *, scales, m0, grad_m0):
        calls.append(("b1", grad_m0, None))
        g, gm = ref.vjp_scaled(pulses[0], df, dp, cot[0], scales, m0)
        return [(g, gm) if grad_m0 else g]

    def bloch_vjp_gr_batch(pulses, df, dp, cot, *, scales, m0, grad_m0, grad_df):
        calls.append(("gr", grad_m0, grad_df))
        g, gg, gm, gd = refg.vjp_gr_scaled(pulses[0], df, dp, cot[0], scales, m0)
        return [(g, gg) + ((gm,) if grad_m0 else ()) + ((gd,) if grad_df else ())]
    monkeypatch.setattr(mbfir, "bloch_batch", bloch_batch)
    monkeypatch.setattr(mbfir, "bloch_vjp_batch", bloch_vjp_batch)
    monkeypatch.setattr(mbfir, "bloch_vjp_gr_batch", bloch_vjp_gr_batch, raising=False)


def _torch_case():
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    gr = torch.tensor(rng.uniform(0.5, 1.5, (6, 2)) * 0.05, dtype=torch.float64, requires_grad=True)
    df = torch.tensor([-100.0, 0.0], dtype=torch.float64, requires_grad=True)
    m0 = torch.tensor(rng.uniform(-0.5, 0.5, (3, 2, 3)), dtype=torch.float64, requires_grad=True)
    dp = np.array([[-1.0, 0.5], [0.0, 0.0], [1.5, -0.7]])
    return b1, gr, df, m0, dp, dt


def test_torchsim_bloch_passes_gradcheck_in_gr_and_df_on_stubbed_calls(monkeypatch):
    """gradcheck in gr (two axes, and one axis as a 1-D tensor), in df and in (b1, gr, df, m0) on 6 samples and 2 x 3 points with
    T2 of the order of the duration; gr's gradient has gr's shape, df's is summed over scales and positions."""
    import torch
    calls = []
    _stub_device_calls(monkeypatch, calls)
    b1, gr, df, m0, dp, dt = _torch_case()
    sc = (1.0, 0.8)

    def f(b, g, d, m):
        return mbfir.torchsim.bloch(b, g, dt, 1.0, 1e-3, d, dp, nucleus="H-1", scales=sc, m0=m)
    b0, g0, d0 = b1.detach(), gr.detach(), df.detach()
    assert torch.autograd.gradcheck(lambda g: f(b0, g, d0, None), (gr,))
    g1 = gr.detach()[:, 0].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda g: f(b0, g, d0, None), (g1,))
    assert torch.autograd.gradcheck(lambda d: f(b0, g0, d, None), (df,))
    assert torch.autograd.gradcheck(f, (b1, gr, df, m0))
    assert calls and all(c[0] == "gr" for c in calls)
    mx, my, mz = f(b1, gr, df, m0)
    (mx * my + mz).sum().backward()
    assert gr.grad.shape == gr.shape and df.grad.shape == df.shape and b1.grad is not None and m0.grad.shape == m0.shape


def test_torchsim_bloch_asks_only_for_what_is_needed(monkeypatch):
    calls = []
    _stub_device_calls(monkeypatch, calls)
    b1, gr, df, m0, dp, dt = _torch_case()

    def run(b, g, d, m):
        del calls[:]
        mx, my, mz = mbfir.torchsim.bloch(b, g, dt, 1.0, 1e-3, d, dp, nucleus="H-1", scales=(1.0, 0.8), m0=m)
        (mx * my + mz).sum().backward()
        return list(calls)
    g0, d0, m00 = gr.detach(), df.detach(), m0.detach()
    # only b1 and / or m0: today's call, never the new one; tensors that do not require grad are constants
    assert run(b1, g0.numpy(), d0.numpy(), None) == [("b1", False, None)]
    assert run(b1, g0, d0, m0) == [("b1", True, None)]
    assert run(b1.detach(), g0, d0, m0) == [("b1", True, None)]
    # gr and / or df: one call of the new function, grad_df and grad_m0 only when needed
    assert run(b1, gr, d0, m00) == [("gr", False, False)]
    assert run(b1, g0, df, m00) == [("gr", False, True)]
    assert run(b1.detach(), gr, df, m0) == [("gr", True, True)]
    assert run(b1, gr, d0, m0) == [("gr", True, False)]


def test_torchsim_bloch_refuses_other_dtypes_shapes_and_forward_tangents(monkeypatch):
    import torch
    _stub_device_calls(monkeypatch, [])
    b1, gr, df, m0, dp, dt = _torch_case()

    def f(b, g, d, **kw):
        return mbfir.torchsim.bloch(b, g, dt, 1.0, 1e-3, d, dp, nucleus="H-1", **kw)
    with pytest.raises(ValueError, match="gr that requires grad"):
        f(b1, gr.detach().float().requires_grad_(True), df)
    with pytest.raises(ValueError, match="gr that requires grad"):
        f(b1, torch.zeros(6, 4, dtype=torch.float64, requires_grad=True), df)
    with pytest.raises(ValueError, match="df that requires grad"):
        f(b1, gr, df.detach().float().requires_grad_(True))
    with pytest.raises(ValueError, match="df that requires grad"):
        f(b1, gr, df.detach().reshape(2, 1).requires_grad_(True))
    for fm in (False, True):
        with pytest.raises(NotImplementedError, match="forward-mode"):
            torch.func.jvp(lambda g: f(b1.detach(), g, df.detach(), forward_mode=fm), (gr.detach(),), (torch.ones_like(gr),))
        with pytest.raises(NotImplementedError, match="forward-mode"):
            torch.func.jvp(lambda d: f(b1.detach(), gr.detach(), d, forward_mode=fm), (df.detach(),), (torch.ones_like(df),))
