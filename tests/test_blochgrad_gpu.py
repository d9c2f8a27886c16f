"""The adjoint of the Bloch simulator with relaxation on the device (mbfir.bloch_vjp_batch: k_bloch_vjp_batch, k_bloch_vjp_fold;
mbfir.torchsim.bloch) against the stored-trajectory NumPy recursion of tests/blochgrad_ref.py, against central differences of the
shipped forward call mbfir.bloch_batch, and for the bit-invariance of a pulse's gradient under the batch's composition.

Bound of every comparison with the reference (blochgrad_ref.bound_b1, bound_m0): 1e-12 N max|s| gamma dt_t per b1 entry, N = the sum
of |cmx| + |cmy| + |cmz| over the pulse's points and scales, and 1e-12 max(|cmx| + |cmy| + |cmz|) per dL/dm0 entry.  A rotation's
derivative and the decay have norm at most 1, and 1e-12 is the forward tolerance of the existing Bloch tests.
tests/test_blochgrad_cpu.py holds the float64 reference within a hundredth of these bounds of its long-double twin."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochgrad_ref", os.path.join(ROOT, "tests", "blochgrad_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
SCALES = ref.SCALES


@functools.lru_cache(maxsize=None)
def _case(shared):
    pulses, dfs, dps, m0s, cots = ref.batch(shared)
    want = [ref.vjp_scaled(p, df, dp, c, SCALES, m0) for p, df, dp, c, m0 in zip(pulses, dfs, dps, cots, m0s)]
    return pulses, dfs, dps, m0s, cots, want


@pytest.mark.parametrize("shared", [False, True])
def test_device_gradient_is_the_reference(shared):
    """Eight pulses of 1 .. 600 samples around the group of 8 and the 256-sample tile, on 1 .. 600 points, scales 1.0, 0.0, 0.9,
    random m0, phi = 0 at a zero sample at df = 0 and position 0, and a 26 ms pulse at T2 = 1 ms (blochgrad_ref.batch)."""
    pulses, dfs, dps, m0s, cots, want = _case(shared)
    got = mbfir.bloch_vjp_batch(pulses, dfs[0] if shared else dfs, dps[0] if shared else dps, cots, scales=SCALES, m0=m0s,
                                grad_m0=True)
    for q, ((g, gm), (wg, wm), p, c) in enumerate(zip(got, want, pulses, cots)):
        eb, bb = np.abs(g - wg), ref.bound_b1(p, c, SCALES)
        em, bm = max(float(np.abs(a - b).max()) for a, b in zip(gm, wm)), ref.bound_m0(c)
        print("shared %s n %d points %s: b1 |dev - ref| %.3g, bound %.3g, max |dev - ref| / bound %.3g, max|g| %.3g; m0 |dev - ref| "
              "%.3g, bound %.3g" % (shared, len(wg), c[0].shape[1:], eb.max(), bb.min(), (eb / bb).max(), np.abs(wg).max(), em, bm))
        assert g.shape == wg.shape and all(a.shape == b.shape for a, b in zip(gm, wm)), q
        assert np.all(eb <= bb) and em <= bm, q
    only_b1 = mbfir.bloch_vjp_batch(pulses, dfs[0] if shared else dfs, dps[0] if shared else dps, cots, scales=SCALES, m0=m0s)
    for (g, _), h in zip(got, only_b1):
        assert np.array_equal(g, h)


def test_zero_scale_gives_exact_zeros():
    pulses, dfs, dps, m0s, cots, _ = _case(False)
    res = mbfir.bloch_vjp_batch(pulses, dfs, dps, [tuple(c[:1] for c in tri) for tri in cots], scales=(0.0,), m0=m0s)
    for g in res:
        assert np.array_equal(g, np.zeros(len(g)))


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, m0s, cots = [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(ref._grid(npos, 3.0))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        cots.append(tuple(rng.standard_normal((3, 2, nf, npos))))
    full = mbfir.bloch_vjp_batch(pulses, dfs, dps, cots, scales=sc, m0=m0s, grad_m0=True)
    again = mbfir.bloch_vjp_batch(pulses, dfs, dps, cots, scales=sc, m0=m0s, grad_m0=True)
    rev = mbfir.bloch_vjp_batch(pulses[::-1], dfs[::-1], dps[::-1], cots[::-1], scales=sc, m0=m0s[::-1], grad_m0=True)[::-1]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))
    for q in range(17):
        assert same(full[q], again[q]) and same(full[q], rev[q]), q
    for q in (0, 5, 16):
        alone, = mbfir.bloch_vjp_batch([pulses[q]], [dfs[q]], [dps[q]], [cots[q]], scales=sc, m0=[m0s[q]], grad_m0=True)
        assert same(alone, full[q]), q


def _problem(seed, n, t2):
    """An n-sample H-1 pulse of about 90 degrees in 4 ms on 3 x 85 points, weights for sum w . m over three scales"""
    rng = np.random.default_rng(seed)
    dur = 4e-3
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (np.pi / 2 / (ref.GAMMA_H1 * dur))
    pulse = (b1, rng.uniform(0.5, 1.5, n) * 0.05, dur / n, 1.0, t2, "H-1")
    return pulse, ref._grid(3, 100.0), ref._grid(85, 3.0), rng.standard_normal((3, 3, 3, 85))


def test_the_vjp_is_the_gradient_of_the_shipped_forward():
    """L = sum (w . m)^2 / 2 on mbfir.bloch_batch at scales 0.9, 1.0, 1.1, a 64-sample pulse on 3 x 85 points with T2 = the
    duration: the directional derivative along g / |g| equals |g| to 1e-6 relative (truncation eps^2 |L'''| and rounding
    eps_machine L / eps are both far below it)."""
    sc = (0.9, 1.0, 1.1)
    pulse, df, dp, w = _problem(90, 64, 4e-3)
    m0 = tuple(np.random.default_rng(91).uniform(-0.5, 0.5, (3, 3, 85)))

    def fwd(b1):
        m, = mbfir.bloch_batch([(b1,) + pulse[1:]], df, dp, scales=sc, m0=m0)
        r = w[0] * m[0] + w[1] * m[1] + w[2] * m[2]
        return 0.5 * float((r * r).sum()), tuple(w[c] * r for c in range(3))
    L0, cot = fwd(pulse[0])
    g, = mbfir.bloch_vjp_batch([pulse], df, dp, [cot], scales=sc, m0=m0)
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, 1e-5 * float(np.linalg.norm(pulse[0]))
    fd = (fwd(pulse[0] + eps * d)[0] - fwd(pulse[0] - eps * d)[0]) / (2 * eps)
    print("loss %.6g, |g| %.9g, central difference %.9g, relative difference %.3g" % (L0, nrm, fd, abs(fd - nrm) / nrm))
    assert abs(fd - nrm) <= 1e-6 * nrm


def test_gm0_chains_two_pulses():
    """Pulse 1, then pulse 2 from pulse 1's end state, the loss on the end: pulse 2's dL/dm0 fed as pulse 1's cotangent gives the
    gradient of pulse 1, which matches the central difference of the two chained bloch_batch calls to 1e-6 relative."""
    p1, df, dp, w = _problem(92, 48, 6e-3)
    p2 = _problem(93, 40, 5e-3)[0]

    def fwd(b1):
        m1, = mbfir.bloch_batch([(b1,) + p1[1:]], df, dp)
        m1 = tuple(v[0] for v in m1)
        m2, = mbfir.bloch_batch([p2], df, dp, m0=m1)
        r = w[0][:1] * m2[0] + w[1][:1] * m2[1] + w[2][:1] * m2[2]
        return 0.5 * float((r * r).sum()), m1, tuple(w[c][:1] * r for c in range(3))
    L0, m1, cot = fwd(p1[0])
    (_, gm), = mbfir.bloch_vjp_batch([p2], df, dp, [cot], m0=m1, grad_m0=True)
    g, = mbfir.bloch_vjp_batch([p1], df, dp, [gm])
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, 1e-5 * float(np.linalg.norm(p1[0]))
    fd = (fwd(p1[0] + eps * d)[0] - fwd(p1[0] - eps * d)[0]) / (2 * eps)
    print("chained loss %.6g, |g| %.9g, central difference %.9g, relative difference %.3g" % (L0, nrm, fd, abs(fd - nrm) / nrm))
    assert abs(fd - nrm) <= 1e-6 * nrm


def test_torchsim_bloch_passes_gradcheck_and_carries_the_device_bits():
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    gr = rng.uniform(0.5, 1.5, 6) * 0.05
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    sc = (1.0, 0.8)
    m00 = rng.uniform(-0.5, 0.5, (3, 2, 3))
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(m00, dtype=torch.float64, requires_grad=True)

    def f(b, m):
        return mbfir.torchsim.bloch(b, gr, dt, 1.0, 1e-3, df, dp, nucleus="H-1", scales=sc, m0=m)
    assert torch.autograd.gradcheck(f, (b1, m0))
    # the forward and the gradients are the NumPy calls' bits
    pulse = (b0, gr, dt, 1.0, 1e-3, "H-1")
    out = f(b1, m0)
    want, = mbfir.bloch_batch([pulse], df, dp, scales=sc, m0=tuple(m00))
    assert out[0].dtype == torch.float64 and tuple(out[0].shape) == (2, 2, 3)
    assert all(np.array_equal(o.detach().numpy(), v) for o, v in zip(out, want))
    cot = tuple(rng.standard_normal((3, 2, 2, 3)))                    # L = sum c . m: the cotangents are c exactly
    sum((torch.tensor(c) * o).sum() for c, o in zip(cot, out)).backward()
    (wg, wm), = mbfir.bloch_vjp_batch([pulse], df, dp, [cot], scales=sc, m0=tuple(m00), grad_m0=True)
    assert np.array_equal(b1.grad.numpy(), wg)
    assert np.array_equal(m0.grad.numpy(), np.stack([v.sum(0) for v in wm]))


def test_errors_of_the_raw_call_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(5)]

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
             m0=(None, None, None), cot=(one, one, one), grad=outs[:2], gm0=outs[2:]):
        o = [p(v) if v is not None else None for v in (*m0, *cot, *grad, *gm0)]
        return lib.mbfir_bloch_vjp_batch(ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None,
                                         lp(tsoff), p(d), p(t1), p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d),
                                         None, None, nscale, p(one), *o)
    big = 2 ** 31 - 1
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
             (dict(npulse=2, toff=L(0, 3, 1), tsoff=L(0, 1, 2)), "inconsistent offsets"), (dict(tsoff=L(0, 2)), "neither 1 nor"),
             (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"), (dict(poff=L(0, 0)), "empty item"),
             (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"), (dict(b1=None), "required array is null"),
             (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"),
             (dict(cot=(one, None, one)), "cotangent or gradient plane is null"),
             (dict(grad=[outs[0], None]), "cotangent or gradient plane is null"),
             (dict(m0=(one, one, None)), "m0x, m0y and m0z"), (dict(gm0=[None, outs[3], outs[4]]), "gm0x, gm0y and gm0z"))
    assert call() == 0
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_vjp_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0 and call(gm0=[None] * 3) == 0 and call(m0=(one, one, one)) == 0
