"""The adjoint of the batched simulators with respect to rf and the gradient waveform on the device (mbfir.abr_vjp_rfg_batch /
abr2_vjp_rfg_batch: k_abr_vjp_rfg_batch, k_abr2_vjp_rfg_batch, k_abr_vjp_rfg_fold; mbfir.torchsim) against the NumPy recursion of
tests/simgradg_ref.py, against the rf adjoint, against central differences of the shipped forward calls, and for the bit-invariance
of a pulse's gradients under the batch's composition.  Pulses, grids and cotangents are those of tests/test_simgrad_gpu.py,
restated.

Bounds.  rf part: 1e-12 N max|s| per entry, N = the sum of |abar| + |bbar| over the pulse's points and scales, as in
tests/test_simgrad_gpu.py.  g part: 1e-12 times the sum over scales and points of |x_i| (|abar| + |bbar|) (|y_j| for the y
component): dQ / d om has norm at most 1, so a point's contribution to dL/dg is at most |x_i| (|abar| + |bbar|), and 1e-12 is the
forward tolerance carried through the coordinate weight."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
SCALES = [1.0, 0.0, 0.9]

_spec = importlib.util.spec_from_file_location("simgradg_ref", os.path.join(ROOT, "tests", "simgradg_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def _pulses(seed, lengths, flips, two_d):
    """rf alone and (rf, g) in turn (g complex in 2D); total flip about flips[q]; for n >= 3 one rf sample is exactly zero"""
    rng = np.random.default_rng(seed)
    out = []
    for q, (n, flip) in enumerate(zip(lengths, flips)):
        rf = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (flip / n)
        if n >= 3:
            rf[n // 3] = 0.0
        g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n
        if two_d:
            g = g + 1j * rng.uniform(-1.5, 1.5, n) * 1e-2
        out.append((rf, g) if q % 2 else rf)
    return out


def _split(p):
    return p if isinstance(p, tuple) else (p, None)


def _grid(nx, span):
    """nx points over +-span with x = 0 among them"""
    x = np.linspace(-span, span, nx)
    x[nx // 2] = 0.0
    return x


def _cot(seed, shape):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(2))


def _bound(cot, scales):
    return TOL * float(np.abs(cot[0]).sum() + np.abs(cot[1]).sum()) * max(abs(s) for s in scales)


def _gbound(cot, x, y=None):
    """(bound of dL/dg) in 1D, (bound of dL/dgx, bound of dL/dgy) in 2D; cot: (S, nx[, ny])"""
    w = np.abs(cot[0]) + np.abs(cot[1])
    if y is None:
        return TOL * float((w * np.abs(x)[None, :]).sum())
    return TOL * float((w * np.abs(x)[None, :, None]).sum()), TOL * float((w * np.abs(y)[None, None, :]).sum())


def _gerr(got, want, two_d):
    if not two_d:
        return float(np.abs(got - want).max())
    return float(np.abs(got.real - want.real).max()), float(np.abs(got.imag - want.imag).max())


LENGTHS = [1, 255, 256, 257, 600]                 # below, at and above the 256-sample staging tile, and two full tiles and a part;
FLIPS = [0.3, 0.02, 1.5, np.pi, 2.0]              # 1, 255 and 257 are no multiple of the 4-sample reduction tile
NXS = [600, 257, 255, 1, 600]                     # one point, partial chunks, more than one chunk


@functools.lru_cache(maxsize=None)
def _case_1d(hard, shared):
    pulses = _pulses(7, LENGTHS, FLIPS, False)
    xs = [_grid(257, 6.0)] * 5 if shared else [_grid(nx, 4.0 + q) for q, nx in enumerate(NXS)]
    cots = [_cot(20 + q, (3, len(x))) for q, x in enumerate(xs)]
    want = [ref.vjp_rfg_scaled(*_split(p), x, c, SCALES, hard_pulse=hard) for p, x, c in zip(pulses, xs, cots)]
    return pulses, xs, cots, want


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hard", [False, True])
def test_1d_device_gradients_are_the_reference(hard, shared):
    pulses, xs, cots, want = _case_1d(hard, shared)
    got = mbfir.abr_vjp_rfg_batch(pulses, xs[0] if shared else xs, cots, scales=SCALES, hard_pulse=hard)
    rf_only = mbfir.abr_vjp_batch(pulses, xs[0] if shared else xs, cots, scales=SCALES, hard_pulse=hard)
    for q, ((g, gg), (w, wg), c, x, g0) in enumerate(zip(got, want, cots, xs, rf_only)):
        err, bound, gerr, gbound = float(np.abs(g - w).max()), _bound(c, SCALES), _gerr(gg, wg, False), _gbound(c, x)
        err0 = float(np.abs(g - g0).max())
        print("1D hard %s shared %s n %d nx %d: rf |dev - ref| %.3g |dev - abr_vjp_batch| %.3g bound %.3g; g |dev - ref| %.3g "
              "bound %.3g max|gg| %.3g" % (hard, shared, len(w), len(x), err, err0, bound, gerr, gbound, np.abs(wg).max()))
        assert g.shape == w.shape and g.dtype == np.complex128 and err <= bound and err0 <= bound, q
        assert gg.shape == wg.shape and gg.dtype == np.float64 and gerr <= gbound, q


GRIDS2 = [(19, 23), (1, 300), (19, 23), (1, 300), (19, 23)]          # 437 and 300 points: two chunks, the last one partial


@functools.lru_cache(maxsize=None)
def _case_2d(hard, shared):
    pulses = _pulses(8, LENGTHS, FLIPS, True)
    grids = [GRIDS2[0]] * 5 if shared else GRIDS2
    xs = [_grid(nx, 3.0) for nx, _ in grids]
    ys = [_grid(ny, 25.0) for _, ny in grids]
    cots = [_cot(40 + q, (3,) + gr) for q, gr in enumerate(grids)]
    want = [ref.vjp_rfg_scaled(*_split(p), x, c, SCALES, y=y, hard_pulse=hard) for p, x, y, c in zip(pulses, xs, ys, cots)]
    return pulses, xs, ys, cots, want


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hard", [False, True])
def test_2d_device_gradients_are_the_reference(hard, shared):
    pulses, xs, ys, cots, want = _case_2d(hard, shared)
    args = (pulses, xs[0] if shared else xs, ys[0] if shared else ys, cots)
    got = mbfir.abr2_vjp_rfg_batch(*args, scales=SCALES, hard_pulse=hard)
    rf_only = mbfir.abr2_vjp_batch(*args, scales=SCALES, hard_pulse=hard)
    for q, ((g, gg), (w, wg), c, x, y, g0) in enumerate(zip(got, want, cots, xs, ys, rf_only)):
        err, bound, gerr, gbound = float(np.abs(g - w).max()), _bound(c, SCALES), _gerr(gg, wg, True), _gbound(c, x, y)
        err0 = float(np.abs(g - g0).max())
        print("2D hard %s shared %s n %d grid %s: rf |dev - ref| %.3g |dev - abr2_vjp_batch| %.3g bound %.3g; gx |dev - ref| %.3g "
              "bound %.3g; gy |dev - ref| %.3g bound %.3g; max|gg| %.3g"
              % (hard, shared, len(w), c[0].shape[1:], err, err0, bound, gerr[0], gbound[0], gerr[1], gbound[1], np.abs(wg).max()))
        assert g.shape == w.shape and err <= bound and err0 <= bound, q
        assert gg.shape == wg.shape and gg.dtype == np.complex128 and gerr[0] <= gbound[0] and gerr[1] <= gbound[1], q


def test_zero_scale_alone():
    """Scale 0: rf's gradient is exact zeros (the fold multiplies by s = 0).  Hard pulse: b and S are exact zeros, so w and dom
    are; mode 0: a = exp(-i om_total / 2) and b = 0, so dL/dg_m = sum_i x_i Re(conj(ca_i) (-i/2) a_i) for every sample m."""
    pulses, xs, cots, _ = _case_1d(False, False)
    c1 = [(c[0][:1], c[1][:1]) for c in cots]
    for hard in (False, True):
        got = mbfir.abr_vjp_rfg_batch(pulses, xs, c1, scales=(0.0,), hard_pulse=hard)
        for (g, gg), p, x, c in zip(got, pulses, xs, c1):
            assert np.array_equal(g, np.zeros(len(g)))
            if hard:
                assert np.array_equal(gg, np.zeros(len(gg)))
                continue
            gw = _split(p)[1]
            tot = 2 * np.pi if gw is None else gw.sum()
            want = float((x * (np.conj(c[0][0]) * (-0.5j) * np.exp(-0.5j * x * tot)).real).sum())
            err, bound = float(np.abs(gg - want).max()), _gbound(c, x)
            print("scale 0, n %d nx %d: |dev - closed form| %.3g, bound %.3g" % (len(g), len(x), err, bound))
            assert err <= bound
    pulses, xs, ys, cots, _ = _case_2d(True, False)
    c2 = [(c[0][:1], c[1][:1]) for c in cots]
    for hard in (False, True):
        got = mbfir.abr2_vjp_rfg_batch(pulses, xs, ys, c2, scales=(0.0,), hard_pulse=hard)
        for (g, gg), p, x, y, c in zip(got, pulses, xs, ys, c2):
            assert np.array_equal(g, np.zeros(len(g)))
            if hard:
                assert np.array_equal(gg, np.zeros(len(gg)))
                continue
            gw = _split(p)[1]
            tot = 2 * np.pi + 0j if gw is None else gw.sum()
            X, Y = np.meshgrid(x, y, indexing="ij")
            d = (np.conj(c[0][0]) * (-0.5j) * np.exp(-0.5j * (X * tot.real + Y * tot.imag))).real
            want = float((X * d).sum()) + 1j * float((Y * d).sum())
            err, bound = _gerr(gg, np.full(len(gg), want), True), _gbound(c, x, y)
            print("scale 0, n %d grid %s: |dev - closed form| %.3g %.3g, bounds %.3g %.3g" % ((len(g), X.shape) + err + bound))
            assert err[0] <= bound[0] and err[1] <= bound[1]


def test_a_pulse_has_the_same_gradient_bits_alone_in_17_and_reversed():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 700, 17)]
    flips = list(np.linspace(0.1, 3.0, 17))
    sc = [0.9]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for hard in (False, True):
        p1 = _pulses(53, lengths, flips, False)
        x1 = [_grid(5 + 40 * q, 6.0) for q in range(17)]
        c1 = [_cot(60 + q, (1, len(x))) for q, x in enumerate(x1)]
        full = mbfir.abr_vjp_rfg_batch(p1, x1, c1, scales=sc, hard_pulse=hard)
        again = mbfir.abr_vjp_rfg_batch(p1, x1, c1, scales=sc, hard_pulse=hard)
        rev = mbfir.abr_vjp_rfg_batch(p1[::-1], x1[::-1], c1[::-1], scales=sc, hard_pulse=hard)[::-1]
        p2 = _pulses(54, lengths, flips, True)
        x2 = [_grid(5 + 3 * q, 3.0) for q in range(17)]
        y2 = [_grid(3 + 5 * (q % 7), 25.0) for q in range(17)]
        c2 = [_cot(80 + q, (1, len(x), len(y))) for q, (x, y) in enumerate(zip(x2, y2))]
        full2 = mbfir.abr2_vjp_rfg_batch(p2, x2, y2, c2, scales=sc, hard_pulse=hard)
        again2 = mbfir.abr2_vjp_rfg_batch(p2, x2, y2, c2, scales=sc, hard_pulse=hard)
        rev2 = mbfir.abr2_vjp_rfg_batch(p2[::-1], x2[::-1], y2[::-1], c2[::-1], scales=sc, hard_pulse=hard)[::-1]
        for q in range(17):
            assert same(full[q], rev[q]) and same(full[q], again[q]), (hard, q)
            assert same(full2[q], rev2[q]) and same(full2[q], again2[q]), (hard, q)
        for q in (0, 5, 16):
            alone, = mbfir.abr_vjp_rfg_batch([p1[q]], [x1[q]], [c1[q]], scales=sc, hard_pulse=hard)
            assert same(alone, full[q]), (hard, q)
            alone, = mbfir.abr2_vjp_rfg_batch([p2[q]], [x2[q]], [y2[q]], [c2[q]], scales=sc, hard_pulse=hard)
            assert same(alone, full2[q]), (hard, q)


@pytest.mark.parametrize("hard", [False, True])
def test_2d_at_y0_with_a_real_g_is_the_1d_call(hard):
    pulses, xs, cots, _ = _case_1d(hard, False)
    p2 = [(rf, None if g is None else g + 0j) for rf, g in map(_split, pulses)]
    p2 = [rf if g is None else (rf, g) for rf, g in p2]
    g1 = mbfir.abr_vjp_rfg_batch(pulses, xs, cots, scales=SCALES, hard_pulse=hard)
    g2 = mbfir.abr2_vjp_rfg_batch(p2, xs, [0.0], [(ca[:, :, None], cb[:, :, None]) for ca, cb in cots], scales=SCALES,
                                  hard_pulse=hard)
    for (a, ga), (b, gb), c, x in zip(g1, g2, cots, xs):
        assert np.abs(a - b).max() <= _bound(c, SCALES)
        assert np.abs(ga - gb.real).max() <= _gbound(c, x)
        assert np.array_equal(gb.imag, np.zeros(len(gb)))


@pytest.mark.parametrize("hard", [False, True])
def test_convention_abr_maps_the_cotangent_of_b(hard):
    """Under 'abr' the forward call returns bo = -conj(b): L(a, bo) has dL/dRe b = -dL/dRe bo and dL/dIm b = dL/dIm bo."""
    pulses, xs, cots, _ = _case_1d(hard, False)
    got = mbfir.abr_vjp_rfg_batch(pulses[:3], xs[:3], cots[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    for p, x, (ca, cb), (g, gg) in zip(pulses, xs, cots, got):
        want, wg = ref.vjp_rfg_scaled(*_split(p), x, (ca, -np.conj(cb)), SCALES, hard_pulse=hard)
        assert np.abs(g - want).max() <= _bound((ca, cb), SCALES)
        assert np.abs(gg - wg).max() <= _gbound((ca, cb), x)
    pulses, xs, ys, cots, _ = _case_2d(hard, False)
    got = mbfir.abr2_vjp_rfg_batch(pulses[:3], xs[:3], ys[:3], cots[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    for p, x, y, (ca, cb), (g, gg) in zip(pulses, xs, ys, cots, got):
        want, wg = ref.vjp_rfg_scaled(*_split(p), x, (ca, -np.conj(cb)), SCALES, y=y, hard_pulse=hard)
        assert np.abs(g - want).max() <= _bound((ca, cb), SCALES)
        err, bound = _gerr(gg, wg, True), _gbound((ca, cb), x, y)
        assert err[0] <= bound[0] and err[1] <= bound[1]


def _disc_loss(a, b, target, w):
    """L = sum w |2 conj(a) b - target|^2 and its cotangents (dL/dRe a + i dL/dIm a, the same for b)"""
    m = 2 * np.conj(a) * b
    r = w * (m - target)
    return float((w * np.abs(m - target) ** 2).sum()), (4 * b * np.conj(r), 4 * a * r)


def _directional_check(forward, vjp_g, g, d):
    """(L(g + h d) - L(g - h d)) / 2h at h = 1e-6 against Re <grad_g, d> (d a unit direction): returns the relative difference"""
    L0, cot = forward(g)
    gg = vjp_g(g, cot)
    ip = float((np.conj(gg) * d).real.sum())
    h = 1e-6
    fd = (forward(g + h * d)[0] - forward(g - h * d)[0]) / (2 * h)
    print("loss %.6g, <grad_g, d> %.9g, central difference %.9g, relative difference %.3g" % (L0, ip, fd, abs(fd - ip) / abs(ip)))
    return abs(fd - ip) / abs(ip)


def test_the_g_gradient_is_the_gradient_of_the_shipped_forward():
    """dz2d spiral at 90 degrees on 24 x 24 points with the disc loss at scales 0.9, 1.0, 1.1, and a 64-sample pulse on 257 points
    in 1D: the directional derivative of the mbfir.abr2_batch / abr_batch loss along a random unit direction of g equals the inner
    product with grad_g to 1e-6 relative."""
    sc = (0.9, 1.0, 1.1)
    rf0, g0, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    rf0 = rf0 * np.pi / 2
    x = np.linspace(-8, 8, 24)
    r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
    target = np.where(r <= 1.0, -1j, 0.0)[None].repeat(3, 0)
    w = np.where((r <= 1.0) | (r >= 3.5), 1.0, 0.0)[None].repeat(3, 0)
    rng = np.random.default_rng(91)

    def fwd2(g):
        (a, b), = mbfir.abr2_batch([(rf0, g)], x, x, scales=sc)
        return _disc_loss(a, b, target, w)

    def vjp2(g, cot):
        return mbfir.abr2_vjp_rfg_batch([(rf0, g)], x, x, [cot], scales=sc)[0][1]
    d = rng.standard_normal(len(rf0)) + 1j * rng.standard_normal(len(rf0))
    assert _directional_check(fwd2, vjp2, np.asarray(g0, dtype=np.complex128), d / np.linalg.norm(d)) <= 1e-6
    rf1, g1 = _pulses(90, [64, 64], [np.pi / 2] * 2, False)[1]
    x1 = _grid(257, 8.0)
    t1 = np.where(np.abs(x1) <= 2.0, -1j, 0.0)[None].repeat(3, 0)
    w1 = np.ones((3, 257))

    def fwd1(g):
        (a, b), = mbfir.abr_batch([(rf1, g)], x1, scales=sc)
        return _disc_loss(a, b, t1, w1)

    def vjp1(g, cot):
        return mbfir.abr_vjp_rfg_batch([(rf1, g)], x1, [cot], scales=sc)[0][1]
    d = rng.standard_normal(64)
    assert _directional_check(fwd1, vjp1, g1, d / np.linalg.norm(d)) <= 1e-6


@pytest.mark.parametrize("hard", [False, True])
def test_torch_functions_pass_gradcheck_in_g_and_keep_the_rf_bits(hard):
    import torch
    rng = np.random.default_rng(5)
    rf0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * 0.3
    g1 = rng.uniform(0.5, 1.5, 6)
    g2 = g1 + 1j * rng.uniform(-1, 1, 6)
    x, x2, y2 = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3), np.linspace(-2, 2, 4)
    sc = (1.0, 0.8)
    rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
    rfc = torch.tensor(rf0, dtype=torch.complex128)
    tg1 = torch.tensor(g1, dtype=torch.float64, requires_grad=True)
    tg2 = torch.tensor(g2, dtype=torch.complex128, requires_grad=True)
    assert torch.autograd.gradcheck(lambda g: mbfir.torchsim.abr(rfc, x, g, scales=sc, hard_pulse=hard), (tg1,))
    assert torch.autograd.gradcheck(lambda r, g: mbfir.torchsim.abr2(r, g, x2, y2, scales=sc, hard_pulse=hard), (rf, tg2))
    # both gradients are the NumPy call's bits
    ca, cb = _cot(7, (2, 3, 4))
    a, b = mbfir.torchsim.abr2(rf, tg2, x2, y2, scales=sc, hard_pulse=hard)
    ((torch.tensor(ca).conj() * a).real.sum() + (torch.tensor(cb).conj() * b).real.sum()).backward()
    (want, wg), = mbfir.abr2_vjp_rfg_batch([(rf0, g2)], x2, y2, [(ca, cb)], scales=sc, hard_pulse=hard)
    assert np.array_equal(rf.grad.numpy(), want) and np.array_equal(tg2.grad.numpy(), wg)
    # g a tensor that does not require grad: the rf call, with its bits
    rf.grad = None
    a, b = mbfir.torchsim.abr2(rf, torch.tensor(g2), x2, y2, scales=sc, hard_pulse=hard)
    ((torch.tensor(ca).conj() * a).real.sum() + (torch.tensor(cb).conj() * b).real.sum()).backward()
    want, = mbfir.abr2_vjp_batch([(rf0, g2)], x2, y2, [(ca, cb)], scales=sc, hard_pulse=hard)
    assert np.array_equal(rf.grad.numpy(), want)
    rf.grad = None
    ca, cb = _cot(6, (2, 5))
    a, b = mbfir.torchsim.abr(rf, x, torch.tensor(g1), scales=sc, hard_pulse=hard)
    ((torch.tensor(ca).conj() * a).real.sum() + (torch.tensor(cb).conj() * b).real.sum()).backward()
    want, = mbfir.abr_vjp_batch([(rf0, g1)], x, [(ca, cb)], scales=sc, hard_pulse=hard)
    assert np.array_equal(rf.grad.numpy(), want)


def test_errors_through_the_abi_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d = np.ones(64)

    def call1(roff=L(0, 3), xoff=L(0, 2), nscale=1, mode=0, npulse=1, nxgrid=1, cot=d, out=None):
        out = [np.zeros(64) for _ in range(3)] if out is None else out
        return lib.mbfir_abr_vjp_rfg_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, nxgrid, lp(xoff), p(d), nscale, p(d), mode,
                                           p(cot) if cot is not None else None, p(d), p(d), p(d),
                                           *[p(v) if v is not None else None for v in out])

    def call2(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 3), nscale=1, mode=0, npulse=1, nxgrid=1, nygrid=1, cot=d, out=None):
        out = [np.zeros(64) for _ in range(4)] if out is None else out
        return lib.mbfir_abr2_vjp_rfg_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid,
                                            lp(yoff), p(d), nscale, p(d), mode, p(cot) if cot is not None else None, p(d), p(d),
                                            p(d), *[p(v) if v is not None else None for v in out])

    big, z = 2 ** 31 - 1, np.zeros(64)
    common = ((dict(roff=L(0, 0)), "no samples"), (dict(npulse=2, roff=L(0, 3, 1)), "inconsistent offsets"),
              (dict(xoff=L(0, 0)), "empty item"), (dict(nscale=0), "scale list is empty"), (dict(mode=2), "mode"),
              (dict(npulse=0), "no pulses"), (dict(nxgrid=2), "1 or npulse"), (dict(cot=None), "null"))
    for call, who, extra in ((call1, "abr_vjp_rfg_batch:", ((dict(out=[z, z, None]), "null"), (dict(out=[z, None, z]), "null"))),
                             (call2, "abr2_vjp_rfg_batch:", ((dict(yoff=L(0, 0)), "empty item"), (dict(nygrid=3), "1 or npulse"),
                                                             (dict(out=[z, z, z, None]), "null"),
                                                             (dict(out=[z, z, None, z]), "null"),
                                                             (dict(xoff=L(0, big), yoff=L(0, big), nscale=4), "overflows")))):
        assert call() == 0
        for kw, why in common + extra:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call() == 0
    rf, xx = np.full(8, 0.1 + 0.05j), np.array([0.0, 1.0])
    ca, cb = _cot(3, (1, 2))
    wr, wg = ref.vjp_rfg(rf, None, xx, ca[0], cb[0])
    (g, gg), = mbfir.abr_vjp_rfg_batch([rf], xx, [(ca, cb)])
    assert np.abs(g - wr).max() <= _bound((ca, cb), [1.0]) and np.abs(gg - wg).max() <= _gbound((ca, cb), xx)
    (g, gg), = mbfir.abr2_vjp_rfg_batch([rf], xx, [0.0], [(ca[:, :, None], cb[:, :, None])])
    assert np.abs(g - wr).max() <= _bound((ca, cb), [1.0]) and np.abs(gg.real - wg).max() <= _gbound((ca, cb), xx)
