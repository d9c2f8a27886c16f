"""The adjoint of the batched simulators on the device (mbfir.abr_vjp_batch / abr2_vjp_batch: k_abr_vjp_batch, k_abr2_vjp_batch,
k_abr_vjp_fold; mbfir.torchsim) against the NumPy recursion of tests/simgrad_ref.py, against central differences of the shipped
forward calls, and for the bit-invariance of a pulse's gradient under the batch's composition.

Bound of every comparison with the reference: 1e-12 N max|s| per entry, N = the sum of |abar| + |bbar| over the pulse's points and
scales.  N max|s| bounds any gradient entry (the derivative of a rotation has norm <= 1), and 1e-12 is the forward tolerance of
tests/test_simbatch_gpu.py: the unitary recursion loses about n eps per sweep."""
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

_spec = importlib.util.spec_from_file_location("simgrad_ref", os.path.join(ROOT, "tests", "simgrad_ref.py"))
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


LENGTHS = [1, 255, 256, 257, 600]                 # below, at and above the 256-sample staging tile, and two full tiles and a part
FLIPS = [0.3, 0.02, 1.5, np.pi, 2.0]              # small tip .. about pi in total
NXS = [600, 257, 255, 1, 600]                     # one point, partial chunks, more than one chunk


@functools.lru_cache(maxsize=None)
def _case_1d(hard, shared):
    pulses = _pulses(7, LENGTHS, FLIPS, False)
    xs = [_grid(257, 6.0)] * 5 if shared else [_grid(nx, 4.0 + q) for q, nx in enumerate(NXS)]
    cots = [_cot(20 + q, (3, len(x))) for q, x in enumerate(xs)]
    want = [ref.vjp_scaled(*_split(p), x, c, SCALES, hard_pulse=hard) for p, x, c in zip(pulses, xs, cots)]
    return pulses, xs, cots, want


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hard", [False, True])
def test_1d_device_gradient_is_the_reference(hard, shared):
    pulses, xs, cots, want = _case_1d(hard, shared)
    got = mbfir.abr_vjp_batch(pulses, xs[0] if shared else xs, cots, scales=SCALES, hard_pulse=hard)
    for q, (g, w, c) in enumerate(zip(got, want, cots)):
        err, bound = float(np.abs(g - w).max()), _bound(c, SCALES)
        print("1D hard %s shared %s n %d nx %d: |dev - ref| %.3g, bound %.3g, max|g| %.3g"
              % (hard, shared, len(w), c[0].shape[1], err, bound, np.abs(w).max()))
        assert g.shape == w.shape and err <= bound, q


GRIDS2 = [(19, 23), (1, 300), (19, 23), (1, 300), (19, 23)]          # 437 and 300 points: two chunks, the last one partial


@functools.lru_cache(maxsize=None)
def _case_2d(hard, shared):
    pulses = _pulses(8, LENGTHS, FLIPS, True)
    grids = [GRIDS2[0]] * 5 if shared else GRIDS2
    xs = [_grid(nx, 3.0) for nx, _ in grids]
    ys = [_grid(ny, 25.0) for _, ny in grids]
    cots = [_cot(40 + q, (3,) + gr) for q, gr in enumerate(grids)]
    want = [ref.vjp_scaled(*_split(p), x, c, SCALES, y=y, hard_pulse=hard) for p, x, y, c in zip(pulses, xs, ys, cots)]
    return pulses, xs, ys, cots, want


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hard", [False, True])
def test_2d_device_gradient_is_the_reference(hard, shared):
    pulses, xs, ys, cots, want = _case_2d(hard, shared)
    got = mbfir.abr2_vjp_batch(pulses, xs[0] if shared else xs, ys[0] if shared else ys, cots, scales=SCALES, hard_pulse=hard)
    for q, (g, w, c) in enumerate(zip(got, want, cots)):
        err, bound = float(np.abs(g - w).max()), _bound(c, SCALES)
        print("2D hard %s shared %s n %d grid %s: |dev - ref| %.3g, bound %.3g, max|g| %.3g"
              % (hard, shared, len(w), c[0].shape[1:], err, bound, np.abs(w).max()))
        assert g.shape == w.shape and err <= bound, q


def test_zero_scale_gives_exact_zeros():
    pulses, xs, cots, _ = _case_1d(False, False)
    for g in mbfir.abr_vjp_batch(pulses, xs, [(c[0][:1], c[1][:1]) for c in cots], scales=(0.0,)):
        assert np.array_equal(g, np.zeros(len(g)))
    pulses, xs, ys, cots, _ = _case_2d(True, False)
    for g in mbfir.abr2_vjp_batch(pulses, xs, ys, [(c[0][:1], c[1][:1]) for c in cots], scales=(0.0,), hard_pulse=True):
        assert np.array_equal(g, np.zeros(len(g)))


def test_a_pulse_has_the_same_gradient_bits_alone_in_17_and_reversed():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 700, 17)]
    flips = list(np.linspace(0.1, 3.0, 17))
    sc = [0.9]
    for hard in (False, True):
        p1 = _pulses(53, lengths, flips, False)
        x1 = [_grid(5 + 40 * q, 6.0) for q in range(17)]
        c1 = [_cot(60 + q, (1, len(x))) for q, x in enumerate(x1)]
        full = mbfir.abr_vjp_batch(p1, x1, c1, scales=sc, hard_pulse=hard)
        again = mbfir.abr_vjp_batch(p1, x1, c1, scales=sc, hard_pulse=hard)
        rev = mbfir.abr_vjp_batch(p1[::-1], x1[::-1], c1[::-1], scales=sc, hard_pulse=hard)[::-1]
        p2 = _pulses(54, lengths, flips, True)
        x2 = [_grid(5 + 3 * q, 3.0) for q in range(17)]
        y2 = [_grid(3 + 5 * (q % 7), 25.0) for q in range(17)]
        c2 = [_cot(80 + q, (1, len(x), len(y))) for q, (x, y) in enumerate(zip(x2, y2))]
        full2 = mbfir.abr2_vjp_batch(p2, x2, y2, c2, scales=sc, hard_pulse=hard)
        again2 = mbfir.abr2_vjp_batch(p2, x2, y2, c2, scales=sc, hard_pulse=hard)
        rev2 = mbfir.abr2_vjp_batch(p2[::-1], x2[::-1], y2[::-1], c2[::-1], scales=sc, hard_pulse=hard)[::-1]
        for q in range(17):
            assert np.array_equal(full[q], rev[q]) and np.array_equal(full[q], again[q]), (hard, q)
            assert np.array_equal(full2[q], rev2[q]) and np.array_equal(full2[q], again2[q]), (hard, q)
        for q in (0, 5, 16):
            alone, = mbfir.abr_vjp_batch([p1[q]], [x1[q]], [c1[q]], scales=sc, hard_pulse=hard)
            assert np.array_equal(alone, full[q]), (hard, q)
            alone, = mbfir.abr2_vjp_batch([p2[q]], [x2[q]], [y2[q]], [c2[q]], scales=sc, hard_pulse=hard)
            assert np.array_equal(alone, full2[q]), (hard, q)


@pytest.mark.parametrize("hard", [False, True])
def test_2d_at_y0_with_a_real_g_is_the_1d_call(hard):
    pulses, xs, cots, _ = _case_1d(hard, False)
    p2 = [(rf, None if g is None else g + 0j) for rf, g in map(_split, pulses)]
    p2 = [rf if g is None else (rf, g) for rf, g in p2]
    g1 = mbfir.abr_vjp_batch(pulses, xs, cots, scales=SCALES, hard_pulse=hard)
    g2 = mbfir.abr2_vjp_batch(p2, xs, [0.0], [(ca[:, :, None], cb[:, :, None]) for ca, cb in cots], scales=SCALES, hard_pulse=hard)
    for a, b, c in zip(g1, g2, cots):
        assert np.abs(a - b).max() <= _bound(c, SCALES)


@pytest.mark.parametrize("hard", [False, True])
def test_convention_abr_maps_the_cotangent_of_b(hard):
    """Under 'abr' the forward call returns bo = -conj(b): L(a, bo) has dL/dRe b = -dL/dRe bo and dL/dIm b = dL/dIm bo."""
    pulses, xs, cots, _ = _case_1d(hard, False)
    got = mbfir.abr_vjp_batch(pulses[:3], xs[:3], cots[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    for p, x, (ca, cb), g in zip(pulses, xs, cots, got):
        want = ref.vjp_scaled(*_split(p), x, (ca, -np.conj(cb)), SCALES, hard_pulse=hard)
        assert np.abs(g - want).max() <= _bound((ca, cb), SCALES)
    pulses, xs, ys, cots, _ = _case_2d(hard, False)
    got = mbfir.abr2_vjp_batch(pulses[:3], xs[:3], ys[:3], cots[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    for p, x, y, (ca, cb), g in zip(pulses, xs, ys, cots, got):
        want = ref.vjp_scaled(*_split(p), x, (ca, -np.conj(cb)), SCALES, y=y, hard_pulse=hard)
        assert np.abs(g - want).max() <= _bound((ca, cb), SCALES)


def _disc_loss(a, b, target, w):
    """L = sum w |2 conj(a) b - target|^2 and its cotangents (dL/dRe a + i dL/dIm a, the same for b)"""
    m = 2 * np.conj(a) * b
    r = w * (m - target)
    return float((w * np.abs(m - target) ** 2).sum()), (4 * b * np.conj(r), 4 * a * r)


def _directional_check(forward, vjp, rf):
    """(L(rf + e d) - L(rf - e d)) / 2e along d = gbar / |gbar| is |gbar|: returns the relative difference"""
    L0, cot = forward(rf)
    g = vjp(rf, cot)
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, 1e-5 * float(np.linalg.norm(rf))
    fd = (forward(rf + eps * d)[0] - forward(rf - eps * d)[0]) / (2 * eps)
    print("loss %.6g, |gbar| %.9g, central difference %.9g, relative difference %.3g" % (L0, nrm, fd, abs(fd - nrm) / nrm))
    return abs(fd - nrm) / nrm


def test_the_vjp_is_the_gradient_of_the_shipped_forward():
    """dz2d spiral at 90 degrees on 24 x 24 points with the disc loss at scales 0.9, 1.0, 1.1, and a 64-sample pulse on 257 points
    in 1D: the directional derivative from mbfir.abr2_batch / abr_batch equals |gbar| to 1e-6 relative (truncation eps^2 |L'''| and
    rounding eps_machine L / eps are both far below it)."""
    sc = (0.9, 1.0, 1.1)
    rf0, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    rf0 = rf0 * np.pi / 2
    x = np.linspace(-8, 8, 24)
    r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
    target = np.where(r <= 1.0, -1j, 0.0)[None].repeat(3, 0)        # abrm's b of a rotation about x is -i sin: 2 conj(a) b = -i
    w = np.where((r <= 1.0) | (r >= 3.5), 1.0, 0.0)[None].repeat(3, 0)

    def fwd2(rf):
        (a, b), = mbfir.abr2_batch([(rf, g)], x, x, scales=sc)
        return _disc_loss(a, b, target, w)

    def vjp2(rf, cot):
        return mbfir.abr2_vjp_batch([(rf, g)], x, x, [cot], scales=sc)[0]
    assert _directional_check(fwd2, vjp2, rf0) <= 1e-6
    rf1 = _pulses(90, [64], [np.pi / 2], False)[0]
    x1 = _grid(257, 8.0)
    t1 = np.where(np.abs(x1) <= 2.0, -1j, 0.0)[None].repeat(3, 0)
    w1 = np.ones((3, 257))

    def fwd1(rf):
        (a, b), = mbfir.abr_batch([rf], x1, scales=sc)
        return _disc_loss(a, b, t1, w1)

    def vjp1(rf, cot):
        return mbfir.abr_vjp_batch([rf], x1, [cot], scales=sc)[0]
    assert _directional_check(fwd1, vjp1, rf1) <= 1e-6


@pytest.mark.parametrize("hard", [False, True])
def test_torch_functions_pass_gradcheck_and_carry_the_device_bits(hard):
    import torch
    rng = np.random.default_rng(5)
    rf0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * 0.3
    g1 = rng.uniform(0.5, 1.5, 6)
    g2 = g1 + 1j * rng.uniform(-1, 1, 6)
    x, x2, y2 = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3), np.linspace(-2, 2, 4)
    sc = (1.0, 0.8)
    rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
    assert torch.autograd.gradcheck(lambda r: mbfir.torchsim.abr(r, x, g1, scales=sc, hard_pulse=hard), (rf,))
    assert torch.autograd.gradcheck(lambda r: mbfir.torchsim.abr2(r, g2, x2, y2, scales=sc, hard_pulse=hard), (rf,))
    # the forward and the gradient are the NumPy calls' bits
    a, b = mbfir.torchsim.abr(rf, torch.tensor(x), None, scales=sc, hard_pulse=hard)
    (an, bn), = mbfir.abr_batch([rf0], x, scales=sc, hard_pulse=hard)
    assert a.dtype == torch.complex128 and tuple(a.shape) == (2, 5)
    assert np.array_equal(a.detach().numpy(), an) and np.array_equal(b.detach().numpy(), bn)
    ca, cb = _cot(6, (2, 5))                                       # L = Re(conj(ca) a + conj(cb) b): the cotangents are ca, cb exactly
    ((torch.tensor(ca).conj() * a).real.sum() + (torch.tensor(cb).conj() * b).real.sum()).backward()
    want, = mbfir.abr_vjp_batch([rf0], x, [(ca, cb)], scales=sc, hard_pulse=hard)
    assert np.array_equal(rf.grad.numpy(), want)
    rf.grad = None
    a, b = mbfir.torchsim.abr2(rf, torch.tensor(g2), x2, y2, scales=sc, hard_pulse=hard)
    (an, bn), = mbfir.abr2_batch([(rf0, g2)], x2, y2, scales=sc, hard_pulse=hard)
    assert np.array_equal(a.detach().numpy(), an) and np.array_equal(b.detach().numpy(), bn)
    ca, cb = _cot(7, (2, 3, 4))
    ((torch.tensor(ca).conj() * a).real.sum() + (torch.tensor(cb).conj() * b).real.sum()).backward()
    want, = mbfir.abr2_vjp_batch([(rf0, g2)], x2, y2, [(ca, cb)], scales=sc, hard_pulse=hard)
    assert np.array_equal(rf.grad.numpy(), want)
    # a loss through conj(): autograd then hands the backward lazily conjugated cotangents
    rf.grad = None
    a, b = mbfir.torchsim.abr2(rf, torch.tensor(g2), x2, y2, scales=sc, hard_pulse=hard)
    ((2 * a.conj() * b - 0.5j).abs() ** 2).sum().backward()
    r = 2 * np.conj(an) * bn - 0.5j
    cot = (4 * bn * np.conj(r), 4 * an * r)
    want, = mbfir.abr2_vjp_batch([(rf0, g2)], x2, y2, [cot], scales=sc, hard_pulse=hard)
    assert np.abs(rf.grad.numpy() - want).max() <= _bound(cot, sc)


def test_errors_and_the_raw_calls_leave_the_context_usable():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    c1, c2 = np.ones((1, 5), dtype=complex), np.ones((1, 5, 3), dtype=complex)
    with pytest.raises(ValueError, match="shapes"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1[:, :4])])
    with pytest.raises(ValueError, match="no samples"):
        mbfir.abr2_vjp_batch([np.zeros(0)], x, y, [(c2, c2)])
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr_vjp_batch([np.ones(4)], x, [(c1, c1)], scales=())
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr2_vjp_batch([np.ones(4)], x, y, [(c2, c2)], convention="abx")
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, o = np.ones(64), [np.zeros(64) for _ in range(2)]

    def call1(roff=L(0, 3), xoff=L(0, 2), nscale=1, mode=0, npulse=1, nxgrid=1, cot=d, out=o):
        return lib.mbfir_abr_vjp_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, nxgrid, lp(xoff), p(d), nscale, p(d), mode,
                                       p(cot) if cot is not None else None, p(d), p(d), p(d),
                                       *[p(v) if v is not None else None for v in out])

    def call2(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 3), nscale=1, mode=0, npulse=1, nxgrid=1, nygrid=1, cot=d, out=o):
        return lib.mbfir_abr2_vjp_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid, lp(yoff),
                                        p(d), nscale, p(d), mode, p(cot) if cot is not None else None, p(d), p(d), p(d),
                                        *[p(v) if v is not None else None for v in out])

    big = 2 ** 31 - 1
    common = ((dict(roff=L(0, 0)), "no samples"), (dict(npulse=2, roff=L(0, 3, 1)), "inconsistent offsets"),
              (dict(xoff=L(0, 0)), "empty item"), (dict(nscale=0), "scale list is empty"), (dict(mode=2), "mode"),
              (dict(npulse=0), "no pulses"), (dict(nxgrid=2), "1 or npulse"), (dict(cot=None), "null"),
              (dict(out=[o[0], None]), "null"))
    for call, who, extra in ((call1, "abr_vjp_batch:", ()),
                             (call2, "abr2_vjp_batch:", ((dict(yoff=L(0, 0)), "empty item"), (dict(nygrid=3), "1 or npulse"),
                                                         (dict(xoff=L(0, big), yoff=L(0, big), nscale=4), "overflows")))):
        assert call() == 0
        for kw, why in common + extra:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call() == 0
    rf, xx = np.full(8, 0.1 + 0.05j), np.array([0.0, 1.0])
    ca, cb = _cot(3, (1, 2))
    g, = mbfir.abr_vjp_batch([rf], xx, [(ca, cb)])
    assert np.abs(g - ref.vjp(rf, None, xx, ca[0], cb[0])).max() <= _bound((ca, cb), [1.0])
    g, = mbfir.abr2_vjp_batch([rf], xx, [0.0], [(ca[:, :, None], cb[:, :, None])])
    assert np.abs(g - ref.vjp(rf, None, xx, ca[0], cb[0])).max() <= _bound((ca, cb), [1.0])
