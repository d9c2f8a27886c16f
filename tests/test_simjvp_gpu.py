"""The tangent of the batched simulators on the device (mbfir.abr_jvp_batch / abr2_jvp_batch: k_abr_jvp_batch, k_abr2_jvp_batch;
the jvp of mbfir.torchsim) against the NumPy recursion of tests/simjvp_ref.py, against the shipped forward calls (primal bits,
central differences) and adjoints (dot-product identity), and for the bit-invariance of a tangent under the batch's composition.

Bound of every comparison with the reference: 1e-12 max|s| sum_m |v_m| per entry.  max|s| sum|v| bounds any tangent entry (the
derivative of a rotation has norm <= 1), and 1e-12 is the forward tolerance of tests/test_simbatch_gpu.py: it is the bound of
tests/test_simgrad_gpu.py with the roles of cotangent and direction swapped."""
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

_spec = importlib.util.spec_from_file_location("simjvp_ref", os.path.join(ROOT, "tests", "simjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


@functools.lru_cache(maxsize=None)
def _ks():
    """direction counts: one, a full group, a full group and a partly filled one"""
    k = mbfir.jvp_group()
    return sorted({1, k, k + 1})


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


def _dirs(seed, k, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n))


def _bound(v, scales):
    return TOL * max(abs(s) for s in scales) * float(np.abs(v).sum())


def _ref_all(p, x, vs, y, hard):
    """the reference's (da, db) for every direction of vs: (K, S, ...) each"""
    res = [ref.jvp_scaled(*_split(p), x, v, SCALES, y=y, hard_pulse=hard)[1] for v in vs]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


LENGTHS = [1, 255, 256, 257, 600]                 # below, at and above the 256-sample staging tile, and two full tiles and a part
FLIPS = [0.3, 0.02, 1.5, np.pi, 2.0]              # small tip .. about pi in total
NXS = [600, 257, 255, 1, 600]                     # one point, partial chunks, more than one chunk


@functools.lru_cache(maxsize=None)
def _case_1d(hard, shared):
    pulses = _pulses(7, LENGTHS, FLIPS, False)
    xs = [_grid(257, 6.0)] * 5 if shared else [_grid(nx, 4.0 + q) for q, nx in enumerate(NXS)]
    dirs = [_dirs(20 + q, _ks()[-1], n) for q, n in enumerate(LENGTHS)]
    want = [_ref_all(p, x, vs, None, hard) for p, x, vs in zip(pulses, xs, dirs)]
    return pulses, xs, dirs, want


def _compare(tag, got, primal, dirs, want, k):
    worst = 0.0
    for q, (((a, b), (da, db)), (a0, b0), vs, (wa, wb)) in enumerate(zip(got, primal, dirs, want)):
        assert np.array_equal(a, a0) and np.array_equal(b, b0), (tag, k, q)              # the forward call's bits
        assert da.shape == wa[:k].shape and db.shape == wb[:k].shape, (tag, k, q)
        assert np.array_equal(da[:, 1], np.zeros_like(da[:, 1])) and np.array_equal(db[:, 1], np.zeros_like(db[:, 1]))   # scale 0
        for j in range(k):
            err = max(float(np.abs(da[j] - wa[j]).max()), float(np.abs(db[j] - wb[j]).max()))
            bound = _bound(vs[j], SCALES)
            worst = max(worst, err / bound)
            print("%s K %d n %d points %s direction %d: |dev - ref| %.3g, bound %.3g, max|d| %.3g"
                  % (tag, k, vs.shape[1], da.shape[2:], j, err, bound, max(np.abs(wa[j]).max(), np.abs(wb[j]).max())))
            assert err <= bound, (tag, k, q, j)
    print("%s K %d: worst |dev - ref| / bound %.3g" % (tag, k, worst))


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hard", [False, True])
def test_1d_device_tangent_is_the_reference_and_the_primal_has_the_forward_bits(hard, shared):
    pulses, xs, dirs, want = _case_1d(hard, shared)
    xa = xs[0] if shared else xs
    primal = mbfir.abr_batch(pulses, xa, scales=SCALES, hard_pulse=hard)
    for k in _ks():
        got = mbfir.abr_jvp_batch(pulses, xa, [v[:k] for v in dirs], scales=SCALES, hard_pulse=hard)
        _compare("1D hard %s shared %s" % (hard, shared), got, primal, dirs, want, k)


GRIDS2 = [(19, 23), (1, 300), (19, 23), (1, 300), (19, 23)]          # 437 and 300 points: two chunks, the last one partial


@functools.lru_cache(maxsize=None)
def _case_2d(hard, shared):
    pulses = _pulses(8, LENGTHS, FLIPS, True)
    grids = [GRIDS2[0]] * 5 if shared else GRIDS2
    xs = [_grid(nx, 3.0) for nx, _ in grids]
    ys = [_grid(ny, 25.0) for _, ny in grids]
    dirs = [_dirs(40 + q, _ks()[-1], n) for q, n in enumerate(LENGTHS)]
    want = [_ref_all(p, x, vs, y, hard) for p, x, y, vs in zip(pulses, xs, ys, dirs)]
    return pulses, xs, ys, dirs, want


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hard", [False, True])
def test_2d_device_tangent_is_the_reference_and_the_primal_has_the_forward_bits(hard, shared):
    pulses, xs, ys, dirs, want = _case_2d(hard, shared)
    xa, ya = (xs[0], ys[0]) if shared else (xs, ys)
    primal = mbfir.abr2_batch(pulses, xa, ya, scales=SCALES, hard_pulse=hard)
    for k in _ks():
        got = mbfir.abr2_jvp_batch(pulses, xa, ya, [v[:k] for v in dirs], scales=SCALES, hard_pulse=hard)
        _compare("2D hard %s shared %s" % (hard, shared), got, primal, dirs, want, k)


def test_a_1d_tangent_drops_the_direction_axis_and_a_zero_direction_gives_exact_zeros():
    pulses, xs, dirs, _ = _case_1d(False, False)
    full = mbfir.abr_jvp_batch(pulses, xs, [v[:1] for v in dirs], scales=SCALES)
    flat = mbfir.abr_jvp_batch(pulses, xs, [v[0] for v in dirs], scales=SCALES)
    for (_, (da, db)), (_, (fa, fb)) in zip(full, flat):
        assert fa.shape == da.shape[1:] and np.array_equal(fa, da[0]) and np.array_equal(fb, db[0])
    for hard in (False, True):
        zero = [np.stack([v[0], np.zeros_like(v[0]), v[1]]) for v in dirs]           # the zero direction between two others
        for _, (da, db) in mbfir.abr_jvp_batch(pulses, xs, zero, scales=SCALES, hard_pulse=hard):
            assert np.array_equal(da[1], np.zeros_like(da[1])) and np.array_equal(db[1], np.zeros_like(db[1]))
            assert np.abs(da[0][0]).max() > 0
        p2, x2, y2, d2, _ = _case_2d(hard, False)
        for _, (da, db) in mbfir.abr2_jvp_batch(p2, x2, y2, [np.zeros_like(v[:2]) for v in d2], scales=SCALES, hard_pulse=hard):
            assert np.array_equal(da, np.zeros_like(da)) and np.array_equal(db, np.zeros_like(db))


def test_a_tangent_has_the_same_bits_alone_in_17_reversed_repeated_and_at_every_place_of_its_group():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 700, 17)]
    flips = list(np.linspace(0.1, 3.0, 17))
    sc = [0.9, 1.1]
    kk = mbfir.jvp_group() + 1

    def same(r, s):
        return all(np.array_equal(u, w) for u, w in zip(r[0] + r[1], s[0] + s[1]))
    for hard in (False, True):
        p1 = _pulses(53, lengths, flips, False)
        x1 = [_grid(5 + 40 * q, 6.0) for q in range(17)]
        v1 = [_dirs(60 + q, kk, n) for q, n in enumerate(lengths)]
        full = mbfir.abr_jvp_batch(p1, x1, v1, scales=sc, hard_pulse=hard)
        again = mbfir.abr_jvp_batch(p1, x1, v1, scales=sc, hard_pulse=hard)
        rev = mbfir.abr_jvp_batch(p1[::-1], x1[::-1], v1[::-1], scales=sc, hard_pulse=hard)[::-1]
        p2 = _pulses(54, lengths, flips, True)
        x2 = [_grid(5 + 3 * q, 3.0) for q in range(17)]
        y2 = [_grid(3 + 5 * (q % 7), 25.0) for q in range(17)]
        v2 = [_dirs(80 + q, kk, n) for q, n in enumerate(lengths)]
        full2 = mbfir.abr2_jvp_batch(p2, x2, y2, v2, scales=sc, hard_pulse=hard)
        again2 = mbfir.abr2_jvp_batch(p2, x2, y2, v2, scales=sc, hard_pulse=hard)
        rev2 = mbfir.abr2_jvp_batch(p2[::-1], x2[::-1], y2[::-1], v2[::-1], scales=sc, hard_pulse=hard)[::-1]
        for q in range(17):
            assert same(full[q], rev[q]) and same(full[q], again[q]), (hard, q)
            assert same(full2[q], rev2[q]) and same(full2[q], again2[q]), (hard, q)
        for q in (0, 5, 16):
            alone, twice = mbfir.abr_jvp_batch([p1[q]] * 2, [x1[q]] * 2, [v1[q]] * 2, scales=sc, hard_pulse=hard)
            assert same(alone, full[q]) and same(twice, full[q]), (hard, q)
            alone, = mbfir.abr_jvp_batch([p1[q]], [x1[q]], [v1[q]], scales=sc, hard_pulse=hard)
            assert same(alone, full[q]), (hard, q)
            alone, twice = mbfir.abr2_jvp_batch([p2[q]] * 2, [x2[q]] * 2, [y2[q]] * 2, [v2[q]] * 2, scales=sc, hard_pulse=hard)
            assert same(alone, full2[q]) and same(twice, full2[q]), (hard, q)
            # direction 0 alone (K = 1), and at every place j of a group of JVP_K + 1 (the last place is the partly filled group)
            for j in range(kk):
                perm = np.roll(np.arange(kk), j)                     # place j holds direction 0
                (_, (da, db)), = mbfir.abr_jvp_batch([p1[q]], [x1[q]], [v1[q][perm]], scales=sc, hard_pulse=hard)
                assert np.array_equal(da[j], full[q][1][0][0]) and np.array_equal(db[j], full[q][1][1][0]), (hard, q, j)
                (_, (da, db)), = mbfir.abr2_jvp_batch([p2[q]], [x2[q]], [y2[q]], [v2[q][perm]], scales=sc, hard_pulse=hard)
                assert np.array_equal(da[j], full2[q][1][0][0]) and np.array_equal(db[j], full2[q][1][1][0]), (hard, q, j)
            (_, (da, db)), = mbfir.abr_jvp_batch([p1[q]], [x1[q]], [v1[q][0]], scales=sc, hard_pulse=hard)
            assert np.array_equal(da, full[q][1][0][0]) and np.array_equal(db, full[q][1][1][0]), (hard, q)


@pytest.mark.parametrize("hard", [False, True])
def test_2d_at_y0_with_a_real_g_is_the_1d_call(hard):
    """the two form om differently (fma(x, gx, 0 gy) against x g), so the comparison is within the bound, not of bits"""
    pulses, xs, dirs, _ = _case_1d(hard, False)
    p2 = [rf if g is None else (rf, g + 0j) for rf, g in map(_split, pulses)]
    t1 = mbfir.abr_jvp_batch(pulses, xs, dirs, scales=SCALES, hard_pulse=hard)
    t2 = mbfir.abr2_jvp_batch(p2, xs, [0.0], dirs, scales=SCALES, hard_pulse=hard)
    for (_, (da, db)), (_, (ea, eb)), vs in zip(t1, t2, dirs):
        assert ea.shape == da.shape + (1,)
        for j in range(len(vs)):
            assert max(np.abs(da[j] - ea[j, :, :, 0]).max(), np.abs(db[j] - eb[j, :, :, 0]).max()) <= _bound(vs[j], SCALES)


def _spiral():
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    return rf * np.pi / 2, g


def test_dot_product_identity_with_the_shipped_adjoints():
    """Re sum(conj(ca) da + conj(cb) db) = Re sum(conj(gbar) v), gbar from abr2_vjp_batch / abr_vjp_batch with the same scales (both
    calls carry the factor s of r = s rf): relative to the larger side at most 1e-11."""
    sc = (0.9, 1.0, 1.1)
    rng = np.random.default_rng(31)

    def cplx(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    rf, g = _spiral()
    x = np.linspace(-8, 8, 17)
    for hard in (False, True):
        v, ca, cb = cplx(len(rf)), cplx((3, 17, 17)), cplx((3, 17, 17))
        (_, (da, db)), = mbfir.abr2_jvp_batch([(rf, g)], x, x, [v], scales=sc, hard_pulse=hard)
        gbar, = mbfir.abr2_vjp_batch([(rf, g)], x, x, [(ca, cb)], scales=sc, hard_pulse=hard)
        lhs, rhs = float((np.conj(ca) * da + np.conj(cb) * db).real.sum()), float((np.conj(gbar) * v).real.sum())
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print("spiral 17 x 17 hard %s: <c, J v> %.15g, <J^H c, v> %.15g, relative difference %.3g" % (hard, lhs, rhs, rel))
        assert rel <= 1e-11
        rf1 = _pulses(90, [257], [np.pi / 2], False)[0]
        x1 = _grid(257, 8.0)
        v, ca, cb = cplx(257), cplx((3, 257)), cplx((3, 257))
        (_, (da, db)), = mbfir.abr_jvp_batch([rf1], x1, [v], scales=sc, hard_pulse=hard)
        gbar, = mbfir.abr_vjp_batch([rf1], x1, [(ca, cb)], scales=sc, hard_pulse=hard)
        lhs, rhs = float((np.conj(ca) * da + np.conj(cb) * db).real.sum()), float((np.conj(gbar) * v).real.sum())
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print("1D n 257 nx 257 hard %s: <c, J v> %.15g, <J^H c, v> %.15g, relative difference %.3g" % (hard, lhs, rhs, rel))
        assert rel <= 1e-11


def test_the_jvp_is_the_directional_derivative_of_the_shipped_forward():
    """central differences (h = 1e-6 along a direction of unit-size entries) of mbfir.abr2_batch on the spiral at 24 x 24 points
    and of mbfir.abr_batch on a 64-sample pulse at 257 points, scales 0.9, 1.0, 1.1: the largest difference is at most 1e-6 of the
    largest tangent entry (truncation h^2 |third derivative| / 6 and rounding eps / h are both far below it)."""
    sc = (0.9, 1.0, 1.1)
    h = 1e-6
    rf, g = _spiral()
    x = np.linspace(-8, 8, 24)
    v = _dirs(5, 1, len(rf))[0]
    (_, (da, db)), = mbfir.abr2_jvp_batch([(rf, g)], x, x, [v], scales=sc)
    (ap, bp), (am, bm) = mbfir.abr2_batch([(rf + h * v, g), (rf - h * v, g)], x, x, scales=sc)
    rel = max(np.abs(da - (ap - am) / (2 * h)).max(), np.abs(db - (bp - bm) / (2 * h)).max()) / max(np.abs(da).max(), np.abs(db).max())
    print("spiral 24 x 24: tangent against central differences, relative %.3g (max|d| %.3g)" % (rel, max(np.abs(da).max(), np.abs(db).max())))
    assert rel <= 1e-6
    for hard in (False, True):
        rf1 = _pulses(90, [64], [np.pi / 2], False)[0]
        x1 = _grid(257, 8.0)
        v = _dirs(6, 1, 64)[0]
        (_, (da, db)), = mbfir.abr_jvp_batch([rf1], x1, [v], scales=sc, hard_pulse=hard)
        (ap, bp), (am, bm) = mbfir.abr_batch([rf1 + h * v, rf1 - h * v], x1, scales=sc, hard_pulse=hard)
        rel = max(np.abs(da - (ap - am) / (2 * h)).max(), np.abs(db - (bp - bm) / (2 * h)).max()) / max(np.abs(da).max(), np.abs(db).max())
        print("1D n 64 nx 257 hard %s: tangent against central differences, relative %.3g" % (hard, rel))
        assert rel <= 1e-6


@pytest.mark.parametrize("hard", [False, True])
def test_convention_abr_maps_b_and_its_tangent(hard):
    """Under 'abr' the forward call returns -conj(b), and the tangent of that is -conj(db)."""
    pulses, xs, dirs, _ = _case_1d(hard, False)
    m = mbfir.abr_jvp_batch(pulses[:3], xs[:3], dirs[:3], scales=SCALES, hard_pulse=hard)
    r = mbfir.abr_jvp_batch(pulses[:3], xs[:3], dirs[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    f = mbfir.abr_batch(pulses[:3], xs[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    for ((a, b), (da, db)), ((ar, br), (dar, dbr)), (af, bf) in zip(m, r, f):
        assert np.array_equal(ar, a) and np.array_equal(br, -np.conj(b)) and np.array_equal(br, bf) and np.array_equal(ar, af)
        assert np.array_equal(dar, da) and np.array_equal(dbr, -np.conj(db))
    pulses, xs, ys, dirs, _ = _case_2d(hard, False)
    m = mbfir.abr2_jvp_batch(pulses[:3], xs[:3], ys[:3], dirs[:3], scales=SCALES, hard_pulse=hard)
    r = mbfir.abr2_jvp_batch(pulses[:3], xs[:3], ys[:3], dirs[:3], scales=SCALES, hard_pulse=hard, convention="abr")
    for ((a, b), (da, db)), ((ar, br), (dar, dbr)) in zip(m, r):
        assert np.array_equal(ar, a) and np.array_equal(br, -np.conj(b))
        assert np.array_equal(dar, da) and np.array_equal(dbr, -np.conj(db))


@pytest.mark.parametrize("hard", [False, True])
def test_torch_functions_pass_forward_mode_gradcheck_and_func_jvp_carries_the_device_bits(hard):
    import torch
    rng = np.random.default_rng(5)
    rf0 = (rng.standard_normal(9) + 1j * rng.standard_normal(9)) * 0.3
    g1 = rng.uniform(0.5, 1.5, 9)
    g2 = g1 + 1j * rng.uniform(-1, 1, 9)
    x, x2, y2 = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3), np.linspace(-2, 2, 3)
    sc = (1.0, 0.8)
    rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
    assert torch.autograd.gradcheck(lambda r: mbfir.torchsim.abr(r, x, g1, scales=sc, hard_pulse=hard), (rf,), check_forward_ad=True)
    assert torch.autograd.gradcheck(lambda r: mbfir.torchsim.abr2(r, g2, x2, y2, scales=sc, hard_pulse=hard), (rf,),
                                    check_forward_ad=True)
    v0 = rng.standard_normal(9) + 1j * rng.standard_normal(9)
    (a, b), (da, db) = torch.func.jvp(lambda r: mbfir.torchsim.abr(r, x, g1, scales=sc, hard_pulse=hard), (rf.detach(),),
                                      (torch.tensor(v0),))
    ((an, bn), (dan, dbn)), = mbfir.abr_jvp_batch([(rf0, g1)], x, [v0], scales=sc, hard_pulse=hard)
    assert da.dtype == torch.complex128 and tuple(da.shape) == (2, 5)
    assert np.array_equal(a.numpy(), an) and np.array_equal(b.numpy(), bn)
    assert np.array_equal(da.numpy(), dan) and np.array_equal(db.numpy(), dbn)
    import torch.autograd.forward_ad as fwad                                        # dual tensors, the 2D function
    with fwad.dual_level():
        a, b = mbfir.torchsim.abr2(fwad.make_dual(rf.detach(), torch.tensor(v0)), g2, x2, y2, scales=sc, hard_pulse=hard)
        da, db = fwad.unpack_dual(a).tangent, fwad.unpack_dual(b).tangent
    (_, (dan, dbn)), = mbfir.abr2_jvp_batch([(rf0, g2)], x2, y2, [v0], scales=sc, hard_pulse=hard)
    assert np.array_equal(da.numpy(), dan) and np.array_equal(db.numpy(), dbn)


def test_errors_and_the_raw_calls_leave_the_context_usable():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 3)
    with pytest.raises(ValueError, match="shape"):
        mbfir.abr_jvp_batch([np.ones(4)], x, [np.ones(3, dtype=complex)])
    with pytest.raises(ValueError, match="no samples"):
        mbfir.abr2_jvp_batch([np.zeros(0)], x, y, [np.zeros(0, dtype=complex)])
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    def pp(vs):
        return [p(v) if v is not None else None for v in vs]

    d, o = np.ones(64), [np.zeros(64) for _ in range(4)]
    none4 = [None] * 4

    def call1(roff=L(0, 3), xoff=L(0, 2), nscale=1, mode=0, npulse=1, nxgrid=1, ndir=2, v=(d, d), prim=o, tan=o):
        return lib.mbfir_abr_jvp_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, nxgrid, lp(xoff), p(d), nscale, p(d), mode, ndir,
                                       *pp(v), *pp(prim), *pp(tan))

    def call2(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 3), nscale=1, mode=0, npulse=1, nxgrid=1, nygrid=1, ndir=2, v=(d, d), prim=o,
              tan=o):
        return lib.mbfir_abr2_jvp_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid, lp(yoff),
                                        p(d), nscale, p(d), mode, ndir, *pp(v), *pp(prim), *pp(tan))

    big = 2 ** 31 - 1
    common = ((dict(roff=L(0, 0)), "no samples"), (dict(npulse=2, roff=L(0, 3, 1)), "inconsistent offsets"),
              (dict(xoff=L(0, 0)), "empty item"), (dict(nscale=0), "scale list is empty"), (dict(mode=2), "mode"),
              (dict(npulse=0), "no pulses"), (dict(nxgrid=2), "1 or npulse"), (dict(v=(d, None)), "null"),
              (dict(tan=[o[0], o[1], None, o[3]]), "null"), (dict(prim=[o[0], None, o[2], o[3]]), "null"),
              (dict(ndir=0), "ndir"), (dict(ndir=-1), "ndir"), (dict(ndir=0, nscale=0), "scale list is empty"),
              (dict(xoff=L(0, big), ndir=2 ** 30), "overflows"))
    for call, who, extra in ((call1, "abr_jvp_batch:", ()),
                             (call2, "abr2_jvp_batch:", ((dict(yoff=L(0, 0)), "empty item"), (dict(nygrid=3), "1 or npulse"),
                                                         (dict(xoff=L(0, big), yoff=L(0, big), nscale=4), "overflows")))):
        assert call() == 0
        for kw, why in common + extra:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call(prim=none4) == 0                                    # the primal may be left out
    rf, xx, v = np.full(8, 0.1 + 0.05j), np.array([0.0, 1.0]), _dirs(3, 1, 8)[0]
    (_, (da, db)), = mbfir.abr_jvp_batch([rf], xx, [v])
    (_, (wa, wb)) = ref.jvp(rf, None, xx, v)
    assert max(np.abs(da[0] - wa).max(), np.abs(db[0] - wb).max()) <= _bound(v, [1.0])
    (_, (da, db)), = mbfir.abr2_jvp_batch([rf], xx, [0.0], [v])
    assert max(np.abs(da[0, :, 0] - wa).max(), np.abs(db[0, :, 0] - wb).max()) <= _bound(v, [1.0])
