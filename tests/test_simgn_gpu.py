"""The fused least-squares products on the device (mbfir.abr_lsq_batch / abr_gn_batch and their 2D twins: k_abr_lsq_batch,
k_abr2_lsq_batch, k_abr_gn_batch, k_abr2_gn_batch, k_abr_gn_fold) and mbfir.refine_batch on them: against the NumPy reference of
tests/simgn_ref.py, against the shipped calls they fuse (abr_batch / abr_jvp_batch -> chain rule -> abr_vjp_batch), for exact zeros
and for the bit-invariance of a result under the batch's composition.

Bounds, per entry of g and H v, composed of the two the project has (tests/test_simgrad_gpu.py: 1e-12 max|s| sum(|ca| + |cb|) for
the adjoint; tests/test_simjvp_gpu.py: 1e-12 max|s| sum|v| per tangent entry) through the seed, whose norm is at most 4 per side
because |a|^2 + |b|^2 = 1.  With N = sum(|lambda_a| + |lambda_b|) of the reference's seed over the points and scales:
    lsq   1e-12 max|s| N
    gn    1e-12 max|s| (N + 16 max|s| sum|v| sum w)      (a tangent error of 1e-12 max|s| sum|v| goes through F, w and F^H: 4 w 4)
    L     1e-13 sum w (|f| + |t|)^2"""
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
SMAX = 1.0
KINDS = ("ex", "se", "inv", "st")

_spec = importlib.util.spec_from_file_location("simgn_ref", os.path.join(ROOT, "tests", "simgn_ref.py"))
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


def _moved(p, d):
    """the pulse with rf + d"""
    return (p[0] + d, p[1]) if isinstance(p, tuple) else p + d


def _grid(nx, span):
    """nx points over +-span with x = 0 among them"""
    x = np.linspace(-span, span, nx)
    x[nx // 2] = 0.0
    return x


def _dirs(seed, k, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n))


def _fit(seed, shape, kind):
    """a target of the profile's size and weights a third of which are zero"""
    rng = np.random.default_rng(seed)
    t = 0.5 * (rng.standard_normal(shape) + (0 if kind == "inv" else 1j) * rng.standard_normal(shape))
    w = rng.uniform(0.5, 2.0, shape) * (rng.uniform(size=shape) > 1 / 3)
    return t, w


LENGTHS = [1, 7, 8, 9, 255, 256, 257, 600]        # the VJP_T group edge; below, at and above the 256-sample tile; three tiles
FLIPS = [0.3, 0.02, 1.0, 2.5, 0.02, 1.5, np.pi, 2.0]
NXS = [600, 257, 255, 1, 257, 600, 255, 1]        # one point, partial chunks, more than one chunk
LEN2 = [7, 9, 256, 257, 600]
FLIP2 = [0.02, 1.0, 1.5, np.pi, 2.0]
GRIDS2 = [(19, 23), (1, 300), (19, 23), (1, 300), (19, 23)]          # 437 and 300 points: two chunks, the last one partial
K_OF = {"ex": 3, "se": 1, "inv": 2, "st": 3}


@functools.lru_cache(maxsize=None)
def _case(two_d, hard, kind, shared):
    """inputs and the reference's (L, g, N, E) and (H v, N) per pulse (and direction)"""
    if two_d:
        pulses = _pulses(8, LEN2, FLIP2, True)
        xs = [_grid(19, 3.0)] * 5 if shared else [_grid(nx, 2.0 + q) for q, (nx, _) in enumerate(GRIDS2)]
        ys = [_grid(23, 30.0)] * 5 if shared else [_grid(ny, 20.0 + q) for q, (_, ny) in enumerate(GRIDS2)]
    else:
        pulses = _pulses(7, LENGTHS, FLIPS, False)
        xs = [_grid(257, 6.0)] * 8 if shared else [_grid(nx, 4.0 + q) for q, nx in enumerate(NXS)]
        ys = [None] * 8
    K = K_OF[kind]
    fits, dirs, lsq, gn = [], [], [], []
    for q, (p, x, y) in enumerate(zip(pulses, xs, ys)):
        shape = (len(SCALES), len(x)) + ((len(y),) if two_d else ())
        t, w = _fit(100 + q, shape, kind)
        vs = _dirs(20 + q, K, len(_split(p)[0]))
        fits.append((t, w))
        dirs.append(vs)
        lsq.append(ref.lsq(*_split(p), x, t, w, SCALES, kind, y, hard, parts=True))
        gn.append([ref.gn(*_split(p), x, v, w, SCALES, kind, y, hard, parts=True) for v in vs])
    return pulses, xs, ys, fits, dirs, lsq, gn


def _call(two_d, which, pulses, xs, ys, shared, *rest, **kw):
    fn = getattr(mbfir, ("abr2_" if two_d else "abr_") + which + "_batch")
    pos = (xs[0] if shared else xs,) + ((ys[0] if shared else ys,) if two_d else ())
    return fn(pulses, *pos, *rest, **kw)


def _check_lsq(tag, got, fits, want):
    worst = 0.0
    for q, ((L, g), (t, w), (L0, g0, N, E)) in enumerate(zip(got, fits, want)):
        err, bound = float(np.abs(g - g0).max()), TOL * SMAX * N
        el, bl = abs(L - L0), 1e-13 * E
        worst = max(worst, err / bound, el / bl)
        print("%s lsq n %d points %s: |g - ref| %.3g, bound %.3g (max|g| %.3g);  |L - ref| %.3g, bound %.3g (L %.6g)"
              % (tag, len(g), t.shape[1:], err, bound, np.abs(g0).max(), el, bl, L0))
        assert err <= bound and el <= bl, (tag, q)
    print("%s lsq: worst difference / bound %.3g" % (tag, worst))


def _check_gn(tag, got, fits, dirs, want):
    worst = 0.0
    for q, (h, (t, w), vs, refs) in enumerate(zip(got, fits, dirs, want)):
        assert h.shape == vs.shape, (tag, q)
        for j, (h0, N) in enumerate(refs):
            err = float(np.abs(h[j] - h0).max())
            bound = TOL * SMAX * (N + 16 * SMAX * float(np.abs(vs[j]).sum()) * float(w.sum()))
            worst = max(worst, err / bound)
            print("%s gn n %d points %s direction %d of %d: |H v - ref| %.3g, bound %.3g (max|H v| %.3g)"
                  % (tag, vs.shape[1], t.shape[1:], j, len(vs), err, bound, np.abs(h0).max()))
            assert err <= bound, (tag, q, j)
    print("%s gn: worst difference / bound %.3g" % (tag, worst))


CASES = ([(False, hard, kind, False) for hard in (False, True) for kind in KINDS]
         + [(True, hard, kind, False) for hard in (False, True) for kind in KINDS]
         + [(False, False, "ex", True), (False, True, "inv", True), (True, True, "ex", True), (True, False, "st", True)])


@pytest.mark.parametrize("two_d,hard,kind,shared", CASES)
def test_device_products_are_the_reference(two_d, hard, kind, shared):
    pulses, xs, ys, fits, dirs, lsq, gn = _case(two_d, hard, kind, shared)
    tag = "%s hard %s %s shared %s" % ("2D" if two_d else "1D", hard, kind, shared)
    kw = dict(profile=kind, scales=SCALES, hard_pulse=hard)
    ts, ws = [f[0] for f in fits], [f[1] for f in fits]
    _check_lsq(tag, _call(two_d, "lsq", pulses, xs, ys, shared, ts, ws, **kw), fits, lsq)
    _check_gn(tag, _call(two_d, "gn", pulses, xs, ys, shared, dirs, ws, **kw), fits, dirs, gn)


@pytest.mark.parametrize("two_d,hard,kind", [(False, False, "ex"), (False, True, "se"), (True, False, "inv"), (True, True, "st"),
                                             (True, False, "ex"), (False, True, "st")])
def test_device_products_are_the_shipped_calls_they_fuse(two_d, hard, kind):
    """gn = abr*_jvp_batch -> chain rule -> abr*_vjp_batch and lsq = abr*_batch -> residual -> abr*_vjp_batch within the bounds of
    the reference comparison; and the central difference of L through the shipped forward along g / |g| (h = 1e-6) is |g| within
    1e-6 relative."""
    pulses, xs, ys, fits, dirs, lsq, gn = _case(two_d, hard, kind, False)
    tag = "%s hard %s %s shipped" % ("2D" if two_d else "1D", hard, kind)
    kw = dict(scales=SCALES, hard_pulse=hard)
    ts, ws = [f[0] for f in fits], [np.broadcast_to(f[1], f[0].shape) for f in fits]
    fn = "abr2" if two_d else "abr"
    pos = (xs, ys) if two_d else (xs,)
    fwd = getattr(mbfir, fn + "_batch")(pulses, *pos, **kw)
    cot = [ref.seed(kind, a, b, w * (ref.profile(kind, a, b) - t)) for (a, b), t, w in zip(fwd, ts, ws)]
    g2 = getattr(mbfir, fn + "_vjp_batch")(pulses, *pos, cot, **kw)
    L2 = [0.5 * float(np.sum(w * np.abs(ref.profile(kind, a, b) - t) ** 2)) for (a, b), t, w in zip(fwd, ts, ws)]
    got = getattr(mbfir, fn + "_lsq_batch")(pulses, *pos, ts, ws, profile=kind, **kw)
    _check_lsq(tag, got, fits, [(L, g, N, E) for L, g, (_, _, N, E) in zip(L2, g2, lsq)])
    tan = getattr(mbfir, fn + "_jvp_batch")(pulses, *pos, dirs, **kw)
    K = dirs[0].shape[0]
    h2 = []
    for j in range(K):
        cot = [ref.seed(kind, a, b, w * ref.dprofile(kind, a, b, da[j], db[j])) for ((a, b), (da, db)), w in zip(tan, ws)]
        h2.append(getattr(mbfir, fn + "_vjp_batch")(pulses, *pos, cot, **kw))
    hv = getattr(mbfir, fn + "_gn_batch")(pulses, *pos, dirs, ws, profile=kind, **kw)
    _check_gn(tag, hv, fits, dirs, [[(h2[j][q], gn[q][j][1]) for j in range(K)] for q in range(len(pulses))])
    h = 1e-6
    unit = [g / np.linalg.norm(g) for _, g in got]
    plus = getattr(mbfir, fn + "_batch")([_moved(p, h * u) for p, u in zip(pulses, unit)], *pos, **kw)
    minus = getattr(mbfir, fn + "_batch")([_moved(p, -h * u) for p, u in zip(pulses, unit)], *pos, **kw)
    for q, ((ap, bp), (am, bm), t, w, (_, g)) in enumerate(zip(plus, minus, ts, ws, got)):
        fd = (0.5 * np.sum(w * np.abs(ref.profile(kind, ap, bp) - t) ** 2) - 0.5 * np.sum(w * np.abs(ref.profile(kind, am, bm) - t) ** 2)) / (2 * h)
        rel = abs(fd - np.linalg.norm(g)) / np.linalg.norm(g)
        print("%s pulse %d: central difference of L along g / |g| %.9g, |g| %.9g, relative %.3g" % (tag, q, fd, np.linalg.norm(g), rel))
        assert rel <= 1e-6, (tag, q)


def test_exact_zeros():
    """v = 0, all weights zero, and scale 0 alone give exact zeros in g and H v (and L = 0 for zero weights)"""
    for two_d, hard, kind in ((False, False, "ex"), (False, True, "inv"), (True, True, "se"), (True, False, "st")):
        pulses, xs, ys, fits, dirs, _, _ = _case(two_d, hard, kind, False)
        ts, ws = [f[0] for f in fits], [f[1] for f in fits]
        kw = dict(profile=kind, hard_pulse=hard)
        zero_w = [np.zeros_like(w) for w in ws]
        for L, g in _call(two_d, "lsq", pulses, xs, ys, False, ts, zero_w, scales=SCALES, **kw):
            assert L == 0.0 and np.array_equal(g, np.zeros_like(g))
        for h in _call(two_d, "gn", pulses, xs, ys, False, dirs, zero_w, scales=SCALES, **kw):
            assert np.array_equal(h, np.zeros_like(h))
        for h in _call(two_d, "gn", pulses, xs, ys, False, [np.zeros_like(v) for v in dirs], ws, scales=SCALES, **kw):
            assert np.array_equal(h, np.zeros_like(h))
        t0, w0 = [t[1:2] for t in ts], [w[1:2] for w in ws]
        for (L, g), t, w in zip(_call(two_d, "lsq", pulses, xs, ys, False, t0, w0, scales=[0.0], **kw), t0, w0):
            assert np.array_equal(g, np.zeros_like(g))
            if kind != "st":                                          # b = 0 and |a| = 1 at every point: f = 0, 0, 1 (st: i a^2)
                f0 = 1.0 if kind == "inv" else 0.0
                assert abs(L - 0.5 * np.sum(w * np.abs(f0 - t) ** 2)) <= 1e-13 * np.sum(w * (1 + np.abs(t)) ** 2)
        for h in _call(two_d, "gn", pulses, xs, ys, False, dirs, w0, scales=[0.0], **kw):
            assert np.array_equal(h, np.zeros_like(h))


def test_results_have_the_same_bits_alone_in_17_reversed_repeated_and_at_every_place_among_3():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 700, 17)]
    flips = list(np.linspace(0.1, 3.0, 17))
    sc = [0.9, 1.1]

    def same_l(r, s):
        return r[0] == s[0] and np.array_equal(r[1], s[1])
    for two_d, hard, kind in ((False, False, "ex"), (False, True, "se"), (True, False, "inv"), (True, True, "st")):
        p = _pulses(53 + two_d, lengths, flips, two_d)
        x = [_grid(5 + 40 * q, 6.0) for q in range(17)] if not two_d else [_grid(5 + 3 * q, 3.0) for q in range(17)]
        y = [_grid(3 + 5 * (q % 7), 25.0) for q in range(17)]
        shapes = [(2, len(x[q])) + ((len(y[q]),) if two_d else ()) for q in range(17)]
        fits = [_fit(300 + q, shapes[q], kind) for q in range(17)]
        t, w = [f[0] for f in fits], [f[1] for f in fits]
        v = [_dirs(60 + q, 3, n) for q, n in enumerate(lengths)]
        kw = dict(profile=kind, scales=sc, hard_pulse=hard)

        def lsq(idx):
            return _call(two_d, "lsq", [p[q] for q in idx], [x[q] for q in idx], [y[q] for q in idx], False, [t[q] for q in idx],
                         [w[q] for q in idx], **kw)

        def gn(idx, vv):
            return _call(two_d, "gn", [p[q] for q in idx], [x[q] for q in idx], [y[q] for q in idx], False, vv, [w[q] for q in idx],
                         **kw)
        every = list(range(17))
        full, again, rev = lsq(every), lsq(every), lsq(every[::-1])[::-1]
        hfull, hagain, hrev = gn(every, v), gn(every, v), gn(every[::-1], v[::-1])[::-1]
        for q in every:
            assert same_l(full[q], again[q]) and same_l(full[q], rev[q]), (two_d, hard, q)
            assert np.array_equal(hfull[q], hagain[q]) and np.array_equal(hfull[q], hrev[q]), (two_d, hard, q)
        for q in (0, 5, 16):
            alone, twice = lsq([q, q])
            assert same_l(alone, full[q]) and same_l(twice, full[q]) and same_l(lsq([q])[0], full[q]), (two_d, hard, q)
            alone, twice = gn([q, q], [v[q], v[q]])
            assert np.array_equal(alone, hfull[q]) and np.array_equal(twice, hfull[q]), (two_d, hard, q)
            for j in range(3):
                perm = np.roll(np.arange(3), j)                      # place j holds direction 0
                assert np.array_equal(gn([q], [v[q][perm]])[0][j], hfull[q][0]), (two_d, hard, q, j)
            one, = gn([q], [v[q][0]])                                # K = 1, without the direction axis
            assert one.shape == (lengths[q],) and np.array_equal(one, hfull[q][0]), (two_d, hard, q)
            two, = gn([q], [v[q][:2]])
            assert np.array_equal(two, hfull[q][:2]), (two_d, hard, q)


@pytest.mark.parametrize("hard", [False, True])
def test_2d_at_y0_with_a_real_g_is_the_1d_call(hard):
    """the two form om differently (fma(x, gx, 0 gy) against x g), so the comparison is within the bounds, not of bits"""
    kind = "ex"
    pulses, xs, _, fits, dirs, lsq, gn = _case(False, hard, kind, False)
    p2 = [rf if g is None else (rf, g + 0j) for rf, g in map(_split, pulses)]
    kw = dict(profile=kind, scales=SCALES, hard_pulse=hard)
    t2, w2 = [f[0][..., None] for f in fits], [f[1][..., None] for f in fits]
    one = mbfir.abr_lsq_batch(pulses, xs, [f[0] for f in fits], [f[1] for f in fits], **kw)
    _check_lsq("2D at y = 0 hard %s" % hard, mbfir.abr2_lsq_batch(p2, xs, [0.0], t2, w2, **kw), fits,
               [(L, g, N, E) for (L, g), (_, _, N, E) in zip(one, lsq)])
    h1 = mbfir.abr_gn_batch(pulses, xs, dirs, [f[1] for f in fits], **kw)
    _check_gn("2D at y = 0 hard %s" % hard, mbfir.abr2_gn_batch(p2, xs, [0.0], dirs, w2, **kw), fits, dirs,
              [[(h1[q][j], gn[q][j][1]) for j in range(len(dirs[q]))] for q in range(len(pulses))])


def test_the_operator_is_symmetric_and_positive_semidefinite_on_the_device():
    """Re <u, H v> = Re <H u, v> within 1e-11 of the larger side, and Re <v, H v> >= 0"""
    for two_d, hard, kind in ((False, False, "ex"), (False, True, "inv"), (True, False, "se"), (True, True, "st")):
        pulses, xs, ys, fits, _, _, _ = _case(two_d, hard, kind, False)
        ws = [f[1] for f in fits]
        uv = [_dirs(400 + q, 2, len(_split(p)[0])) for q, p in enumerate(pulses)]
        hs = _call(two_d, "gn", pulses, xs, ys, False, uv, ws, profile=kind, scales=SCALES, hard_pulse=hard)
        for q, (d, h) in enumerate(zip(uv, hs)):
            lhs, rhs = float((np.conj(d[0]) * h[1]).real.sum()), float((np.conj(h[0]) * d[1]).real.sum())
            rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
            quad = [float((np.conj(d[j]) * h[j]).real.sum()) for j in range(2)]
            print("%s hard %s %s pulse %d: <u, H v> %.15g, <H u, v> %.15g, relative %.3g; <u, H u> %.6g, <v, H v> %.6g"
                  % ("2D" if two_d else "1D", hard, kind, q, lhs, rhs, rel, quad[0], quad[1]))
            assert rel <= 1e-11 and min(quad) >= 0.0, (two_d, hard, kind, q)


def test_refine_batch_lowers_the_loss_and_a_pulse_in_a_batch_has_its_bits_alone():
    """a 64-sample pulse at 90 degrees, 65 points, three gains, two outer iterations"""
    n, x, sc = 64, np.linspace(-8, 8, 65), (0.9, 1.0, 1.1)
    win = np.hanning(n + 2)[1:-1] * np.sinc(np.linspace(-2, 2, n))
    probs = []
    for k, flip in enumerate((np.pi / 2, 0.45 * np.pi, 0.55 * np.pi)):
        rf = win * (flip / win.sum()) + 0j
        (a, b), = mbfir.abr_batch([rf], x, scales=(1.0,))
        phase = np.exp(1j * np.angle(2 * np.conj(a[0, 32]) * b[0, 32]))
        band, stop = np.abs(x) <= 0.6, np.abs(x) >= 2.5
        t = np.stack([np.where(band, phase * np.sin(s * flip), 0.0) for s in sc])
        probs.append((rf, t, (band | stop).astype(float)))
    kw = dict(scales=sc, iters=2)
    rfs, infos = mbfir.refine_batch([p[0] for p in probs], x, [p[1] for p in probs], [p[2] for p in probs], **kw)
    for q, (rf, t, w) in enumerate(probs):
        L = infos[q]["losses"]
        print("pulse %d: losses %s, refused %d, calls %s" % (q, ["%.6g" % v for v in L], infos[q]["refused"], infos[q]["calls"]))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), q
        (r1,), (i1,) = mbfir.refine_batch([rf], x, [t], [w], **kw)
        assert np.array_equal(r1, rfs[q]) and i1 == infos[q], q
        (Lend, _), = mbfir.abr_lsq_batch([rfs[q]], x, [t], [w], scales=sc)
        assert Lend == L[-1]


def test_errors_and_the_raw_calls_leave_the_context_usable():
    """the MBFIR_E_ARG messages through ctypes: the forward calls' first, then a null array, the profile, a weight, ndir, overflow"""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    def pp(vs):
        return [p(v) if v is not None else None for v in vs]

    d, o = np.ones(64), [np.zeros(64) for _ in range(3)]
    neg, nan = np.ones(64), np.ones(64)
    neg[5], nan[5] = -1.0, np.nan                               # among the 6 weights of the default call

    def lsq1(roff=L(0, 3), xoff=L(0, 2), nscale=3, mode=0, npulse=1, nxgrid=1, profile=0, w=d, t=(d, d), out=o, **_):
        return lib.mbfir_abr_lsq_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, nxgrid, lp(xoff), p(d), nscale, p(d), mode, profile,
                                       *pp((w,) + tuple(t)), *pp(out))

    def lsq2(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 1), nscale=3, mode=0, npulse=1, nxgrid=1, nygrid=1, profile=0, w=d, t=(d, d),
             out=o, **_):
        return lib.mbfir_abr2_lsq_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid, lp(yoff),
                                        p(d), nscale, p(d), mode, profile, *pp((w,) + tuple(t)), *pp(out))

    def gn1(roff=L(0, 3), xoff=L(0, 2), nscale=3, mode=0, npulse=1, nxgrid=1, profile=0, w=d, ndir=2, v=(d, d), out=o, **_):
        return lib.mbfir_abr_gn_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, nxgrid, lp(xoff), p(d), nscale, p(d), mode, profile,
                                      p(w) if w is not None else None, ndir, *pp(v), *pp(out[:2]))

    def gn2(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 1), nscale=3, mode=0, npulse=1, nxgrid=1, nygrid=1, profile=0, w=d, ndir=2,
            v=(d, d), out=o, **_):
        return lib.mbfir_abr2_gn_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid, lp(yoff),
                                       p(d), nscale, p(d), mode, profile, p(w) if w is not None else None, ndir, *pp(v), *pp(out[:2]))

    common = ((dict(roff=L(0, 0)), "no samples"), (dict(npulse=2, roff=L(0, 3, 1)), "inconsistent offsets"),
              (dict(xoff=L(0, 0)), "empty item"), (dict(nscale=0), "scale list is empty"), (dict(mode=2), "mode"),
              (dict(npulse=0), "no pulses"), (dict(nxgrid=2), "1 or npulse"), (dict(w=None), "null"),
              (dict(out=[o[0], None, o[2]]), "null"), (dict(profile=4), "profile"), (dict(profile=-1), "profile"),
              (dict(w=neg), "weight"), (dict(w=nan), "weight"),
              (dict(w=None, profile=9), "null"), (dict(profile=9, w=neg), "profile"), (dict(profile=9, nscale=0), "scale list is empty"))
    only_lsq = ((dict(t=(None, d)), "null"),)
    only_gn = ((dict(v=(d, None)), "null"), (dict(ndir=0), "ndir"), (dict(ndir=-1), "ndir"), (dict(ndir=0, w=neg), "weight"),
               (dict(ndir=2 ** 31 - 1), "overflows"))
    for call, who, extra in ((lsq1, "abr_lsq_batch:", only_lsq), (lsq2, "abr2_lsq_batch:", only_lsq + ((dict(nygrid=3), "1 or npulse"),)),
                             (gn1, "abr_gn_batch:", only_gn), (gn2, "abr2_gn_batch:", only_gn + ((dict(yoff=L(0, 0)), "empty item"),))):
        assert call() == 0, ctx.last_error()
        for kw, why in common + extra:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
    assert lsq1(t=(d, None)) == 0 and lsq2(t=(d, None)) == 0       # a real target
    rf, xx, v = np.full(8, 0.1 + 0.05j), np.array([0.0, 1.0]), _dirs(3, 1, 8)[0]
    t, w = np.array([[0.1, 0.2j]]), np.ones((1, 2))
    (L1, g1), = mbfir.abr_lsq_batch([rf], xx, [t], [w])
    L0, g0, N, E = ref.lsq(rf, None, xx, t, w, [1.0], parts=True)
    assert np.abs(g1 - g0).max() <= TOL * N and abs(L1 - L0) <= 1e-13 * E
    h1, = mbfir.abr2_gn_batch([rf], xx, [0.0], [v], [w[..., None]])
    h0, N = ref.gn(rf, None, xx, v, w, [1.0], parts=True)
    assert np.abs(h1 - h0).max() <= TOL * (N + 16 * np.abs(v).sum() * w.sum())
