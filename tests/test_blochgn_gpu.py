"""The least-squares products of the Bloch simulator with relaxation on the device (mbfir.bloch_lsq_batch: k_bloch_lsq_batch;
mbfir.bloch_gn_batch: k_bloch_gn_batch; both folded by k_bloch_gn_fold) against the long-double NumPy recursion of
tests/blochgn_ref.py, against the shipped two-call paths (bloch_batch + residual + bloch_vjp_batch; bloch_jvp_batch + weights +
bloch_vjp_batch), against central differences of the shipped forward call, for exact zeros, for the bit-invariance of a result under
the batch's composition and a direction's place among K, and mbfir.refine_bloch_batch on the device.

Bounds (tests/blochgn_ref.py derives them): per b1 entry t, g within 1e-12 max|s| gamma dt_t (N + sum w) and H v within 1e-12 max|s|
gamma dt_t (N + B_k sum w), N = sum|lambda_n| of the reference's seed and B_k = bound_jvp / 1e-12 of the direction; L within
1e-12 sum w |m - t| + 1e-13 sum w (m - t)^2.  tests/test_blochgn_cpu.py holds the float64 reference within a twentieth of these
of its long-double twin."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochgn_ref", os.path.join(ROOT, "tests", "blochgn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
SCALES = ref.SCALES
KMAX = 3


@functools.lru_cache(maxsize=None)
def _case(shared):
    """The cases with three directions per pulse, their long-double references (with the bounds' parts) and the device's results"""
    pulses, dfs, dps, m0s, tgs, wts, vs = ref.cases(shared, KMAX)
    want = []
    for p, df, dp, m0, t, w, v in zip(pulses, dfs, dps, m0s, tgs, wts, vs):
        L, g, li = ref.lsq(p, df, dp, t, w, SCALES, m0, dtype=np.longdouble, parts=True)
        h, hi = ref.gn(p, df, dp, v, w, SCALES, m0, dtype=np.longdouble, parts=True)
        want.append((L, g, li, h, hi))
    D, P = (dfs[0], dps[0]) if shared else (dfs, dps)
    lsq = mbfir.bloch_lsq_batch(pulses, D, P, tgs, wts, scales=SCALES, m0=m0s)
    gn = mbfir.bloch_gn_batch(pulses, D, P, vs, wts, scales=SCALES, m0=m0s)
    return pulses, dfs, dps, D, P, m0s, tgs, wts, vs, want, lsq, gn


@pytest.mark.parametrize("shared", [False, True])
def test_device_loss_gradient_and_products_are_the_reference(shared):
    """Eight pulses of 1 .. 600 samples around the group of 8 and the 256-sample tile, on 1 .. 600 points, scales 1.0, 0.0, 0.9,
    random m0, phi = 0 at a zero sample at df = 0 and position 0, a 26 ms pulse at T2 = 1 ms, a third of the weights zero
    (blochgn_ref.cases); H v at K = 1, 2 and 3."""
    pulses, dfs, dps, D, P, m0s, tgs, wts, vs, want, lsq, gn = _case(shared)
    by_k = {KMAX: gn}
    for K in (1, 2):
        by_k[K] = mbfir.bloch_gn_batch(pulses, D, P, [v[:K] for v in vs], wts, scales=SCALES, m0=m0s)
    for q, (p, v, (L, g, li, h, hi)) in enumerate(zip(pulses, vs, want)):
        bg, bh, bl = ref.bound_g(p, li, SCALES), ref.bound_h(p, v, hi, SCALES), ref.bound_L(li)
        eg, el = np.abs(lsq[q][1] - g).astype(np.float64), abs(float(lsq[q][0] - L))
        eh = np.abs(gn[q] - h).astype(np.float64)
        print("shared %s n %d points %dx%d: L %.6g |dev - ref| %.3g bound %.3g; g max %.3g worst share %.3g; H v max %.3g worst share %.3g"
              % (shared, len(p[0]), len(dfs[q]), np.shape(dps[q])[0], float(L), el, bl, np.abs(lsq[q][1]).max(), (eg / bg).max(),
                 np.abs(gn[q]).max(), (eh / bh).max()))
        assert lsq[q][1].shape == (len(p[0]),) and gn[q].shape == (KMAX, len(p[0])), q
        assert el <= bl and np.all(eg <= bg) and np.all(eh <= bh), q
        for K in (1, 2):
            assert by_k[K][q].shape == (K, len(p[0])) and np.array_equal(by_k[K][q], gn[q][:K]), (q, K)      # K does not change a direction's bits


@pytest.mark.parametrize("shared", [False, True])
def test_device_results_are_the_shipped_two_call_paths(shared):
    """L and g against bloch_batch + NumPy residual + bloch_vjp_batch, H v against bloch_jvp_batch + NumPy weights +
    bloch_vjp_batch, within the same bounds (taken from the reference's parts)"""
    pulses, dfs, dps, D, P, m0s, tgs, wts, vs, want, lsq, gn = _case(shared)
    fwd = mbfir.bloch_batch(pulses, D, P, scales=SCALES, m0=m0s)
    res = [tuple(m[c] - t[c] for c in range(3)) for m, t in zip(fwd, tgs)]
    g2 = mbfir.bloch_vjp_batch(pulses, D, P, [tuple(w[c] * r[c] for c in range(3)) for w, r in zip(wts, res)], scales=SCALES, m0=m0s)
    tan = mbfir.bloch_jvp_batch(pulses, D, P, vs, scales=SCALES, m0=m0s)
    for q, (p, v, w, r, (L, g, li, h, hi)) in enumerate(zip(pulses, vs, wts, res, want)):
        L2 = 0.5 * sum(float((w[c] * r[c] * r[c]).sum()) for c in range(3))
        bg, bh, bl = ref.bound_g(p, li, SCALES), ref.bound_h(p, v, hi, SCALES), ref.bound_L(li)
        print("shared %s n %d: |L - two calls| %.3g bound %.3g; g worst share %.3g" % (shared, len(p[0]), abs(lsq[q][0] - L2), bl,
                                                                                         (np.abs(lsq[q][1] - g2[q]) / bg).max()))
        assert abs(lsq[q][0] - L2) <= bl and np.all(np.abs(lsq[q][1] - g2[q]) <= bg), q
    for k in range(KMAX):
        h2 = mbfir.bloch_vjp_batch(pulses, D, P, [tuple(w[c] * t[1][c][k] for c in range(3)) for w, t in zip(wts, tan)],
                                   scales=SCALES, m0=m0s)
        for q, (p, v, (L, g, li, h, hi)) in enumerate(zip(pulses, vs, want)):
            assert np.all(np.abs(gn[q][k] - h2[q]) <= ref.bound_h(p, v, hi, SCALES)[k]), (q, k)


def _fd_case():
    sc, n, dur = (0.9, 1.0, 1.1), 64, 4e-3
    rng = np.random.default_rng(90)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (np.pi / 2 / (ref.GAMMA_H1 * dur))
    rest = (rng.uniform(0.5, 1.5, n) * 0.05, dur / n, 1.0, 4e-3, "H-1")
    df, dp = ref._grid(3, 100.0), ref._grid(85, 3.0)
    m0 = tuple(rng.uniform(-0.5, 0.5, (3, 3, 85)))
    w = rng.uniform(0, 1, (3, 3, 3, 85))
    w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
    t = rng.uniform(-1, 1, (3, 3, 3, 85))
    return sc, b1, rest, df, dp, m0, tuple(w), tuple(t)


def test_the_gradient_is_the_central_difference_of_the_loss_through_the_shipped_forward():
    """A 64-sample pulse on 3 x 85 points with T2 = the duration at scales 0.9, 1.0, 1.1: along d = g / |g| times max|b1|,
    (L(b1 + h d) - L(b1 - h d)) / 2h at h = 1e-6 with L summed in long double from bloch_batch's end points equals Re <g, d> to
    1e-6 relative (truncation h^2 and the forward call's rounding over h are both far below it)."""
    sc, b1, rest, df, dp, m0, w, t = _fd_case()
    (L, g), = mbfir.bloch_lsq_batch([(b1,) + rest], df, dp, [t], [w], scales=sc, m0=m0)
    d, h = g / np.sqrt((np.abs(g) ** 2).sum()) * np.abs(b1).max(), 1e-6

    def loss(b):
        m, = mbfir.bloch_batch([(b,) + rest], df, dp, scales=sc, m0=m0)
        return sum((np.asarray(w[c], dtype=np.longdouble) * (m[c] - np.asarray(t[c], dtype=np.longdouble)) ** 2).sum() for c in range(3)) / 2
    fd = float((loss(b1 + h * d) - loss(b1 - h * d)) / (2 * h))
    want = float((np.conj(g) * d).real.sum())
    print("L %.9g (forward call %.9g), Re <g, d> %.9g, central difference %.9g, relative difference %.3g"
          % (L, float(loss(b1)), want, fd, abs(fd - want) / abs(want)))
    assert abs(fd - want) <= 1e-6 * abs(want)


def test_zero_direction_zero_weights_and_scale_zero_give_exact_zeros():
    pulses, dfs, dps, D, P, m0s, tgs, wts, vs, _, _, _ = _case(False)
    for h, v in zip(mbfir.bloch_gn_batch(pulses, D, P, [np.zeros_like(v) for v in vs], wts, scales=SCALES, m0=m0s), vs):
        assert np.array_equal(h, np.zeros(v.shape))
    zero = [(0.0, 0.0, 0.0)] * len(pulses)
    for (L, g), v in zip(mbfir.bloch_lsq_batch(pulses, D, P, tgs, zero, scales=SCALES, m0=m0s), vs):
        assert L == 0.0 and np.array_equal(g, np.zeros(v.shape[1]))
    for h, v in zip(mbfir.bloch_gn_batch(pulses, D, P, vs, zero, scales=SCALES, m0=m0s), vs):
        assert np.array_equal(h, np.zeros(v.shape))
    at0 = [tuple(x[:1] for x in tri) for tri in wts]                       # scale 0 alone: m0 relaxes, and the loss does not depend on b1
    for (L, g), v in zip(mbfir.bloch_lsq_batch(pulses, D, P, [tuple(x[:1] for x in tri) for tri in tgs], at0, scales=(0.0,), m0=m0s), vs):
        assert np.isfinite(L) and np.array_equal(g, np.zeros(v.shape[1]))
    for h, v in zip(mbfir.bloch_gn_batch(pulses, D, P, vs, at0, scales=(0.0,), m0=m0s), vs):
        assert np.array_equal(h, np.zeros(v.shape))


def test_results_have_the_same_bits_alone_in_17_reversed_repeated_and_at_every_place_among_three_directions():
    K = KMAX
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, m0s, vs, wts, tgs = [], [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(ref._grid(npos, 3.0))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        vs.append((rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * np.abs(b1).max())
        w = rng.uniform(0, 1, (3, 2, nf, npos))
        w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
        wts.append(tuple(w))
        tgs.append(tuple(rng.uniform(-1, 1, (3, 2, nf, npos))))

    def both(idx, dirs=None):
        a = [pulses[q] for q in idx], [dfs[q] for q in idx], [dps[q] for q in idx]
        kw = dict(scales=sc, m0=[m0s[q] for q in idx])
        return (mbfir.bloch_lsq_batch(*a, [tgs[q] for q in idx], [wts[q] for q in idx], **kw),
                mbfir.bloch_gn_batch(*a, dirs or [vs[q] for q in idx], [wts[q] for q in idx], **kw))

    def same(a, b):
        return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[1], b[1])
    every = list(range(17))
    full, again, rev = both(every), both(every), both(every[::-1])
    for q in every:
        one = (full[0][q], full[1][q])
        assert same(one, (again[0][q], again[1][q])) and same(one, (rev[0][16 - q], rev[1][16 - q])), q
    for q in (0, 5, 16):
        alone = both([q])
        assert same((alone[0][0], alone[1][0]), (full[0][q], full[1][q])), q
    q = 5                                                                   # every direction at every place of the K = 3 list
    for j in range(1, K):
        h, = both([q], [np.roll(vs[q], j, 0)])[1]
        assert np.array_equal(np.roll(h, -j, 0), full[1][q]), j
    h1, = both([q], [vs[q][2]])[1]                                          # a 1-D direction: no K axis
    assert h1.shape == (lengths[q],) and np.array_equal(h1, full[1][q][2])


def test_the_operator_is_symmetric_and_positive_semidefinite():
    """Re <u, H v> = Re <H u, v> within 1e-11 of the larger side, and Re <v, H v> >= 0, on every case"""
    pulses, _, _, _, _, _, _, _, vs, _, _, gn = _case(False)
    for q, (v, h) in enumerate(zip(vs, gn)):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            l, r = float((np.conj(v[a]) * h[b]).real.sum()), float((np.conj(h[a]) * v[b]).real.sum())
            assert abs(l - r) <= 1e-11 * max(abs(l), abs(r)), (q, a, b, l, r)
        for k in range(KMAX):
            assert float((np.conj(v[k]) * h[k]).real.sum()) >= 0.0, (q, k)


def test_none_for_m0_is_explicit_equilibrium():
    pulses, _, _, D, P, _, tgs, wts, vs, _, _, _ = _case(False)
    eq = [(0.0, 0.0, 1.0)] * len(pulses)
    for (La, ga), (Lb, gb) in zip(mbfir.bloch_lsq_batch(pulses, D, P, tgs, wts, scales=SCALES),
                                  mbfir.bloch_lsq_batch(pulses, D, P, tgs, wts, scales=SCALES, m0=eq)):
        assert La == Lb and np.array_equal(ga, gb)
    for ha, hb in zip(mbfir.bloch_gn_batch(pulses, D, P, vs, wts, scales=SCALES), mbfir.bloch_gn_batch(pulses, D, P, vs, wts, scales=SCALES, m0=eq)):
        assert np.array_equal(ha, hb)


def test_refine_bloch_batch_lowers_the_loss_and_a_pulse_in_a_batch_has_the_bits_of_the_pulse_alone():
    """64 samples, 3 x 33 points, three gains, two outer iterations: a saturation-like fit of mz with a little weight on mx, my"""
    sc, n, dur = (0.9, 1.0, 1.1), 64, 4e-3
    df, dp = ref._grid(3, 100.0), ref._grid(33, 3.0)
    probs = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        b1 = (np.hanning(n + 2)[1:-1] + 0.1 * rng.standard_normal(n)) * (np.pi / 2 / (ref.GAMMA_H1 * dur / n * np.hanning(n + 2).sum())) + 0j
        p = (b1, np.full(n, 0.05), dur / n, 1.0, 10e-3, "H-1")
        tz = np.where(np.abs(dp) < 1.0, 0.0, 1.0)[None, :] * np.ones((3, 1))
        w = np.where((np.abs(dp) > 0.8) & (np.abs(dp) < 1.2), 0.0, 1.0)[None, :] * np.ones((3, 1))
        probs.append((p, (0.0, 0.0, tz), (0.1 * w, 0.1 * w, w)))
    kw = dict(scales=sc, iters=2, cg=4)
    alone = [mbfir.refine_bloch_batch([p], df, dp, [t], [w], **kw) for p, t, w in probs]
    for ((b,), (info,)), (p, t, w) in zip(alone, probs):
        print("losses %s, mu %.3g, calls %s" % (info["losses"], info["mu"], info["calls"]))
        assert len(info["losses"]) >= 2 and info["losses"][-1] < info["losses"][0]
        assert info["losses"][-1] == mbfir.bloch_lsq_batch([(b,) + p[1:]], df, dp, [t], [w], scales=sc)[0][0]
    b1s, infos = mbfir.refine_bloch_batch([p for p, _, _ in probs], df, dp, [t for _, t, _ in probs], [w for _, _, w in probs], **kw)
    for k in range(3):
        assert np.array_equal(b1s[k], alone[k][0][0]) and infos[k] == alone[k][1][0], k


def test_errors_of_the_raw_calls_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, one, neg, nan = np.full(64, 1e-5), np.ones(64), np.ones(64), np.ones(64)
    neg[5], nan[4] = -1.0, np.nan
    outs = [np.zeros(64) for _ in range(3)]

    def q(t):
        return [p(a) if a is not None else None for a in t]

    def head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1):
        return [ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None, lp(tsoff), p(d), p(t1), p(one),
                p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d), None, None, nscale, p(one)]

    def lsq(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
            m0=(None, None, None), w=(one, one, one), t=(d, d, d), out=outs, **_):
        return lib.mbfir_bloch_lsq_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), *q(m0), *q(w), *q(t),
                                         *q(out))

    def gn(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
           m0=(None, None, None), w=(one, one, one), ndir=2, v=(d, d), out=outs[:2], **_):
        return lib.mbfir_bloch_gn_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), *q(m0), *q(w), ndir,
                                        *q(v), *q(out))
    big = 2 ** 31 - 1
    shared = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
              (dict(npulse=2, toff=L(0, 3, 1), tsoff=L(0, 1, 2)), "inconsistent offsets"), (dict(tsoff=L(0, 2)), "neither 1 nor"),
              (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"), (dict(poff=L(0, 0)), "empty item"),
              (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"), (dict(b1=None), "required array is null"),
              (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"),
              (dict(w=(one, None, one)), "plane is null"), (dict(m0=(one, one, None)), "m0x, m0y and m0z"),
              (dict(w=(one, neg, one)), "negative or not finite"), (dict(w=(one, one, nan)), "negative or not finite"))
    own = {lsq: ((dict(t=(d, d, None)), "plane is null"), (dict(out=[outs[0], None, outs[2]]), "plane is null"),
                 (dict(out=[None, outs[1], outs[2]]), "plane is null")),
           gn: ((dict(v=(d, None)), "plane is null"), (dict(out=[outs[0], None]), "plane is null"),
                (dict(ndir=0), "ndir must be at least 1"), (dict(ndir=2 ** 30, toff=L(0, 2 ** 28)), "overflows"))}
    for call, who in ((lsq, "bloch_lsq_batch:"), (gn, "bloch_gn_batch:")):
        assert call() == 0
        for kw, why in shared + own[call]:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (who, kw, ctx.last_error())
        assert call() == 0 and call(m0=(one, one, one)) == 0
