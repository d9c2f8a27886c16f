"""The fused least-squares products of the Bloch simulator's steady state on the device (mbfir.bloch_ss_lsq_batch:
k_bloch_ss_lsq_batch; mbfir.bloch_ss_gn_batch: k_bloch_ss_gn_batch; both folded by k_bloch_gn_fold) against the long-double NumPy
reference of tests/blochssgn_ref.py, against the shipped forward call mbfir.bloch_batch(mode=1) (bits of M, exact zeros at its own
output, central differences), against the shipped two-call paths they fuse, for the exact zeros, the bit-invariance of a pulse's
results under the batch's composition, the symmetry of the operator, and mbfir.refine_bloch_batch(steady_state=True) on them.

Bounds of every comparison with the reference and with the two-call paths (blochssgn_ref, which derives them): with k = kappa of
the pulse, per b1 entry bound_b1(pulse, c, scales, k) + k max|s| gamma dt_t e sum (wx + wy + wz), c the reference's cotangent and e
the bound of an entry of M (g) or of dM (H v), and bound_m(k) sum w |M - t| + 1e-13 sum w (M - t)^2 for L;
tests/test_blochssgn_cpu.py holds the float64 reference within a hundredth of these of its long-double twin.

Measured on an MI355X (worst over the sixteen cases, as a fraction of the bound; printed by every case with -s): against the
reference L 7.4e-6, g 3.4e-8, H v 7.0e-7; against the two-call paths L 3.4e-6, g 7.6e-10, H v 3.5e-7; the central difference of
the shipped forward along g / |g| 1.7e-9 relative."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochssgn_ref", os.path.join(ROOT, "tests", "blochssgn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
ssref = ref.ssref
SCALES = ref.SCALES
KMAX = 3
FD_STEP, FD_TOL = 1e-5, 2e-7          # fixed with the long-double reference: tests/test_blochssgn_cpu.py says how


@functools.lru_cache(maxsize=None)
def _case(shared):
    """The cases, the long-double reference (computed once per grid choice) with its bounds, and the device's results at K = 3"""
    pulses, dfs, dps, tgs, wts, vs = ref.cases(shared, KMAX)
    ks, want = [], []
    for p, df, dp, t, w, v in zip(pulses, dfs, dps, tgs, wts, vs):
        L, g, li, h, hi = ref.products(p, df, dp, t, w, v, SCALES, dtype=np.longdouble)
        k = li["kappa"]
        ks.append(k)
        want.append((float(L), g.astype(np.complex128), h.astype(np.complex128), ref.bound_L(li, k), ref.bound_g(p, li, SCALES, k),
                     ref.bound_h(p, v, hi, SCALES, k)))
    D, P = (dfs[0], dps[0]) if shared else (dfs, dps)
    lsq = mbfir.bloch_ss_lsq_batch(pulses, D, P, tgs, wts, scales=SCALES, steady=True)
    gn = mbfir.bloch_ss_gn_batch(pulses, D, P, vs, wts, scales=SCALES)
    return pulses, dfs, dps, D, P, tgs, wts, vs, ks, want, lsq, gn


@pytest.mark.parametrize("shared", [False, True])
def test_device_loss_gradient_and_products_are_the_reference(shared):
    """Eight periods of 1 .. 600 samples around the group of 8 and the 256-sample tile, on 1 .. 600 points, scales 1.0, 0.0, 0.9,
    kappa from 4.5 to 5001 (blochss_ref.batch); H v at K = 1, 2, 3 with a direction's bits the same at every K; M is
    bloch_batch(mode=1)'s, bit for bit; without steady the loss and the gradient keep their bits."""
    pulses, dfs, dps, D, P, tgs, wts, vs, ks, want, lsq, gn = _case(shared)
    fwd = mbfir.bloch_batch(pulses, D, P, scales=SCALES, mode=1)
    plain = mbfir.bloch_ss_lsq_batch(pulses, D, P, tgs, wts, scales=SCALES)
    two = mbfir.bloch_ss_gn_batch(pulses, D, P, [v[:2] for v in vs], wts, scales=SCALES)
    one = mbfir.bloch_ss_gn_batch(pulses, D, P, [v[0] for v in vs], wts, scales=SCALES)
    for q, (p, (L, g, h, bl, bg, bh), k) in enumerate(zip(pulses, want, ks)):
        dl, dg, dm = lsq[q]
        sl, sg, sh = abs(dl - L) / bl, float((np.abs(dg - g) / bg).max()), float((np.abs(gn[q] - h) / bh).max())
        print("shared %s n %d points %s kappa %.4g: |dev - ref| / bound: L %.3g, g %.3g, H v %.3g; L %.6g max|g| %.3g max|H v| %.3g"
              % (shared, len(p[0]), dm[0].shape[1:], k, sl, sg, sh, L, np.abs(g).max(), np.abs(h).max()))
        assert dg.shape == g.shape and gn[q].shape == h.shape and one[q].shape == g.shape, q
        assert sl <= 1 and sg <= 1 and sh <= 1, q
        assert np.array_equal(two[q], gn[q][:2]) and np.array_equal(one[q], gn[q][0]), q
        assert all(np.array_equal(dm[c], fwd[q][c]) for c in range(3)), q
        assert plain[q][0] == dl and np.array_equal(plain[q][1], dg), q


@pytest.mark.parametrize("shared", [False, True])
def test_targets_at_the_shipped_steady_state_give_exact_zeros(shared):
    """The residual is formed from mode 1's own bits: targets set to bloch_batch(mode=1)'s output give L == 0.0 and g == 0"""
    pulses, _, _, D, P, _, wts, _, _, _, _, _ = _case(shared)
    fwd = mbfir.bloch_batch(pulses, D, P, scales=SCALES, mode=1)
    for q, (L, g) in enumerate(mbfir.bloch_ss_lsq_batch(pulses, D, P, fwd, wts, scales=SCALES)):
        assert L == 0.0 and np.array_equal(g, np.zeros(len(g))), q


@pytest.mark.parametrize("shared", [False, True])
def test_the_fused_calls_are_the_shipped_two_call_paths(shared):
    """bloch_batch(mode=1) + NumPy + bloch_ss_vjp_batch, and bloch_ss_jvp_batch + NumPy + bloch_ss_vjp_batch direction by direction,
    within the bounds of the comparison with the reference"""
    pulses, _, _, D, P, tgs, wts, vs, _, want, lsq, gn = _case(shared)
    fwd = mbfir.bloch_batch(pulses, D, P, scales=SCALES, mode=1)
    res = [[fwd[q][c] - tgs[q][c] for c in range(3)] for q in range(len(pulses))]
    g2 = mbfir.bloch_ss_vjp_batch(pulses, D, P, [tuple(wts[q][c] * res[q][c] for c in range(3)) for q in range(len(pulses))], scales=SCALES)
    tan = mbfir.bloch_ss_jvp_batch(pulses, D, P, vs, scales=SCALES)
    h2 = [mbfir.bloch_ss_vjp_batch(pulses, D, P, [tuple(wts[q][c] * tan[q][1][c][j] for c in range(3)) for q in range(len(pulses))],
                                   scales=SCALES) for j in range(KMAX)]
    for q, (_, _, _, bl, bg, bh) in enumerate(want):
        L2 = 0.5 * float(sum((wts[q][c] * res[q][c] * res[q][c]).sum() for c in range(3)))
        sl, sg = abs(lsq[q][0] - L2) / bl, float((np.abs(lsq[q][1] - g2[q]) / bg).max())
        sh = max(float((np.abs(gn[q][j] - h2[j][q]) / bh[j]).max()) for j in range(KMAX))
        print("shared %s pulse %d: |fused - two calls| / bound: L %.3g, g %.3g, H v %.3g" % (shared, q, sl, sg, sh))
        assert sl <= 1 and sg <= 1 and sh <= 1, q


@functools.lru_cache(maxsize=None)
def _problem():
    """tests/test_blochss_gpu.py's: 64 samples of 10 us and a dead time of 160 us at T1 = 0.1 s, T2 = 0.03 s on 3 x 85 points, kappa
    119; weights with a third zero and targets in [-1, 1] over three scales"""
    rng = np.random.default_rng(7)
    n, gamma = 65, ssref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 / (gamma * 64e-5))
    b1[20], b1[-1] = 0.0, 0.0
    gr = np.append(rng.uniform(0.5, 1.5, 64) * 0.1, 0.0)
    tp = np.append(np.full(64, 1e-5), 1.6e-4)
    pulse, df, dp = (b1, gr, tp, 0.1, 0.03, "H-1"), ref._grid(3, 100.0), ref._grid(85, 3.0)
    w = rng.uniform(0, 1, (3, 3, 3, 85))
    w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
    return pulse, df, dp, tuple(rng.uniform(-1, 1, (3, 3, 3, 85))), tuple(w), ref.kappa(pulse, df, dp, (0.9, 1.0, 1.1))


def _loss(b1):
    """L through the shipped forward call"""
    pulse, df, dp, t, w, _ = _problem()
    m, = mbfir.bloch_batch([(b1,) + pulse[1:]], df, dp, scales=(0.9, 1.0, 1.1), mode=1)
    return 0.5 * float(sum((w[c] * (m[c] - t[c]) ** 2).sum() for c in range(3)))


def test_the_gradient_is_the_central_difference_of_the_loss_through_the_shipped_steady_state():
    """L on mbfir.bloch_batch(mode=1) at scales 0.9, 1.0, 1.1: the directional derivative along g / |g| equals |g| within the
    tolerance fixed with the long-double reference (which reaches 1.5e-8 at this step)"""
    pulse, df, dp, t, w, k = _problem()
    assert k <= 300
    (L0, g), = mbfir.bloch_ss_lsq_batch([pulse], df, dp, [t], [w], scales=(0.9, 1.0, 1.1))
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, FD_STEP * float(np.linalg.norm(pulse[0]))
    fd = (_loss(pulse[0] + eps * d) - _loss(pulse[0] - eps * d)) / (2 * eps)
    print("kappa %.4g, loss %.6g (two calls %.6g), |g| %.9g, central difference %.9g, relative difference %.3g"
          % (k, L0, _loss(pulse[0]), nrm, fd, abs(fd - nrm) / nrm))
    assert abs(fd - nrm) <= FD_TOL * nrm


def test_exact_zeros():
    """v = 0, all-zero weights, and the gradient and H v at the scale list (0,), whose loss is that of M = [0 0 1]"""
    pulses, _, _, D, P, tgs, wts, vs, ks, _, _, _ = _case(False)
    zw = [(0.0, 0.0, 0.0)] * len(pulses)
    for q, h in enumerate(mbfir.bloch_ss_gn_batch(pulses, D, P, [np.zeros_like(v) for v in vs], wts, scales=SCALES)):
        assert np.array_equal(h, np.zeros_like(h)), q
    for q, h in enumerate(mbfir.bloch_ss_gn_batch(pulses, D, P, vs, zw, scales=SCALES)):
        assert np.array_equal(h, np.zeros_like(h)), q
    for q, (L, g) in enumerate(mbfir.bloch_ss_lsq_batch(pulses, D, P, tgs, zw, scales=SCALES)):
        assert L == 0.0 and np.array_equal(g, np.zeros_like(g)), q
    t0, w0 = [tuple(c[:1] for c in t) for t in tgs], [tuple(c[:1] for c in w) for w in wts]
    for q, (L, g) in enumerate(mbfir.bloch_ss_lsq_batch(pulses, D, P, t0, w0, scales=(0.0,))):
        r = (t0[q][0], t0[q][1], 1.0 - t0[q][2])                               # M = [0 0 1] up to bound_m
        at_rest = 0.5 * float(sum((w0[q][c] * r[c] ** 2).sum() for c in range(3)))
        slack = ref.bound_m(ks[q]) * float(sum((w0[q][c] * np.abs(r[c])).sum() for c in range(3))) + 1e-13 * 2 * at_rest
        assert np.array_equal(g, np.zeros_like(g)) and abs(L - at_rest) <= slack, q
    for q, h in enumerate(mbfir.bloch_ss_gn_batch(pulses, D, P, vs, w0, scales=(0.0,))):
        assert np.array_equal(h, np.zeros_like(h)), q


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_repeated_and_at_each_place_among_the_directions():
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, tgs, wts, vs = [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ssref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(ref._grid(npos, 3.0))
        w = rng.uniform(0, 1, (3, 2, nf, npos))
        w[rng.uniform(size=w.shape) < 1 / 3] = 0.0
        wts.append(tuple(w))
        tgs.append(tuple(rng.uniform(-1, 1, (3, 2, nf, npos))))
        vs.append((rng.standard_normal((KMAX, n)) + 1j * rng.standard_normal((KMAX, n))) * np.abs(b1).max())

    def both(idx, dirs=None):
        a = [pulses[q] for q in idx], [dfs[q] for q in idx], [dps[q] for q in idx]
        return (mbfir.bloch_ss_lsq_batch(*a, [tgs[q] for q in idx], [wts[q] for q in idx], scales=sc, steady=True),
                mbfir.bloch_ss_gn_batch(*a, dirs or [vs[q] for q in idx], [wts[q] for q in idx], scales=sc))

    def same(a, b):
        return (a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and all(np.array_equal(u, v) for u, v in zip(a[0][2], b[0][2]))
                and np.array_equal(a[1], b[1]))
    every = list(range(17))
    full, again, rev = both(every), both(every), both(every[::-1])
    for q in every:
        one = (full[0][q], full[1][q])
        assert same(one, (again[0][q], again[1][q])) and same(one, (rev[0][16 - q], rev[1][16 - q])), q
    for q in (0, 5, 16):
        alone = both([q])
        assert same((alone[0][0], alone[1][0]), (full[0][q], full[1][q])), q
    q = 5                                                                   # every direction at every place of the K = 3 list
    for j in range(1, KMAX):
        h, = both([q], [np.roll(vs[q], j, 0)])[1]
        assert np.array_equal(np.roll(h, -j, 0), full[1][q]), j
    h1, = both([q], [vs[q][2]])[1]                                          # a 1-D direction: no K axis
    assert h1.shape == (lengths[q],) and np.array_equal(h1, full[1][q][2])


def test_the_operator_is_symmetric_and_positive_semidefinite():
    """Re <u, H v> = Re <H u, v> within 1e-11 of the larger side, and Re <v, H v> >= 0, on every case"""
    _, _, _, _, _, _, _, vs, _, _, _, gn = _case(False)
    for q, (v, h) in enumerate(zip(vs, gn)):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            l, r = float((np.conj(v[a]) * h[b]).real.sum()), float((np.conj(h[a]) * v[b]).real.sum())
            assert abs(l - r) <= 1e-11 * max(abs(l), abs(r)), (q, a, b, l, r)
        for k in range(KMAX):
            assert float((np.conj(v[k]) * h[k]).real.sum()) >= 0.0, (q, k)


def test_refine_bloch_batch_fits_a_steady_state_and_a_pulse_in_a_batch_has_the_bits_of_the_pulse_alone():
    """A 64-sample pulse and a dead time (a period of 2 ms, T1 = 0.2 s, T2 = 0.05 s), 3 x 33 points, three gains, two outer
    iterations: the target is the steady state of the pulse's smooth part at 1.15 times its amplitude"""
    sc, n, dt = (0.9, 1.0, 1.1), 64, 1e-5
    df, dp = ref._grid(3, 100.0), ref._grid(33, 3.0)
    tp, gr = np.append(np.full(n, dt), 2e-3 - n * dt), np.append(np.full(n, 0.05), 0.0)
    probs = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        smooth = np.hanning(n + 2)[1:-1] * (np.pi / 4 / (ssref.GAMMA_H1 * dt * np.hanning(n + 2).sum()))
        b1 = np.append(smooth * (1 + 0.1 * rng.standard_normal(n)), 0.0) + 0j
        t, = mbfir.bloch_batch([(np.append(1.15 * smooth, 0.0) + 0j, gr, tp, 0.2, 0.05, "H-1")], df, dp, mode=1)
        probs.append(((b1, gr, tp, 0.2, 0.05, "H-1"), tuple(c[0] for c in t), (1.0, 1.0, 1.0)))
    kw = dict(scales=sc, iters=2, cg=4, steady_state=True)
    alone = [mbfir.refine_bloch_batch([p], df, dp, [t], [w], **kw) for p, t, w in probs]
    for ((b,), (info,)), (p, t, w) in zip(alone, probs):
        print("losses %s, mu %.3g, calls %s" % (info["losses"], info["mu"], info["calls"]))
        assert len(info["losses"]) >= 2 and info["losses"][-1] < info["losses"][0]
        assert info["losses"][-1] == mbfir.bloch_ss_lsq_batch([(b,) + p[1:]], df, dp, [t], [w], scales=sc)[0][0]
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
    outs = [np.zeros(64) for _ in range(6)]

    def q(t):
        return [p(a) if a is not None else None for a in t]

    def head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1):
        return [ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None, lp(tsoff), p(d), p(t1), p(one),
                p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d), None, None, nscale, p(one)]

    def lsq(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
            w=(one, one, one), t=(d, d, d), out=outs[:3], m=outs[3:], **_):
        return lib.mbfir_bloch_ss_lsq_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), *q(w), *q(t),
                                            *q(out), *q(m))

    def gn(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
           w=(one, one, one), ndir=2, v=(d, d), out=outs[:2], **_):
        return lib.mbfir_bloch_ss_gn_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), *q(w), ndir, *q(v),
                                           *q(out))
    big = 2 ** 31 - 1
    shared = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
              (dict(npulse=2, toff=L(0, 3, 1), tsoff=L(0, 1, 2)), "inconsistent offsets"), (dict(tsoff=L(0, 2)), "neither 1 nor"),
              (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"), (dict(poff=L(0, 0)), "empty item"),
              (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"), (dict(b1=None), "required array is null"),
              (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"),
              (dict(w=(one, None, one)), "plane is null"),
              (dict(w=(one, neg, one)), "negative or not finite"), (dict(w=(one, one, nan)), "negative or not finite"))
    own = {lsq: ((dict(t=(d, d, None)), "plane is null"), (dict(out=[outs[0], None, outs[2]]), "plane is null"),
                 (dict(out=[None, outs[1], outs[2]]), "plane is null"), (dict(m=[None, outs[4], outs[5]]), "mx, my and mz"),
                 (dict(m=[outs[3], outs[4], None]), "mx, my and mz")),
           gn: ((dict(v=(d, None)), "plane is null"), (dict(out=[outs[0], None]), "plane is null"),
                (dict(ndir=0), "ndir must be at least 1"), (dict(ndir=2 ** 30, toff=L(0, 2 ** 28)), "overflows"))}
    for call, who in ((lsq, "bloch_ss_lsq_batch:"), (gn, "bloch_ss_gn_batch:")):
        assert call() == 0
        for kw, why in shared + own[call]:
            assert call(**kw) == mbfir.E_ARG, (who, kw)
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (who, kw, ctx.last_error())
        assert call() == 0 and call(m=[None] * 3) == 0
