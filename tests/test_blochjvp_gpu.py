"""The tangent of the Bloch simulator with relaxation on the device (mbfir.bloch_jvp_batch: k_bloch_jvp_batch;
mbfir.torchsim.bloch(forward_mode=True)) against the long-double NumPy recursion of tests/blochjvp_ref.py, against the shipped
adjoint mbfir.bloch_vjp_batch through the dot-product identity, against central differences of the shipped forward call
mbfir.bloch_batch, and for the bit-invariance of a tangent under the batch's composition and the direction's place in its group.

Bound of every comparison with the reference (blochjvp_ref.bound_jvp), per entry of direction k: 1e-12 (max|s| gamma sum_t dt_t
|v_t| + (|dmx_0| + |dmy_0| + |dmz_0|) at that point).  dR[dn] has norm at most |dn|, R and D have norm at most 1, |m| <= 1 because
|m0| <= 1, and 1e-12 is the forward tolerance of the existing Bloch tests.  tests/test_blochjvp_cpu.py holds the float64 reference
within a twentieth of this bound of its long-double twin."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochjvp_ref", os.path.join(ROOT, "tests", "blochjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
SCALES = ref.SCALES


@functools.lru_cache(maxsize=None)
def _case(shared):
    """The cases with BJVP_K + 1 directions per pulse, their long-double tangents and the device's at all BJVP_K + 1 directions"""
    G = mbfir.bloch_jvp_group()
    pulses, dfs, dps, m0s, cots, vs, dms = ref.cases(shared, G + 1)
    want = [ref.jvp_scaled(p, df, dp, v, SCALES, m0, dm, dtype=np.longdouble)[1]
            for p, df, dp, m0, v, dm in zip(pulses, dfs, dps, m0s, vs, dms)]
    got = mbfir.bloch_jvp_batch(pulses, dfs[0] if shared else dfs, dps[0] if shared else dps, vs, scales=SCALES, m0=m0s,
                                tangents_m0=dms)
    return G, pulses, dfs, dps, m0s, cots, vs, dms, want, got


@pytest.mark.parametrize("shared", [False, True])
def test_device_tangent_is_the_reference_and_the_primal_is_the_forward_call(shared):
    """Eight pulses of 1 .. 600 samples around the 256-sample tile, on 1 .. 600 points, scales 1.0, 0.0, 0.9, random m0, phi = 0 at
    a zero sample at df = 0 and position 0, and a 26 ms pulse at T2 = 1 ms (blochgrad_ref.batch), at K = 1, BJVP_K and BJVP_K + 1."""
    G, pulses, dfs, dps, m0s, _, vs, dms, want, full = _case(shared)
    fwd = mbfir.bloch_batch(pulses, dfs[0] if shared else dfs, dps[0] if shared else dps, scales=SCALES, m0=m0s)
    for K in sorted({1, G, G + 1}):
        got = full if K == G + 1 else mbfir.bloch_jvp_batch(
            pulses, dfs[0] if shared else dfs, dps[0] if shared else dps, [v[:K] for v in vs], scales=SCALES, m0=m0s,
            tangents_m0=[tuple(d[:K] for d in dm) for dm in dms])
        for q, ((m, tan), w, f, p, v, dm) in enumerate(zip(got, want, fwd, pulses, vs, dms)):
            bound = ref.bound_jvp(p, v[:K], tuple(d[:K] for d in dm), SCALES)[:, None]
            err = np.max([np.abs(a - b[:K]).astype(np.float64) for a, b in zip(tan, w)], 0)
            print("shared %s K %d n %d points %s: |dev - ref| %.3g, bound %.3g, max |dev - ref| / bound %.3g, max|dm| %.3g"
                  % (shared, K, len(p[0]), m[0].shape[1:], err.max(), bound.min(), (err / bound).max(), np.abs(tan[0]).max()))
            assert all(t.shape == (K,) + m[0].shape for t in tan), q
            assert all(np.array_equal(a, b) for a, b in zip(m, f)), q
            assert np.all(err <= bound), (q, K)
            assert all(np.array_equal(a, b[:K]) for a, b in zip(tan, full[q][1])), (q, K)       # K does not change a direction's bits


def test_zero_scale_and_zero_direction_give_exact_zeros():
    _, pulses, dfs, dps, m0s, _, vs, dms, _, full = _case(False)
    for q, (_, tan) in enumerate(full):                                    # at scale 0 the m0 direction alone moves the end point
        assert any(np.any(t[:, 1] != 0) for t in tan), q
    for (_, tan), v in zip(mbfir.bloch_jvp_batch(pulses, dfs, dps, vs, scales=(0.0,), m0=m0s), vs):
        assert all(np.array_equal(t, np.zeros((len(v), 1) + t.shape[2:])) for t in tan)
    zero = mbfir.bloch_jvp_batch(pulses, dfs, dps, [np.zeros_like(v) for v in vs], scales=SCALES, m0=m0s,
                                 tangents_m0=[tuple(np.zeros_like(d) for d in dm) for dm in dms])
    for (_, tan) in zero:
        assert all(np.array_equal(t, np.zeros(t.shape)) for t in tan)


def test_a_pure_m0_direction_is_dm0_pushed_through_the_forward_call():
    """With v = 0 the tangent is the homogeneous recursion dm_t = D_t R_t dm_{t-1}.  At T1 = 1e300 E1 is exactly 1 and c_t exactly
    0, so the forward call started from dm_0 steps the same recursion: the two are equal to the bit, direction by direction."""
    G, pulses, dfs, dps, m0s, _, vs, dms, _, _ = _case(False)
    slow = [p[:3] + (1e300,) + p[4:] for p in pulses]
    got = mbfir.bloch_jvp_batch(slow, dfs, dps, [np.zeros_like(v) for v in vs], scales=SCALES, m0=m0s, tangents_m0=dms)
    for k in (0, G):
        want = mbfir.bloch_batch(slow, dfs, dps, scales=SCALES, m0=[tuple(d[k] for d in dm) for dm in dms])
        for q, ((_, tan), w) in enumerate(zip(got, want)):
            assert all(np.array_equal(t[k], b) for t, b in zip(tan, w)), (q, k)


def test_none_for_the_m0_directions_is_explicit_zeros():
    _, pulses, dfs, dps, m0s, _, vs, dms, _, _ = _case(False)
    a = mbfir.bloch_jvp_batch(pulses, dfs, dps, vs, scales=SCALES, m0=m0s)
    b = mbfir.bloch_jvp_batch(pulses, dfs, dps, vs, scales=SCALES, m0=m0s, tangents_m0=[tuple(np.zeros_like(d) for d in dm) for dm in dms])
    for (ma, ta), (mb, tb) in zip(a, b):
        assert all(np.array_equal(u, v) for u, v in zip(ma + ta, mb + tb))


def test_a_tangent_has_the_same_bits_alone_in_17_reversed_repeated_and_at_every_place_of_its_group():
    G = mbfir.bloch_jvp_group()
    K = G + 1
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, m0s, vs, dms = [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(ref._grid(npos, 3.0))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        vs.append((rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * np.abs(b1).max())
        dms.append(tuple(rng.standard_normal((3, K, nf, npos))))
    full = mbfir.bloch_jvp_batch(pulses, dfs, dps, vs, scales=sc, m0=m0s, tangents_m0=dms)
    again = mbfir.bloch_jvp_batch(pulses, dfs, dps, vs, scales=sc, m0=m0s, tangents_m0=dms)
    rev = mbfir.bloch_jvp_batch(pulses[::-1], dfs[::-1], dps[::-1], vs[::-1], scales=sc, m0=m0s[::-1], tangents_m0=dms[::-1])[::-1]

    def same(a, b):
        return all(np.array_equal(u, v) for u, v in zip(a[0] + a[1], b[0] + b[1]))
    for q in range(17):
        assert same(full[q], again[q]) and same(full[q], rev[q]), q
    for q in (0, 5, 16):
        alone, = mbfir.bloch_jvp_batch([pulses[q]], [dfs[q]], [dps[q]], [vs[q]], scales=sc, m0=[m0s[q]], tangents_m0=[dms[q]])
        assert same(alone, full[q]), q
    q = 5                                                                   # every direction at every place of the K = BJVP_K + 1 list
    for j in range(1, K):
        (_, tan), = mbfir.bloch_jvp_batch([pulses[q]], [dfs[q]], [dps[q]], [np.roll(vs[q], j, 0)], scales=sc, m0=[m0s[q]],
                                          tangents_m0=[tuple(np.roll(d, j, 0) for d in dms[q])])
        assert all(np.array_equal(np.roll(t, -j, 0), w) for t, w in zip(tan, full[q][1])), j
    (_, one), = mbfir.bloch_jvp_batch([pulses[q]], [dfs[q]], [dps[q]], [vs[q][G]], scales=sc, m0=[m0s[q]],
                                      tangents_m0=[tuple(d[G] for d in dms[q])])           # a 1-D tangent: no K axis
    assert all(t.shape == w.shape[1:] and np.array_equal(t, w[G]) for t, w in zip(one, full[q][1]))


@pytest.mark.parametrize("shared", [False, True])
def test_the_identity_with_the_shipped_adjoint(shared):
    """sum cot . dm = Re sum conj(g) v + sum gm0 . dm_0 with g, gm0 of mbfir.bloch_vjp_batch(grad_m0=True), within the two sides'
    own bounds (blochjvp_ref.identity_tol)"""
    G, pulses, dfs, dps, m0s, cots, vs, dms, _, full = _case(shared)
    adj = mbfir.bloch_vjp_batch(pulses, dfs[0] if shared else dfs, dps[0] if shared else dps, cots, scales=SCALES, m0=m0s,
                                grad_m0=True)
    for q, ((_, tan), (g, gm), p, cot, v, dm) in enumerate(zip(full, adj, pulses, cots, vs, dms)):
        for k in (0, G):
            d0 = tuple(d[k] for d in dm)
            lhs = float(sum((cot[c] * tan[c][k]).sum() for c in range(3)))
            rhs = float((np.conj(g) * v[k]).real.sum()) + float(sum((gm[c] * d0[c]).sum() for c in range(3)))
            tol = ref.identity_tol(p, cot, v[k], d0, SCALES)
            print("shared %s n %d direction %d: lhs %.9g rhs %.9g |lhs - rhs| %.3g tolerance %.3g"
                  % (shared, len(p[0]), k, lhs, rhs, abs(lhs - rhs), tol))
            assert abs(lhs - rhs) <= tol, (q, k)


def test_the_jvp_is_the_central_difference_of_the_shipped_forward():
    """A 64-sample pulse on 3 x 85 points with T2 = the duration at scales 0.9, 1.0, 1.1, along a b1 direction of the pulse's size
    together with an m0 direction: (m(b1 + h v, m0 + h dm0) - m(b1 - h v, m0 - h dm0)) / 2h at h = 1e-6 equals the tangent to 1e-6
    of its largest entry (truncation h^2 |m'''| and rounding eps_machine / h are both far below it)."""
    sc, n, dur, h = (0.9, 1.0, 1.1), 64, 4e-3, 1e-6
    rng = np.random.default_rng(90)
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (np.pi / 2 / (ref.GAMMA_H1 * dur))
    rest = (rng.uniform(0.5, 1.5, n) * 0.05, dur / n, 1.0, 4e-3, "H-1")
    df, dp = ref._grid(3, 100.0), ref._grid(85, 3.0)
    m0 = rng.uniform(-0.5, 0.5, (3, 3, 85))
    v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.abs(b1).max()
    dm0 = rng.standard_normal((3, 3, 85))

    def fwd(b, m):
        out, = mbfir.bloch_batch([(b,) + rest], df, dp, scales=sc, m0=tuple(m))
        return np.stack(out)
    (_, tan), = mbfir.bloch_jvp_batch([(b1,) + rest], df, dp, [v], scales=sc, m0=tuple(m0), tangents_m0=[tuple(dm0)])
    tan = np.stack(tan)
    fd = (fwd(b1 + h * v, m0 + h * dm0) - fwd(b1 - h * v, m0 - h * dm0)) / (2 * h)
    rel = float(np.abs(fd - tan).max() / np.abs(tan).max())
    print("max|tangent| %.6g, |central difference - tangent| / max|tangent| %.3g" % (np.abs(tan).max(), rel))
    assert rel <= 1e-6


def test_torchsim_bloch_forward_mode_on_the_device():
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
        return mbfir.torchsim.bloch(b, gr, dt, 1.0, 1e-3, df, dp, nucleus="H-1", scales=sc, m0=m, forward_mode=True)
    assert torch.autograd.gradcheck(f, (b1, m0), check_forward_ad=True)
    assert torch.autograd.gradcheck(lambda b: f(b, None), (b1,), check_forward_ad=True)
    # the primal and the tangent are the NumPy calls' bits
    v, dm = rng.standard_normal(6) + 1j * rng.standard_normal(6), rng.standard_normal((3, 2, 3))
    out, tan = torch.func.jvp(f, (b1.detach(), m0.detach()), (torch.tensor(v), torch.tensor(dm)))
    (wm, wt), = mbfir.bloch_jvp_batch([(b0, gr, dt, 1.0, 1e-3, "H-1")], df, dp, [v], scales=sc, m0=tuple(m00), tangents_m0=[tuple(dm)])
    assert tan[0].dtype == torch.float64 and tuple(tan[0].shape) == (2, 2, 3)
    assert all(np.array_equal(o.numpy(), w) for o, w in zip(out, wm))
    assert all(np.array_equal(t.numpy(), w) for t, w in zip(tan, wt))


def test_errors_of_the_raw_call_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(6)]

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
             m0=(None, None, None), ndir=2, v=(d, d), dm0=(None, None, None), m=outs[:3], dm=outs[3:]):
        def q(t):
            return [p(a) if a is not None else None for a in t]
        return lib.mbfir_bloch_jvp_batch(ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None,
                                         lp(tsoff), p(d), p(t1), p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d),
                                         None, None, nscale, p(one), *q(m0), ndir, *q(v), *q(dm0), *q(m), *q(dm))
    big = 2 ** 31 - 1
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
             (dict(npulse=2, toff=L(0, 3, 1), tsoff=L(0, 1, 2)), "inconsistent offsets"), (dict(tsoff=L(0, 2)), "neither 1 nor"),
             (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"), (dict(poff=L(0, 0)), "empty item"),
             (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"), (dict(b1=None), "required array is null"),
             (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"),
             (dict(v=(d, None)), "direction or tangent plane is null"), (dict(dm=[outs[3], None, outs[5]]), "direction or tangent plane is null"),
             (dict(m0=(one, one, None)), "m0x, m0y and m0z"), (dict(dm0=(None, one, one)), "dm0x, dm0y and dm0z"),
             (dict(m=[None, outs[1], outs[2]]), "mx, my and mz"), (dict(ndir=0), "ndir must be at least 1"),
             (dict(foff=L(0, 2 ** 15), poff=L(0, 2 ** 15), ndir=2 ** 30), "overflows"))
    assert call() == 0
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_jvp_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0 and call(m=[None] * 3) == 0 and call(m0=(one, one, one), dm0=(one, one, one)) == 0
