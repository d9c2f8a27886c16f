"""The adjoint of the Bloch simulator with relaxation in b1, m0, the gradient waveform and the off-resonance on the device
(mbfir.bloch_vjp_gr_batch: k_bloch_vjp_gr_batch, k_bloch_vjp_gr_fold; mbfir.torchsim.bloch) against the long-double
stored-trajectory recursion of tests/blochgradg_ref.py, against mbfir.bloch_vjp_batch, against central differences of the shipped
forward call mbfir.bloch_batch, and for the bit-invariance of a pulse's results under the batch's composition.

Bounds of every comparison with the reference: blochgrad_ref.bound_b1 / bound_m0 for b1 and dL/dm0, and (blochgradg_ref.bound_gr,
bound_df) 1e-12 gamma dt_t sum_{s,f,p} |pos_{p,a}| (|cmx| + |cmy| + |cmz|) per entry (t, a) of the gr gradient and 1e-12 TWOPI
(sum_t dt_t) (|cmx| + |cmy| + |cmz|)(s, f, p) per entry of the df gradient: the forward tolerance of the Bloch tests carried through
the coordinate weight.  Where a gr bound is zero the result must be exactly zero.  tests/test_blochgradg_cpu.py holds the float64
reference within a hundredth of these bounds of the long-double one used here.

Measured on an MI355X (the worst over the 20 pulses of the three batches): see DESIGN section 8w."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochgradg_ref", os.path.join(ROOT, "tests", "blochgradg_ref.py"))
refg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refg)
ref = refg.base
SCALES = ref.SCALES


@functools.lru_cache(maxsize=None)
def _case(which):
    """which: 'own' (per-pulse grids), 'shared' (one grid) or 'sub' (2 .. 5 samples: every remainder of the sub-group of 3)"""
    pulses, dfs, dps, m0s, cots = refg.batch_sub() if which == "sub" else ref.batch(which == "shared")
    want = [refg.vjp_gr_scaled(p, df, dp, c, SCALES, m0, dtype=np.longdouble) for p, df, dp, c, m0 in zip(pulses, dfs, dps, cots, m0s)]
    return pulses, dfs, dps, m0s, cots, want


def _grids(which, dfs, dps):
    return (dfs[0], dps[0]) if which == "shared" else (dfs, dps)


@pytest.mark.parametrize("which", ["own", "shared", "sub"])
def test_device_is_the_longdouble_reference_and_agrees_with_the_b1_call(which):
    """Pulses of 1 .. 600 samples around the group of 8, its sub-groups of 3 and the 256-sample tile, on 1 .. 600 points, scales 1.0,
    0.0, 0.9, 1 - 3 gradient and position axes, tp scalar and per sample, random m0, phi = 0 at a zero b1 sample at df = 0 and
    position 0, and a 26 ms pulse at T2 = 1 ms.  The b1 part and dL/dm0 also against mbfir.bloch_vjp_batch within the same bounds
    (equality to the bit is reported, not promised), and grad_df=False against grad_df=True to the bit."""
    pulses, dfs, dps, m0s, cots, want = _case(which)
    D, P = _grids(which, dfs, dps)
    got = mbfir.bloch_vjp_gr_batch(pulses, D, P, cots, scales=SCALES, m0=m0s, grad_m0=True, grad_df=True)
    old = mbfir.bloch_vjp_batch(pulses, D, P, cots, scales=SCALES, m0=m0s, grad_m0=True)
    worst = {k: [0.0, 0.0] for k in ("b1", "gr", "m0", "df")}
    bits = True
    for q, ((g, gg, gm, gd), (wg, wgg, wm, wd), (og, om), p, dp, c) in enumerate(zip(got, want, old, pulses, dps, cots)):
        assert g.shape == wg.shape and gg.shape == wgg.shape == (len(wg), 3) and gd.shape == wd.shape, q
        assert all(a.shape == b.shape for a, b in zip(gm, wm)), q
        eb, bb = np.abs(g - wg).astype(np.float64), ref.bound_b1(p, c, SCALES)
        eg, bg = np.abs(gg - wgg).astype(np.float64), refg.bound_gr(p, dp, c)
        em, bm = max(float(np.abs(a - b).max()) for a, b in zip(gm, wm)), ref.bound_m0(c)
        ed, bd = np.abs(gd - wd).astype(np.float64), refg.bound_df(p, c)
        pos = bg > 0
        sg = float((eg[pos] / bg[pos]).max()) if pos.any() else 0.0
        for k, e, s in (("b1", eb.max(), (eb / bb).max()), ("gr", eg.max(), sg), ("m0", em, em / bm), ("df", ed.max(), (ed / bd).max())):
            worst[k] = [max(worst[k][0], float(e)), max(worst[k][1], float(s))]
        print("%s n %d points %s: |dev - ref| / bound  b1 %.3g  gr %.3g  m0 %.3g  df %.3g;  max|gr grad| %.3g, zero-bound gr "
              "entries %d" % (which, len(wg), c[0].shape[1:], (eb / bb).max(), sg, em / bm, (ed / bd).max(), np.abs(wgg).max(),
                              int((~pos).sum())))
        assert np.all(eb <= bb) and np.all(eg <= bg) and em <= bm and np.all(ed <= bd), q
        assert np.all(gg[~pos] == 0.0), q                               # an axis without positions, or position 0 alone
        assert np.all(np.abs(g - og) <= bb) and max(float(np.abs(a - b).max()) for a, b in zip(gm, om)) <= bm, q
        bits = bits and np.array_equal(g, og) and all(np.array_equal(a, b) for a, b in zip(gm, om))
    print("%s worst |dev - ref| and worst share of the bound: %s; b1 and m0 equal mbfir.bloch_vjp_batch to the bit: %s"
          % (which, {k: "%.3g / %.3g" % tuple(v) for k, v in worst.items()}, bits))
    lean = mbfir.bloch_vjp_gr_batch(pulses, D, P, cots, scales=SCALES, m0=m0s)
    half = mbfir.bloch_vjp_gr_batch(pulses, D, P, cots, scales=SCALES, m0=m0s, grad_df=True)
    for (g, gg, gm, gd), a, b in zip(got, lean, half):
        assert len(a) == 2 and len(b) == 3
        assert np.array_equal(a[0], g) and np.array_equal(a[1], gg) and np.array_equal(b[0], g) and np.array_equal(b[1], gg)
        assert np.array_equal(b[2], gd)


def test_zero_scale_gives_exact_zeros_in_b1_and_not_in_gr():
    pulses, dfs, dps, m0s, cots, _ = _case("own")
    res = mbfir.bloch_vjp_gr_batch(pulses, dfs, dps, [tuple(c[:1] for c in tri) for tri in cots], scales=(0.0,), m0=m0s)
    for q, (g, gg) in enumerate(res):
        assert np.array_equal(g, np.zeros(len(g))), q
        assert q % 4 == 0 or np.abs(gg).max() > 0, q                    # a scale multiplies b1, not gr (the 1 x 1 grid is position 0)


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, m0s, cots = [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, (n, 1 + q % 3)) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(np.stack([ref._grid(npos, 3.0) * (1.0 - 0.3 * a) for a in range(1 + (q + 1) % 3)], 1))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        cots.append(tuple(rng.standard_normal((3, 2, nf, npos))))
    kw = dict(scales=sc, grad_m0=True, grad_df=True)
    full = mbfir.bloch_vjp_gr_batch(pulses, dfs, dps, cots, m0=m0s, **kw)
    again = mbfir.bloch_vjp_gr_batch(pulses, dfs, dps, cots, m0=m0s, **kw)
    rev = mbfir.bloch_vjp_gr_batch(pulses[::-1], dfs[::-1], dps[::-1], cots[::-1], m0=m0s[::-1], **kw)[::-1]

    def same(a, b):
        return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))
                and np.array_equal(a[3], b[3]))
    for q in range(17):
        assert same(full[q], again[q]) and same(full[q], rev[q]), q
    for q in (0, 5, 16):
        alone, = mbfir.bloch_vjp_gr_batch([pulses[q]], [dfs[q]], [dps[q]], [cots[q]], m0=[m0s[q]], **kw)
        assert same(alone, full[q]), q


def test_the_vjp_is_the_directional_derivative_of_the_shipped_forward():
    """L = sum (w . m)^2 / 2 on mbfir.bloch_batch at scales 0.9, 1.0, 1.1, a 64-sample pulse with two gradient axes on 3 x 85
    points with T2 = the duration: the central difference along a random unit direction of gr (h = 1e-6) equals <grad_gr, d>, and
    the one along a shift of every df (h = 1e-3 Hz) equals the sum of grad_df, to 1e-6 relative (truncation h^2 |L'''| and rounding
    eps_machine L / h are both far below it)."""
    sc = (0.9, 1.0, 1.1)
    rng = np.random.default_rng(90)
    n, dur = 64, 4e-3
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (np.pi / 2 / (ref.GAMMA_H1 * dur))
    gr = rng.uniform(0.5, 1.5, (n, 2)) * 0.05
    df, dp = ref._grid(3, 100.0), np.stack([ref._grid(85, 3.0), ref._grid(85, 1.0)[::-1]], 1)
    w = rng.standard_normal((3, 3, 3, 85))
    m0 = tuple(rng.uniform(-0.5, 0.5, (3, 3, 85)))

    def fwd(g, f):
        m, = mbfir.bloch_batch([(b1, g, dur / n, 1.0, dur, "H-1")], f, dp, scales=sc, m0=m0)
        r = w[0] * m[0] + w[1] * m[1] + w[2] * m[2]
        return 0.5 * float((r * r).sum()), tuple(w[c] * r for c in range(3))
    L0, cot = fwd(gr, df)
    (_, gg, gd), = mbfir.bloch_vjp_gr_batch([(b1, gr, dur / n, 1.0, dur, "H-1")], df, dp, [cot], scales=sc, m0=m0, grad_df=True)
    d = rng.standard_normal((n, 2))
    d /= np.linalg.norm(d)
    dd, fd = float((gg[:, :2] * d).sum()), (fwd(gr + 1e-6 * d, df)[0] - fwd(gr - 1e-6 * d, df)[0]) / 2e-6
    ds, fs = float(gd.sum()), (fwd(gr, df + 1e-3)[0] - fwd(gr, df - 1e-3)[0]) / 2e-3
    print("loss %.6g; gr: <g, d> %.9g central difference %.9g relative %.3g; df: sum %.9g central difference %.9g relative %.3g"
          % (L0, dd, fd, abs(fd - dd) / abs(dd), ds, fs, abs(fs - ds) / abs(ds)))
    assert np.array_equal(gg[:, 2], np.zeros(n))                        # no position has a z coordinate
    assert abs(fd - dd) <= 1e-6 * abs(dd) and abs(fs - ds) <= 1e-6 * abs(ds)


def test_torchsim_bloch_passes_gradcheck_in_gr_and_df_and_keeps_the_b1_path():
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(6) + 1j * rng.standard_normal(6)) * (0.5 / (gamma * dt))
    g0 = rng.uniform(0.5, 1.5, (6, 2)) * 0.05
    d0, dp = np.array([-100.0, 0.0]), np.array([[-1.0, 0.5], [0.0, 0.0], [1.5, -0.7]])
    sc = (1.0, 0.8)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    gr = torch.tensor(g0, dtype=torch.float64, requires_grad=True)
    df = torch.tensor(d0, dtype=torch.float64, requires_grad=True)

    def f(b, g, d):
        return mbfir.torchsim.bloch(b, g, dt, 1.0, 1e-3, d, dp, nucleus="H-1", scales=sc)
    assert torch.autograd.gradcheck(f, (b1, gr, df))
    cot = tuple(rng.standard_normal((3, 2, 2, 3)))                    # L = sum c . m: the cotangents are c exactly
    sum((torch.tensor(c) * o).sum() for c, o in zip(cot, f(b1, gr, df))).backward()
    (wg, wgg, wd), = mbfir.bloch_vjp_gr_batch([(b0, g0, dt, 1.0, 1e-3, "H-1")], d0, dp, [cot], scales=sc, grad_df=True)
    assert np.array_equal(b1.grad.numpy(), wg) and np.array_equal(gr.grad.numpy(), wgg[:, :2])
    assert np.array_equal(df.grad.numpy(), wd.sum(axis=(0, 2)))
    # when gr and df do not require grad, b1.grad is today's path to the bit
    b2 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    sum((torch.tensor(c) * o).sum() for c, o in zip(cot, f(b2, g0, d0))).backward()
    og, = mbfir.bloch_vjp_batch([(b0, g0, dt, 1.0, 1e-3, "H-1")], d0, dp, [cot], scales=sc)
    assert np.array_equal(b2.grad.numpy(), og)


def test_errors_of_the_raw_call_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(9)]

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
             m0=(None, None, None), cot=(one, one, one), grad=outs[:2], gm0=outs[2:5], gg=outs[5:8], gdf=outs[8]):
        o = [p(v) if v is not None else None for v in (*m0, *cot, *grad, *gm0, *gg, gdf)]
        return lib.mbfir_bloch_vjp_gr_batch(ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None,
                                            lp(tsoff), p(d), p(t1), p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d),
                                            None, None, nscale, p(one), *o)
    big = 2 ** 31 - 1
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
             (dict(npulse=2, toff=L(0, 3, 1), tsoff=L(0, 1, 2)), "inconsistent offsets"), (dict(tsoff=L(0, 2)), "neither 1 nor"),
             (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"), (dict(poff=L(0, 0)), "empty item"),
             (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"), (dict(b1=None), "required array is null"),
             (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"),
             # 2^30 workgroups x 2^25 samples: the forward sizes fit, the partials and checkpoints of the adjoint do not
             (dict(toff=L(0, 2 ** 25), foff=L(0, 2 ** 19), poff=L(0, 2 ** 19)), "overflows"),
             (dict(cot=(one, None, one)), "cotangent or gradient plane is null"),
             (dict(grad=[outs[0], None]), "cotangent or gradient plane is null"),
             (dict(gg=[outs[5], None, outs[7]]), "(ggx, ggy, ggz) is null"), (dict(gg=[None, outs[6], outs[7]]), "(ggx, ggy, ggz) is null"),
             (dict(gg=[outs[5], outs[6], None]), "(ggx, ggy, ggz) is null"),
             (dict(m0=(one, one, None)), "m0x, m0y and m0z"), (dict(gm0=[None, outs[3], outs[4]]), "gm0x, gm0y and gm0z"))
    assert call() == 0
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_vjp_gr_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0 and call(gm0=[None] * 3) == 0 and call(m0=(one, one, one)) == 0 and call(gdf=None) == 0
