"""The adjoint of the Bloch simulator's steady state in b1, the gradient waveform and the off-resonance on the device
(mbfir.bloch_ss_vjp_gr_batch: k_bloch_ss_vjp_gr_batch, k_bloch_vjp_gr_fold; mbfir.torchsim.bloch(steady_state=True)) against the
float64 NumPy reference of tests/blochssg_ref.py, against mbfir.bloch_ss_vjp_batch and the shipped forward call
mbfir.bloch_batch(mode=1) (bits of M, central differences), against the composition of the shipped transient calls, and for the
bit-invariance of a pulse's results under the batch's composition.

Bounds of every comparison with the reference (blochssg_ref): with kappa = max ||(I - A)^-1||_2 over the pulse's points and scales,
blochgrad_ref.bound_b1 times kappa per b1 entry, 1e-12 kappa^2 per entry of M, blochgradg_ref.bound_gr times kappa per entry (t, a)
of the gr gradient and blochgradg_ref.bound_df times kappa^2 per entry of the df gradient.  Where a gr bound is zero the result must
be exactly zero.  tests/test_blochssg_cpu.py holds the float64 reference within a hundredth of these of its long-double twin.

Measured on an MI355X (the worst over the 20 periods of the three batches): see DESIGN section 8x."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochssg_ref", os.path.join(ROOT, "tests", "blochssg_ref.py"))
refg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refg)
ref = refg.ss
SCALES = ref.SCALES


@functools.lru_cache(maxsize=None)
def _case(which):
    """which: 'own' (per-pulse grids), 'shared' (one grid) or 'sub' (2 .. 5 samples: every remainder of the sub-group of 3)"""
    pulses, dfs, dps, cots = refg.batch_sub() if which == "sub" else ref.batch(which == "shared")
    ks = [ref.kappa(p, df, dp, SCALES) for p, df, dp in zip(pulses, dfs, dps)]
    want = [refg.ss_vjp_gr_scaled(p, df, dp, c, SCALES) for p, df, dp, c in zip(pulses, dfs, dps, cots)]
    return pulses, dfs, dps, cots, ks, want


def _grids(which, dfs, dps):
    return (dfs[0], dps[0]) if which == "shared" else (dfs, dps)


def _shares(got, want, p, dp, c, sc, k):
    """The largest |got - want| / bound of (b1, gr, df, M); gr over the entries with a positive bound, and whether the others are 0"""
    (g, gg, gd, M), (wg, wgg, wd, wM) = got, want
    bg = refg.bound_gr(p, dp, c, k)
    pos = bg > 0
    bb = refg.bound_b1(p, c, sc, k) + np.zeros(len(g))
    sb = float((np.abs(g - wg)[bb > 0] / bb[bb > 0]).max()) if (bb > 0).any() else 0.0          # scale 0 alone: exact zeros, held there
    sg = float((np.abs(gg - wgg)[pos] / bg[pos]).max()) if pos.any() else 0.0
    sd = float((np.abs(gd - wd) / refg.bound_df(p, c, k)).max())
    sm = max(float(np.abs(a - b).max()) for a, b in zip(M, wM)) / refg.bound_m(k)
    return (sb, sg, sd, sm), bool(np.all(gg[~pos] == 0.0)), int((~pos).sum())


@pytest.mark.parametrize("which", ["own", "shared", "sub"])
def test_device_is_the_reference_and_agrees_with_the_b1_call(which):
    """Periods of 1 .. 600 samples around the group of 8, its sub-groups of 3 and the 256-sample tile, on 1 .. 600 points, scales 1.0,
    0.0, 0.9, kappa from 4.5 to 5001, 1 - 3 gradient and position axes, tp scalar and per sample with a dead time.  M has
    bloch_batch(mode=1)'s bits; the b1 part lies within its bound of mbfir.bloch_ss_vjp_batch (equality to the bit is reported, not
    promised); grad_df and steady change no bit of the other results."""
    pulses, dfs, dps, cots, ks, want = _case(which)
    D, P = _grids(which, dfs, dps)
    got = mbfir.bloch_ss_vjp_gr_batch(pulses, D, P, cots, scales=SCALES, grad_df=True, steady=True)
    old = mbfir.bloch_ss_vjp_batch(pulses, D, P, cots, scales=SCALES)
    fwd = mbfir.bloch_batch(pulses, D, P, scales=SCALES, mode=1)
    worst, bits = np.zeros(4), True
    for q, (r, w, og, p, dp, c, k) in enumerate(zip(got, want, old, pulses, dps, cots, ks)):
        g, gg, gd, M = r
        assert g.shape == w[0].shape and gg.shape == w[1].shape == (len(g), 3) and gd.shape == w[2].shape == c[0].shape, q
        assert all(a.shape == b.shape for a, b in zip(M, w[3])), q
        s, zeros, nz = _shares(r, w, p, dp, c, SCALES, k)
        worst = np.maximum(worst, s)
        print("%s n %d points %s kappa %.4g: |dev - ref| / bound  b1 %.3g  gr %.3g  df %.3g  M %.3g;  max|gr grad| %.3g, zero-bound gr "
              "entries %d" % ((which, len(g), c[0].shape[1:], k) + s + (np.abs(w[1]).max(), nz)))
        assert max(s) <= 1, q
        assert zeros, q                                                 # an axis without positions, or position 0 alone
        assert all(np.array_equal(M[i], fwd[q][i]) for i in range(3)), q
        assert np.all(np.abs(g - og) <= refg.bound_b1(p, c, SCALES, k)), q
        bits = bits and np.array_equal(g, og)
    print("%s worst share of the bound: b1 %.3g, gr %.3g, df %.3g, M %.3g; b1 equals mbfir.bloch_ss_vjp_batch to the bit: %s"
          % ((which,) + tuple(worst) + (bits,)))
    lean = mbfir.bloch_ss_vjp_gr_batch(pulses, D, P, cots, scales=SCALES)
    half = mbfir.bloch_ss_vjp_gr_batch(pulses, D, P, cots, scales=SCALES, grad_df=True)
    stdy = mbfir.bloch_ss_vjp_gr_batch(pulses, D, P, cots, scales=SCALES, steady=True)
    for (g, gg, gd, M), a, b, c in zip(got, lean, half, stdy):
        assert len(a) == 2 and len(b) == 3 and len(c) == 3
        assert all(np.array_equal(v[0], g) and np.array_equal(v[1], gg) for v in (a, b, c))
        assert np.array_equal(b[2], gd) and all(np.array_equal(u, v) for u, v in zip(c[2], M))


def test_zero_scale_gives_exact_zeros_in_b1_and_the_reference_in_gr_and_df():
    """Scale 0 alone: equilibrium is the fixed point of a z rotation, so gr and df gradients are zero analytically; they are held to
    their bounds of the reference, not to exact zeros"""
    pulses, dfs, dps, cots, _, _ = _case("own")
    sc = (0.0,)
    c1 = [tuple(c[:1] for c in tri) for tri in cots]
    res = mbfir.bloch_ss_vjp_gr_batch(pulses, dfs, dps, c1, scales=sc, grad_df=True, steady=True)
    for q, (r, p, df, dp, c) in enumerate(zip(res, pulses, dfs, dps, c1)):
        assert np.array_equal(r[0], np.zeros(len(r[0]))), q
        k = ref.kappa(p, df, dp, sc)
        s, zeros, _ = _shares(r, refg.ss_vjp_gr_scaled(p, df, dp, c, sc), p, dp, c, sc, k)
        print("n %d kappa %.4g: |dev - ref| / bound gr %.3g df %.3g M %.3g; max|gr grad| %.3g max|df grad| %.3g"
              % (len(r[0]), k, s[1], s[2], s[3], np.abs(r[1]).max(), np.abs(r[2]).max()))
        assert s[1] <= 1 and s[2] <= 1 and s[3] <= 1 and zeros, q


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, cots = [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, (n, 1 + q % 3)) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(np.stack([ref._grid(npos, 3.0) * (1.0 - 0.3 * a) for a in range(1 + (q + 1) % 3)], 1))
        cots.append(tuple(rng.standard_normal((3, 2, nf, npos))))
    kw = dict(scales=sc, grad_df=True, steady=True)
    full = mbfir.bloch_ss_vjp_gr_batch(pulses, dfs, dps, cots, **kw)
    again = mbfir.bloch_ss_vjp_gr_batch(pulses, dfs, dps, cots, **kw)
    rev = mbfir.bloch_ss_vjp_gr_batch(pulses[::-1], dfs[::-1], dps[::-1], cots[::-1], **kw)[::-1]

    def same(a, b):
        return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
                and all(np.array_equal(u, v) for u, v in zip(a[3], b[3])))
    for q in range(17):
        assert all(np.all(np.isfinite(v)) for v in full[q][:3]), q
        assert same(full[q], again[q]) and same(full[q], rev[q]), q
    for q in (0, 5, 16):
        alone, = mbfir.bloch_ss_vjp_gr_batch([pulses[q]], [dfs[q]], [dps[q]], [cots[q]], **kw)
        assert same(alone, full[q]), q


@functools.lru_cache(maxsize=None)
def _problem():
    """The period of tests/test_blochss_gpu.py: 64 samples of 10 us and a dead time of 160 us at T1 = 0.1 s, T2 = 0.03 s on 3 x 85
    points (kappa 119), weights for w . M over three scales"""
    rng = np.random.default_rng(7)
    n, gamma = 65, ref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 / (gamma * 64e-5))
    b1[20], b1[-1] = 0.0, 0.0
    gr = np.append(rng.uniform(0.5, 1.5, 64) * 0.1, 0.0)
    tp = np.append(np.full(64, 1e-5), 1.6e-4)
    pulse, df, dp = (b1, gr, tp, 0.1, 0.03, "H-1"), ref._grid(3, 100.0), ref._grid(85, 3.0)
    return pulse, df, dp, rng.standard_normal((3, 3, 3, 85)), ref.kappa(pulse, df, dp, (0.9, 1.0, 1.1))


def test_the_vjp_is_the_directional_derivative_of_the_shipped_steady_state():
    """L = sum (w . M)^2 / 2 on mbfir.bloch_batch(mode=1) at scales 0.9, 1.0, 1.1: the central difference along a random unit
    direction of gr (h = 1e-5 G/cm) equals <grad_gr, d>, and the one along a common shift of df (h = 1e-2 Hz) equals the sum of
    grad_df, to 1e-6 relative (the float64 reference gives 8.5e-10 and 2.8e-9 at these steps, which sit at the minimum over h)"""
    pulse, df, dp, w, k = _problem()
    sc = (0.9, 1.0, 1.1)
    assert k <= 300

    def fwd(g, f):
        m, = mbfir.bloch_batch([(pulse[0], g) + pulse[2:]], f, dp, scales=sc, mode=1)
        r = w[0] * m[0] + w[1] * m[1] + w[2] * m[2]
        return 0.5 * float((r * r).sum()), tuple(w[c] * r for c in range(3))
    gr = pulse[1]
    L0, cot = fwd(gr, df)
    (_, gg, gd), = mbfir.bloch_ss_vjp_gr_batch([pulse], df, dp, [cot], scales=sc, grad_df=True)
    d = np.random.default_rng(91).standard_normal(len(gr))
    d /= np.linalg.norm(d)
    dd, fd = float((gg[:, 0] * d).sum()), (fwd(gr + 1e-5 * d, df)[0] - fwd(gr - 1e-5 * d, df)[0]) / 2e-5
    ds, fs = float(gd.sum()), (fwd(gr, df + 1e-2)[0] - fwd(gr, df - 1e-2)[0]) / 2e-2
    print("kappa %.4g loss %.6g; gr: <g, d> %.9g central difference %.9g relative %.3g; df: sum %.9g central difference %.9g relative %.3g"
          % (k, L0, dd, fd, abs(fd - dd) / abs(dd), ds, fs, abs(fs - ds) / abs(ds)))
    assert np.array_equal(gg[:, 1:], np.zeros((len(gr), 2)))            # no position has a y or z coordinate
    assert abs(fd - dd) <= 1e-6 * abs(dd) and abs(fs - ds) <= 1e-6 * abs(ds)


@pytest.mark.parametrize("q", [3, 6])
def test_the_fused_adjoint_is_the_composition_of_the_shipped_calls(q):
    """The 9-sample (kappa 5001) and the 257-sample (kappa 3001) period of blochss_ref.batch: per scale bloch_batch(mode=1) for M,
    three grad_m0 adjoints with unit cotangents for the rows of A, NumPy solves for lambda = (I - A)^-T c, and bloch_vjp_gr_batch
    from M; gr summed over the scales; gr and df within twice their bounds."""
    pulses, dfs, dps, cots, ks, _ = _case("own")
    p, df, dp, cot, k = pulses[q], dfs[q], dps[q], cots[q], ks[q]
    (_, fg, fd), = mbfir.bloch_ss_vjp_gr_batch([p], df, dp, [cot], scales=SCALES, grad_df=True)
    nf, npos = cot[0].shape[1:]
    cg, cd = np.zeros((len(p[0]), 3)), np.zeros_like(fd)
    for si, s in enumerate(SCALES):
        (Mx, My, Mz), = mbfir.bloch_batch([p], df, dp, scales=(s,), mode=1)
        M = (Mx[0], My[0], Mz[0])
        unit = [tuple(np.full((1, nf, npos), 1.0 if c == i else 0.0) for c in range(3)) for i in range(3)]
        rows = mbfir.bloch_vjp_batch([p] * 3, df, dp, unit, scales=(s,), m0=M, grad_m0=True)
        A = np.stack([np.stack([rows[i][1][j][0] for j in range(3)], -1) for i in range(3)], -2)          # (nf, npos, 3, 3): A[i, j]
        c = np.stack([cot[i][si] for i in range(3)], -1)[..., None]
        lam = np.linalg.solve(np.swapaxes(np.eye(3) - A, -1, -2), c)[..., 0]
        (_, g3, gd), = mbfir.bloch_vjp_gr_batch([p], df, dp, [tuple(lam[None, ..., i] for i in range(3))], scales=(s,), m0=M,
                                                grad_df=True)
        cg += g3
        cd[si] = gd[0]
    eg, bg = np.abs(fg - cg), refg.bound_gr(p, dp, cot, k)
    ed, bd = np.abs(fd - cd), refg.bound_df(p, cot, k)
    pos = bg > 0
    print("n %d kappa %.4g: |fused - composition| / bound gr %.3g df %.3g; max|gr grad| %.3g max|df grad| %.3g"
          % (len(p[0]), k, (eg[pos] / bg[pos]).max(), (ed / bd).max(), np.abs(fg).max(), np.abs(fd).max()))
    assert np.all(eg <= 2 * bg) and np.all(ed <= 2 * bd)


def test_torchsim_steady_state_passes_gradcheck_in_b1_gr_and_df_and_carries_the_device_bits():
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(7) + 1j * rng.standard_normal(7)) * (0.5 / (gamma * dt))
    b0[-1] = 0.0
    g0 = rng.uniform(0.5, 1.5, (7, 2)) * 0.05
    g0[-1] = 0.0
    tp = np.append(np.full(6, dt), 2e-3)
    d0, dp = np.array([-100.0, 30.0]), np.array([[-1.0, 0.5], [0.0, 0.0], [1.5, -0.7]])
    sc = (1.0, 0.8)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    gr = torch.tensor(g0, dtype=torch.float64, requires_grad=True)
    df = torch.tensor(d0, dtype=torch.float64, requires_grad=True)

    def f(b, g, d):
        return mbfir.torchsim.bloch(b, g, tp, 0.13, 0.03, d, dp, nucleus="H-1", scales=sc, steady_state=True)
    assert torch.autograd.gradcheck(f, (b1, gr, df))
    pulse = (b0, g0, tp, 0.13, 0.03, "H-1")
    want, = mbfir.bloch_batch([pulse], d0, dp, scales=sc, mode=1)
    res = f(b1, gr, df)
    assert all(np.array_equal(o.detach().numpy(), w) for o, w in zip(res, want))
    cot = tuple(rng.standard_normal((3, 2, 2, 3)))                    # L = sum c . M: the cotangents are c exactly
    sum((torch.tensor(c) * o).sum() for c, o in zip(cot, res)).backward()
    (wg, wgg, wd), = mbfir.bloch_ss_vjp_gr_batch([pulse], d0, dp, [cot], scales=sc, grad_df=True)
    assert np.array_equal(b1.grad.numpy(), wg) and np.array_equal(gr.grad.numpy(), wgg[:, :2])
    assert np.array_equal(df.grad.numpy(), wd.sum(axis=(0, 2)))
    # when gr and df do not require grad, b1.grad is today's path to the bit
    b2 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    sum((torch.tensor(c) * o).sum() for c, o in zip(cot, f(b2, g0, d0))).backward()
    og, = mbfir.bloch_ss_vjp_batch([pulse], d0, dp, [cot], scales=sc)
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
             cot=(one, one, one), grad=outs[:2], m=outs[2:5], gg=outs[5:8], gdf=outs[8]):
        o = [p(v) if v is not None else None for v in (*cot, *grad, *m, *gg, gdf)]
        return lib.mbfir_bloch_ss_vjp_gr_batch(ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None,
                                               lp(tsoff), p(d), p(t1), p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff),
                                               p(d), None, None, nscale, p(one), *o)
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
             (dict(gg=[outs[5], outs[6], None]), "(ggx, ggy, ggz) is null"), (dict(m=[None, outs[3], outs[4]]), "mx, my and mz"))
    assert call() == 0
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_ss_vjp_gr_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0 and call(m=[None] * 3) == 0 and call(gdf=None) == 0
