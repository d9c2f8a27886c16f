"""The adjoint and the tangent of the Bloch simulator's steady state on the device (mbfir.bloch_ss_vjp_batch: k_bloch_ss_vjp_batch,
k_bloch_vjp_fold; mbfir.bloch_ss_jvp_batch: k_bloch_ss_jvp_batch; mbfir.torchsim.bloch(steady_state=True)) against the NumPy
reference of tests/blochss_ref.py, against the shipped forward call mbfir.bloch_batch(mode=1) (bits of M, central differences),
against each other (the dot-product identity), against the composition of the shipped transient calls, and for the bit-invariance
of a pulse's results under the batch's composition.

Bounds of every comparison with the reference (blochss_ref): with kappa = max ||(I - A)^-1||_2 over the pulse's points and scales,
blochgrad_ref.bound_b1 times kappa per b1 entry, 1e-12 kappa^2 per entry of M and 1e-12 kappa^2 max|s| gamma sum_t dt_t |v_t| per
tangent entry; tests/test_blochss_cpu.py holds the float64 reference within a hundredth of these of its long-double twin."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochss_ref", os.path.join(ROOT, "tests", "blochss_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
SCALES = ref.SCALES
KMANY = 9                                             # a full group of directions and a partial one


@functools.lru_cache(maxsize=None)
def _case(shared):
    pulses, dfs, dps, cots = ref.batch(shared)
    vs, _ = ref.directions(pulses, dfs, dps, KMANY)
    ks = [ref.kappa(p, df, dp, SCALES) for p, df, dp in zip(pulses, dfs, dps)]
    adj = [ref.ss_vjp_scaled(p, df, dp, c, SCALES) for p, df, dp, c in zip(pulses, dfs, dps, cots)]
    tan = [ref.ss_jvp(p, df, dp, v, SCALES)[1] for p, df, dp, v in zip(pulses, dfs, dps, vs)]
    return pulses, dfs, dps, cots, vs, ks, adj, tan


@pytest.mark.parametrize("shared", [False, True])
def test_device_gradient_steady_state_and_tangents_are_the_reference(shared):
    """Eight periods of 1 .. 600 samples around the group of 8 and the 256-sample tile, on 1 .. 600 points, scales 1.0, 0.0, 0.9,
    kappa from 4.5 to 5001 (blochss_ref.batch); tangents at K = 1 and K = 9; M of both calls has bloch_batch(mode=1)'s bits."""
    pulses, dfs, dps, cots, vs, ks, adj, tan = _case(shared)
    df, dp = (dfs[0], dps[0]) if shared else (dfs, dps)
    fwd = mbfir.bloch_batch(pulses, df, dp, scales=SCALES, mode=1)
    got = mbfir.bloch_ss_vjp_batch(pulses, df, dp, cots, scales=SCALES, steady=True)
    many = mbfir.bloch_ss_jvp_batch(pulses, df, dp, vs, scales=SCALES)
    one = mbfir.bloch_ss_jvp_batch(pulses, df, dp, [v[0] for v in vs], scales=SCALES)
    only = mbfir.bloch_ss_vjp_batch(pulses, df, dp, cots, scales=SCALES)
    for q, (p, c, v, k) in enumerate(zip(pulses, cots, vs, ks)):
        (g, M), (wg, wM) = got[q], adj[q]
        assert g.shape == wg.shape and all(a.shape == b.shape for a, b in zip(M, wM)), q
        sg = float((np.abs(g - wg) / ref.bound_b1(p, c, SCALES, k)).max())
        sm = max(float(np.abs(a - b).max()) for a, b in zip(M, wM)) / ref.bound_m(k)
        bj = ref.bound_jvp(p, v, SCALES, k)[:, None]
        s9 = max(float((np.abs(a - b) / bj).max()) for a, b in zip(many[q][1], tan[q]))
        s1 = max(float((np.abs(a - b[0]) / bj[0]).max()) for a, b in zip(one[q][1], tan[q]))
        print("shared %s n %d points %s kappa %.4g: |dev - ref| / bound: gradient %.3g, M %.3g, tangent K=9 %.3g, K=1 %.3g; max|g| %.3g"
              % (shared, len(wg), c[0].shape[1:], k, sg, sm, s9, s1, np.abs(wg).max()))
        assert many[q][1][0].shape == (KMANY,) + c[0].shape and one[q][1][0].shape == c[0].shape, q
        assert sg <= 1 and sm <= 1 and s9 <= 1 and s1 <= 1, q
        for c3 in range(3):
            assert np.array_equal(M[c3], fwd[q][c3]) and np.array_equal(many[q][0][c3], fwd[q][c3]), q
            assert np.array_equal(one[q][0][c3], fwd[q][c3]), q
        assert np.array_equal(g, only[q]), q


def test_zero_scale_gives_an_exactly_zero_gradient():
    pulses, dfs, dps, cots = ref.batch(False)
    res = mbfir.bloch_ss_vjp_batch(pulses, dfs, dps, [tuple(c[:1] for c in tri) for tri in cots], scales=(0.0,))
    for g in res:
        assert np.array_equal(g, np.zeros(len(g)))


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(50)
    lengths = [int(v) for v in rng.integers(1, 700, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, cots, vs = [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, dt, 0.8, 3e-3 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(ref._grid(npos, 3.0))
        cots.append(tuple(rng.standard_normal((3, 2, nf, npos))))
        vs.append((rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))) * np.abs(b1).max())

    def run(idx):
        sel = lambda a: [a[i] for i in idx]
        adj = mbfir.bloch_ss_vjp_batch(sel(pulses), sel(dfs), sel(dps), sel(cots), scales=sc, steady=True)
        tan = mbfir.bloch_ss_jvp_batch(sel(pulses), sel(dfs), sel(dps), sel(vs), scales=sc)
        return [(a[0],) + tuple(a[1]) + tuple(t[0]) + tuple(t[1]) for a, t in zip(adj, tan)]

    def same(a, b):
        return all(np.array_equal(u, v) for u, v in zip(a, b))
    order = list(range(17))
    full, again, rev = run(order), run(order), run(order[::-1])[::-1]
    for q in range(17):
        assert same(full[q], again[q]) and same(full[q], rev[q]), q
    for q in (0, 5, 16):
        assert same(run([q])[0], full[q]), q


@functools.lru_cache(maxsize=None)
def _problem():
    """64 samples of 10 us and a dead time of 160 us at T1 = 0.1 s, T2 = 0.03 s on 3 x 85 points (tests/test_blochss_cpu.py says why
    the dead time is short), weights for w . M over three scales"""
    rng = np.random.default_rng(7)
    n, gamma = 65, ref.GAMMA_H1
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 / (gamma * 64e-5))
    b1[20], b1[-1] = 0.0, 0.0
    gr = np.append(rng.uniform(0.5, 1.5, 64) * 0.1, 0.0)
    tp = np.append(np.full(64, 1e-5), 1.6e-4)
    pulse, df, dp = (b1, gr, tp, 0.1, 0.03, "H-1"), ref._grid(3, 100.0), ref._grid(85, 3.0)
    return pulse, df, dp, rng.standard_normal((3, 3, 3, 85)), ref.kappa(pulse, df, dp, (0.9, 1.0, 1.1))


def _loss(b1):
    pulse, df, dp, w, _ = _problem()
    m, = mbfir.bloch_batch([(b1,) + pulse[1:]], df, dp, scales=(0.9, 1.0, 1.1), mode=1)
    r = w[0] * m[0] + w[1] * m[1] + w[2] * m[2]
    return 0.5 * float((r * r).sum()), tuple(w[c] * r for c in range(3))


def test_the_vjp_is_the_gradient_of_the_shipped_steady_state():
    """L = sum (w . M)^2 / 2 on mbfir.bloch_batch(mode=1) at scales 0.9, 1.0, 1.1: the directional derivative along g / |g| equals
    |g| to 1e-6 relative (the bound of the transient adjoint's test; the CPU reference gives 3.3e-8 on this period at 5 x 7 points)"""
    pulse, df, dp, _, k = _problem()
    assert k <= 300
    L0, cot = _loss(pulse[0])
    g, = mbfir.bloch_ss_vjp_batch([pulse], df, dp, [cot], scales=(0.9, 1.0, 1.1))
    nrm = float(np.linalg.norm(g))
    d, eps = g / nrm, 1e-5 * float(np.linalg.norm(pulse[0]))
    fd = (_loss(pulse[0] + eps * d)[0] - _loss(pulse[0] - eps * d)[0]) / (2 * eps)
    print("kappa %.4g, loss %.6g, |g| %.9g, central difference %.9g, relative difference %.3g" % (k, L0, nrm, fd, abs(fd - nrm) / nrm))
    assert abs(fd - nrm) <= 1e-6 * nrm


def test_device_tangent_and_adjoint_satisfy_the_dot_product_identity():
    """<c, J v> = <J' c, v> to 1e-10 relative on the same problem, three directions of the pulse's size"""
    pulse, df, dp, _, _ = _problem()
    sc = (0.9, 1.0, 1.1)
    _, cot = _loss(pulse[0])
    rng = np.random.default_rng(8)
    v = (rng.standard_normal((3, 65)) + 1j * rng.standard_normal((3, 65))) * np.abs(pulse[0]).max()
    g, = mbfir.bloch_ss_vjp_batch([pulse], df, dp, [cot], scales=sc)
    (_, dM), = mbfir.bloch_ss_jvp_batch([pulse], df, dp, [v], scales=sc)
    for k in range(3):
        lhs = float(sum((cot[c] * dM[c][k]).sum() for c in range(3)))
        rhs = float((np.conj(g) * v[k]).real.sum())
        print("direction %d: lhs %.12g rhs %.12g relative difference %.3g" % (k, lhs, rhs, abs(lhs - rhs) / max(abs(lhs), abs(rhs))))
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), k


@pytest.mark.parametrize("q", [3, 6])
def test_the_fused_adjoint_is_the_composition_of_the_shipped_calls(q):
    """The 9-sample (kappa 5001) and the 257-sample (kappa 3001) period of blochss_ref.batch: bloch_batch(mode=1) for M, three grad_m0
    adjoints with unit cotangents for the rows of A, NumPy solves for lambda = (I - A)^-T c, and bloch_vjp_batch from M, scale by
    scale (one m0 serves every scale there); within twice the gradient's bound."""
    pulses, dfs, dps, cots, _, ks, _, _ = _case(False)
    p, df, dp, cot, k = pulses[q], dfs[q], dps[q], cots[q], ks[q]
    fused, = mbfir.bloch_ss_vjp_batch([p], df, dp, [cot], scales=SCALES)
    (Mx, My, Mz), = mbfir.bloch_batch([p], df, dp, scales=SCALES, mode=1)
    nf, npos = Mx.shape[1:]
    comp = np.zeros(len(p[0]), dtype=np.complex128)
    for si, s in enumerate(SCALES):
        M = (Mx[si], My[si], Mz[si])
        unit = [tuple(np.full((1, nf, npos), 1.0 if c == i else 0.0) for c in range(3)) for i in range(3)]
        rows = mbfir.bloch_vjp_batch([p] * 3, df, dp, unit, scales=(s,), m0=M, grad_m0=True)
        A = np.stack([np.stack([rows[i][1][j][0] for j in range(3)], -1) for i in range(3)], -2)          # (nf, npos, 3, 3): A[i, j]
        c = np.stack([cot[i][si] for i in range(3)], -1)[..., None]
        lam = np.linalg.solve(np.swapaxes(np.eye(3) - A, -1, -2), c)[..., 0]
        g, = mbfir.bloch_vjp_batch([p], df, dp, [tuple(lam[None, ..., i] for i in range(3))], scales=(s,), m0=M)
        comp += g
    share = float((np.abs(fused - comp) / ref.bound_b1(p, cot, SCALES, k)).max())
    print("n %d kappa %.4g: |fused - composition| / bound %.3g, max|g| %.3g" % (len(p[0]), k, share, np.abs(fused).max()))
    assert share <= 2


def test_torchsim_steady_state_passes_gradcheck_and_carries_the_device_bits():
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = ref.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(7) + 1j * rng.standard_normal(7)) * (0.5 / (gamma * dt))
    b0[-1] = 0.0
    gr = np.append(rng.uniform(0.5, 1.5, 6) * 0.05, 0.0)
    tp = np.append(np.full(6, dt), 2e-3)
    df, dp = np.array([-100.0, 0.0]), np.array([-1.0, 0.0, 1.5])
    sc = (1.0, 0.8)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)

    def f(b, forward_mode=True):
        return mbfir.torchsim.bloch(b, gr, tp, 0.1, 0.02, df, dp, nucleus="H-1", scales=sc, forward_mode=forward_mode, steady_state=True)
    assert torch.autograd.gradcheck(lambda b: f(b, False), (b1,))
    assert torch.autograd.gradcheck(f, (b1,), check_forward_ad=True)
    pulse = (b0, gr, tp, 0.1, 0.02, "H-1")
    v = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    out, tan = torch.func.jvp(f, (b1.detach(),), (torch.tensor(v),))
    (wm, wt), = mbfir.bloch_ss_jvp_batch([pulse], df, dp, [v], scales=sc)
    want, = mbfir.bloch_batch([pulse], df, dp, scales=sc, mode=1)
    assert out[0].dtype == torch.float64 and tuple(out[0].shape) == (2, 2, 3)
    assert all(np.array_equal(o.numpy(), w) for o, w in zip(out, want))
    assert all(np.array_equal(t.numpy(), w) for t, w in zip(tan, wt))
    res = f(b1, False)
    assert all(np.array_equal(o.detach().numpy(), w) for o, w in zip(res, want))
    cot = tuple(rng.standard_normal((3, 2, 2, 3)))                    # L = sum c . M: the cotangents are c exactly
    sum((torch.tensor(c) * o).sum() for c, o in zip(cot, res)).backward()
    wg, = mbfir.bloch_ss_vjp_batch([pulse], df, dp, [cot], scales=sc)
    assert np.array_equal(b1.grad.numpy(), wg)
    with pytest.raises(ValueError, match="does not depend on m0"):
        mbfir.torchsim.bloch(b1, gr, tp, 0.1, 0.02, df, dp, nucleus="H-1", m0=(0.0, 0.0, 1.0), steady_state=True)


def test_errors_of_the_raw_calls_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(8)]

    def head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1):
        return (ctx._h, npulse, lp(toff), p(b1) if b1 is not None else None, p(d), None, None, None, lp(tsoff), p(d), p(t1), p(one),
                p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d), None, None, nscale, p(one))

    def vjp(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
            cot=(one, one, one), grad=outs[:2], m=outs[2:5]):
        o = [p(v) if v is not None else None for v in (*cot, *grad, *m)]
        return lib.mbfir_bloch_ss_vjp_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), *o)

    def jvp(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d, ndir=2,
            v=(one, one), m=outs[2:5], dm=outs[5:8]):
        o = [p(a) if a is not None else None for a in (*v, *m, *dm)]
        return lib.mbfir_bloch_ss_jvp_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), ndir, *o)
    big = 2 ** 31 - 1
    shared = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
              (dict(npulse=2, toff=L(0, 3, 1), tsoff=L(0, 1, 2)), "inconsistent offsets"), (dict(tsoff=L(0, 2)), "neither 1 nor"),
              (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"), (dict(poff=L(0, 0)), "empty item"),
              (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"), (dict(b1=None), "required array is null"),
              (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"), (dict(m=[None, outs[3], outs[4]]), "mx, my and mz"))
    own = {vjp: ((dict(cot=(one, None, one)), "cotangent or gradient plane is null"),
                 (dict(grad=[outs[0], None]), "cotangent or gradient plane is null")),
           jvp: ((dict(v=(one, None)), "direction or tangent plane is null"),
                 (dict(dm=[outs[5], None, outs[7]]), "direction or tangent plane is null"), (dict(ndir=0), "ndir must be at least 1"),
                 (dict(ndir=big, foff=L(0, 2 ** 20), poff=L(0, 2 ** 20)), "overflows"))}
    for call, who in ((vjp, "bloch_ss_vjp_batch:"), (jvp, "bloch_ss_jvp_batch:")):
        assert call() == 0
        for kw, why in shared + own[call]:
            assert call(**kw) == mbfir.E_ARG, kw
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call() == 0 and call(m=[None] * 3) == 0
