"""The adjoint of the pulse train in b1, m0, the gradient waveform and the off-resonance on the device
(mbfir.bloch_train_vjp_gr_batch: k_bloch_train_prop, k_bloch_train_run_vjp, k_bloch_train_prop_vjp_gr, k_bloch_train_vjp_gr_fold,
k_bloch_train_vjp_df_fold; mbfir.torchsim.bloch_train) against the float64 NumPy reference of tests/blochtrainvjpg_ref.py, against
the shipped mbfir.bloch_train_vjp_batch, against the shipped mbfir.bloch_vjp_gr_batch on the tiled waveform, against central
differences of the shipped mbfir.bloch_train_batch, and for the bit-invariance of a train's results under the batch's composition.

Bounds of every comparison with the reference (blochtrainvjpg_ref): TOL ntr gamma dt_t sum_p |pos_{p,a}| sum_{s,f} mu W per entry
(t, a) of the gr gradient and TOL ntr TWOPI (sum_t dt_t) mu W per entry of the df gradient, W the 1-norm of the point's cotangents,
mu = max(|m0|inf, |meq|, 1), TOL = 1e-12; blochtrainvjp_ref's bounds for b1 and m0.  Where a gr bound is zero the result must be
exactly zero.  tests/test_blochtrainvjpg_cpu.py holds the float64 reference within a hundredth of these of its long-double twin.

Measured on an MI355X: see DESIGN section 8aj."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainvjpg_ref", os.path.join(ROOT, "tests", "blochtrainvjpg_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
vjp, tr, gradg = ref.vjp, ref.tr, ref.gradg
CASES = list(ref.cases())


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _opt(v):
    return None if v[0] is None else list(v)


def _args(c, **kw):
    df, dp = _grids(c)
    args = dict(cot_final=_opt(c["cf"]), phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"],
                m0=_opt(c["m0"]), meq=c["meq"], demod=c["demod"], grad_m0=True)
    args.update(kw)
    return (c["pulses"], df, dp, list(c["ntr"]), _opt(c["ce"])), args


def _vjpg(c, **kw):
    a, k = _args(c, **dict(dict(grad_df=True), **kw))
    return mbfir.bloch_train_vjp_gr_batch(*a, **k)


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))
            and np.array_equal(a[3], b[3]))


@pytest.mark.parametrize("name", CASES)
def test_device_gradients_are_the_reference_and_agree_with_the_b1_adjoint(name):
    c = ref.cases()[name]
    got, want = _vjpg(c), ref.reference(name)
    a, k = _args(c)
    old = mbfir.bloch_train_vjp_batch(*a, **k)
    assert len(got) == len(c["pulses"])
    for q, (g, gg, gm, gd) in enumerate(got):
        G, GG, GM, GD = want[q]
        assert g.shape == G.shape and gg.shape == GG.shape and gd.shape == GD.shape and all(a.shape == b.shape for a, b in zip(gm, GM))
        bg, bd, bb = ref.bound_gr(c, q), ref.bound_df(c, q), ref.bound_b1(c, q)
        pos = bg > 0
        sg = float((np.abs(gg - GG)[pos] / bg[pos]).max()) if pos.any() else 0.0
        sd = float((np.abs(gd - GD) / bd).max())
        sb = float((np.abs(g - G) / bb).max())
        sm = max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(gm, GM))
        so = float((np.abs(g - old[q][0]) / bb).max())
        print("%s pulse %d: device against the float64 reference, share of the bounds gr %.3g df %.3g b1 %.3g m0 %.3g; %d entries of gr "
              "without a bound; b1 against bloch_train_vjp_batch %.3g of the bound, equal to the bit: %s"
              % (name, q, sg, sd, sb, sm, int((~pos).sum()), so, np.array_equal(g, old[q][0])))
        assert sg <= 1 and sd <= 1 and sb <= 1 and sm <= 1, (q, sg, sd, sb, sm)
        assert np.all(gg[~pos] == 0.0), q
        assert all(np.array_equal(u, v) for u, v in zip(gm, old[q][1])), q          # dL/dm0 has the b1 adjoint's bits
        assert so <= 1, (q, so)


@pytest.mark.parametrize("name", ["sub", "batch", "allgains"])
def test_asking_for_df_or_m0_leaves_the_other_results_alone(name):
    c = ref.cases()[name]
    full = _vjpg(c)
    no_df, no_m0, bare = _vjpg(c, grad_df=False), _vjpg(c, grad_m0=False), _vjpg(c, grad_df=False, grad_m0=False)
    for q, (g, gg, gm, gd) in enumerate(full):
        assert len(no_df[q]) == 3 and len(no_m0[q]) == 3 and len(bare[q]) == 2
        for other in (no_df[q], no_m0[q], bare[q]):
            assert np.array_equal(other[0], g) and np.array_equal(other[1], gg), q
        assert all(np.array_equal(u, v) for u, v in zip(no_df[q][2], gm)) and np.array_equal(no_m0[q][2], gd), q


def test_a_train_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(57)
    lengths = [int(v) for v in rng.integers(1, 300, 17)]
    reps = [int(v) for v in rng.integers(1, 20, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, phs, gns, ech, m0s, ce, cf = [], [], [], [], [], [], [], [], []
    for q, (n, ntr) in enumerate(zip(lengths, reps)):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (tr.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, (n, 1 + q % 3)) * 0.1, np.append(np.full(n - 1, dt), 1e-3), 0.8, 3e-2 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 20 * q
        dfs.append(tr._grid(nf, 150.0))
        dps.append(np.stack([tr._grid(npos, 3.0) * (1.0 - 0.3 * a) for a in range(1 + (q + 1) % 3)], 1))
        phs.append(rng.uniform(-np.pi, np.pi, ntr))
        gns.append(rng.choice([0.5, 0.8, 1.0, 1.2][:1 + q % 4], ntr))
        ech.append(int(rng.integers(0, n + 1)))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        ce.append(tuple(rng.standard_normal((3, 2, ntr, nf, npos))))
        cf.append(tuple(rng.standard_normal((3, 2, nf, npos))))

    def run(idx):
        sel = lambda a: [a[i] for i in idx]
        return mbfir.bloch_train_vjp_gr_batch(sel(pulses), sel(dfs), sel(dps), sel(reps), sel(ce), cot_final=sel(cf), phases=sel(phs),
                                              gains=sel(gns), echo=sel(ech), scales=sc, m0=sel(m0s), meq=0.3, grad_m0=True, grad_df=True)
    order = list(range(17))
    full, again, rev = run(order), run(order), run(order[::-1])[::-1]
    for q in range(17):
        assert all(np.all(np.isfinite(v)) for v in (full[q][0], full[q][1], full[q][3])), q
        assert _same(full[q], again[q]) and _same(full[q], rev[q]), q
    for q in (0, 5, 16):
        assert _same(run([q])[0], full[q]), q
        assert _same(run([q, q])[1], full[q]), q


def test_final_cotangents_alone_are_the_shipped_adjoint_of_the_tiled_waveform():
    """h1_long (257 samples x 2 repetitions x 300 points, meq = 1, cotangents on the final state only): grad_gr is the tiled call's
    rows summed over the repetitions and grad_df is the tiled call's, within twice the sum of the two calls' bounds"""
    c = ref.cases()["h1_long"]
    assert c["meq"] == 1.0 and c["cot"] == "final"
    p, df, dp, ph, gn = c["pulses"][0], c["dfs"][0], c["dps"][0], c["phases"][0], c["gains"][0]
    (_, gg, gd), = _vjpg(c, grad_m0=False)
    tiled = tr.tile_pulse(p, ph, gn)
    (_, tg, td), = mbfir.bloch_vjp_gr_batch([tiled], df, dp, [c["cf"][0]], scales=c["scales"], m0=[c["m0"][0]], grad_df=True)
    n = len(p[0])
    bg = ref.bound_gr(c, 0) + gradg.bound_gr(tiled, dp, c["cf"][0]).reshape(len(ph), n, 3).sum(0)
    bd = ref.bound_df(c, 0) + gradg.bound_df(tiled, c["cf"][0])
    eg, ed = np.abs(gg - tg.reshape(len(ph), n, 3).sum(0)), np.abs(gd - td)
    pos = bg > 0
    print("against bloch_vjp_gr_batch on the tiled waveform: share of the summed bounds gr %.3g df %.3g; max|gr grad| %.3g max|df grad| "
          "%.3g" % ((eg[pos] / bg[pos]).max(), (ed / bd).max(), np.abs(gg).max(), np.abs(gd).max()))
    assert np.all(eg <= 2 * bg) and np.all(ed <= 2 * bd)
    assert gg[:, 0].any() and not gg[:, 1:].any()                                   # no gradient is played: the derivative at zero


def test_the_vjp_is_the_directional_derivative_of_the_shipped_train():
    """L = sum (w . echo)^2 / 2 on mbfir.bloch_train_batch (9 samples, 5 repetitions at three gains, 3 x 85 points, scales 0.9, 1.0,
    1.1): the central difference along a random unit direction of gr equals <grad_gr, d>, and the one along a common shift of df the
    sum of grad_df, at the steps where the float64 reference's own difference is smallest and within ten times that minimum
    (blochtrainvjpg_ref: 3.7e-10 at 1e-6 G/cm, 2.3e-9 at 1e-4 Hz)"""
    pulse, df, dp, kw, w, d = ref.fd_problem()

    def fwd(g, f):
        E, = mbfir.bloch_train_batch([(pulse[0], g) + tuple(pulse[2:])], f, dp, 5, **kw)
        return ref.fd_loss(E, w)
    gr = np.asarray(pulse[1], dtype=np.float64).reshape(-1)
    L0, cot = fwd(gr, df)
    (_, gg, gd), = mbfir.bloch_train_vjp_gr_batch([pulse], df, dp, 5, [cot], grad_df=True, **kw)
    hg, hd = ref.FD_DIR_GR, ref.FD_DIR_DF
    dd, fd = float((gg[:, 0] * d).sum()), (fwd(gr + hg * d, df)[0] - fwd(gr - hg * d, df)[0]) / (2 * hg)
    ds, fs = float(gd.sum()), (fwd(gr, df + hd)[0] - fwd(gr, df - hd)[0]) / (2 * hd)
    print("loss %.6g; gr: <g, d> %.9g central difference %.9g relative %.3g (tolerance %.3g); df: sum %.9g central difference %.9g "
          "relative %.3g (tolerance %.3g)" % (L0, dd, fd, abs(fd - dd) / abs(dd), 10 * ref.FD_DIR_GR_MIN, ds, fs, abs(fs - ds) / abs(ds),
                                             10 * ref.FD_DIR_DF_MIN))
    assert np.array_equal(gg[:, 1:], np.zeros((9, 2)))                              # no position has a y or z coordinate
    assert abs(fd - dd) <= 10 * ref.FD_DIR_GR_MIN * abs(dd) and abs(fs - ds) <= 10 * ref.FD_DIR_DF_MIN * abs(ds)


def test_torchsim_bloch_train_passes_gradcheck_in_b1_gr_and_df_and_carries_the_device_bits():
    import torch
    rng = np.random.default_rng(5)
    gamma, dt = tr.GAMMA_H1, 1e-4
    b0 = (rng.standard_normal(7) + 1j * rng.standard_normal(7)) * (0.5 / (gamma * dt))
    b0[-1] = 0.0
    g0 = rng.uniform(0.5, 1.5, (7, 2)) * 0.05
    g0[-1] = 0.0
    tp = np.append(np.full(6, dt), 2e-3)
    d0, dp = np.array([-100.0, 30.0]), np.array([[-1.0, 0.5], [0.0, 0.0], [1.5, -0.7]])
    kw = dict(phases=np.array([0.0, 2.0, -1.0]), gains=np.array([0.5, 1.0, 1.0]), echo=3, scales=(1.0, 0.8), meq=0.0)
    b1 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    gr = torch.tensor(g0, dtype=torch.float64, requires_grad=True)
    df = torch.tensor(d0, dtype=torch.float64, requires_grad=True)

    def f(b, g, d):
        out = mbfir.torchsim.bloch_train(b, g, tp, 0.13, 0.03, d, dp, 3, nucleus="H-1", final=True, **kw)
        return out[0] + out[1]
    # b1 is a few hundredths of a gauss, gr a few hundredths of a gauss per centimetre: the step is set to their size
    assert torch.autograd.gradcheck(f, (b1, gr, df), eps=1e-6, atol=1e-6, rtol=1e-4)
    pulse = (b0, g0, tp, 0.13, 0.03, "H-1")
    (we, wf), = mbfir.bloch_train_batch([pulse], d0, dp, 3, final=True, **kw)
    res = f(b1, gr, df)
    assert all(np.array_equal(o.detach().numpy(), w) for o, w in zip(res, we + wf))
    ce, cf = tuple(rng.standard_normal((3, 2, 3, 2, 3))), tuple(rng.standard_normal((3, 2, 2, 3)))
    sum((torch.from_numpy(c) * o).sum() for c, o in zip(ce + cf, res)).backward()
    (wg, wgg, wd), = mbfir.bloch_train_vjp_gr_batch([pulse], d0, dp, 3, [ce], cot_final=[cf], grad_df=True, **kw)
    assert np.array_equal(b1.grad.numpy(), wg) and np.array_equal(gr.grad.numpy(), wgg[:, :2])
    assert np.array_equal(df.grad.numpy(), wd.sum(axis=(0, 2)))
    # when gr and df do not require grad, b1.grad is the shipped path to the bit
    b2 = torch.tensor(b0, dtype=torch.complex128, requires_grad=True)
    sum((torch.from_numpy(c) * o).sum() for c, o in zip(ce + cf, f(b2, g0, d0))).backward()
    og, = mbfir.bloch_train_vjp_batch([pulse], d0, dp, 3, [ce], cot_final=[cf], **kw)
    assert np.array_equal(b2.grad.numpy(), og)


def test_errors_of_the_raw_call_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(9)]

    def opt(a, f):
        return f(a) if a is not None else None

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d, ntr=I(4),
             roff=L(0, 4), cs=one, sn=np.zeros(64), gidx=I(0, 1, 1, 0), goff=L(0, 2), gains=np.array([0.5, 1.0]), echo=I(2), meq=one,
             m0=(None, None, None), ce=(one, one, one), cf=(one, one, one), g=outs[:2], gm=outs[2:5], gg=outs[5:8], gdf=outs[8]):
        return lib.mbfir_bloch_train_vjp_gr_batch(ctx._h, npulse, lp(toff), opt(b1, p), p(d), None, None, None, lp(tsoff), p(d), p(t1),
                                                  p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d), None, None, nscale,
                                                  p(one), opt(ntr, ip), opt(roff, lp), opt(cs, p), opt(sn, p), opt(gidx, ip),
                                                  opt(goff, lp), opt(gains, p), opt(echo, ip), opt(meq, p), 0,
                                                  *[opt(v, p) for v in (*m0, *ce, *cf, *g, *gm, *gg, gdf)])
    big = 2 ** 31 - 1
    nan, inf = float("nan"), float("inf")
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
             (dict(tsoff=L(0, 2)), "neither 1 nor"), (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"),
             (dict(nfgrid=2), "1 or npulse"), (dict(b1=None), "required array is null"), (dict(echo=None), "required array is null"),
             (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
             (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(roff=L(0, 3)), "does not span its ntr"),
             (dict(goff=L(0, 0)), "between 1 and ntr distinct gains"), (dict(gidx=I(0, 2, 1, 0)), "gain index of pulse 0 lies outside"),
             (dict(gains=np.array([0.5, inf])), "a gain is not finite"), (dict(cs=np.full(64, nan)), "cosine or sine"),
             (dict(meq=np.full(64, nan)), "meq of pulse 0 is not finite"), (dict(m0=(one, None, one)), "m0x, m0y and m0z"),
             (dict(ce=(one, None, one)), "echo cotangents are given together"),
             (dict(cf=(None, one, one)), "final cotangents are given together"),
             (dict(ce=(None,) * 3, cf=(None,) * 3), "neither echo cotangents nor final cotangents"),
             (dict(g=[outs[0], None]), "a gradient plane is null"), (dict(g=[None, outs[1]]), "a gradient plane is null"),
             (dict(gm=[outs[2], None, outs[4]]), "gmx, gmy and gmz"),
             (dict(gg=[None, outs[6], outs[7]]), "(ggx, ggy, ggz) is null"), (dict(gg=[outs[5], None, outs[7]]), "(ggx, ggy, ggz) is null"),
             (dict(gg=[outs[5], outs[6], None]), "(ggx, ggy, ggz) is null"),
             (dict(ntr=I(big), roff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
             # the train itself would fit: 2^30 points, 4 repetitions; the checkpoints of 2^31 - 1 samples on them do not
             (dict(toff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_train_vjp_gr_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0
    assert call(ce=(None,) * 3) == 0 and call(cf=(None,) * 3) == 0 and call(gm=[None] * 3) == 0 and call(gdf=None) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    ce, cf = (np.ones((1, 4, 2, 3)),) * 3, (np.ones((1, 2, 3)),) * 3
    (wg, wgg, wm, wd), = mbfir.bloch_train_vjp_gr_batch([pulse], d[:2], d[:3], 4, [ce], cot_final=[cf], phases=0.0,
                                                        gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2, grad_m0=True, grad_df=True)
    assert call() == 0
    assert np.array_equal(outs[0][:3], wg.real) and np.array_equal(outs[1][:3], wg.imag)
    assert all(np.array_equal(o[:6], w.ravel()) for o, w in zip(outs[2:5], wm))
    assert all(np.array_equal(o[:3], wgg[:, a]) for a, o in enumerate(outs[5:8])) and np.array_equal(outs[8][:6], wd.ravel())
