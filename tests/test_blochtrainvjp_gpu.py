"""The adjoint of the pulse train on the device (mbfir.bloch_train_vjp_batch: k_bloch_train_prop, k_bloch_train_run_vjp,
k_bloch_train_prop_vjp, k_bloch_train_vjp_fold) against the long-double reference of tests/blochtrainvjp_ref.py, against central
differences of the shipped mbfir.bloch_train_batch, against the shipped mbfir.bloch_vjp_batch on the tiled waveform, for the
bit-invariance of a gradient under the batch's composition, and through mbfir.torchsim.bloch_train.

Bounds of every comparison with the reference (blochtrainvjp_ref): TOL ntr N max|scale gain| gamma dt_t per b1 entry and TOL ntr
max|c|_1 per dL/dm0 entry, TOL = 1e-12, N the 1-norm of the pulse's cotangents.  Measured worst shares on the device: 1.1e-3 of
the b1 bound (the 257-sample period of shared) and 2.9e-2 of the m0 bound (the 257-sample period of batch); DESIGN section 8z
quotes them from this file's output."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainvjp_ref", os.path.join(ROOT, "tests", "blochtrainvjp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
tr = ref.tr
CASES = list(ref.cases())


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _m0(c):
    return None if c["m0"][0] is None else list(c["m0"])


def _opt(v):
    return None if v[0] is None else list(v)


def _vjp(c, **kw):
    df, dp = _grids(c)
    args = dict(cot_final=_opt(c["cf"]), phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"],
                m0=_m0(c), meq=c["meq"], demod=c["demod"], grad_m0=True)
    args.update(kw)
    return mbfir.bloch_train_vjp_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["ce"]), **args)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))


@pytest.mark.parametrize("name", CASES)
def test_device_gradients_are_the_longdouble_reference(name):
    c = ref.cases()[name]
    got, want = _vjp(c), ref.reference(name)
    assert len(got) == len(c["pulses"])
    for q, (g, gm) in enumerate(got):
        G, GM = want[q]
        assert g.shape == G.shape and all(a.shape == b.shape for a, b in zip(gm, GM)), q
        sb = float((np.abs(g - G) / ref.bound_b1(c, q)).max())
        sm = max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(gm, GM))
        print("%s pulse %d: device against long double, share of the b1 bound %.3g, of the m0 bound %.3g" % (name, q, sb, sm))
        assert sb <= 1 and sm <= 1, (q, sb, sm)


def test_central_differences_of_the_shipped_train():
    """The small case: every b1 entry moved by the step of blochtrainvjp_ref (all 36 trains in one bloch_train_batch call), m0 by
    FD_M0 per component with the loss taken per point; the tolerance is the one fixed on the CPU"""
    c = ref.small()
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    n = len(p[0])
    kw = dict(phases=c["phases"][0], gains=c["gains"][0], echo=c["echo"][0], scales=c["scales"], meq=c["meq"], demod=c["demod"], final=True)
    (g, gm), = _vjp(c)
    h = ref.FD_ANGLE / (tr.gamma_of(p[5]) * tr.intervals(p) * ref.amax_of(c, 0))
    moved = []
    for t in range(n):
        for unit in (1.0, 1j):
            for sgn in (1, -1):
                d = np.zeros(n, dtype=complex)
                d[t] = sgn * unit * h[t]
                moved.append((p[0] + d,) + p[1:])
    res = mbfir.bloch_train_batch(moved, df, dp, c["ntr"][0], m0=c["m0"][0], **kw)
    L = [float(ref.loss(c, 0, e, f).sum()) for e, f in res]
    sb = ref.scale_b1(c, 0)
    worst = 0.0
    for t in range(n):
        fr, fi = (L[4 * t] - L[4 * t + 1]) / (2 * h[t]), (L[4 * t + 2] - L[4 * t + 3]) / (2 * h[t])
        worst = max(worst, abs(fr - g[t].real) / sb[t], abs(fi - g[t].imag) / sb[t])
    print("central differences in b1: worst %.3g of the scale (FD_TOL %.0e)" % (worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL
    m0 = np.stack(c["m0"][0])
    sm = ref.scale_m0(c, 0)[0]
    for i in range(3):
        d = np.zeros_like(m0)
        d[i] = ref.FD_M0
        (ep, fp), (em, fm) = mbfir.bloch_train_batch([p, p], df, dp, c["ntr"][0], m0=[tuple(m0 + d), tuple(m0 - d)], **kw)
        fd = (ref.loss(c, 0, ep, fp) - ref.loss(c, 0, em, fm)) / (2 * ref.FD_M0)
        assert float((np.abs(fd - gm[i][0]) / sm).max()) <= ref.FD_TOL, i


def test_final_cotangents_alone_are_the_chain_rule_on_the_shipped_adjoint_of_the_tiled_waveform():
    """h1_long (meq = 1, cotangents on the final state only): G_b1[t] = sum_k gains[k] e^{-i phi_k} G_tiled[k, t] with G_tiled from
    mbfir.bloch_vjp_batch on tile_pulse(...); dL/dm0 is the tiled call's.  Tolerance: the two bounds added, the tiled call's
    (blochgrad_ref.bound_b1, per tiled sample) through the same chain rule."""
    c = ref.cases()["h1_long"]
    assert c["meq"] == 1.0 and c["cot"] == "final"
    p, df, dp, ph, gn = c["pulses"][0], c["dfs"][0], c["dps"][0], c["phases"][0], c["gains"][0]
    (g, gm), = _vjp(c)
    tiled = tr.tile_pulse(p, ph, gn)
    (gt, gmt), = mbfir.bloch_vjp_batch([tiled], df, dp, [c["cf"][0]], scales=c["scales"], m0=[c["m0"][0]], grad_m0=True)
    n, w = len(p[0]), gn * np.exp(-1j * ph)
    chain = (w[:, None] * gt.reshape(len(ph), n)).sum(0)
    bt = tr._grad.bound_b1(tiled, c["cf"][0], c["scales"]).reshape(len(ph), n)
    bound = ref.bound_b1(c, 0) + (np.abs(w)[:, None] * bt).sum(0)
    sh = float((np.abs(g - chain) / bound).max())
    shm = max(float((np.abs(a - b) / (ref.bound_m0(c, 0) + tr._grad.bound_m0(c["cf"][0]))).max()) for a, b in zip(gm, gmt))
    print("against bloch_vjp_batch on the tiled waveform: share of the summed bounds %.3g (b1), %.3g (m0)" % (sh, shm))
    assert sh <= 1 and shm <= 1


def test_a_gradient_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(53)
    lengths = [int(v) for v in rng.integers(1, 300, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, ntr, phs, gns, ech, m0s, ce, cf = [], [], [], [], [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (tr.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, np.append(np.full(n - 1, dt), 1e-3), 0.8, 3e-2 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 20 * q
        dfs.append(tr._grid(nf, 150.0))
        dps.append(tr._grid(npos, 3.0))
        ntr.append(1 + 19 * q)                                                  # 1 .. 305 repetitions: two tiles of the table
        phs.append(rng.uniform(-np.pi, np.pi, ntr[-1]))
        gns.append(rng.choice([0.5, 0.8, 1.0, 1.2][:1 + q % 4], ntr[-1]))
        ech.append(int(rng.integers(0, n + 1)))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        ce.append(tuple(rng.standard_normal((3, 2, ntr[-1], nf, npos))))
        cf.append(tuple(rng.standard_normal((3, 2, nf, npos))))

    def run(idx):
        sel = lambda a: [a[i] for i in idx]
        return mbfir.bloch_train_vjp_batch(sel(pulses), sel(dfs), sel(dps), sel(ntr), sel(ce), cot_final=sel(cf), phases=sel(phs),
                                           gains=sel(gns), echo=sel(ech), scales=sc, m0=sel(m0s), meq=0.3, grad_m0=True)
    order = list(range(17))
    full, again, rev = run(order), run(order), run(order[::-1])[::-1]
    for q in range(17):
        assert _same(full[q], again[q]) and _same(full[q], rev[q]), q
    for q in (0, 5, 16):
        assert _same(run([q])[0], full[q]), q
        assert _same(run([q, q])[1], full[q]), q


def test_dldm0_bits_do_not_depend_on_m0_or_meq_and_asking_for_it_leaves_the_gradient_alone():
    for name in ("groups", "allgains"):
        c = ref.cases()[name]
        base = _vjp(c)
        rng = np.random.default_rng(5)
        other = [tuple(rng.uniform(-1, 1, (3, len(f), len(x)))) for f, x in zip(c["dfs"], c["dps"])]
        for kw in (dict(m0=other), dict(meq=0.37), dict(m0=None, meq=1.0 - c["meq"])):
            got = _vjp(c, **kw)
            for (_, a), (_, b) in zip(base, got):
                assert all(np.array_equal(u, v) for u, v in zip(a, b)), (name, kw)
        bare = _vjp(c, grad_m0=False)
        assert all(np.array_equal(g, b[0]) for g, b in zip(bare, base)), name


def test_scale_zero_gives_an_exactly_zero_b1_gradient():
    c = ref.cases()["c13_ramp"]
    S0 = (0.0,)
    ce, cf = [tuple(v[:1] for v in c["ce"][0])], [tuple(v[:1] for v in c["cf"][0])]
    (g, gm), = mbfir.bloch_train_vjp_batch(c["pulses"], c["dfs"][0], c["dps"][0], 257, ce, cot_final=cf, phases=c["phases"][0],
                                           gains=c["gains"][0], echo=4, scales=S0, m0=c["m0"], meq=1.0, grad_m0=True)
    assert g.shape == (9,) and not g.any()
    assert any(v.any() for v in gm)


def test_outputs_are_written_in_full_and_nowhere_else():
    """The raw call with NaN sentinels: every entry of the gradient planes and of the wanted dL/dm0 planes is written, the 16
    entries after them are not, and the bits are the Python call's"""
    c = ref.cases()["c13_ramp"]
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], 11
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    ce, cf = tuple(np.ascontiguousarray(v[:, :ntr]) for v in c["ce"][0]), c["cf"][0]
    (wg, wm), = mbfir.bloch_train_vjp_batch([p], df, dp, ntr, [ce], cot_final=[cf], gains=c["gains"][0][:ntr], echo=4,
                                            scales=c["scales"], m0=c["m0"], meq=1e-4, grad_m0=True)
    A = mbfir._BlochArgs("raw", [p], df, dp, c["scales"])
    uq, gi = np.unique(c["gains"][0][:ntr], return_inverse=True)
    phi = np.pi * np.arange(ntr)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([4], dtype=np.int32), np.array([1e-4])]
    ip, lp = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp))
    targs = [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8]), 0]
    m0 = A.m0_planes(c["m0"], np.array([0, 3 * 6]), [1])
    cep, cfp = [np.ascontiguousarray(v.ravel()) for v in ce], [np.ascontiguousarray(v.ravel()) for v in cf]
    T, O = 9, 3 * 6
    for want_m in (True, False):
        g = [np.full(T + 16, np.nan) for _ in range(2)]
        m = [np.full(O + 16, np.nan) for _ in range(3)]
        rc = lib.mbfir_bloch_train_vjp_batch(ctx._h, *A.head, *targs, *[ptr(v) for v in m0], *[ptr(v) for v in cep],
                                             *[ptr(v) for v in cfp], ptr(g[0]), ptr(g[1]), *[ptr(v) if want_m else None for v in m])
        assert rc == 0, ctx.last_error()
        assert all(np.all(np.isnan(v[T:])) for v in g)
        assert np.array_equal(g[0][:T], wg.real) and np.array_equal(g[1][:T], wg.imag)
        for v, w in zip(m, wm):
            assert np.all(np.isnan(v[O:])) and (np.array_equal(v[:O], w.ravel()) if want_m else np.all(np.isnan(v)))


def test_torchsim_bloch_train_is_the_numpy_calls():
    """The forward has bloch_train_batch's bits, b1.grad and m0.grad are bloch_train_vjp_batch's, and gradcheck passes"""
    import torch
    c = ref.small()
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    kw = dict(phases=c["phases"][0], gains=c["gains"][0], echo=c["echo"][0], scales=(0.9, 1.1), meq=0.5)
    m0h = np.stack(c["m0"][0])
    b1 = torch.tensor(p[0], dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(m0h, dtype=torch.float64, requires_grad=True)
    args = (p[1], p[2], p[3], p[4], df, dp, 3)
    E, F = mbfir.torchsim.bloch_train(b1, *args, nucleus=p[5], m0=m0, final=True, **kw)
    (we, wf), = mbfir.bloch_train_batch([p], df, dp, 3, m0=[tuple(m0h)], final=True, **kw)
    assert all(np.array_equal(a.detach().numpy(), b) for a, b in zip(E + F, we + wf))
    rng = np.random.default_rng(9)
    ce, cf = tuple(rng.standard_normal((3, 2, 3, 3, 2))), tuple(rng.standard_normal((3, 2, 3, 2)))
    sum((a * torch.from_numpy(w)).sum() for a, w in zip(E + F, ce + cf)).backward()
    (g, gm), = mbfir.bloch_train_vjp_batch([p], df, dp, 3, [ce], cot_final=[cf], m0=[tuple(m0h)], grad_m0=True, **kw)
    assert np.array_equal(b1.grad.numpy(), g)
    assert np.array_equal(m0.grad.numpy(), np.stack([v.sum(0) for v in gm]))
    b1.grad = None
    Eo = mbfir.torchsim.bloch_train(b1, *args, nucleus=p[5], m0=m0h, **kw)       # echoes only, m0 a constant
    sum((a * torch.from_numpy(w)).sum() for a, w in zip(Eo, ce)).backward()
    go, = mbfir.bloch_train_vjp_batch([p], df, dp, 3, [ce], m0=[tuple(m0h)], **kw)
    assert np.array_equal(b1.grad.numpy(), go)

    def f(b, m):
        out = mbfir.torchsim.bloch_train(b, *args, nucleus=p[5], m0=m, final=True, demod=True, **kw)
        return out[0] + out[1]
    # b1 is a few hundredths of a gauss: the step is set to its size, the tolerances to the float64 forward's rounding over it
    assert torch.autograd.gradcheck(f, (b1, m0), eps=1e-6, atol=1e-6, rtol=1e-4)
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: f(b, m0.detach()), (b1.detach(),), (torch.ones_like(b1),))


def test_errors_of_the_raw_call_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(5)]

    def opt(a, f):
        return f(a) if a is not None else None

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d, ntr=I(4),
             roff=L(0, 4), cs=one, sn=np.zeros(64), gidx=I(0, 1, 1, 0), goff=L(0, 2), gains=np.array([0.5, 1.0]), echo=I(2), meq=one,
             m0=(None, None, None), ce=(one, one, one), cf=(one, one, one), g=outs[:2], gm=outs[2:]):
        return lib.mbfir_bloch_train_vjp_batch(ctx._h, npulse, lp(toff), opt(b1, p), p(d), None, None, None, lp(tsoff), p(d), p(t1),
                                               p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d), None, None, nscale,
                                               p(one), opt(ntr, ip), opt(roff, lp), opt(cs, p), opt(sn, p), opt(gidx, ip),
                                               opt(goff, lp), opt(gains, p), opt(echo, ip), opt(meq, p), 0,
                                               *[opt(v, p) for v in (*m0, *ce, *cf, *g, *gm)])
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
             (dict(ntr=I(big), roff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
             # the train itself would fit: 2^30 points, 4 repetitions; the checkpoints of 2^31 - 1 samples on them do not
             (dict(toff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_train_vjp_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0
    assert call(ce=(None,) * 3) == 0 and call(cf=(None,) * 3) == 0 and call(gm=[None] * 3) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    ce, cf = (np.ones((1, 4, 2, 3)),) * 3, (np.ones((1, 2, 3)),) * 3
    (wg, wm), = mbfir.bloch_train_vjp_batch([pulse], d[:2], d[:3], 4, [ce], cot_final=[cf], phases=0.0,
                                            gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2, grad_m0=True)
    assert call() == 0
    assert np.array_equal(outs[0][:3], wg.real) and np.array_equal(outs[1][:3], wg.imag)
    assert all(np.array_equal(o[:6], w.ravel()) for o, w in zip(outs[2:], wm))
