"""The adjoint of the pulse train in its schedule on the device (mbfir.bloch_train_vjp_sched_batch: k_bloch_train_prop,
k_bloch_train_prop_dgain, k_bloch_train_run_sched, k_bloch_train_sched_fold) against the long-double reference of
tests/blochtrainsched_ref.py, against central differences of the shipped mbfir.bloch_train_batch one repetition at a time, against
the shipped mbfir.bloch_vjp_batch on the tiled waveform, against the shipped mbfir.bloch_train_vjp_batch through the two Euler
identities and, to the bit, in dL/dm0, for the bit-invariance of a gradient under the batch's composition and under what else the
call is asked for, for the refused calls, and through mbfir.torchsim.bloch_train.

Bounds of every comparison with the reference (blochtrainsched_ref): TOL ntr N max|scale| Theta per gains entry and TOL ntr N per
phases entry, TOL = 1e-12, N the 1-norm of the pulse's cotangents times sqrt(3) max(|m0|inf, |meq|, 1), Theta = gamma sum |b1| dt.
Measured worst shares on the device: 4.1e-4 of the gains bound and 3.3e-4 of the phases bound (both on the 257-sample period of
shared) and 2.9e-2 of the m0 bound (the 257-sample period of batch); DESIGN section 8ad quotes them from this file's output."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainsched_ref", os.path.join(ROOT, "tests", "blochtrainsched_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
vjp, tr = ref.vjp, ref.tr
CASES = list(ref.cases())


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _opt(v):
    return None if v[0] is None else list(v)


def _kw(c):
    return dict(cot_final=_opt(c["cf"]), phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"],
                m0=None if c["m0"][0] is None else list(c["m0"]), meq=c["meq"], demod=c["demod"], grad_m0=True)


def _sched(c, **kw):
    df, dp = _grids(c)
    return mbfir.bloch_train_vjp_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["ce"]), **dict(_kw(c), **kw))


def _b1_adjoint(c):
    df, dp = _grids(c)
    return mbfir.bloch_train_vjp_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["ce"]), **_kw(c))


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a[:2], b[:2])) and \
        all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))


@pytest.mark.parametrize("name", CASES)
def test_device_gradients_are_the_longdouble_reference(name):
    c = ref.cases()[name]
    got, want = _sched(c), ref.reference(name)
    assert len(got) == len(c["pulses"])
    for q, (gg, gp, gm) in enumerate(got):
        GG, GP, GM = want[q]
        assert gg.shape == gp.shape == (c["ntr"][q],) and gg.dtype == gp.dtype == np.float64, q
        assert np.isfinite(gg).all() and np.isfinite(gp).all(), q
        sg = float(np.abs(gg - GG).max() / ref.bound_gains(c, q))
        sp = float(np.abs(gp - GP).max() / ref.bound_phases(c, q))
        sm = max(float((np.abs(a - b) / ref.bound_m0(c, q)).max()) for a, b in zip(gm, GM))
        print("%s pulse %d: device against long double, share of the gains bound %.3g, of the phases bound %.3g, of the m0 bound %.3g"
              % (name, q, sg, sp, sm))
        assert sg <= 1 and sp <= 1 and sm <= 1, (q, sg, sp, sm)


def test_the_hard_pulse_case_has_its_closed_forms():
    c = ref.cases()["hard"]
    (gg, gp, _), = _sched(c)
    wg, wp = ref.hard_closed()
    assert np.abs(gg - wg).max() <= ref.bound_gains(c, 0) and np.abs(gp - wp).max() <= ref.bound_phases(c, 0)


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_central_differences_of_the_shipped_train(name):
    """One repetition moved at a time by the steps of blochtrainsched_ref, all 4 ntr trains in one bloch_train_batch call; on
    'repeat' that moves one of three repetitions that share a gain value, on 'zerogain' the repetition whose gain is 0"""
    c, q = ref.case(name), 0
    p, df, dp, ntr = c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q]
    sch = ref.fd_schedules(c, q)
    res = mbfir.bloch_train_batch([p] * len(sch), df, dp, ntr, phases=[s[1] for s in sch], gains=[s[0] for s in sch], echo=c["echo"][q],
                                  scales=c["scales"], m0=[c["m0"][q]] * len(sch), meq=c["meq"], demod=c["demod"], final=True)
    dg, dph = ref.fd_quotients(c, q, [float(ref.loss(c, q, e, f).sum()) for e, f in res])
    (gg, gp, _), = _sched(c)
    sg, sp = float(np.abs(dg - gg).max() / ref.scale_gains(c, q)), float(np.abs(dph - gp).max() / ref.scale_phases(c, q))
    print("%s: central differences of the shipped train off by %.3g of the gains scale and %.3g of the phases scale (FD_TOL %.0e)"
          % (name, sg, sp, ref.FD_TOL))
    assert sg <= ref.FD_TOL and sp <= ref.FD_TOL, (sg, sp)


def test_final_cotangents_alone_are_the_shipped_adjoint_of_the_tiled_waveform_contracted():
    """h1_long (cotangents on the final state only): with G_w[k, t] from mbfir.bloch_vjp_batch on tile_pulse(...) and w = scale
    gains[k] e^{i phi_k} b1_t, gg[k] = sum_t Re(conj(G_w) scale e^{i phi_k} b1_t) and gp[k] = sum_t Re(conj(G_w) i w).  Tolerance: the
    two bounds added, the tiled call's (blochgrad_ref.bound_b1, per tiled sample) through the same contraction."""
    c = ref.cases()["h1_long"]
    assert c["cot"] == "final" and not c["demod"] and c["scales"] == (1.0,)
    p, df, dp, ph, gn = c["pulses"][0], c["dfs"][0], c["dps"][0], c["phases"][0], c["gains"][0]
    (gg, gp, gm), = _sched(c)
    tiled = tr.tile_pulse(p, ph, gn)
    (gt, gmt), = mbfir.bloch_vjp_batch([tiled], df, dp, [c["cf"][0]], scales=c["scales"], m0=[c["m0"][0]], grad_m0=True)
    n, N = len(p[0]), len(ph)
    Gw = gt.reshape(N, n)
    dwg = np.exp(1j * ph)[:, None] * np.asarray(p[0])[None, :]
    w = gn[:, None] * dwg
    bt = tr._grad.bound_b1(tiled, c["cf"][0], c["scales"]).reshape(N, n)
    sg = float((np.abs(gg - (np.conj(Gw) * dwg).real.sum(1)) / (ref.bound_gains(c, 0) + (bt * np.abs(dwg)).sum(1))).max())
    sp = float((np.abs(gp - (np.conj(Gw) * 1j * w).real.sum(1)) / (ref.bound_phases(c, 0) + (bt * np.abs(w)).sum(1))).max())
    print("against bloch_vjp_batch on the tiled waveform: share of the summed bounds %.3g (gains), %.3g (phases)" % (sg, sp))
    assert sg <= 1 and sp <= 1
    assert all(np.array_equal(a, b) for a, b in zip(gm, _b1_adjoint(c)[0][1]))


@pytest.mark.parametrize("name", CASES)
def test_the_euler_identities_and_the_bits_of_dldm0_against_the_shipped_b1_adjoint(name):
    """sum_k gains[k] gg[k] = sum_t (Re b1 Re G + Im b1 Im G) and, without demod, sum_k gp[k] = sum_t (-Im b1 Re G + Re b1 Im G), G
    from mbfir.bloch_train_vjp_batch, within the two sides' bounds; dL/dm0 has that call's bits"""
    c = ref.cases()[name]
    for q, ((gg, gp, gm), (G, gmv)) in enumerate(zip(_sched(c), _b1_adjoint(c))):
        b1, bb = np.asarray(c["pulses"][q][0], dtype=np.complex128), vjp.bound_b1(c, q)
        lhs, rhs = float((c["gains"][q] * gg).sum()), float((b1.real * G.real + b1.imag * G.imag).sum())
        tol = np.abs(c["gains"][q]).sum() * ref.bound_gains(c, q) + (np.abs(b1) * bb).sum()
        assert abs(lhs - rhs) <= tol, (q, lhs, rhs, tol)
        if not c["demod"]:
            rhs = float((-b1.imag * G.real + b1.real * G.imag).sum())
            tol = c["ntr"][q] * ref.bound_phases(c, q) + (np.abs(b1) * bb).sum()
            assert abs(gp.sum() - rhs) <= tol, (q, gp.sum(), rhs, tol)
        assert all(np.array_equal(a, b) for a, b in zip(gm, gmv)), q


def test_a_gradient_has_the_same_bits_alone_in_a_batch_reversed_and_repeated():
    rng = np.random.default_rng(59)
    lengths = [int(v) for v in rng.integers(1, 300, 9)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, ntr, phs, gns, ech, m0s, ce, cf = [], [], [], [], [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (tr.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, np.append(np.full(n - 1, dt), 1e-3), 0.8, 3e-2 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(tr._grid(nf, 150.0))
        dps.append(tr._grid(npos, 3.0))
        ntr.append(1 + 37 * q)                                                  # 1 .. 297 repetitions: two tiles of the table
        phs.append(rng.uniform(-np.pi, np.pi, ntr[-1]))
        gns.append(rng.choice([0.5, 0.0, 1.0, 1.2][:1 + q % 4], ntr[-1]))
        ech.append(int(rng.integers(0, n + 1)))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))
        ce.append(tuple(rng.standard_normal((3, 2, ntr[-1], nf, npos))))
        cf.append(tuple(rng.standard_normal((3, 2, nf, npos))))

    def run(idx, **kw):
        sel = lambda a: [a[i] for i in idx]
        return mbfir.bloch_train_vjp_sched_batch(sel(pulses), sel(dfs), sel(dps), sel(ntr), sel(ce), cot_final=sel(cf), phases=sel(phs),
                                                 gains=sel(gns), echo=sel(ech), scales=sc, m0=sel(m0s), meq=0.3, grad_m0=True, **kw)
    order = list(range(len(lengths)))
    full, again, rev = run(order), run(order), run(order[::-1])[::-1]
    for q in order:
        assert _same(full[q], again[q]) and _same(full[q], rev[q]), q
    for q in (0, 5, 8):
        assert _same(run([q])[0], full[q]), q
        assert _same(run([q, q])[1], full[q]), q
    # what else the call is asked for does not change a bit of what it returns
    po, go = run(order, grad_gains=False), run(order, grad_phases=False)
    bare = mbfir.bloch_train_vjp_sched_batch(pulses, dfs, dps, ntr, ce, cot_final=cf, phases=phs, gains=gns, echo=ech, scales=sc, m0=m0s,
                                             meq=0.3)
    for q in order:
        assert po[q][0] is None and np.array_equal(po[q][1], full[q][1]), q
        assert go[q][1] is None and np.array_equal(go[q][0], full[q][0]), q
        assert len(bare[q]) == 2 and np.array_equal(bare[q][0], full[q][0]) and np.array_equal(bare[q][1], full[q][1]), q
        assert all(np.array_equal(a, b) for a, b in zip(po[q][2], full[q][2])) and all(np.array_equal(a, b) for a, b in zip(go[q][2], full[q][2])), q


def test_scalar_schedules_still_give_one_entry_per_repetition():
    c = ref.small()
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    kw = dict(cot_final=[c["cf"][0]], echo=4, m0=[c["m0"][0]])
    (a, b), = mbfir.bloch_train_vjp_sched_batch([p], df, dp, 3, [c["ce"][0]], phases=0.7, gains=0.8, **kw)
    (wa, wb), = mbfir.bloch_train_vjp_sched_batch([p], df, dp, 3, [c["ce"][0]], phases=0.7 * np.arange(3), gains=np.full(3, 0.8), **kw)
    assert a.shape == b.shape == (3,) and np.array_equal(a, wa) and np.array_equal(b, wb)


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

    def call(npulse=1, toff=L(0, 3), foff=L(0, 2), poff=L(0, 3), nscale=1, b1=d, ntr=I(4), roff=L(0, 4), gidx=I(0, 1, 1, 0), goff=L(0, 2),
             gains=np.array([0.5, 0.0]), echo=I(2), m0=(None, None, None), ce=(one, one, one), cf=(one, one, one), g=outs[:2],
             gm=outs[2:]):
        return lib.mbfir_bloch_train_vjp_sched_batch(ctx._h, npulse, lp(toff), opt(b1, p), p(d), None, None, None, lp(L(0, 1)), p(d),
                                                     p(one), p(one), p(one), 1, lp(foff), p(d), 1, lp(poff), p(d), None, None, nscale,
                                                     p(one), opt(ntr, ip), opt(roff, lp), p(one), p(np.zeros(64)), opt(gidx, ip),
                                                     opt(goff, lp), opt(gains, p), opt(echo, ip), p(one), 0,
                                                     *[opt(v, p) for v in (*m0, *ce, *cf, *g, *gm)])
    big = 2 ** 31 - 1
    cases = ((dict(npulse=0), "no pulses"), (dict(b1=None), "required array is null"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
             (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(gidx=I(0, 2, 1, 0)), "gain index of pulse 0 lies outside"),
             (dict(gains=np.array([0.5, float("inf")])), "a gain is not finite"), (dict(m0=(one, None, one)), "m0x, m0y and m0z"),
             (dict(g=[None, None]), "neither the gradient in the gains nor the gradient in the phases is wanted"),
             (dict(ce=(one, None, one)), "echo cotangents are given together"),
             (dict(cf=(None, one, one)), "final cotangents are given together"),
             (dict(gm=[outs[2], None, outs[4]]), "gmx, gmy and gmz"),
             (dict(ce=(None,) * 3, cf=(None,) * 3), "neither echo cotangents nor final cotangents"),
             # the train itself would fit: 2^30 points; the checkpoints and partials of 2^31 - 1 repetitions on them do not
             (dict(ntr=I(big), roff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_train_vjp_sched_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    null = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS["mbfir_bloch_train_vjp_sched_batch"][1][1:]]
    assert lib.mbfir_bloch_train_vjp_sched_batch(*null) == mbfir.E_ARG                # a NULL context
    assert call() == 0
    assert call(ce=(None,) * 3) == 0 and call(cf=(None,) * 3) == 0 and call(gm=[None] * 3) == 0
    assert call(g=[outs[0], None]) == 0 and call(g=[None, outs[1]]) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    ce, cf = (np.ones((1, 4, 2, 3)),) * 3, (np.ones((1, 2, 3)),) * 3
    (wg, wp, wm), = mbfir.bloch_train_vjp_sched_batch([pulse], d[:2], d[:3], 4, [ce], cot_final=[cf], phases=0.0,
                                                      gains=np.array([0.5, 0.0, 0.0, 0.5]), echo=2, grad_m0=True)
    assert call() == 0
    assert np.array_equal(outs[0][:4], wg) and np.array_equal(outs[1][:4], wp) and not outs[0][4:].any() and not outs[1][4:].any()
    assert all(np.array_equal(o[:6], w.ravel()) for o, w in zip(outs[2:], wm))


def test_torchsim_bloch_train_backward_in_the_schedule_is_the_batch_call():
    """gains.grad and phases.grad are bloch_train_vjp_sched_batch's bits, b1.grad and m0.grad next to them bloch_train_vjp_batch's,
    the forward has bloch_train_batch's bits, and a forward-mode tangent in the schedule raises"""
    import torch
    c = ref.cases()["zerogain"]
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    kw = dict(echo=c["echo"][0], scales=c["scales"], meq=0.5, demod=True)
    m0h = np.stack(c["m0"][0])
    b1 = torch.tensor(p[0], dtype=torch.complex128, requires_grad=True)
    m0 = torch.tensor(m0h, dtype=torch.float64, requires_grad=True)
    gains = torch.tensor(c["gains"][0], dtype=torch.float64, requires_grad=True)
    phases = torch.tensor(c["phases"][0], dtype=torch.float64, requires_grad=True)
    args = (p[1], p[2], p[3], p[4], df, dp, 3)
    E, F = mbfir.torchsim.bloch_train(b1, *args, nucleus=p[5], m0=m0, gains=gains, phases=phases, final=True, **kw)
    (we, wf), = mbfir.bloch_train_batch([p], df, dp, 3, m0=[tuple(m0h)], gains=c["gains"][0], phases=c["phases"][0], final=True, **kw)
    assert all(np.array_equal(a.detach().numpy(), b) for a, b in zip(E + F, we + wf))
    ce, cf = c["ce"][0], c["cf"][0]
    sum((a * torch.from_numpy(np.ascontiguousarray(w))).sum() for a, w in zip(E + F, ce + cf)).backward()
    both = dict(kw, gains=c["gains"][0], phases=c["phases"][0], m0=[tuple(m0h)], cot_final=[cf])
    (gg, gp), = mbfir.bloch_train_vjp_sched_batch([p], df, dp, 3, [ce], **both)
    (g, gm), = mbfir.bloch_train_vjp_batch([p], df, dp, 3, [ce], grad_m0=True, **both)
    assert np.array_equal(gains.grad.numpy(), gg) and np.array_equal(phases.grad.numpy(), gp)
    assert np.array_equal(b1.grad.numpy(), g) and np.array_equal(m0.grad.numpy(), np.stack([v.sum(0) for v in gm]))
    gains.grad = None
    Eo = mbfir.torchsim.bloch_train(b1.detach(), *args, nucleus=p[5], m0=m0h, gains=gains, phases=c["phases"][0], **kw)
    sum((a * torch.from_numpy(np.ascontiguousarray(w))).sum() for a, w in zip(Eo, ce)).backward()
    (go, none), = mbfir.bloch_train_vjp_sched_batch([p], df, dp, 3, [ce], grad_phases=False, **dict(both, cot_final=None))
    assert none is None and np.array_equal(gains.grad.numpy(), go)
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda g: mbfir.torchsim.bloch_train(b1.detach(), *args, nucleus=p[5], gains=g, **kw), (gains.detach(),),
                       (torch.ones_like(gains),))
