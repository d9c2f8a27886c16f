"""The tangent of the pulse train in its schedule on the device (mbfir.bloch_train_jvp_sched_batch: k_bloch_train_prop,
k_bloch_train_prop_dgain, k_bloch_train_run_sched_jvp) against the long-double reference of tests/blochtrainschedjvp_ref.py, against
the shipped adjoint mbfir.bloch_train_vjp_sched_batch through the pairing (row by row of the whole Jacobian on the small cases),
against central differences of the shipped mbfir.bloch_train_batch, against the closed forms of the case 'hard', for the
bit-invariance of a tangent under the composition of the direction groups and of the batch and under what the call is given, for
linearity, for the refused calls of the C ABI, and through mbfir.torchsim.bloch_train(forward_mode=True).

Bound of every comparison with the reference (blochtrainschedjvp_ref.bound_jvp): TOL ntr (mu (sum |dg| max|scale| Theta + 2 sum |dp|)
+ |dm0|_1) per entry, TOL = 1e-12.  Measured worst share on the device: 3.1e-2 of the bound (the 257-sample period of h1_long; 1.2e-2
on that of batch); DESIGN section 8ae quotes it from this file's output."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainschedjvp_ref", os.path.join(ROOT, "tests", "blochtrainschedjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
sched, tr = ref.sched, ref.tr
CASES = list(ref.cases())


def _group():
    return mbfir.bloch_train_sched_jvp_group()


def _kmax():
    """One more than a group, so that the last group is partial, and no fewer than the three kinds of direction"""
    return max(_group() + 1, 3)


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _kw(c, **more):
    kw = dict(phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"],
              m0=None if c["m0"][0] is None else list(c["m0"]), meq=c["meq"], demod=c["demod"])
    kw.update(more)
    return kw


def _jvp(c, dirs, parts=(1, 1, 1), **more):
    """dirs: per pulse (dg, dp, dm0); parts: which of the three are handed over"""
    df, dp = _grids(c)
    pick = lambda i: [d[i] for d in dirs] if parts[i] else None
    return mbfir.bloch_train_jvp_sched_batch(c["pulses"], df, dp, list(c["ntr"]), tangents_gains=pick(0), tangents_phases=pick(1),
                                             tangents_m0=pick(2), **_kw(c, **more))


def _one(dirs, k):
    return [(dg[k], dp[k], tuple(d[k] for d in dm)) for dg, dp, dm in dirs]


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _same(a, b):
    return _eq(a[0], b[0]) and _eq(a[1], b[1])


@pytest.mark.parametrize("name", CASES)
def test_device_tangents_are_the_longdouble_reference_and_the_primal_is_the_forward_calls(name):
    c = ref.cases()[name]
    df, dp = _grids(c)
    K = _kmax()
    fwd = mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), final=True, **_kw(c))
    dirs, want = ref.directions(name, K), ref.reference(name, K)
    got = _jvp(c, dirs, final=True, primal=True)
    assert len(got) == len(c["pulses"])
    for q, ((pe, pf), (te, tf)) in enumerate(got):
        assert _eq(pe, fwd[q][0]) and _eq(pf, fwd[q][1]), q                      # the primal has bloch_train_batch's bits
        assert te[0].shape == want[q][0][0].shape and tf[0].shape == want[q][1][0].shape, q
        bound = ref.bound_jvp(c, q, *dirs[q])
        se, sf = ref.worst((te, None), want[q], bound), ref.worst((None, tf), want[q], bound)
        print("%s pulse %d K %d: device against long double, share of the bound %.3g (echoes), %.3g (final)" % (name, q, K, se, sf))
        assert se <= 1 and sf <= 1, (q, se, sf)


def _adjoint(c):
    df, dp = _grids(c)
    opt = lambda v: None if v[0] is None else list(v)
    return mbfir.bloch_train_vjp_sched_batch(c["pulses"], df, dp, list(c["ntr"]), opt(c["ce"]), cot_final=opt(c["cf"]), grad_m0=True,
                                             **_kw(c))


def _cot_bound(c, q, bound):
    """sum |cot| bound over the entries of a tangent: bound (nf, npos)"""
    ae, af = ref.cot_norms(c, q)
    return float(((ae + af) * bound).sum())


@pytest.mark.parametrize("name", CASES)
def test_the_pairing_with_the_shipped_adjoint(name):
    """<cot, J d> = gg . dg + gp . dp + <dL/dm0, dm0> with the cases' cotangents along every kind of direction; the tolerance is the
    two calls' own bounds, each contracted with the other side"""
    c = ref.cases()[name]
    K = 3
    dirs = ref.directions(name, K)
    adj, tan = _adjoint(c), _jvp(c, dirs, final=True)
    for q, ((gg, gp, gm), (te, tf)) in enumerate(zip(adj, tan)):
        dg, dp, dm = dirs[q]
        bj = ref.bound_jvp(c, q, dg, dp, dm)
        for k in range(K):
            left = ref.pairing(c, q, [e[k] for e in te], [f[k] for f in tf])
            right = float((gg * dg[k]).sum() + (gp * dp[k]).sum()) + sum(float((g * d[k]).sum()) for g, d in zip(gm, dm))
            tol = (_cot_bound(c, q, bj[k]) + sched.bound_gains(c, q) * np.abs(dg[k]).sum() + sched.bound_phases(c, q) * np.abs(dp[k]).sum()
                   + sum(float((sched.bound_m0(c, q) * np.abs(d[k])).sum()) for d in dm))
            print("%s pulse %d direction %d: pairing off by %.3g of its tolerance" % (name, q, k, abs(left - right) / tol))
            assert abs(left - right) <= tol, (q, k, left, right, tol)


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_every_row_of_the_jacobian_pairs_with_the_shipped_adjoint(name):
    c = ref.case(name)
    n = c["ntr"][0]
    (gg, gp, _), = _adjoint(c)
    (te, tf), = mbfir.bloch_train_jacobian_sched_batch(c["pulses"], c["dfs"][0], c["dps"][0], n, final=True, **_kw(c))
    assert te[0].shape[0] == 2 * n and tf[0].shape[0] == 2 * n
    bj = ref.bound_jvp(c, 0, *ref.unit_directions(n), None)
    for j in range(2 * n):
        left = ref.pairing(c, 0, [e[j] for e in te], [f[j] for f in tf])
        right, own = (gg[j], sched.bound_gains(c, 0)) if j < n else (gp[j - n], sched.bound_phases(c, 0))
        tol = _cot_bound(c, 0, bj[j]) + own
        assert abs(left - right) <= tol, (j, left, right, tol)
        assert abs(right) > 1e3 * tol or name == "zerogain", (j, right, tol)     # a row is not matched by smallness


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_central_differences_of_the_shipped_train(name):
    """Along the dense direction, both perturbed trains in one bloch_train_batch call; the step and FD_TOL as blochtrainschedjvp_ref
    derives them"""
    c = ref.case(name)
    dg, dp, dm = _one(ref.directions(name, 3), 2)[0]
    p, df, pos, n = c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0]
    kw = dict(echo=c["echo"][0], scales=c["scales"], meq=c["meq"], demod=c["demod"], final=True)
    (te, tf), = mbfir.bloch_train_jvp_sched_batch([p], df, pos, n, tangents_gains=[dg], tangents_phases=[dp], tangents_m0=[dm],
                                                  phases=c["phases"][0], gains=c["gains"][0], m0=[c["m0"][0]], **kw)
    h = ref.fd_step(c, 0, dg, dp)
    m0, d = np.stack(c["m0"][0]), np.stack(dm)
    (ep, fp), (em, fm) = mbfir.bloch_train_batch([p, p], df, pos, n, phases=[c["phases"][0] + h * dp, c["phases"][0] - h * dp],
                                                 gains=[c["gains"][0] + h * dg, c["gains"][0] - h * dg],
                                                 m0=[tuple(m0 + h * d), tuple(m0 - h * d)], **kw)
    scale = n * ref.size_jvp(c, 0, dg[None], dp[None], tuple(x[None] for x in dm))[0]
    worst = max(max(float((np.abs((ep[i] - em[i]) / (2 * h) - te[i]) / scale).max()),
                    float((np.abs((fp[i] - fm[i]) / (2 * h) - tf[i]) / scale).max())) for i in range(3))
    print("%s: central differences along the dense direction, worst %.3g of ntr size (FD_TOL %.0e)" % (name, worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL


def test_the_case_hard_against_its_closed_forms():
    c = ref.cases()["hard"]
    N = c["ntr"][0]
    (te, tf), = mbfir.bloch_train_jacobian_sched_batch(c["pulses"], c["dfs"][0], c["dps"][0], N, final=True, **_kw(c))
    wE, wF = ref.hard_closed()
    bound = ref.bound_jvp(c, 0, *ref.unit_directions(N), None)                    # (2 N, 1, 1)
    for i in range(3):
        assert np.all(np.abs(te[i][:, 0, :, 0, 0] - wE[:, :, i]) <= bound[:, 0]), i
        assert np.all(np.abs(tf[i][:, 0, 0, 0] - wF[:, i]) <= bound[:, 0, 0]), i


def test_a_direction_has_the_same_bits_alone_first_last_and_whatever_the_call_is_given():
    c = ref.cases()["allgains"]
    K = _group() + 1
    dirs = ref.directions("allgains", 3)
    dense = _one(dirs, 2)
    other = _one(dirs, 0)
    stack = lambda first, last: [(np.stack([a[0]] * (K - 1) + [b[0]]), np.stack([a[1]] * (K - 1) + [b[1]]),
                                  tuple(np.stack([x] * (K - 1) + [y]) for x, y in zip(a[2], b[2]))) for a, b in zip(first, last)]
    alone, = _jvp(c, dense, final=True)
    again, = _jvp(c, dense, final=True)
    assert _same(alone, again)                                                    # two runs
    as_last, = _jvp(c, stack(other, dense), final=True)
    as_first, = _jvp(c, stack(dense, other), final=True)
    assert _same(alone, ([e[K - 1] for e in as_last[0]], [f[K - 1] for f in as_last[1]]))
    assert _same(alone, ([e[0] for e in as_first[0]], [f[0] for f in as_first[1]]))
    f_only, = _jvp(c, dense, echoes=False, final=True)                            # the final planes alone
    assert _eq(f_only, alone[1])
    (pr, both), = _jvp(c, dense, final=True, primal=True)
    assert _same(both, alone)
    zero = [(0 * d[0], 0 * d[1], tuple(0 * x for x in d[2])) for d in dense]
    mix = lambda i: [tuple(z[j] if j == i else d[j] for j in range(3)) for d, z in zip(dense, zero)]
    for i in range(3):                                                            # a part that is None is a part of zeros
        parts = tuple(int(j != i) for j in range(3))
        a, = _jvp(c, dense, parts, final=True)
        b, = _jvp(c, mix(i), final=True)
        assert _same(a, b), i


def test_a_tangent_has_the_same_bits_alone_in_9_reversed_and_repeated():
    rng = np.random.default_rng(59)
    lengths = [int(v) for v in rng.integers(1, 40, 9)]
    sc = [0.9, 1.1]
    K = _group() + 1
    pulses, dfs, dps, ntr, phs, gns, ech, m0s, dirs = [], [], [], [], [], [], [], [], []
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
        dirs.append((rng.standard_normal((K, ntr[-1])), rng.standard_normal((K, ntr[-1])), tuple(rng.standard_normal((3, K, nf, npos)))))

    def run(idx):
        sel = lambda a: [a[i] for i in idx]
        d = sel(dirs)
        return mbfir.bloch_train_jvp_sched_batch(sel(pulses), sel(dfs), sel(dps), sel(ntr), tangents_gains=[x[0] for x in d],
                                                 tangents_phases=[x[1] for x in d], tangents_m0=[x[2] for x in d], phases=sel(phs),
                                                 gains=sel(gns), echo=sel(ech), scales=sc, m0=sel(m0s), meq=0.3, final=True)
    order = list(range(9))
    full, rev = run(order), run(order[::-1])[::-1]
    for q in range(9):
        assert _same(full[q], rev[q]), q
    for q in (0, 4, 8):
        assert _same(run([q])[0], full[q]), q
        assert _same(run([q, q])[1], full[q]), q


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_the_jacobians_rows_add_up_to_the_dense_directions_tangent(name):
    c = ref.case(name)
    n = c["ntr"][0]
    dg, dp, _ = _one(ref.directions(name, 3), 2)[0]
    kw = _kw(c)
    (je, jf), = mbfir.bloch_train_jacobian_sched_batch(c["pulses"], c["dfs"][0], c["dps"][0], n, final=True, **kw)
    (te, tf), = mbfir.bloch_train_jvp_sched_batch(c["pulses"], c["dfs"][0], c["dps"][0], n, tangents_gains=[dg], tangents_phases=[dp],
                                                  final=True, **kw)
    w = np.concatenate([dg, dp])
    bound = 2 * ref.bound_jvp(c, 0, dg[None], dp[None], None)[0]
    for a, b in zip(je + jf, te + tf):
        s = np.tensordot(w, a, 1)
        assert np.all(np.abs(s - b) <= bound), name
        assert np.abs(b).max() > 1e6 * bound.max()


def test_refused_calls_of_the_raw_call_leave_the_outputs_alone_and_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(12)]
    N = (None,) * 3

    def opt(a, f):
        return f(a) if a is not None else None

    def call(npulse=1, toff=L(0, 3), nscale=1, foff=L(0, 2), poff=L(0, 3), ntr=I(4), roff=L(0, 4), gidx=I(0, 1, 1, 0), echo=I(2),
             m0=N, ndir=2, v=(one, one), dm0=N, pe=outs[:3], pf=outs[3:6], te=outs[6:9], tf=outs[9:]):
        return lib.mbfir_bloch_train_jvp_sched_batch(ctx._h, npulse, lp(toff), p(d), p(d), None, None, None, lp(L(0, 1)), p(d), p(one),
                                                     p(one), p(one), 1, lp(foff), p(d), 1, lp(poff), p(d), None, None, nscale,
                                                     p(one), opt(ntr, ip), lp(roff), p(one), p(np.zeros(64)), ip(gidx),
                                                     lp(L(0, 2)), p(np.array([0.5, 1.0])), opt(echo, ip), p(one), 0,
                                                     *[opt(a, p) for a in m0], ndir, *[opt(a, p) for a in (*v, *dm0, *pe, *pf, *te, *tf)])
    big = 2 ** 31 - 1
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(echo=None), "required array is null"),
             (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"), (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"),
             (dict(gidx=I(0, 2, 1, 0)), "gain index of pulse 0 lies outside"), (dict(m0=(one, None, one)), "m0x, m0y and m0z"),
             (dict(dm0=(one, None, one)), "dm0x, dm0y and dm0z"), (dict(pe=(outs[0], None, outs[2])), "the echo planes are given together"),
             (dict(pf=(None, outs[4], outs[5])), "the final planes are given together"),
             (dict(te=(outs[6], outs[7], None)), "the tangent echo planes are given together"),
             (dict(tf=(None, outs[10], None)), "the tangent final planes are given together"),
             (dict(v=(None, None)), "no direction is given"),
             (dict(te=N, tf=N), "neither the tangent echo planes nor the tangent final planes"),
             (dict(ndir=0), "ndir must be at least 1"), (dict(ndir=-3), "ndir must be at least 1"),
             # one direction fits (2^30 points, 4 repetitions, 2 combinations); 2^31 - 1 of them overflow the tangent echoes
             (dict(ndir=big, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
             # 2^30 points x 4 repetitions x ndir tangent echo entries exceed 2^56 from ndir = 2^24 on; the workspace does not grow
             (dict(ndir=2 ** 25, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        for o in outs:
            o[:] = np.nan
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_train_jvp_sched_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
        assert all(np.all(np.isnan(o)) for o in outs), kw                         # nothing was written
    assert call() == 0
    assert call(pe=N) == 0 and call(pf=N) == 0 and call(te=N) == 0 and call(tf=N) == 0
    assert call(v=(one, None)) == 0 and call(v=(None, one)) == 0 and call(v=(None, None), dm0=(one, one, one)) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    v = np.ones((2, 4))
    ((we, wf), (wte, wtf)), = mbfir.bloch_train_jvp_sched_batch([pulse], d[:2], d[:3], 4, tangents_gains=[v], tangents_phases=[v],
                                                                phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2, final=True,
                                                                primal=True)
    assert call() == 0
    for o, w in zip(outs, we + wf + wte + wtf):
        assert np.array_equal(o[:w.size], w.ravel())


def test_torchsim_forward_mode_in_the_schedule_is_the_direct_call_and_reverse_mode_keeps_its_bits():
    import torch
    fwAD = torch.autograd.forward_ad
    c = ref.small()
    p, df, dp, n = c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0]
    dg, dph, _ = _one(ref.directions("small", 3), 2)[0]
    vs, _ = ref.jvp.directions("small", 1)
    kw = dict(echo=c["echo"][0], scales=(0.9, 1.1), meq=0.5)
    m0h = np.stack(c["m0"][0])
    b1 = torch.tensor(p[0], dtype=torch.complex128)
    g, ph = torch.tensor(c["gains"][0], dtype=torch.float64), torch.tensor(c["phases"][0], dtype=torch.float64)
    vg, vp, vb = torch.tensor(dg), torch.tensor(dph), torch.tensor(vs[0][0])
    args = (p[1], p[2], p[3], p[4], df, dp, n)
    direct = dict(phases=c["phases"][0], gains=c["gains"][0], m0=[tuple(m0h)], final=True, **kw)

    def f(b, gg, pp, forward_mode=True):
        out = mbfir.torchsim.bloch_train(b, *args, nucleus=p[5], m0=m0h, gains=gg, phases=pp, final=True, forward_mode=forward_mode, **kw)
        return out[0] + out[1]
    out, tan = torch.func.jvp(lambda gg, pp: f(b1, gg, pp), (g, ph), (vg, vp))
    ((we, wf), (wte, wtf)), = mbfir.bloch_train_jvp_sched_batch([p], df, dp, n, tangents_gains=[dg], tangents_phases=[dph], primal=True,
                                                                **direct)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(out, we + wf))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(tan, wte + wtf))
    _, tan = torch.func.jvp(lambda gg: f(b1, gg, c["phases"][0]), (g,), (vg,))    # the gains alone
    (wte, wtf), = mbfir.bloch_train_jvp_sched_batch([p], df, dp, n, tangents_gains=[dg], **direct)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(tan, wte + wtf))
    with fwAD.dual_level():                                                      # a dual tensor in the phases alone
        out = f(b1, c["gains"][0], fwAD.make_dual(ph, vp))
        te = [fwAD.unpack_dual(e).tangent.numpy() for e in out]
    (wte, wtf), = mbfir.bloch_train_jvp_sched_batch([p], df, dp, n, tangents_phases=[dph], **direct)
    assert _eq(te, wte + wtf)
    _, tan = torch.func.jvp(lambda b, gg: f(b, gg, c["phases"][0]), (b1, g), (vb, vg))         # jointly with b1: the two calls' sum
    (ste, stf), = mbfir.bloch_train_jvp_sched_batch([p], df, dp, n, tangents_gains=[dg], **direct)
    (bte, btf), = mbfir.bloch_train_jvp_batch([p], df, dp, n, [vs[0][0]], **direct)
    assert all(np.array_equal(t.numpy(), a + b) for t, a, b in zip(tan, ste + stf, bte + btf))
    grads = []
    for fm in (True, False):                                                      # reverse mode: the new class against its parent
        gr, pr = g.clone().requires_grad_(True), ph.clone().requires_grad_(True)
        out = f(b1, gr, pr, forward_mode=fm)
        sum((o * (i + 1.0)).sum() for i, o in enumerate(out)).backward()
        grads.append((gr.grad.numpy().copy(), pr.grad.numpy().copy()))
    assert _eq(grads[0], grads[1]) and np.abs(grads[0][0]).max() > 0
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda gg: f(b1, gg, c["phases"][0], forward_mode=False), (g,), (vg,))
