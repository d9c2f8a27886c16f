"""The fused least-squares and Gauss-Newton products of the pulse train on the device (mbfir.bloch_train_lsq_batch,
mbfir.bloch_train_gn_batch: k_bloch_train_run_lsq, k_bloch_train_run_gn, k_bloch_train_gn_fold with the shipped k_bloch_train_prop,
k_bloch_train_prop_jvp and k_bloch_train_prop_vjp) against the long-double reference of tests/blochtraingn_ref.py, against the two
shipped two-call paths, against central differences of the shipped mbfir.bloch_train_batch, for exact zeros and for the
bit-invariance of a result under the batch's composition; and mbfir.refine_bloch_train_batch on the device.

Every comparison with the reference is held to the bounds that blochtraingn_ref composes through the seed and fixed on the CPU;
each test prints the share of its bound that the device takes, and DESIGN section 8ab quotes the worst ones."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtraingn_ref", os.path.join(ROOT, "tests", "blochtraingn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
tr, vjp = ref.tr, ref.vjp
CASES = list(ref.cases())


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _opt(v):
    return None if v[0] is None else list(v)


def _train_kw(c):
    return dict(phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"], m0=_opt(c["m0"]),
                meq=c["meq"], demod=c["demod"])


def _kw(c):
    return dict(_train_kw(c), rep_weights=None if c["rw"] is None else list(c["rw"]), weights_final=_opt(c["wf"]))


def _lsq(c, **over):
    df, dp = _grids(c)
    kw = dict(_kw(c), targets_final=_opt(c["tf"]), grad_m0=True)
    kw.update(over)
    return mbfir.bloch_train_lsq_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["t"]), _opt(c["w"]), **kw)


def _gn(c, vs, **over):
    df, dp = _grids(c)
    kw = _kw(c)
    kw.update(over)
    return mbfir.bloch_train_gn_batch(c["pulses"], df, dp, list(c["ntr"]), list(vs), _opt(c["w"]), **kw)


def _sub(c, idx):
    """the pulses idx of a case as a case"""
    d = dict(c)
    for k in ("pulses", "dfs", "dps", "ntr", "phases", "gains", "echo", "m0", "w", "t", "wf", "tf", "ce", "cf"):
        d[k] = [c[k][q] for q in idx]
    d["rw"] = None if c["rw"] is None else [c["rw"][q] for q in idx]
    return d


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))


@pytest.mark.parametrize("name", CASES)
def test_device_loss_gradient_and_products_are_the_longdouble_reference(name):
    c = ref.cases()[name]
    got, want = _lsq(c), ref.reference(name)
    vs = ref.directions(name, 3)
    hs = {K: _gn(c, [v[:K] for v in vs]) for K in (1, 2, 3)}
    assert len(got) == len(c["pulses"])
    for q, (L, g, gm) in enumerate(got):
        Lr, gr, gmr = want[q]
        assert g.shape == gr.shape and all(a.shape == b.shape for a, b in zip(gm, gmr)), q
        sl, sg = ref.share(L - Lr, ref.bound_l(c, q)), ref.share(g - gr, ref.bound_g(c, q))
        sm = max(ref.share(a - b, ref.bound_gm(c, q)) for a, b in zip(gm, gmr))
        H, bh = ref.reference_gn(name, 3)[q], ref.bound_h(c, q, vs[q])
        sh = max(ref.share(hs[K][q] - H[:K], bh[:K]) for K in (1, 2, 3))
        assert all(hs[K][q].shape == (K, len(gr)) for K in (1, 2, 3))
        print("%s pulse %d: device against long double, shares: L %.3g, g %.3g, dL/dm0 %.3g, H v %.3g" % (name, q, sl, sg, sm, sh))
        assert max(sl, sg, sm, sh) <= 1, (q, sl, sg, sm, sh)


@pytest.mark.parametrize("name", CASES)
def test_fused_results_against_the_two_shipped_two_call_paths(name):
    c = ref.cases()[name]
    df, dp = _grids(c)
    P, ntr = len(c["pulses"]), list(c["ntr"])
    fwd = mbfir.bloch_train_batch(c["pulses"], df, dp, ntr, final=True, **_train_kw(c))
    W = [ref.full(c, q, c["w"][q]) for q in range(P)]
    T = [ref.full(c, q, c["t"][q]) for q in range(P)]
    rw = [ref.rw_of(c, q)[None, :, None, None] for q in range(P)]
    echo, final = c["w"][0] is not None, c["wf"][0] is not None
    ce = [tuple(rw[q] * W[q][i] * (fwd[q][0][i] - T[q][i]) for i in range(3)) for q in range(P)] if echo else None
    cf = [tuple(c["wf"][q][i] * (fwd[q][1][i] - c["tf"][q][i]) for i in range(3)) for q in range(P)] if final else None
    two = mbfir.bloch_train_vjp_batch(c["pulses"], df, dp, ntr, ce, cot_final=cf, grad_m0=True, **_train_kw(c))
    got = _lsq(c)
    vs = ref.directions(name, 2)
    tan = mbfir.bloch_train_jvp_batch(c["pulses"], df, dp, ntr, list(vs), final=True, **_train_kw(c))
    hv = _gn(c, vs)
    for q in range(P):
        L2 = 0.0
        if echo:
            L2 += sum(0.5 * float((rw[q] * W[q][i] * (fwd[q][0][i] - T[q][i]) ** 2).sum()) for i in range(3))
        if final:
            L2 += sum(0.5 * float((c["wf"][q][i] * (fwd[q][1][i] - c["tf"][q][i]) ** 2).sum()) for i in range(3))
        sl, sg = ref.share(got[q][0] - L2, ref.bound_l(c, q)), ref.share(got[q][1] - two[q][0], ref.bound_g(c, q))
        sm = max(ref.share(a - b, ref.bound_gm(c, q)) for a, b in zip(got[q][2], two[q][1]))
        bh, sh = ref.bound_h(c, q, vs[q]), 0.0
        for k in range(2):
            cek = [tuple(rw[q] * W[q][i] * tan[q][0][i][k] for i in range(3))] if echo else None
            cfk = [tuple(c["wf"][q][i] * tan[q][1][i][k] for i in range(3))] if final else None
            s1 = _sub(c, [q])
            h2, = mbfir.bloch_train_vjp_batch(s1["pulses"], c["dfs"][q], c["dps"][q], [ntr[q]], cek, cot_final=cfk, **_train_kw(s1))
            sh = max(sh, ref.share(hv[q][k] - h2, bh[k]))
        print("%s pulse %d: fused against the two-call paths, shares: L %.3g, g %.3g, dL/dm0 %.3g, H v %.3g" % (name, q, sl, sg, sm, sh))
        assert max(sl, sg, sm, sh) <= 1, (q, sl, sg, sm, sh)


@pytest.mark.parametrize("name", ["groups", "batch", "allgains", "h1_long"])
def test_targets_equal_to_the_trains_own_output_give_a_zero_loss_and_exact_zero_gradients(name):
    c = ref.cases()[name]
    assert not c["bcast"]
    df, dp = _grids(c)
    fwd = mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), final=True, **_train_kw(c))
    over = dict(targets_final=[f for _, f in fwd] if c["wf"][0] is not None else None)
    kw = dict(_kw(c), grad_m0=True, **over)
    res = mbfir.bloch_train_lsq_batch(c["pulses"], df, dp, list(c["ntr"]), [e for e, _ in fwd] if c["w"][0] is not None else None,
                                      _opt(c["w"]), **kw)
    for L, g, gm in res:
        assert L == 0.0 and np.all(g == 0) and all(np.all(v == 0) for v in gm)


@pytest.mark.parametrize("name", ref.BCAST)
def test_the_broadcast_form_has_the_bits_of_the_full_form_with_the_planes_repeated(name):
    c = ref.cases()[name]
    P = len(c["pulses"])
    rep = dict(c, w=[ref.full(c, q, c["w"][q]) for q in range(P)], t=[ref.full(c, q, c["t"][q]) for q in range(P)])
    assert np.ndim(c["w"][0][0]) == 3 and np.ndim(rep["w"][0][0]) == 4
    vs = ref.directions(name, 2)
    for a, b in zip(_lsq(c), _lsq(rep)):
        assert _same(a, b)
    for a, b in zip(_gn(c, vs), _gn(rep, vs)):
        assert np.array_equal(a, b)


def test_central_difference_of_the_shipped_train_along_the_gradient():
    c = ref.small()
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    (_, g, _), = _lsq(c)
    ghat = g / np.sqrt(ref.redot(g, g))
    h = float((ref.fd_steps(c, 0) / np.maximum(np.maximum(np.abs(ghat.real), np.abs(ghat.imag)), 1e-300)).min())       # no sample turns by more than FD_ANGLE
    moved = [(p[0] + s * h * ghat,) + tuple(p[1:]) for s in (1, -1)]
    res = mbfir.bloch_train_batch(moved, df, dp, c["ntr"][0], final=True, **dict(_train_kw(c), phases=c["phases"][0], gains=c["gains"][0],
                                                                                echo=c["echo"][0], m0=c["m0"][0]))
    W, T, rw = ref.full(c, 0, c["w"][0]), ref.full(c, 0, c["t"][0]), ref.rw_of(c, 0)[None, :, None, None]
    Ls = [sum(0.5 * float((rw * W[i] * (e[i] - T[i]) ** 2).sum()) + 0.5 * float((c["wf"][0][i] * (f[i] - c["tf"][0][i]) ** 2).sum())
              for i in range(3)) for e, f in res]
    fd, want = (Ls[0] - Ls[1]) / (2 * h), float(ref.redot(ghat, g))
    scale = float((ref.scale_fd(c, 0) * (np.abs(ghat.real) + np.abs(ghat.imag))).sum())
    print("central difference along g: %.3g of the scale (FD_TOL %.0e)" % (abs(fd - want) / scale, ref.FD_TOL))
    assert abs(fd - want) <= ref.FD_TOL * scale


def test_exact_zeros():
    c = ref.cases()["groups"]
    vs = ref.directions("groups", 2)
    P = len(c["pulses"])
    for h in _gn(c, [np.zeros_like(v) for v in vs]):
        assert np.all(h == 0)
    zero = lambda tri: tuple(np.zeros_like(v) for v in tri)
    z = dict(c, w=[zero(t) for t in c["w"]], wf=[zero(t) for t in c["wf"]])
    for L, g, gm in _lsq(z):
        assert L == 0.0 and np.all(g == 0) and all(np.all(v == 0) for v in gm)
    for h in _gn(z, vs):
        assert np.all(h == 0)
    norw = dict(c, rw=[np.zeros(n) for n in c["ntr"]], wf=[None] * P, tf=[None] * P)
    for L, g, gm in _lsq(norw):
        assert L == 0.0 and np.all(g == 0) and all(np.all(v == 0) for v in gm)
    for h in _gn(norw, vs):
        assert np.all(h == 0)
    s0 = dict(c, scales=(0.0,))
    for (L, g, gm), h in zip(_lsq(s0), _gn(s0, vs)):
        assert L > 0 and np.all(g == 0) and np.all(h == 0)


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated():
    c = ref.cases()["groups"]
    vs = ref.directions("groups", 3)
    alone = [(_lsq(_sub(c, [q]))[0], _gn(_sub(c, [q]), [vs[q]])[0]) for q in range(3)]
    idx = [k % 3 for k in range(17)]
    for order in (idx, idx[::-1], [1, 1, 1]):
        s = _sub(c, order)
        for q, a, h in zip(order, _lsq(s), _gn(s, [vs[q] for q in order])):
            assert _same(a, alone[q][0]) and np.array_equal(h, alone[q][1]), (order, q)


def test_a_direction_has_the_same_bits_at_every_place_and_at_every_k():
    c = ref.cases()["allgains"]
    v = ref.directions("allgains", 3)[0]
    one, = _gn(c, [v[1]])
    assert one.shape == v[1].shape
    for K in (1, 2, 3):
        for place in range(K):
            order = [k for k in range(3) if k != 1][:K - 1]
            order.insert(place, 1)
            h, = _gn(c, [v[order]])
            assert np.array_equal(h[place], one), (K, place)


@pytest.mark.parametrize("name", [n for n in CASES if len(ref.cases()[n]["scales"]) > 1])
def test_each_scale_alone_sums_to_the_sweep_within_the_bound(name):
    c = ref.cases()[name]
    vs = ref.directions(name, 1)
    whole, hw = _lsq(c), _gn(c, vs)
    parts = []
    for k, s in enumerate(c["scales"]):
        at = lambda tris: [None if t is None else tuple(np.asarray(v)[k:k + 1] for v in t) for t in tris]
        d = dict(c, scales=(s,), w=at(c["w"]), t=at(c["t"]), wf=at(c["wf"]), tf=at(c["tf"]))
        parts.append((_lsq(d), _gn(d, vs)))
    for q in range(len(c["pulses"])):
        L = sum(p[0][q][0] for p in parts)
        g = sum(p[0][q][1] for p in parts)
        h = sum(p[1][q] for p in parts)
        sl, sg = ref.share(L - whole[q][0], ref.bound_l(c, q)), ref.share(g - whole[q][1], ref.bound_g(c, q))
        sh = ref.share(h - hw[q], ref.bound_h(c, q, vs[q]))
        print("%s pulse %d: the scales one by one against the sweep, shares: L %.3g, g %.3g, H v %.3g" % (name, q, sl, sg, sh))
        assert max(sl, sg, sh) <= 1


@pytest.mark.parametrize("name", ["small", "groups", "p65"])
def test_the_products_are_symmetric_and_positive_semidefinite(name):
    c = ref.case_of(name)
    vs = ref.directions(name, 2)
    for q, h in enumerate(_gn(c, vs)):
        u, v = vs[q]
        assert abs(ref.redot(u, h[1]) - ref.redot(h[0], v)) <= ref.pair_tol(c, q, u, v)
        assert ref.redot(v, h[1]) >= -ref.pair_tol(c, q, v, v) / 2 and ref.redot(u, h[0]) >= -ref.pair_tol(c, q, u, u) / 2


def _raw_tables(ntr, gains, phi, echo, meq):
    uq, gi = np.unique(gains, return_inverse=True)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([echo], dtype=np.int32), np.array([meq])]
    ip, lp, ptr = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp)), mbfir._ptr
    return tab, [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8])]


def test_outputs_are_written_in_full_and_nowhere_else():
    """The raw calls with NaN sentinels: every entry of the wanted outputs is written, the 16 entries after them are not, unwanted
    dL/dm0 planes are left alone, and the bits are the Python calls'"""
    c = ref.cases()["allgains"]
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0]
    n, S, O = len(p[0]), 2, 2 * 6
    vs = ref.directions("allgains", 3)[0]
    wf = tuple(np.full((S, 3, 2), 0.5 + i) for i in range(3))
    tf = tuple(np.full((S, 3, 2), 0.1 * i) for i in range(3))
    d = dict(c, wf=[wf], tf=[tf])
    (Lp, gp, gmp), = _lsq(d)
    hp, = _gn(d, [vs])
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    A = mbfir._BlochArgs("raw", [p], df, dp, c["scales"])
    keep, targs = _raw_tables(ntr, c["gains"][0], c["phases"][0], c["echo"][0], c["meq"])
    m0 = A.m0_planes(c["m0"][0], np.array([0, O]), [1])
    flat = lambda tri: [np.ascontiguousarray(np.ravel(v)) for v in tri]
    w, t, wfp, tfp = flat(c["w"][0]), flat(c["t"][0]), flat(wf), flat(tf)
    for want_m0 in (True, False):
        loss, gr, gi = np.full(1 + 16, np.nan), np.full(n + 16, np.nan), np.full(n + 16, np.nan)
        gm = [np.full(O + 16, np.nan) for _ in range(3)]
        rc = lib.mbfir_bloch_train_lsq_batch(ctx._h, *A.head, *targs, int(c["demod"]), *[ptr(a) for a in m0], 0,
                                             *[ptr(a) for a in w + t], None, *[ptr(a) for a in wfp + tfp], ptr(loss), ptr(gr), ptr(gi),
                                             *[ptr(a) if want_m0 else None for a in gm])
        assert rc == 0, ctx.last_error()
        assert loss[0] == Lp and np.all(np.isnan(loss[1:]))
        assert np.array_equal(gr[:n] + 1j * gi[:n], gp) and np.all(np.isnan(gr[n:])) and np.all(np.isnan(gi[n:]))
        for a, b in zip(gm, gmp):
            assert np.array_equal(a[:O], b.ravel()) and np.all(np.isnan(a[O:])) if want_m0 else np.all(np.isnan(a))
    K = 3
    v = [np.ascontiguousarray(vs.real.ravel()), np.ascontiguousarray(vs.imag.ravel())]
    hr, hi = np.full(K * n + 16, np.nan), np.full(K * n + 16, np.nan)
    rc = lib.mbfir_bloch_train_gn_batch(ctx._h, *A.head, *targs, int(c["demod"]), *[ptr(a) for a in m0], 0, *[ptr(a) for a in w], None,
                                        *[ptr(a) for a in wfp], K, ptr(v[0]), ptr(v[1]), ptr(hr), ptr(hi))
    assert rc == 0, ctx.last_error()
    assert np.array_equal((hr[:K * n] + 1j * hi[:K * n]).reshape(K, n), hp) and np.all(np.isnan(hr[K * n:])) and np.all(np.isnan(hi[K * n:]))


def test_refine_on_the_device_lowers_the_loss_and_a_pulse_alone_has_its_bits_in_a_batch():
    """the 9-sample period, 3 x 2 points, 9 repetitions, three gains, two outer iterations"""
    c = ref.small()
    p = c["pulses"][0]
    rng = np.random.default_rng(5)
    ntr, gains = 9, np.tile([0.5, 0.75, 1.0], 3)
    pulses = [(p[0] * s,) + tuple(p[1:]) for s in (1.0, 0.9, 1.1)]
    w = (np.ones((3, 2)), np.ones((3, 2)), 0.5)
    tg = tuple(rng.uniform(-0.5, 0.5, (3, 2)) for _ in range(3))
    rw = np.r_[0.0, 0.0, np.ones(7)]
    kw = dict(rep_weights=rw, phases=np.pi, gains=gains, echo=c["echo"][0], m0=c["m0"][0], demod=True, iters=2, cg=4)
    b1s, infos = mbfir.refine_bloch_train_batch(pulses, c["dfs"][0], c["dps"][0], ntr, [tg] * 3, [w] * 3, **kw)
    for q in range(3):
        L = infos[q]["losses"]
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
        (b1,), (info,) = mbfir.refine_bloch_train_batch([pulses[q]], c["dfs"][0], c["dps"][0], ntr, [tg], [w], **kw)
        assert np.array_equal(b1, b1s[q]) and info["losses"] == L


def test_errors_of_the_raw_calls_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    neg, nan = np.r_[one[:5], -1.0, one[:58]], np.r_[one[:5], np.nan, one[:58]]
    rneg, rnan = np.r_[1.0, -1.0, one[:62]], np.r_[1.0, 1.0, 1.0, np.inf, one[:60]]
    outs = [np.zeros(64) for _ in range(6)]
    N3, N6 = (None,) * 3, (None,) * 6

    def opt(a, f=p):
        return f(a) if a is not None else None

    def head(npulse, toff, tsoff, nfgrid, foff, npgrid, poff, nscale, ntr, roff, echo):
        return (ctx._h, npulse, lp(toff), p(d), p(d), None, None, None, lp(tsoff), p(d), p(one), p(one), p(one), nfgrid, lp(foff), p(d),
                npgrid, lp(poff), p(d), None, None, nscale, p(one), opt(ntr, ip), lp(roff), p(one), p(np.zeros(64)), ip(I(0, 1, 1, 0)),
                lp(L(0, 2)), p(np.array([0.5, 1.0])), opt(echo, ip), p(one), 0, None, None, None)

    def lsq(npulse=1, toff=L(0, 3), tsoff=L(0, 1), nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, ntr=I(4), roff=L(0, 4),
            echo=I(2), ebcast=0, wt=(one,) * 6, rw=None, wtf=(one,) * 6, loss=outs[0], g=(outs[1], outs[2]), gm=tuple(outs[3:6])):
        return lib.mbfir_bloch_train_lsq_batch(*head(npulse, toff, tsoff, nfgrid, foff, npgrid, poff, nscale, ntr, roff, echo), ebcast,
                                               *[opt(a) for a in wt], opt(rw), *[opt(a) for a in wtf], opt(loss), *[opt(a) for a in g],
                                               *[opt(a) for a in gm])

    def gn(npulse=1, toff=L(0, 3), tsoff=L(0, 1), nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, ntr=I(4), roff=L(0, 4),
           echo=I(2), ebcast=0, w=(one,) * 3, rw=None, wf=(one,) * 3, ndir=2, v=(d, d), h=(outs[1], outs[2])):
        return lib.mbfir_bloch_train_gn_batch(*head(npulse, toff, tsoff, nfgrid, foff, npgrid, poff, nscale, ntr, roff, echo), ebcast,
                                              *[opt(a) for a in w], opt(rw), *[opt(a) for a in wf], ndir, *[opt(a) for a in v],
                                              *[opt(a) for a in h])
    big = 2 ** 31 - 1
    shared = ((dict(npulse=0), "no pulses"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
              (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(ebcast=2), "ebcast must be 0 or 1"),
              (dict(ebcast=-1), "ebcast must be 0 or 1"), (dict(rw=rneg), "a repetition weight is negative or not finite"),
              (dict(rw=rnan), "a repetition weight is negative or not finite"))
    lsq_cases = shared + ((dict(wt=(one, None) + (one,) * 4), "the echo weights and targets are given together"),
                          (dict(wt=(one,) * 5 + (None,)), "the echo weights and targets are given together"),
                          (dict(wtf=(None,) + (one,) * 5), "the final weights and targets are given together"),
                          (dict(wt=N6, wtf=N6), "neither an echo term nor a final term"), (dict(loss=None), "a loss or gradient plane is null"),
                          (dict(g=(None, outs[2])), "a loss or gradient plane is null"),
                          (dict(gm=(outs[3], None, outs[5])), "gmx, gmy and gmz"), (dict(wt=(neg,) + (one,) * 5), "a weight is negative"),
                          (dict(wtf=(one, nan) + (one,) * 4), "a weight is negative or not finite"),
                          (dict(ebcast=1, wt=(one, one, neg) + (one,) * 3), "a weight is negative"))
    gn_cases = shared + ((dict(w=(one, None, one)), "the echo weights are given together"),
                         (dict(wf=(None, one, one)), "the final weights are given together"),
                         (dict(w=N3, wf=N3), "neither an echo term nor a final term"), (dict(v=(None, d)), "a direction or product plane is null"),
                         (dict(h=(outs[1], None)), "a direction or product plane is null"), (dict(ndir=0), "ndir must be at least 1"),
                         (dict(ndir=-3), "ndir must be at least 1"), (dict(w=(one, neg, one)), "a weight is negative"),
                         (dict(wf=(nan, one, one)), "a weight is negative or not finite"),
                         # 2^30 points, 2^31 - 1 directions: the workgroups and the planes' tangents overflow before a plane is read
                         (dict(ndir=big, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
                         (dict(ndir=2 ** 21, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    for call, who, cases in ((lsq, "bloch_train_lsq_batch:", lsq_cases), (gn, "bloch_train_gn_batch:", gn_cases)):
        assert call() == 0, ctx.last_error()
        for kw, why in cases:
            assert call(**kw) == mbfir.E_ARG, kw
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call() == 0
    assert lsq(wt=N6) == 0 and lsq(wtf=N6) == 0 and lsq(gm=N3) == 0 and lsq(ebcast=1) == 0 and lsq(rw=one) == 0
    assert gn(w=N3) == 0 and gn(wf=N3) == 0 and gn(ebcast=1, rw=one) == 0
    assert lib.mbfir_bloch_train_lsq_batch(None, *head(1, L(0, 3), L(0, 1), 1, L(0, 2), 1, L(0, 3), 1, I(4), L(0, 4), I(2))[1:], 0,
                                           *[p(one)] * 6, None, *[p(one)] * 6, p(outs[0]), p(outs[1]), p(outs[2]), None, None,
                                           None) == mbfir.E_ARG
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    kw = dict(phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2)
    (Lw, gw, gmw), = mbfir.bloch_train_lsq_batch([pulse], d[:2], d[:3], 4, [(1.0, 1.0, 1.0)], [(1.0, 1.0, 1.0)], targets_final=[(1.0,) * 3],
                                                 weights_final=[(1.0,) * 3], grad_m0=True, **kw)
    assert lsq() == 0
    assert outs[0][0] == Lw and np.array_equal(outs[1][:3] + 1j * outs[2][:3], gw)
    assert all(np.array_equal(o[:6], m.ravel()) for o, m in zip(outs[3:6], gmw))
    v = np.stack([d[:3] * (1 + 1j), d[3:6] * (1 + 1j)])
    hw, = mbfir.bloch_train_gn_batch([pulse], d[:2], d[:3], 4, [v], [(1.0, 1.0, 1.0)], weights_final=[(1.0,) * 3], **kw)
    assert gn() == 0
    assert np.array_equal((outs[1][:6] + 1j * outs[2][:6]).reshape(2, 3), hw)
