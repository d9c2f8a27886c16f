"""The tangent of the pulse train on the device (mbfir.bloch_train_jvp_batch: k_bloch_train_prop, k_bloch_train_prop_jvp,
k_bloch_train_run_jvp) against the long-double reference of tests/blochtrainjvp_ref.py, against central differences of the shipped
mbfir.bloch_train_batch, against the shipped adjoint mbfir.bloch_train_vjp_batch through the adjoint identity, against the shipped
mbfir.bloch_jvp_batch on the tiled waveform, for the bit-invariance of a tangent under the composition of the direction groups and
of the batch, and through mbfir.torchsim.bloch_train(forward_mode=True).

Bound of every comparison with the reference (blochtrainjvp_ref.bound_jvp): TOL ntr (ntr max|scale gain| gamma sum dt |v| mu +
|dm0|_1) per entry, TOL = 1e-12.  Measured worst share on the device: 1.4e-2 of the bound (the 257-sample period of batch at K = 4
and 5); DESIGN section 8aa quotes it from this file's output."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainjvp_ref", os.path.join(ROOT, "tests", "blochtrainjvp_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
tr = ref.tr
CASES = list(ref.cases())


def _groups():
    return mbfir.bloch_train_jvp_group()


def _kmax():
    return max(_groups()) + 1


def _counts():
    """K = 1, each kernel's group size and each group size + 1"""
    return sorted({1} | {g + d for g in _groups() for d in (0, 1)})


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _m0(c):
    return None if c["m0"][0] is None else list(c["m0"])


def _kw(c, **more):
    kw = dict(phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"], m0=_m0(c), meq=c["meq"],
              demod=c["demod"])
    kw.update(more)
    return kw


def _jvp(c, vs, dms, **more):
    df, dp = _grids(c)
    return mbfir.bloch_train_jvp_batch(c["pulses"], df, dp, list(c["ntr"]), vs, tangents_m0=dms, **_kw(c, **more))


def _cut(vs, dms, K):
    return [v[:K] for v in vs], None if dms is None else [tuple(d[:K] for d in tri) for tri in dms]


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", CASES)
def test_device_tangents_are_the_longdouble_reference_and_the_primal_is_the_forward_calls(name):
    c = ref.cases()[name]
    df, dp = _grids(c)
    fwd = mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), final=True, **_kw(c))
    vs, dms = ref.directions(name, _kmax())
    want = ref.reference(name, _kmax())
    for K in _counts():
        v, d = _cut(vs, dms, K)
        got = _jvp(c, v, d, final=True, primal=True)
        assert len(got) == len(c["pulses"])
        for q, ((pe, pf), (te, tf)) in enumerate(got):
            assert _eq(pe, fwd[q][0]) and _eq(pf, fwd[q][1]), (K, q)             # the primal has bloch_train_batch's bits
            dE, dF = want[q]
            bound = ref.bound_jvp(c, q, v[q], d[q])
            assert te[0].shape == dE[0][:K].shape and tf[0].shape == dF[0][:K].shape, (K, q)
            se = max(float((np.abs(a - b[:K]) / bound[:, None, None]).max()) for a, b in zip(te, dE))
            sf = max(float((np.abs(a - b[:K]) / bound[:, None]).max()) for a, b in zip(tf, dF))
            print("%s pulse %d K %d: device against long double, share of the bound %.3g (echoes), %.3g (final)" % (name, q, K, se, sf))
            assert se <= 1 and sf <= 1, (K, q, se, sf)


def test_central_differences_of_the_shipped_train():
    """The small case along each of two directions: b1 moved by +-h v (h as blochtrainjvp_ref derives it), all four trains in one
    bloch_train_batch call; then m0 moved by +-FD_M0 dm0.  Tolerances: FD_TOL of the scales in the reference's docstring."""
    c = ref.small()
    K = 2
    vs, dms = ref.directions("small", K)
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    kw = dict(phases=c["phases"][0], gains=c["gains"][0], echo=c["echo"][0], scales=c["scales"], meq=c["meq"], demod=c["demod"], final=True)
    (te, tf), = mbfir.bloch_train_jvp_batch([p], df, dp, c["ntr"][0], [vs[0]], m0=c["m0"], **kw)
    h = ref.FD_ANGLE / ref.drive(c, 0, vs[0])
    moved = [(p[0] + sgn * h[k] * vs[0][k],) + p[1:] for k in range(K) for sgn in (1, -1)]
    res = mbfir.bloch_train_batch(moved, df, dp, c["ntr"][0], m0=c["m0"][0], **kw)
    scale = c["ntr"][0] * ref.drive(c, 0, vs[0])[:, None, None] * ref.mu_of(c, 0)
    worst = 0.0
    for k in range(K):
        (ep, fp), (em, fm) = res[2 * k], res[2 * k + 1]
        for i in range(3):
            worst = max(worst, float((np.abs((ep[i] - em[i]) / (2 * h[k]) - te[i][k]) / scale[k]).max()),
                        float((np.abs((fp[i] - fm[i]) / (2 * h[k]) - tf[i][k]) / scale[k]).max()))
    print("central differences along v: worst %.3g of the scale (FD_TOL %.0e)" % (worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL
    (te, tf), = mbfir.bloch_train_jvp_batch([p], df, dp, c["ntr"][0], [np.zeros_like(vs[0])], tangents_m0=[dms[0]], m0=c["m0"], **kw)
    m0 = np.stack(c["m0"][0])
    worst = 0.0
    for k in range(K):
        d = np.stack([x[k] for x in dms[0]])
        sm = np.maximum(np.abs(d).sum(0), 1.0)
        (ep, fp), (em, fm) = mbfir.bloch_train_batch([p, p], df, dp, c["ntr"][0],
                                                     m0=[tuple(m0 + ref.FD_M0 * d), tuple(m0 - ref.FD_M0 * d)], **kw)
        for i in range(3):
            worst = max(worst, float((np.abs((ep[i] - em[i]) / (2 * ref.FD_M0) - te[i][k]) / sm).max()),
                        float((np.abs((fp[i] - fm[i]) / (2 * ref.FD_M0) - tf[i][k]) / sm).max()))
    print("central differences along dm0: worst %.3g of the scale (FD_TOL %.0e)" % (worst, ref.FD_TOL))
    assert worst <= ref.FD_TOL


@pytest.mark.parametrize("name", CASES)
def test_the_adjoint_identity_against_the_shipped_adjoint(name):
    """sum ce . decho + sum cf . dm_N = Re sum conj(G) v + sum gm0 . dm_0 with the cases' cotangents; the tolerance is the two
    sides' own bounds added"""
    c = ref.cases()[name]
    df, dp = _grids(c)
    opt = lambda v: None if v[0] is None else list(v)
    adj = mbfir.bloch_train_vjp_batch(c["pulses"], df, dp, list(c["ntr"]), opt(c["ce"]), cot_final=opt(c["cf"]), grad_m0=True, **_kw(c))
    vs, dms = ref.directions(name, 1)
    tan = _jvp(c, [v[0] for v in vs], [tuple(d[0] for d in tri) for tri in dms], final=True)
    for q, ((G, gm), (te, tf)) in enumerate(zip(adj, tan)):
        d0 = tuple(d[0] for d in dms[q])
        left = ref.pairing(c, q, te, tf)
        right = float((np.conj(G) * vs[q][0]).real.sum()) + sum(float((g * d).sum()) for g, d in zip(gm, d0))
        tol = ref.identity_tol(c, q, vs[q][0], d0)
        print("%s pulse %d: adjoint identity off by %.3g of its tolerance" % (name, q, abs(left - right) / tol))
        assert abs(left - right) <= tol, (q, left, right, tol)


def test_the_final_tangent_is_the_shipped_bloch_jvp_batch_on_the_tiled_waveform():
    """h1_long: the direction tiled as gains[k] e^{+i phi_k} v_t, the sense of the tiled waveform itself; tolerance: the two bounds
    added (blochjvp_ref.bound_jvp for the tiled call)"""
    c = ref.cases()["h1_long"]
    p, df, dp, ph, gn = c["pulses"][0], c["dfs"][0], c["dps"][0], c["phases"][0], c["gains"][0]
    K = 2
    vs, dms = ref.directions("h1_long", K)
    tf, = _jvp(c, [vs[0]], [dms[0]], echoes=False, final=True)
    tiled = tr.tile_pulse(p, ph, gn)
    vt = np.stack([tr.tile_b1(v, ph, gn) for v in vs[0]])
    (_, tt), = mbfir.bloch_jvp_batch([tiled], df, dp, [vt], scales=c["scales"], m0=[c["m0"][0]], tangents_m0=[dms[0]])
    bound = ref.bound_jvp(c, 0, vs[0], dms[0]) + ref.jv.bound_jvp(tiled, vt, dms[0], c["scales"])
    sh = max(float((np.abs(a - b) / bound[:, None]).max()) for a, b in zip(tf, tt))
    print("against bloch_jvp_batch on the tiled waveform: share of the summed bounds %.3g" % sh)
    assert sh <= 1
    wrong = np.stack([tr.tile_b1(v, -ph, gn) for v in vs[0]])                     # the opposite sense is far off
    (_, tw), = mbfir.bloch_jvp_batch([tiled], df, dp, [wrong], scales=c["scales"], m0=[c["m0"][0]], tangents_m0=[dms[0]])
    assert max(float((np.abs(a - b) / bound[:, None]).max()) for a, b in zip(tf, tw)) > 1e6


def test_a_direction_has_the_same_bits_alone_among_others_first_or_last_in_its_group():
    c = ref.cases()["allgains"]
    gmax = max(_groups())
    K = 2 * gmax + 1
    vs, dms = ref.directions("allgains", K)
    full, = _jvp(c, vs, dms, final=True)
    for k in sorted({0, gmax - 1, gmax, K - 1} | {g - 1 for g in _groups()} | set(_groups())):
        alone, = _jvp(c, [vs[0][k]], [tuple(d[k] for d in dms[0])], final=True)
        assert _eq(alone[0], [e[k] for e in full[0]]) and _eq(alone[1], [f[k] for f in full[1]]), k
    rev, = _jvp(c, [vs[0][::-1]], [tuple(d[::-1] for d in dms[0])], final=True)
    assert _eq([e[::-1] for e in rev[0]], full[0]) and _eq([f[::-1] for f in rev[1]], full[1])


def test_a_tangent_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(57)
    lengths = [int(v) for v in rng.integers(1, 300, 17)]
    sc = [0.9, 1.1]
    K = max(_groups()) + 1
    pulses, dfs, dps, ntr, phs, gns, ech, m0s, vs, dms = [], [], [], [], [], [], [], [], [], []
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
        vs.append((rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * np.abs(b1).max())
        dms.append(tuple(rng.standard_normal((3, K, nf, npos))))

    def run(idx):
        sel = lambda a: [a[i] for i in idx]
        return mbfir.bloch_train_jvp_batch(sel(pulses), sel(dfs), sel(dps), sel(ntr), sel(vs), tangents_m0=sel(dms), phases=sel(phs),
                                           gains=sel(gns), echo=sel(ech), scales=sc, m0=sel(m0s), meq=0.3, final=True)
    same = lambda a, b: _eq(a[0], b[0]) and _eq(a[1], b[1])
    order = list(range(17))
    full, again, rev = run(order), run(order), run(order[::-1])[::-1]
    for q in range(17):
        assert same(full[q], again[q]) and same(full[q], rev[q]), q
    for q in (0, 5, 16):
        assert same(run([q])[0], full[q]), q
        assert same(run([q, q])[1], full[q]), q


def test_bits_do_not_depend_on_the_sweep_the_trains_length_or_what_is_asked_for():
    c = ref.cases()["allgains"]
    K = max(_groups()) + 1
    vs, dms = ref.directions("allgains", K)
    (te, tf), = _jvp(c, vs, dms, final=True)
    for k, s in enumerate(c["scales"]):                                          # each scale alone and in the sweep
        (e1, f1), = _jvp(c, vs, dms, final=True, scales=(s,))
        assert _eq([e[:, 0] for e in e1], [e[:, k] for e in te]) and _eq([f[:, 0] for f in f1], [f[:, k] for f in tf]), s
    n = 3                                                                        # the prefix of a longer train
    cut = dict(c, ntr=[n], phases=[c["phases"][0][:n]], gains=[c["gains"][0][:n]])
    e3, = _jvp(cut, vs, dms)
    uq = np.unique(c["gains"][0][:n])
    assert len(uq) < len(np.unique(c["gains"][0]))                               # other combinations, another workspace
    assert _eq(e3, [e[:, :, :n] for e in te])
    e_only, = _jvp(c, vs, dms)                                                   # with and without final, primal, echoes
    assert _eq(e_only, te)
    f_only, = _jvp(c, vs, dms, echoes=False, final=True)
    assert _eq(f_only, tf)
    (pr, (e2, f2)), = _jvp(c, vs, dms, final=True, primal=True)
    assert _eq(e2, te) and _eq(f2, tf)
    (pf, f3), = _jvp(c, vs, dms, echoes=False, final=True, primal=True)
    assert _eq(f3, tf) and _eq(pf, pr[1])
    one, = _jvp(c, [vs[0][0]], None)                                             # a 1-D tangent drops the K axis
    assert one[0].shape == te[0].shape[1:]


def test_scale_zero_without_an_m0_direction_gives_exact_zeros():
    c = ref.cases()["c13_ramp"]
    vs, _ = ref.directions("c13_ramp", 2)
    (te, tf), = _jvp(c, vs, None, final=True, scales=(0.0,))
    assert te[0].shape == (2, 1, 257, 3, 2) and not any(v.any() for v in te + tf)
    (te, _), = _jvp(c, vs, None, final=True)
    assert all(v.any() for v in te)


def test_the_m0_direction_alone_is_the_trains_linear_part():
    """v = 0: the tangent is the forward train of m0 = dm_0 at meq = 0, within the forward bound (blochtrain_ref.bound_train)"""
    for name in ("c13_ramp", "batch"):
        c = ref.cases()[name]
        df, dp = _grids(c)
        vs, dms = ref.directions(name, 1)
        tan = _jvp(c, [np.zeros_like(v[0]) for v in vs], [tuple(d[0] for d in tri) for tri in dms], final=True)
        lin = mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), final=True,
                                      **_kw(c, m0=[tuple(d[0] for d in tri) for tri in dms], meq=0.0))
        for q, ((te, tf), (le, lf)) in enumerate(zip(tan, lin)):
            mu = tr.mu_of(tuple(d[0] for d in dms[q]), 0.0, len(c["dfs"][q]), len(c["dps"][q]))
            bound = tr.bound_train(c["ntr"][q], len(c["pulses"][q][0]), mu)
            assert max(float((np.abs(a - b) / bound).max()) for a, b in zip(te + tf, le + lf)) <= 1, (name, q)


def _raw_tables(ntr, gains, phi, echo, meq):
    uq, gi = np.unique(gains, return_inverse=True)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([echo], dtype=np.int32), np.array([meq])]
    ip, lp, ptr = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp)), mbfir._ptr
    return tab, [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8]), 0]


def test_outputs_are_written_in_full_and_nowhere_else():
    """The raw call with NaN sentinels: every entry of the wanted planes is written, the 16 entries after them are not, an unwanted
    triple is left alone, and the bits are the Python call's"""
    c = ref.cases()["c13_ramp"]
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], 11
    K = max(_groups()) + 1
    vs, dms = ref.directions("c13_ramp", K)
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    (wp, (we, wf)), = mbfir.bloch_train_jvp_batch([p], df, dp, ntr, [vs[0]], tangents_m0=[dms[0]], gains=c["gains"][0][:ntr], echo=4,
                                                  scales=c["scales"], m0=c["m0"], meq=1e-4, final=True, primal=True)
    A = mbfir._BlochArgs("raw", [p], df, dp, c["scales"])
    keep, targs = _raw_tables(ntr, c["gains"][0][:ntr], np.pi * np.arange(ntr), 4, 1e-4)
    S, O = 3, 3 * 6
    E = O * ntr
    m0 = A.m0_planes(c["m0"], np.array([0, O]), [1])
    v = [np.ascontiguousarray(vs[0].real.ravel()), np.ascontiguousarray(vs[0].imag.ravel())]
    d0 = [np.ascontiguousarray(np.broadcast_to(d[:, None], (K, S, 3, 2)).ravel()) for d in dms[0]]
    for want in ((1, 1, 1, 1), (0, 0, 1, 0), (0, 1, 0, 1), (1, 0, 1, 1)):
        sizes = (E, O, K * E, K * O)
        out = [[np.full(n + 16, np.nan) for _ in range(3)] for n in sizes]
        planes = [ptr(a) if w else None for w, tri in zip(want, out) for a in tri]
        rc = lib.mbfir_bloch_train_jvp_batch(ctx._h, *A.head, *targs, *[ptr(a) for a in m0], K, ptr(v[0]), ptr(v[1]),
                                             *[ptr(a) for a in d0], *planes)
        assert rc == 0, ctx.last_error()
        for w, n, tri, py in zip(want, sizes, out, (wp[0], wp[1], we, wf)):
            for a, b in zip(tri, py):
                assert np.all(np.isnan(a[n:])), want
                assert np.array_equal(a[:n], b.ravel()) if w else np.all(np.isnan(a)), want


def test_errors_of_the_raw_call_leave_the_context_usable():
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

    def call(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d, ntr=I(4),
             roff=L(0, 4), cs=one, sn=np.zeros(64), gidx=I(0, 1, 1, 0), goff=L(0, 2), gains=np.array([0.5, 1.0]), echo=I(2), meq=one,
             m0=N, ndir=2, v=(d, d), dm0=N, pe=outs[:3], pf=outs[3:6], te=outs[6:9], tf=outs[9:]):
        return lib.mbfir_bloch_train_jvp_batch(ctx._h, npulse, lp(toff), opt(b1, p), p(d), None, None, None, lp(tsoff), p(d), p(t1),
                                               p(one), p(one), nfgrid, lp(foff), p(d), npgrid, lp(poff), p(d), None, None, nscale,
                                               p(one), opt(ntr, ip), opt(roff, lp), opt(cs, p), opt(sn, p), opt(gidx, ip),
                                               opt(goff, lp), opt(gains, p), opt(echo, ip), opt(meq, p), 0, *[opt(a, p) for a in m0],
                                               ndir, *[opt(a, p) for a in (*v, *dm0, *pe, *pf, *te, *tf)])
    big = 2 ** 31 - 1
    nan, inf = float("nan"), float("inf")
    cases = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
             (dict(b1=None), "required array is null"), (dict(echo=None), "required array is null"),
             (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"), (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"),
             (dict(roff=L(0, 3)), "does not span its ntr"), (dict(goff=L(0, 0)), "between 1 and ntr distinct gains"),
             (dict(gidx=I(0, 2, 1, 0)), "gain index of pulse 0 lies outside"), (dict(gains=np.array([0.5, inf])), "a gain is not finite"),
             (dict(cs=np.full(64, nan)), "cosine or sine"), (dict(meq=np.full(64, nan)), "meq of pulse 0 is not finite"),
             (dict(m0=(one, None, one)), "m0x, m0y and m0z"),
             (dict(v=(None, d)), "a direction plane is null"), (dict(v=(d, None)), "a direction plane is null"),
             (dict(dm0=(one, None, one)), "dm0x, dm0y and dm0z"), (dict(pe=(outs[0], None, outs[2])), "the echo planes are given together"),
             (dict(pf=(None, outs[4], outs[5])), "the final planes are given together"),
             (dict(te=(outs[6], outs[7], None)), "the tangent echo planes are given together"),
             (dict(tf=(None, outs[10], None)), "the tangent final planes are given together"),
             (dict(te=N, tf=N), "neither the tangent echo planes nor the tangent final planes"),
             (dict(ndir=0), "ndir must be at least 1"), (dict(ndir=-3), "ndir must be at least 1"),
             # one direction fits (2^30 points, 4 repetitions, 2 combinations); 2^31 - 1 of them overflow every count
             (dict(ndir=big, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
             # ndir x 24 x 2 x 2^30 doubles of tangent planes exceed 2^56 from ndir = 2^21 on
             (dict(ndir=2 ** 21, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    assert call() == 0, ctx.last_error()
    for kw, why in cases:
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("bloch_train_jvp_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0
    assert call(pe=N) == 0 and call(pf=N) == 0 and call(te=N) == 0 and call(tf=N) == 0 and call(dm0=(one, one, one)) == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    v = np.stack([d[:3] * (1 + 1j), d[3:6] * (1 + 1j)])
    ((we, wf), (wte, wtf)), = mbfir.bloch_train_jvp_batch([pulse], d[:2], d[:3], 4, [v], phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]),
                                                          echo=2, final=True, primal=True)
    assert call() == 0
    for o, w in zip(outs, we + wf + wte + wtf):
        assert np.array_equal(o[:w.size], w.ravel())


def test_torch_func_jvp_through_torchsim_is_the_direct_call():
    import torch
    c = ref.small()
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    vs, dms = ref.directions("small", 1)
    kw = dict(phases=c["phases"][0], gains=c["gains"][0], echo=c["echo"][0], scales=(0.9, 1.1), meq=0.5)
    m0h = np.stack(c["m0"][0])
    b1, m0 = torch.tensor(p[0], dtype=torch.complex128), torch.tensor(m0h, dtype=torch.float64)
    vb, vm = torch.tensor(vs[0][0]), torch.tensor(np.stack([d[0] for d in dms[0]]))
    args = (p[1], p[2], p[3], p[4], df, dp, 3)

    def f(b, m):
        out = mbfir.torchsim.bloch_train(b, *args, nucleus=p[5], m0=m, final=True, forward_mode=True, **kw)
        return out[0] + out[1]
    out, tan = torch.func.jvp(f, (b1, m0), (vb, vm))
    ((we, wf), (wte, wtf)), = mbfir.bloch_train_jvp_batch([p], df, dp, 3, [vs[0][0]], tangents_m0=[tuple(d[0] for d in dms[0])],
                                                          m0=[tuple(m0h)], final=True, primal=True, **kw)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(out, we + wf))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(tan, wte + wtf))
    with torch.autograd.forward_ad.dual_level():                                 # a dual tensor in b1 alone, echoes only
        dual = torch.autograd.forward_ad.make_dual(b1, vb)
        E = mbfir.torchsim.bloch_train(dual, *args, nucleus=p[5], m0=m0h, forward_mode=True, **kw)
        te = [torch.autograd.forward_ad.unpack_dual(e).tangent.numpy() for e in E]
    wt, = mbfir.bloch_train_jvp_batch([p], df, dp, 3, [vs[0][0]], m0=[tuple(m0h)], **kw)
    assert _eq(te, wt)
    with pytest.raises(NotImplementedError, match="forward-mode"):
        torch.func.jvp(lambda b: mbfir.torchsim.bloch_train(b, *args, nucleus=p[5], **kw), (b1,), (vb,))
