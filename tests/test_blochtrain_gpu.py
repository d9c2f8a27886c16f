"""The pulse train on the device (mbfir.bloch_train_batch: k_bloch_train_prop, k_bloch_train_run; mbfir.bloch_prop_batch: the first
kernel alone) against the long-double recursion over the tiled waveform of tests/blochtrain_ref.py, against the shipped steady state
(mbfir.bloch_batch(mode=1)) through the device's own propagators, against the shipped recording call (mode=2) on the tiled waveform,
and for the bit-invariance of a train's results under the batch's composition, the scale sweep and the train's length.

Bound of every comparison with the reference: C u ntr (ntime + 4) mu per echo or final entry and C u (ntime + 4) per propagator entry,
C = 200, u = 2^-53, mu = max(|m0|inf, |meq|, 1) over the point (blochtrain_ref counts C; tests/test_blochtrain_cpu.py holds the
float64 reference within a hundredth of it).  Measured worst shares on the device: 7.0e-3 for the trains (h1_long) and 5.3e-3 for
the propagators (the 257-sample period of batch)."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrain_ref", os.path.join(ROOT, "tests", "blochtrain_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
CASES = list(ref.cases())


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _m0(c):
    return None if c["m0"][0] is None else list(c["m0"])


def _run(name, meq, **kw):
    c = ref.cases()[name]
    df, dp = _grids(c)
    return mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), phases=list(c["phases"]), gains=list(c["gains"]),
                                   echo=list(c["echo"]), scales=c["scales"], m0=_m0(c), meq=meq, **kw)


def _planes(tri, axis):
    return np.stack(tri, axis)


@pytest.mark.parametrize("name", CASES)
def test_device_trains_are_the_longdouble_tiled_recursion(name):
    """Echo planes and final planes of every case, demod off and on, meq in {1, 1e-4, 0}"""
    c = ref.cases()[name]
    worst = 0.0
    for meq in ref.MEQS:
        want, bd = ref.reference(name, meq), ref.case_bounds(name, meq)
        for demod in (False, True):
            got = _run(name, meq, demod=demod, final=True)
            assert len(got) == len(c["pulses"])
            for q, (e, f) in enumerate(got):
                E, F = _planes(e, 2), _planes(f, 1)                                # (S, ntr, 3, nf, npos), (S, 3, nf, npos)
                assert E.shape == want[q][0].shape and F.shape == want[q][1].shape, (q, E.shape, F.shape)
                wE = want[q][0]
                if demod:
                    wE = np.stack([ref.demodulate(w, c["phases"][q], np.longdouble) for w in wE])
                sE = float((np.abs(E - wE).astype(np.float64) / bd[q]).max())
                sF = float((np.abs(F - want[q][1]).astype(np.float64) / bd[q]).max())
                print("%s meq %g demod %d pulse %d (n %d, ntr %d, echo %d): |dev - ref| / bound: echoes %.3g, final %.3g; bound %.3g"
                      % (name, meq, demod, q, len(c["pulses"][q][0]), c["ntr"][q], c["echo"][q], sE, sF, float(np.max(bd[q]))))
                worst = max(worst, sE, sF)
                assert np.all(np.isfinite(E)) and np.all(np.isfinite(F)) and sE <= 1 and sF <= 1, (meq, demod, q)
    print("%s: worst share of the bound %.3g" % (name, worst))


def test_echoes_without_the_final_planes_have_the_same_bits():
    full = _run("batch", 1e-4, final=True)
    only = _run("batch", 1e-4)
    for (e, _), o in zip(full, only):
        assert all(np.array_equal(a, b) for a, b in zip(e, o))


@pytest.mark.parametrize("name", CASES)
def test_device_propagators_are_the_longdouble_ones_entry_by_entry(name):
    c = ref.cases()[name]
    df, dp = _grids(c)
    got = mbfir.bloch_prop_batch(c["pulses"], df, dp, echo=list(c["echo"]), scales=c["scales"])
    for q, p in enumerate(c["pulses"]):
        want = ref.prop_arrays(p, c["dfs"][q], c["dps"][q], c["scales"], c["echo"][q], np.longdouble)
        assert ref.max_angle(p, c["dfs"][q], c["dps"][q], max(c["scales"])) <= 2 * np.pi
        bd = ref.bound_prop(len(p[0]))
        sh = [float(np.abs(g - w).max()) / bd for g, w in zip(got[q], want)]
        print("%s pulse %d (n %d, echo %d): |dev - ref| / bound: A %.3g, B %.3g, Ae %.3g, Be %.3g"
              % ((name, q, len(p[0]), c["echo"][q]) + tuple(sh)))
        assert all(g.shape == w.shape for g, w in zip(got[q], want)) and max(sh) <= 1, q
        if c["echo"][q] == 0:                                                      # (I, 0), exactly
            assert np.array_equal(got[q][2], np.broadcast_to(np.eye(3), got[q][2].shape)) and not got[q][3].any()
        if c["echo"][q] == len(p[0]):                                              # (A, B), to the bit
            assert np.array_equal(got[q][2], got[q][0]) and np.array_equal(got[q][3], got[q][1])


@pytest.mark.parametrize("name", ["c13_ramp", "h1_long", "batch"])
def test_fixed_point_of_the_device_propagators_is_the_shipped_steady_state(name):
    """(I - A)^-1 B in long double from the device's (A, B) against bloch_batch(mode=1), within blochss_ref's 1e-12 kappa^2"""
    c = ref.cases()[name]
    df, dp = _grids(c)
    prop = mbfir.bloch_prop_batch(c["pulses"], df, dp, scales=c["scales"])
    ss = mbfir.bloch_batch(c["pulses"], df, dp, scales=c["scales"], mode=1)
    for q, p in enumerate(c["pulses"]):
        k = ref.ss.kappa(p, c["dfs"][q], c["dps"][q], c["scales"])
        A, B = prop[q][0].astype(np.longdouble), prop[q][1].astype(np.longdouble)
        Ae = [[A[..., i, j] for j in range(3)] for i in range(3)]
        inv = ref.ss.inverse(Ae)
        M = ref._grad._mat_vec(inv, [B[..., i] for i in range(3)])
        err = max(float(np.abs(M[i] - ss[q][i]).max()) for i in range(3))
        print("%s pulse %d: kappa %.4g, |(I - A)^-1 B - mode 1| %.3g of the bound %.3g" % (name, q, k, err, ref.ss.bound_m(k)))
        assert err <= ref.ss.bound_m(k), q


@pytest.mark.parametrize("name", CASES)
def test_device_trains_are_the_shipped_recording_call_on_the_tiled_waveform(name):
    """bloch_batch(mode=2) on concat_k gains[k] e^{i phi_k} b1 at the echo samples (meq = 1, the only one it knows), two device
    paths against each other: the sum of the two bounds, C u mu (ntr (ntime + 4) + ntr ntime)"""
    c = ref.cases()[name]
    got = _run(name, 1.0, final=True)
    for q, p in enumerate(c["pulses"]):
        n, N, echo = len(p[0]), c["ntr"][q], c["echo"][q]
        rec, = mbfir.bloch_batch([ref.tile_pulse(p, c["phases"][q], c["gains"][q])], c["dfs"][q], c["dps"][q], scales=c["scales"],
                                 mode=2, m0=c["m0"][q])
        rec = np.stack(rec, -1)                                                    # (S, nf, npos, N n, 3)
        mu = ref.mu_of(c["m0"][q], 1.0, rec.shape[1], rec.shape[2])
        bd = ref.C_BOUND * ref.U * mu * (N * (n + 4) + N * n)
        start = np.broadcast_to(np.stack([np.asarray(v, dtype=np.float64) for v in ref._grad._m0(c["m0"][q], rec.shape[1], rec.shape[2],
                                                                                                 np.float64)], -1), rec[:, :, :, 0].shape)
        E = np.stack(got[q][0], -1)                                                # (S, ntr, nf, npos, 3)
        worst = 0.0
        for k in range(N):
            t = k * n + echo - 1
            w = rec[:, :, :, t] if t >= 0 else start
            worst = max(worst, float((np.abs(E[:, k] - w).max(-1) / bd).max()))
        sF = float((np.abs(np.stack(got[q][1], -1) - rec[:, :, :, -1]).max(-1) / bd).max())
        print("%s pulse %d: |train - tiled mode 2| / bound: echoes %.3g, final %.3g" % (name, q, worst, sF))
        assert worst <= 1 and sF <= 1, q


def _raw_head(ctx, pulse, df, dp, scales):
    A = mbfir._BlochArgs("raw", [pulse], df, dp, scales)
    return A, [ctx._h] + A.head


def test_outputs_are_written_in_full_and_nowhere_else():
    """The raw call with NaN sentinels: every entry of a given plane is written, the 16 entries after it are not, and a call that
    asks for one triple alone returns that triple's bits"""
    c = ref.cases()["c13_ramp"]
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], 5
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    (we, wf), = mbfir.bloch_train_batch([p], df, dp, ntr, gains=c["gains"][0][:ntr], echo=4, scales=c["scales"], m0=c["m0"], meq=1e-4,
                                        final=True)
    A, head = _raw_head(ctx, p, df, dp, c["scales"])
    uq, gi = np.unique(c["gains"][0][:ntr], return_inverse=True)
    phi = np.pi * np.arange(ntr)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([4], dtype=np.int32), np.array([1e-4])]
    ip, lp = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp))
    targs = [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8]), 0]
    m0 = A.m0_planes(c["m0"], np.array([0, 3 * 6]), [1])
    E, O = 3 * ntr * 6, 3 * 6
    for want_e, want_f in ((True, False), (False, True), (True, True)):
        e = [np.full(E + 16, np.nan) for _ in range(3)]
        f = [np.full(O + 16, np.nan) for _ in range(3)]
        rc = lib.mbfir_bloch_train_batch(*head, *targs, *[ptr(v) for v in m0], *[ptr(v) if want_e else None for v in e],
                                         *[ptr(v) if want_f else None for v in f])
        assert rc == 0, ctx.last_error()
        for v, w in zip(e, we):
            assert np.all(np.isnan(v[E:])) and (np.array_equal(v[:E], w.ravel()) if want_e else np.all(np.isnan(v)))
        for v, w in zip(f, wf):
            assert np.all(np.isnan(v[O:])) and (np.array_equal(v[:O], w.ravel()) if want_f else np.all(np.isnan(v)))


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_a_train_has_the_same_bits_alone_in_17_reversed_and_repeated():
    rng = np.random.default_rng(51)
    lengths = [int(v) for v in rng.integers(1, 300, 17)]
    sc = [0.9, 1.1]
    pulses, dfs, dps, ntr, phs, gns, ech, m0s = [], [], [], [], [], [], [], []
    for q, n in enumerate(lengths):
        dt = 8e-6
        b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (1.0 + 0.1 * q) / (ref.GAMMA_H1 * n * dt)
        pulses.append((b1, rng.uniform(0.5, 1.5, n) * 0.1, np.append(np.full(n - 1, dt), 1e-3), 0.8, 3e-2 + 1e-3 * q, "H-1"))
        nf, npos = 1 + q % 3, 5 + 40 * q
        dfs.append(ref._grid(nf, 150.0))
        dps.append(ref._grid(npos, 3.0))
        ntr.append(1 + 37 * q)                                                  # 1 .. 593 repetitions: up to three tiles of the table
        phs.append(rng.uniform(-np.pi, np.pi, ntr[-1]))
        gns.append(rng.choice([0.5, 0.8, 1.0, 1.2][:1 + q % 4], ntr[-1]))
        ech.append(int(rng.integers(0, n + 1)))
        m0s.append(tuple(rng.uniform(-0.5, 0.5, (3, nf, npos))))

    def run(idx, scales=sc):
        sel = lambda a: [a[i] for i in idx]
        res = mbfir.bloch_train_batch(sel(pulses), sel(dfs), sel(dps), sel(ntr), phases=sel(phs), gains=sel(gns), echo=sel(ech),
                                      scales=scales, m0=sel(m0s), meq=0.3, final=True)
        return [tuple(e) + tuple(f) for e, f in res]
    order = list(range(17))
    full, again, rev = run(order), run(order), run(order[::-1])[::-1]
    for q in range(17):
        assert _same(full[q], again[q]) and _same(full[q], rev[q]), q
    for q in (0, 5, 16):
        assert _same(run([q])[0], full[q]), q
        assert _same(run([q, q])[1], full[q]), q
        for si, s in enumerate(sc):                                              # each scale alone has the sweep's bits
            assert _same(run([q], (s,))[0], [v[si:si + 1] for v in full[q]]), (q, s)


def test_a_train_is_the_prefix_of_a_longer_one():
    """257 and 600 repetitions of the ramp (three distinct gains) against their first 2 (two distinct gains), 3 (three) and 256:
    the repetition table's tiles and the hoisted planes of a train with one distinct gain make no difference to the bits"""
    c = ref.cases()["c13_ramp"]
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    N = 600
    ph, gn = 0.7 * np.arange(N) ** 1.5, np.minimum(1.0, 0.5 + 0.25 * np.arange(N))

    def run(n, gains=gn):
        (e, f), = mbfir.bloch_train_batch([p], df, dp, n, phases=ph[:n], gains=gains[:n], echo=4, scales=c["scales"], m0=c["m0"],
                                          meq=1e-4, final=True)
        return e, f
    long_e, long_f = run(N)
    for n in (1, 2, 3, 256, 257):
        e, f = run(n)
        assert all(np.array_equal(a, b[:, :n]) for a, b in zip(e, long_e)), n
        assert f[0].shape == long_f[0].shape
    flat = np.ones(N)
    one_e, _ = run(300, flat)                                                    # one distinct gain: the planes are hoisted
    mix = flat.copy()
    mix[299] = 0.5                                                               # two distinct gains: they are loaded per repetition
    two_e, _ = run(300, mix)
    assert all(np.array_equal(a[:, :299], b[:, :299]) for a, b in zip(one_e, two_e))
    assert not np.array_equal(one_e[0][:, 299], two_e[0][:, 299])


def test_a_final_state_chains_trains_to_the_bit():
    c = ref.cases()["c13_ramp"]
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    ph, gn = np.pi * np.arange(40), c["gains"][0][:40]
    kw = dict(echo=9, scales=(1.1,), meq=1e-4, final=True)
    (e, f), = mbfir.bloch_train_batch([p], df, dp, 40, phases=ph, gains=gn, m0=c["m0"], **kw)
    (e1, f1), = mbfir.bloch_train_batch([p], df, dp, 25, phases=ph[:25], gains=gn[:25], m0=c["m0"], **kw)
    (e2, f2), = mbfir.bloch_train_batch([p], df, dp, 15, phases=ph[25:], gains=gn[25:], m0=[tuple(v[0] for v in f1)], **kw)
    assert all(np.array_equal(a[:, 25:], b) for a, b in zip(e, e2)) and _same(f, f2)
    assert all(np.array_equal(a[:, -1], b) for a, b in zip(e, f))                # echo = ntime: the last echo is the final state


def test_zero_magnetisation_without_recovery_stays_exactly_zero():
    for name in ("c13_ramp", "batch"):
        c = ref.cases()[name]
        df, dp = _grids(c)
        zero = [(0.0, 0.0, 0.0)] * len(c["pulses"])
        res = mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), phases=list(c["phases"]), gains=list(c["gains"]),
                                      echo=list(c["echo"]), scales=c["scales"], m0=zero, meq=0.0, final=True)
        for e, f in res:
            assert not any(v.any() for v in e) and not any(v.any() for v in f)


def test_scale_zero_is_the_zero_b1_train():
    c = ref.cases()["c13_ramp"]
    p, df, dp = c["pulses"][0], c["dfs"][0], c["dps"][0]
    z = (np.zeros_like(p[0]),) + p[1:]
    kw = dict(phases=c["phases"][0], gains=c["gains"][0], echo=4, m0=c["m0"], meq=1e-4, final=True)
    (e0, f0), = mbfir.bloch_train_batch([p], df, dp, 257, scales=(0.0,), **kw)
    (ez, fz), = mbfir.bloch_train_batch([z], df, dp, 257, scales=(1.0,), **kw)
    assert _same(e0, ez) and _same(f0, fz)
    E, F = ref.tiled(z, df, dp, 257, c["phases"][0], c["gains"][0], 4, 1.0, c["m0"][0], 1e-4, np.longdouble)
    bd = ref.bound_train(257, 9, ref.mu_of(c["m0"][0], 1e-4, 3, 2))
    sh = max(float((np.abs(np.stack(e0, 2)[0] - E).astype(np.float64) / bd).max()),
             float((np.abs(np.stack(f0, 1)[0] - F).astype(np.float64) / bd).max()))
    print("scale 0 against the long-double zero-b1 recursion: share of the bound %.3g" % sh)
    assert sh <= 1


def test_errors_of_the_raw_calls_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    outs = [np.zeros(64) for _ in range(6)]
    mats = [np.zeros(9 * 6), np.zeros(3 * 6), np.zeros(9 * 6), np.zeros(3 * 6)]

    def opt(a, f):
        return f(a) if a is not None else None

    def head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1):
        return (ctx._h, npulse, lp(toff), opt(b1, p), p(d), None, None, None, lp(tsoff), p(d), p(t1), p(one), p(one), nfgrid, lp(foff),
                p(d), npgrid, lp(poff), p(d), None, None, nscale, p(one))

    def train(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
              ntr=I(4), roff=L(0, 4), cs=one, sn=np.zeros(64), gidx=I(0, 1, 1, 0), goff=L(0, 2), gains=np.array([0.5, 1.0]),
              echo=I(2), meq=one, m0=(None, None, None), e=outs[:3], f=outs[3:]):
        return lib.mbfir_bloch_train_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), opt(ntr, ip),
                                           opt(roff, lp), opt(cs, p), opt(sn, p), opt(gidx, ip), opt(goff, lp), opt(gains, p),
                                           opt(echo, ip), opt(meq, p), 0, *[opt(v, p) for v in (*m0, *e, *f)])

    def prop(npulse=1, toff=L(0, 3), tsoff=L(0, 1), t1=one, nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, b1=d,
             echo=I(2), out=mats):
        return lib.mbfir_bloch_prop_batch(*head(npulse, toff, tsoff, t1, nfgrid, foff, npgrid, poff, nscale, b1), opt(echo, ip),
                                          *[opt(v, p) for v in out])
    big = 2 ** 31 - 1
    nan, inf = float("nan"), float("inf")
    shared = ((dict(npulse=0), "no pulses"), (dict(nscale=0), "scale list is empty"), (dict(toff=L(0, 0)), "no samples"),
              (dict(tsoff=L(0, 2)), "neither 1 nor"), (dict(t1=np.zeros(64)), "must be positive"), (dict(foff=L(0, 0)), "empty item"),
              (dict(poff=L(0, 0)), "empty item"), (dict(nfgrid=2), "1 or npulse"), (dict(npgrid=3), "1 or npulse"),
              (dict(b1=None), "required array is null"), (dict(echo=None), "required array is null"),
              (dict(foff=L(0, big), poff=L(0, big), nscale=4), "overflows"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
              (dict(echo=I(-1)), "echo of pulse 0 must lie in [0, ntime]"))
    own = {train: ((dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(roff=L(0, 3)), "does not span its ntr"),
                   (dict(goff=L(0, 0)), "between 1 and ntr distinct gains"),
                   (dict(gidx=I(0, 2, 1, 0)), "gain index of pulse 0 lies outside"),
                   (dict(gidx=I(0, -1, 1, 0)), "gain index of pulse 0 lies outside"),
                   (dict(gains=np.array([0.5, inf])), "a gain is not finite"),
                   (dict(cs=np.full(64, nan)), "cosine or sine"), (dict(sn=np.full(64, inf)), "cosine or sine"),
                   (dict(meq=np.full(64, nan)), "meq of pulse 0 is not finite"), (dict(gains=None), "required array is null"),
                   (dict(m0=(one, None, one)), "m0x, m0y and m0z"), (dict(e=[outs[0], None, outs[2]]), "echo planes are given together"),
                   (dict(f=[None, outs[4], outs[5]]), "final planes are given together"),
                   (dict(e=[None] * 3, f=[None] * 3), "neither the echo planes nor the final planes"),
                   (dict(ntr=I(big), roff=L(0, big), foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows")),
           prop: ((dict(out=[mats[0], None, mats[2], mats[3]]), "required array is null"),)}
    for call, who in ((train, "bloch_train_batch:"), (prop, "bloch_prop_batch:")):
        assert call() == 0, ctx.last_error()
        for kw, why in shared + own[call]:
            assert call(**kw) == mbfir.E_ARG, kw
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call() == 0
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    assert train(f=[None] * 3) == 0 and train(e=[None] * 3) == 0
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    (we, wf), = mbfir.bloch_train_batch([pulse], d[:2], d[:3], 4, phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2, final=True)
    assert train() == 0
    assert all(np.array_equal(o[:24], w.ravel()) for o, w in zip(outs[:3], we))
    assert all(np.array_equal(o[:6], w.ravel()) for o, w in zip(outs[3:], wf))
