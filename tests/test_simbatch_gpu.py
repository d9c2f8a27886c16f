"""Batched device simulators (mbfir.bloch_batch, abr_batch, sim_rf_scale_batch: k_bloch_batch, k_abr_batch) against one
single-pulse call per (pulse, scale), against the oracle, bit for bit against themselves in other batches, and their argument
errors."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir
from oracle import bloch as obloch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
LENGTHS = [1, 7, 255, 256, 257, 2000, 5000]
GRIDS = [(3, 5), (16, 16), (37, 11), (256, 1), (1, 300), (50, 6), (20, 20)]     # (nf, npos): below, at and above 256 pairs
SMALL = [(2, 3), (3, 2), (1, 4), (4, 1), (2, 2), (3, 1), (1, 1)]                 # record modes: the output stays small
NUCLEI = ["C-13", "H-1", 10000.0]
SCALES = [1.0, 0.0, 0.9, 1.2]


def _cpu():
    spec = importlib.util.spec_from_file_location("ssmb_cpu", os.path.join(ROOT, "tests", "test_ssmb_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pulses(seed, lengths, relax):
    """bloch pulses: 1 .. 3 gradient axes, tp a scalar / intervals / end times, C-13, H-1 and a numeric gamma in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for q, nt in enumerate(lengths):
        b1 = (rng.standard_normal(nt) + 1j * rng.standard_normal(nt)) * 0.05     # G
        gr = rng.standard_normal((nt, 1 + q % 3)) * 0.2                           # G/cm
        ts = rng.uniform(2e-6, 6e-6, nt)                                          # s
        tp = (4e-6, ts, np.cumsum(ts))[q % 3]
        t1, t2 = relax(q)
        out.append((b1, gr, tp, t1, t2, NUCLEI[q % 3]))
    return out


def _grids(seed, shapes):
    rng = np.random.default_rng(seed)
    dfs = [np.linspace(-3000, 3000, nf) + rng.uniform(-10, 10) for nf, _ in shapes]
    dps = [rng.standard_normal((npos, 1 + q % 3)) for q, (_, npos) in enumerate(shapes)]
    return dfs, dps


def _against_single(res, pulses, scales, dfs, dps, mode, m0=None):
    """largest |batch - single mbfir.bloch call| over every (pulse, scale), and whether every entry is bit-identical"""
    worst, same = 0.0, True
    for q, (pulse, got) in enumerate(zip(pulses, res)):
        b1, gr, tp, t1, t2, nuc = pulse
        df, dp = dfs[q % len(dfs)], dps[q % len(dps)]
        kw = {} if m0 is None else dict(zip(("mx", "my", "mz"), m0))
        for k, s in enumerate(scales):
            want = mbfir.bloch(np.asarray(b1) * s, gr, tp, t1, t2, df, dp, mode, nucleus=nuc, **kw)
            for c in range(3):
                # bloch drops the time axis of a one-sample pulse in record mode; bloch_batch keeps (S, nf, npos, ntime)
                assert got[c][k].shape == (want[c].shape + (1,) if got[c][k].ndim > want[c].ndim else want[c].shape)
                w = want[c].reshape(got[c][k].shape)
                worst = max(worst, float(np.abs(got[c][k] - w).max()))
                same = same and np.array_equal(got[c][k], w)
    return worst, same


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_bloch_batch_matches_single_calls(mode):
    relax = (lambda q: (2e-3, 1e-3)) if mode & 1 else (lambda q: (0.08, 0.03) if q % 2 else (1e3, 1e3))
    shapes = SMALL if mode & 2 else GRIDS
    pulses = _pulses(100 + mode, LENGTHS, relax)
    dfs, dps = _grids(200 + mode, shapes)
    res = mbfir.bloch_batch(pulses, dfs, dps, scales=SCALES, mode=mode)
    for (nf, npos), nt, r in zip(shapes, LENGTHS, res):
        assert r[0].shape == ((len(SCALES), nf, npos, nt) if mode & 2 else (len(SCALES), nf, npos))
    worst, same = _against_single(res, pulses, SCALES, dfs, dps, mode)
    print("bloch_batch mode %d: max |batch - single| %.3g, bit-identical %s" % (mode, worst, same))
    assert worst <= TOL and same                                    # measured: bit-identical


def test_bloch_batch_shared_grid_and_initial_magnetisation():
    pulses = _pulses(7, [300, 1, 520], lambda q: (0.05, 0.02))
    rng = np.random.default_rng(8)
    df, dp = np.linspace(-800, 800, 23), rng.standard_normal((13, 3))
    m0 = tuple(rng.standard_normal((23, 13)) * 0.4 for _ in range(3))
    for mode in (0, 1, 2):
        res = mbfir.bloch_batch(pulses, df, dp, scales=[1.1, 1.0], mode=mode, m0=m0)
        worst, same = _against_single(res, pulses, [1.1, 1.0], [df], [dp], mode, m0=[m.ravel() for m in m0])
        print("bloch_batch shared grid, m0, mode %d: max |batch - single| %.3g, bit-identical %s" % (mode, worst, same))
        assert worst <= TOL and same
    eq = mbfir.bloch_batch(pulses[:1], df, dp)[0]                   # m0 None: equilibrium
    want = mbfir.bloch(*pulses[0][:5], df, dp, 0, nucleus=pulses[0][5])
    assert all(np.abs(g[0] - w).max() <= TOL for g, w in zip(eq, want))


def test_bloch_batch_against_the_oracle():
    pulses = _pulses(9, [300, 40, 257], lambda q: (0.01, 0.005))
    rng = np.random.default_rng(10)
    df, pos = np.linspace(-500, 500, 17), rng.standard_normal((5, 3))
    gam = {"C-13": obloch.GAMMA_C13, "H-1": obloch.GAMMA_H1}
    for mode in (0, 1):                                             # relaxation; steady state
        res = mbfir.bloch_batch(pulses, df, pos, scales=[1.0, 0.8], mode=mode)
        for (b1, gr, tp, t1, t2, nuc), r in zip(pulses, res):
            ts = np.diff(np.concatenate([[0.0], tp])) if np.size(tp) > 1 and np.all(np.diff(tp) > 0) else tp
            g3 = np.concatenate([gr, np.zeros((len(b1), 3 - gr.shape[1]))], 1)
            for k, s in enumerate([1.0, 0.8]):
                ref = obloch.blochsimfz(b1 * s, g3, ts, t1, t2, df, pos, mode, gamma=gam.get(nuc, nuc))
                got = np.stack([r[0][k], r[1][k], r[2][k]], -1).reshape(ref.shape)
                assert np.abs(got - ref).max() <= TOL, (mode, len(b1), s)


def _rf_pulses(seed, lengths):
    """abr pulses: rf alone (2 pi / n per sample) and (rf, g) in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for q, n in enumerate(lengths):
        rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (np.pi / n)
        out.append((rf, rng.uniform(0.5, 1.5, n) * 2 * np.pi / n) if q % 2 else rf)
    return out


@pytest.mark.parametrize("hard_pulse", [False, True])
def test_abr_batch_matches_single_calls_and_the_oracle(hard_pulse):
    lengths = [1, 7, 255, 256, 257, 2000]
    pulses = _rf_pulses(30 + hard_pulse, lengths)
    xs = [np.linspace(-n / 2 - 3, n / 2 + 3, nx) for n, nx in zip(lengths, (5, 256, 300, 257, 1000, 100))]
    res = mbfir.abr_batch(pulses, xs, scales=SCALES, hard_pulse=hard_pulse)
    res_abr = mbfir.abr_batch(pulses, xs, scales=SCALES, hard_pulse=hard_pulse, convention="abr")
    worst, same = 0.0, True
    for q, (p, (a, b), (a2, b2)) in enumerate(zip(pulses, res, res_abr)):
        rf, g = p if isinstance(p, tuple) else (p, None)
        assert a.shape == b.shape == (len(SCALES), len(xs[q]))
        assert np.array_equal(a2, a) and np.array_equal(b2, -np.conj(b))
        for k, s in enumerate(SCALES):
            a1, b1 = mbfir.abrm(rf * s, g, xs[q], hard_pulse=hard_pulse)
            worst = max(worst, float(np.abs(a[k] - a1).max()), float(np.abs(b[k] - b1).max()))
            same = same and np.array_equal(a[k], a1) and np.array_equal(b[k], b1)
            if not hard_pulse:
                ao, bo = mbfir.abr(rf * s, g, xs[q])
                assert np.abs(a2[k] - ao).max() <= TOL and np.abs(b2[k] - bo).max() <= TOL
            if len(rf) <= 257 and not (hard_pulse and g is not None):
                ao, bo = obloch.hard_pulse_ab(rf * s, xs[q]) if hard_pulse else obloch.abrm(rf * s, g, xs[q])
                assert np.abs(a[k] - ao).max() <= TOL and np.abs(b[k] - bo).max() <= TOL, (q, s)
    print("abr_batch hard_pulse=%s: max |batch - single| %.3g, bit-identical %s" % (hard_pulse, worst, same))
    assert worst <= TOL and same


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_at_another_scale_place():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 700, 17)]
    pulses = _pulses(51, lengths, lambda q: (0.05, 0.02))
    dfs, dps = _grids(52, [(7 + q, 5 + q % 4) for q in range(17)])
    sc = [0.9, 1.0, 1.1]
    full = mbfir.bloch_batch(pulses, dfs, dps, scales=sc)
    rev = mbfir.bloch_batch(pulses[::-1], dfs[::-1], dps[::-1], scales=sc)[::-1]
    rfs = _rf_pulses(53, lengths)
    xs = [np.linspace(-40, 40, 200 + 13 * q) for q in range(17)]
    afull = mbfir.abr_batch(rfs, xs, scales=sc)
    arev = mbfir.abr_batch(rfs[::-1], xs[::-1], scales=sc)[::-1]
    for q in (0, 5, 16):
        alone = mbfir.bloch_batch([pulses[q]], [dfs[q]], [dps[q]], scales=[1.0, 0.9])[0]
        aalone = mbfir.abr_batch([rfs[q]], [xs[q]], scales=[1.0, 0.9])[0]
        for c in range(3):
            assert np.array_equal(full[q][c], rev[q][c])
            assert np.array_equal(alone[c][0], full[q][c][1]) and np.array_equal(alone[c][1], full[q][c][0])
        for c in range(2):
            assert np.array_equal(afull[q][c], arev[q][c])
            assert np.array_equal(aalone[c][0], afull[q][c][1]) and np.array_equal(aalone[c][1], afull[q][c][0])


def test_sim_rf_scale_batch_matches_sim_rf_scale():
    rf1 = 0.05 * np.sinc(np.linspace(-4, 4, 150)) * np.hamming(150)                                  # G
    rf2 = 0.03 * np.sinc(np.linspace(-2, 2, 300)) * np.exp(1j * np.linspace(0, 2, 300))
    f1 = np.array([-0.3, -0.2, 0.2, 0.3])
    cases = [(rf1, 0.064, f1, None), (rf2, 0.04, None, 1.0), (rf1, 0.05, None, 0.5)]
    for nucleus in ("C-13", "H-1"):
        res = mbfir.sim_rf_scale_batch([c[0] for c in cases], [c[1] for c in cases], None, nucleus, f=[c[2] for c in cases],
                                       bw=[c[3] for c in cases])
        for (rf, dt, f, bw), (df, mxy, mz) in zip(cases, res):
            df1, mxy1, mz1 = mbfir.sim_rf_scale(rf, dt, None, nucleus, f=f, bw=bw)
            assert np.array_equal(df, df1) and mxy.shape == mxy1.shape == (5, 2048)
            assert np.abs(mxy - mxy1).max() <= TOL and np.abs(mz - mz1).max() <= TOL
    df, mxy, mz = mbfir.sim_rf_scale_batch([rf2], 0.04, [1.0], bw=1.0)[0]                           # one pulse, shared values
    assert mxy.shape == (1, 2048)


def _trap(n, ramp, amp):
    t = np.full(n, float(amp))
    t[:ramp] = amp * (np.arange(ramp) + 0.5) / ramp
    t[n - ramp:] = t[:ramp][::-1]
    return t


def test_bloch_batch_on_eight_pulses_of_the_dzss_mb_schedule():
    """8 of the 80 flyback pulses of tools/gpu_ssmb_batch.py from one dzss_mb_batch call, simulated by one bloch_batch call on the
    x x df grid of tests/test_ssmb_gpu.py (physics_grids), against one mbfir.bloch call per pulse."""
    cpu = _cpu()
    cs = mbfir.spec.spectrum_c13(3.0) * 1e-3
    base = dict(gx=_trap(80, 16, 4.0), dt=0.004, ngx=25, mb_cf=[cs[4], cs[0], cs[2], cs[1]], mb_range=[0.06] * 4,
                mb_ripple=[0.01] * 4, gfb=-_trap(40, 8, 8.0))
    specs = [dict(base, mb_FA=[fa if i == t else 0 for i in range(4)]) for t in range(4) for fa in range(2, 42, 2)][::10]
    designs = [(s, d) for s, d in zip(specs, mbfir.dzss_mb_batch(specs)) if d[2]["status"] == "Solved"]
    assert len(designs) >= 6
    grids = [cpu.physics_grids(s, info) for s, (_, _, info) in designs]
    pulses = [(rf, g, s["dt"] * 1e-3, 1e6, 1e6, "C-13") for s, (rf, g, _) in designs]
    res = mbfir.bloch_batch(pulses, [fr for fr, _ in grids], [x for _, x in grids])
    worst = 0.0
    for (rf, g, tp, _, _, _), (fr, x), got in zip(pulses, grids, res):
        want = mbfir.bloch(rf, g, tp, 1e6, 1e6, fr, x)
        for c in range(3):
            assert got[c].shape == (1,) + want[c].shape
            worst = max(worst, float(np.abs(got[c][0] - want[c]).max()))
    print("dzss_mb schedule, %d pulses: max |batch - single| %.3g" % (len(pulses), worst))
    assert worst <= TOL


def test_argument_errors_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, o = np.ones(64), [np.zeros(64) for _ in range(4)]

    def bloch(toff=L(0, 3), tsoff=L(0, 1), foff=L(0, 2), poff=L(0, 2), nscale=1, mode=0, npulse=1, t1=1.0):
        t1a = np.full(4, t1)
        return lib.mbfir_bloch_batch(ctx._h, npulse, lp(toff), p(d), p(d), None, None, None, lp(tsoff), p(d), p(t1a), p(t1a), p(d),
                                     1, lp(foff), p(d), 1, lp(poff), None, None, None, nscale, p(d), mode, *[p(x) for x in o[:3]])

    def abr(roff=L(0, 3), xoff=L(0, 2), nscale=1, mode=0, npulse=1):
        return lib.mbfir_abr_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, 1, lp(xoff), p(d), nscale, p(d), mode,
                                   *[p(x) for x in o])

    big = 2 ** 31 - 1
    for name, call, cases in (
            ("bloch_batch", bloch, [dict(toff=L(0, 0)), dict(npulse=2, toff=L(0, 3, 2), tsoff=L(0, 1, 2)), dict(toff=L(1, 3)),
                                    dict(tsoff=L(0, 2)), dict(nscale=0), dict(foff=L(0, big), poff=L(0, big), nscale=4),
                                    dict(mode=4), dict(t1=0.0), dict(npulse=0)]),
            ("abr_batch", abr, [dict(roff=L(0, 0)), dict(npulse=2, roff=L(0, 3, 1)), dict(xoff=L(0, 0)), dict(nscale=0),
                                dict(xoff=L(0, big), nscale=big), dict(mode=2), dict(npulse=0)])):
        assert call() == 0
        for kw in cases:
            assert call(**kw) == mbfir.E_ARG, (name, kw)
            assert ctx.last_error().startswith(name + ":"), (name, kw, ctx.last_error())
        assert call() == 0
    assert "no samples" in (bloch(toff=L(0, 0)), ctx.last_error())[1]
    assert "neither 1 nor" in (bloch(tsoff=L(0, 2)), ctx.last_error())[1]
    assert "overflows" in (bloch(foff=L(0, big), poff=L(0, big), nscale=4), ctx.last_error())[1]
    assert "inconsistent offsets" in (bloch(npulse=2, toff=L(0, 3, 2), tsoff=L(0, 1, 2)), ctx.last_error())[1]
    # the Python layer: ValueError / MbfirError with a message, then a valid call
    df = np.linspace(-100, 100, 5)
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.bloch_batch([(np.ones(8), None, 4e-6, 1.0, 1.0, "C-13")], df, 0.0, scales=[])
    with pytest.raises(mbfir.MbfirError, match="Time-point length"):
        mbfir.bloch_batch([(np.ones(8), None, np.full(5, 4e-6), 1.0, 1.0, "C-13")], df, 0.0)
    with pytest.raises(ValueError, match="no samples"):
        mbfir.abr_batch([np.zeros(0)], df)
    mx, my, mz = mbfir.bloch_batch([(np.full(8, 0.1), None, 4e-6, 1.0, 1.0, "C-13")], df, 0.0)[0]
    w = mbfir.bloch(np.full(8, 0.1), None, 4e-6, 1.0, 1.0, df, 0.0)
    assert np.abs(mx[0] - w[0]).max() <= TOL and np.abs(mz[0] - w[2]).max() <= TOL
