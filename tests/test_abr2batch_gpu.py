"""Batched 2D Cayley-Klein simulation (mbfir.abr2_batch, k_abr2_batch): mode 0 bit for bit against one 2D mbfir.abrm call per
(pulse, scale), the hard-pulse model against the 1D call and a NumPy restatement, bit-invariance under the batch's composition, the
dzepse fixtures, the disc profile of the dz2d spiral, and the argument errors of the raw C call."""
import json
import os

import numpy as np
import pytest

import mbfir
from oracle import bloch as obloch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-12                  # tests/test_simbatch_gpu.py's tolerance for abr_batch against the oracle
SCALES = [1.0, 0.0, 0.9]


def abr2_np(rf, g, x, y, hard_pulse=False):
    """Both models vectorised over the (x, y) grid, om = x Re g + y Im g per sample.  hard_pulse False: abrm.m:39-57, one rotation
    about (Re rf, Im rf, om).  True: free precession z^-1 = exp(-i om) on beta, then the hard pulse (C, S) of the sample, as
    oracle.bloch.hard_pulse_ab does in 1D with om = 2 pi x / n."""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    n = len(rf)
    g = np.full(n, 2 * np.pi / n + 0j) if g is None else np.asarray(g, dtype=np.complex128).ravel()
    X, Y = np.meshgrid(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), indexing="ij")
    a = np.ones(X.shape, dtype=np.complex128)
    b = np.zeros(X.shape, dtype=np.complex128)
    for m in range(n):
        om = X * g[m].real + Y * g[m].imag
        if hard_pulse:
            th = abs(rf[m])
            C, S, zi = np.cos(th / 2), 1j * np.exp(1j * np.angle(rf[m])) * np.sin(th / 2), np.exp(-1j * om)
            a, b = C * a - np.conj(S) * zi * b, S * a + C * zi * b
        else:
            phi = np.sqrt(abs(rf[m]) ** 2 + om ** 2)
            safe = np.where(phi > 0, phi, 1.0)
            av = np.cos(phi / 2) - 1j * (om / safe) * np.sin(phi / 2)
            bv = -1j * (rf[m] / safe) * np.sin(phi / 2)
            a, b = av * a - np.conj(bv) * b, bv * a + np.conj(av) * b
    return a, b


def _pulses(seed, lengths):
    """2D pulses: rf alone (2 pi / n along x, no y gradient) and (rf, complex g) in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for q, n in enumerate(lengths):
        rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (np.pi / n)
        g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n + 1j * rng.uniform(-1.5, 1.5, n) * 1e-3
        out.append((rf, g) if q % 2 else rf)
    return out


def _split(p):
    return p if isinstance(p, tuple) else (p, None)


def test_restatement_is_the_oracle_at_y0():
    rf, g = _pulses(1, [7, 60])[1]
    x = np.linspace(-20, 20, 31)
    a, b = abr2_np(rf, g.real, x, [0.0])
    ao, bo = obloch.abrm(rf, g.real, x)
    assert np.abs(a[:, 0] - ao).max() <= 1e-14 and np.abs(b[:, 0] - bo).max() <= 1e-14
    a, b = abr2_np(rf, None, x, [0.0], hard_pulse=True)
    ao, bo = obloch.hard_pulse_ab(rf, x)
    assert np.abs(a[:, 0] - ao).max() <= 1e-14 and np.abs(b[:, 0] - bo).max() <= 1e-14


LENGTHS = [1, 255, 256, 257, 1024]
GRIDS = [(5, 3), (16, 16), (37, 11), (1, 300), (20, 13)]          # nx ny = 15, 256, 407, 300, 260: below, at and above a chunk


def test_mode0_is_bit_identical_to_single_abrm_calls_on_per_pulse_grids():
    pulses = _pulses(30, LENGTHS)
    xs = [np.linspace(-n / 2 - 3, n / 2 + 3, nx) for n, (nx, _) in zip(LENGTHS, GRIDS)]
    ys = [np.linspace(-400, 300, ny) for _, ny in GRIDS]
    res = mbfir.abr2_batch(pulses, xs, ys, scales=SCALES)
    res_abr = mbfir.abr2_batch(pulses, xs, ys, scales=SCALES, convention="abr")
    worst = 0.0
    for q, (p, (a, b), (a2, b2)) in enumerate(zip(pulses, res, res_abr)):
        rf, g = _split(p)
        assert a.shape == b.shape == (len(SCALES),) + GRIDS[q]
        for k, s in enumerate(SCALES):
            a1, b1 = mbfir.abrm(rf * s, g, xs[q], ys[q])
            worst = max(worst, float(np.abs(a[k] - a1).max()), float(np.abs(b[k] - b1).max()))
            assert np.array_equal(a[k], a1) and np.array_equal(b[k], b1), (q, s)
            ao, bo = mbfir.abr(rf * s, g, xs[q], ys[q])
            assert np.array_equal(a2[k], ao) and np.array_equal(b2[k], bo), (q, s)
    print("abr2_batch mode 0, per-pulse grids: max |batch - single| %.3g" % worst)


def test_mode0_is_bit_identical_to_single_abrm_calls_on_a_shared_grid():
    pulses = _pulses(31, LENGTHS)
    x, y = np.linspace(-9, 9, 7), np.linspace(-350, 350, 41)      # 287 points
    res = mbfir.abr2_batch(pulses, x, y, scales=SCALES)
    for q, (p, (a, b)) in enumerate(zip(pulses, res)):
        rf, g = _split(p)
        assert a.shape == (3, 7, 41)
        for k, s in enumerate(SCALES):
            a1, b1 = mbfir.abrm(rf * s, g, x, y)
            assert np.array_equal(a[k], a1) and np.array_equal(b[k], b1), (q, s)
        assert np.abs(np.abs(a[1]) ** 2 + np.abs(b[1]) ** 2 - 1).max() <= TOL and np.abs(b[1]).max() == 0    # scale 0: no rf
    # a list of plain numbers is one shared grid
    r2 = mbfir.abr2_batch(pulses[:2], list(x), list(y))
    assert np.array_equal(r2[1][0][0], res[1][0][0]) and np.array_equal(r2[1][1][0], res[1][1][0])


def test_hard_pulse_at_y0_equals_the_1d_hard_pulse_model():
    pulses = _pulses(32, [200, 257])
    x = np.linspace(-6, 6, 41)
    res = mbfir.abr2_batch(pulses, x, [0.0], scales=[1.0, 0.8], hard_pulse=True)
    worst = 0.0
    for p, (a, b) in zip(pulses, res):
        rf, g = _split(p)
        for k, s in enumerate([1.0, 0.8]):
            a1, b1 = mbfir.abrm(rf * s, None if g is None else g.real, x, hard_pulse=True)
            worst = max(worst, float(np.abs(a[k][:, 0] - a1).max()), float(np.abs(b[k][:, 0] - b1).max()))
    print("abr2_batch hard pulse at y = [0] against the 1D call: %.3g" % worst)
    assert worst <= 1e-15                                          # section 8f's bound for the same check in mode 0


def test_hard_pulse_matches_the_numpy_restatement_on_64_by_48():
    pulses = _pulses(33, [200, 300])
    x, y = np.linspace(-6, 6, 64), np.linspace(-400, 400, 48)
    worst = {}
    for hard in (True, False):
        res = mbfir.abr2_batch(pulses, x, y, scales=[1.0, 0.7], hard_pulse=hard)
        w = 0.0
        for p, (a, b) in zip(pulses, res):
            rf, g = _split(p)
            assert a.shape == (2, 64, 48)
            for k, s in enumerate([1.0, 0.7]):
                ar, br = abr2_np(rf * s, g, x, y, hard_pulse=hard)
                w = max(w, float(np.abs(a[k] - ar).max()), float(np.abs(b[k] - br).max()))
        worst[hard] = w
    print("abr2_batch against NumPy on 64 x 48: hard pulse %.3g, abrm %.3g" % (worst[True], worst[False]))
    assert worst[True] <= TOL and worst[False] <= TOL


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_at_another_scale_place():
    lengths = [int(v) for v in np.random.default_rng(50).integers(1, 700, 17)]
    pulses = _pulses(53, lengths)
    xs = [np.linspace(-40, 40, 5 + 3 * q) for q in range(17)]
    ys = [np.linspace(-300, 300, 3 + q % 7) for q in range(17)]
    sc = [0.9, 1.0, 1.1]
    for hard in (False, True):
        full = mbfir.abr2_batch(pulses, xs, ys, scales=sc, hard_pulse=hard)
        rev = mbfir.abr2_batch(pulses[::-1], xs[::-1], ys[::-1], scales=sc, hard_pulse=hard)[::-1]
        for q in (0, 5, 16):
            alone = mbfir.abr2_batch([pulses[q]], [xs[q]], [ys[q]], scales=[1.0, 0.9], hard_pulse=hard)[0]
            for c in range(2):
                assert np.array_equal(full[q][c], rev[q][c])
                assert np.array_equal(alone[c][0], full[q][c][1]) and np.array_equal(alone[c][1], full[q][c][0])


@pytest.fixture(scope="module")
def epse():
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        meta = json.load(fh)["dzepse"]
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        for name, v in meta.items():
            v["gx"] = z["dzepse/%s/gx" % name]
            v["rf"] = z["dzepse/%s/rf" % name]
    return meta


def _epse_gradient(v):
    """Re g: the lobes with alternating sign, 2 pi per lobe (x in cycles of the spatial profile); Im g = 2 pi dt (y in Hz)"""
    dt = v["tgx"] / v["lgx"] * 1e-3
    lobe = v["gx"] * 2 * np.pi / v["gx"].sum()
    return np.concatenate([lobe * (-1) ** k for k in range(v["ngx"])]) + 1j * 2 * np.pi * dt


def test_the_dzepse_fixtures_at_three_scales_in_one_call(epse):
    """The six pulses of tests/golden/epse.npz x three scales in one launch against their single 2D abrm calls; the 180 degree
    fixture ls_trap64_n13_180 sits on the spin-echo grid of tests/test_epse_gpu.py (3 x 93 points), where section 8f's ab2se figures
    must hold at scale 1: >= 0.98 at the centre, <= 5e-3 over 450 .. 900 Hz at x = 0."""
    names = list(epse)
    assert len(names) == 6 and "ls_trap64_n13_180" in names
    pulses = [(epse[n]["rf"].ravel(), _epse_gradient(epse[n])) for n in names]
    se_x = np.array([0.0, 0.5, -0.5])
    se_y = np.concatenate([[0.0], np.linspace(450, 900, 46), -np.linspace(450, 900, 46)])
    xs = [se_x if n == "ls_trap64_n13_180" else np.linspace(-1, 1, 5) for n in names]
    ys = [se_y if n == "ls_trap64_n13_180" else np.linspace(-600, 600, 9) for n in names]
    sc = [0.9, 1.0, 1.1]
    res = mbfir.abr2_batch(pulses, xs, ys, scales=sc, convention="abr")
    for n, (rf, g), x, y, (a, b) in zip(names, pulses, xs, ys, res):
        for k, s in enumerate(sc):
            a1, b1 = mbfir.abr(rf * s, g, x, y)
            assert np.array_equal(a[k], a1) and np.array_equal(b[k], b1), (n, s)
    a, b = res[names.index("ls_trap64_n13_180")]
    se = np.abs(mbfir.ab2se(a[1], b[1]))
    print("spin echo at scale 1: centre %.4f, stop band max %.2e" % (se[0, 0], se[0, 1:].max()))
    assert se[:, 0].min() >= 0.98
    assert se[0, 1:].max() <= 5e-3


def test_the_dz2d_spiral_excites_a_disc():
    """The reference's example dz2d(8, 1, 4, 512, 1, 2) scaled to 90 degrees on 65 x 65 points over +-8 cm.  The NumPy restatement
    gives |Mxy| = 1.000 at the centre, >= 0.9931 for r <= 1 cm and <= 0.0216 for 3.5 <= r <= 8 cm over the whole grid (DESIGN.md
    section 8i); the device profile is held against the restatement's two figures, recomputed here: pass >= CPU - 0.01 and
    stop <= 1.5 x CPU."""
    rf, g, _ = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    x = np.linspace(-8, 8, 65)
    sc = [0.8, 1.0, 1.2]
    (a, b), = mbfir.abr2_batch([(rf * np.pi / 2, g)], x, x, scales=sc, convention="abr")
    r = np.hypot(*np.meshgrid(x, x, indexing="ij"))
    disc, ring = r <= 1.0, (r >= 3.5) & (r <= 8.0)
    ar, br = abr2_np(rf * np.pi / 2, g, x, x)
    mref = np.abs(2 * np.conj(ar) * br)
    cpu_pass, cpu_stop = float(mref[disc].min()), float(mref[ring].max())
    assert 0.99 <= cpu_pass <= 1.0 and cpu_stop <= 0.025            # the restatement itself shows a disc
    m = np.abs(2 * np.conj(a) * b)                                  # abr.m:11
    dev_pass, dev_stop = float(m[1][disc].min()), float(m[1][ring].max())
    print("spiral disc: centre %.4f, pass min %.4f (CPU %.4f), stop max %.4f (CPU %.4f)"
          % (m[1][32, 32], dev_pass, cpu_pass, dev_stop, cpu_stop))
    assert dev_pass >= cpu_pass - 0.01 and dev_stop <= 1.5 * cpu_stop
    assert np.abs(a[1] - ar).max() <= TOL and np.abs(b[1] - (-np.conj(br))).max() <= TOL
    # at the centre every sample rotates about the same axis, so the flip angle is s pi / 2 sum(rf): |Mxy| = sin(s pi / 2)
    for k, s in enumerate(sc):
        assert abs(m[k][32, 32] - np.sin(s * np.pi / 2)) <= TOL


def test_argument_errors_of_the_raw_call_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, o = np.ones(64), [np.zeros(64) for _ in range(4)]

    def call(roff=L(0, 3), xoff=L(0, 2), yoff=L(0, 3), nscale=1, mode=0, npulse=1, nxgrid=1, nygrid=1, y=d, out=o):
        return lib.mbfir_abr2_batch(ctx._h, npulse, lp(roff), p(d), p(d), None, None, nxgrid, lp(xoff), p(d), nygrid, lp(yoff),
                                    p(y) if y is not None else None, nscale, p(d), mode,
                                    *[p(v) if v is not None else None for v in out])

    big = 2 ** 31 - 1
    assert call() == 0
    for kw, why in ((dict(roff=L(0, 0)), "no samples"), (dict(npulse=2, roff=L(0, 3, 1)), "inconsistent offsets"),
                    (dict(roff=L(1, 3)), "inconsistent offsets"), (dict(xoff=L(0, 0)), "empty item"),
                    (dict(yoff=L(0, 0)), "empty item"), (dict(nscale=0), "scale list is empty"),
                    (dict(xoff=L(0, big), yoff=L(0, big), nscale=4), "overflows"), (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
                    (dict(npulse=0), "no pulses"), (dict(nxgrid=2), "1 or npulse"), (dict(nygrid=3), "1 or npulse"),
                    (dict(y=None), "null"), (dict(out=[o[0], None, o[2], o[3]]), "null")):
        assert call(**kw) == mbfir.E_ARG, kw
        assert ctx.last_error().startswith("abr2_batch:") and why in ctx.last_error(), (kw, ctx.last_error())
    assert call() == 0
    a, b = mbfir.abr2_batch([np.full(8, 0.1)], [0.0, 1.0], [0.0])[0]
    a1, b1 = mbfir.abrm(np.full(8, 0.1), None, [0.0, 1.0], [0.0])
    assert np.array_equal(a[0], a1) and np.array_equal(b[0], b1)
