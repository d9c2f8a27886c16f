"""Spectral-spatial designer on the device: the batched inverse SLR (mbfir.b2rf_batch) against the multi-launch b2rf, the 2D
Cayley-Klein simulation (mbfir_abr2) against a NumPy restatement of abrm.m, dzepse against tests/golden/epse.json, and the
simulated spin-echo profile of a designed 180 degree pulse."""
import json
import math
import os

import numpy as np
import pytest

import mbfir
from oracle import bloch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _polys(n, count, cplx, seed):
    """count beta polynomials of n taps; the spread of scales puts max|B| above 1 for some, so b2a's rescale runs too."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((count, n)) + (1j * rng.standard_normal((count, n)) if cplx else 0)
    return B * (rng.uniform(0.2, 1.4, count)[:, None] / np.sqrt(n))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [2, 3, 16, 64, 255, 1024, 2048])
def test_b2rf_batch_matches_b2rf_row_by_row(n, cplx):
    ctx = mbfir.get_context()
    for count in (1, 7, 300):
        B = _polys(n, count, cplx, n * 10 + count)
        got = mbfir.b2rf_batch(B, ctx=ctx)
        assert got.shape == (count, n)
        rows = range(count) if count <= 7 else ((0, 1, 150, 299) if n <= 255 else (0, 299))
        for q in rows:
            want = mbfir.b2rf(B[q], ctx=ctx)
            assert np.abs(got[q] - want).max() <= 1e-12 * np.abs(want).max(), (n, count, q)


def test_b2rf_batch_is_position_independent_and_repeatable():
    for n in (16, 255, 2048):
        B = _polys(n, 300, True, 99)
        ref = mbfir.b2rf_batch(B)
        assert np.array_equal(mbfir.b2rf_batch(B), ref)
        for q in (0, 3, 299):
            assert np.array_equal(mbfir.b2rf_batch(B[q:q + 1])[0], ref[q])
        assert np.array_equal(mbfir.b2rf_batch(B[::-1])[::-1], ref)


def test_b2rf_batch_rejects_bad_sizes():
    with pytest.raises(ValueError):
        mbfir.b2rf_batch(np.ones((2, 2049)))
    with pytest.raises(ValueError):
        mbfir.b2rf_batch(np.ones((0, 16)))
    ctx = mbfir.get_context()
    lib = mbfir.load_library()
    b = np.ones(2049)
    o = np.zeros(2049)
    p = mbfir._ptr
    assert lib.mbfir_b2rf_batch(ctx._h, 2049, 1, p(b), None, p(o), p(o)) == mbfir.E_ARG
    assert lib.mbfir_b2rf_batch(ctx._h, 16, 0, p(b), None, p(o), p(o)) == mbfir.E_ARG
    assert lib.mbfir_b2rf_batch(ctx._h, 1, 1, p(b), None, p(o), p(o)) == mbfir.E_ARG


def abrm2_np(rf, g, x, y):
    """abrm.m:39-57 vectorised over the (x, y) grid: om = x Re g + y Im g, one rotation per sample."""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    g = np.asarray(g, dtype=np.complex128).ravel()
    X, Y = np.meshgrid(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), indexing="ij")
    a = np.ones(X.shape, dtype=np.complex128)
    b = np.zeros(X.shape, dtype=np.complex128)
    for m in range(len(rf)):
        om = X * g[m].real + Y * g[m].imag
        phi = np.sqrt(abs(rf[m]) ** 2 + om ** 2)
        safe = np.where(phi > 0, phi, 1.0)
        n1, n2, n3 = rf[m].real / safe, rf[m].imag / safe, om / safe
        av = np.cos(phi / 2) - 1j * n3 * np.sin(phi / 2)
        bv = -1j * (n1 + 1j * n2) * np.sin(phi / 2)
        a, b = av * a - np.conj(bv) * b, bv * a + np.conj(av) * b
    return a, b


def _pulse2d(n=200, seed=3):
    rng = np.random.default_rng(seed)
    rf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05
    g = np.cos(np.linspace(0, 6 * np.pi, n)) * 2 * np.pi / n + 1j * rng.uniform(0.5, 1.5, n) * 1e-3
    return rf, g


def test_abrm2_restatement_is_abrm_at_y0():
    rf, g = _pulse2d()
    x = np.linspace(-5, 5, 31)
    a, b = abrm2_np(rf, g.real, x, [0.0])
    ao, bo = bloch.abrm(rf, g.real, x)
    assert np.abs(a[:, 0] - ao).max() <= 1e-14 and np.abs(b[:, 0] - bo).max() <= 1e-14


def test_abrm2_matches_numpy_restatement():
    rf, g = _pulse2d()
    x = np.linspace(-6, 6, 64)
    y = np.linspace(-400, 400, 48)
    a, b = mbfir.abrm(rf, g, x, y)
    ar, br = abrm2_np(rf, g, x, y)
    assert a.shape == (64, 48) and b.shape == (64, 48)
    err = max(np.abs(a - ar).max(), np.abs(b - br).max())
    print("abrm 2D: max abs err %.2e" % err)
    assert err <= 1e-12
    # g omitted (2 pi / n, no y gradient): y has no effect
    a0, b0 = mbfir.abrm(rf, None, x, [0.0, 5.0])
    a1, b1 = mbfir.abrm(rf, x)
    assert np.array_equal(a0[:, 0], a0[:, 1]) and np.array_equal(b0[:, 0], b0[:, 1])
    assert np.abs(a0[:, 0] - a1).max() <= 1e-15 and np.abs(b0[:, 0] - b1).max() <= 1e-15


def test_abrm2_at_y0_equals_1d():
    rf, g = _pulse2d()
    x = np.linspace(-6, 6, 41)
    a2, b2 = mbfir.abrm(rf, g.real, x, [0.0])
    a1, b1 = mbfir.abrm(rf, g.real, x)
    assert np.abs(a2[:, 0] - a1).max() <= 1e-15 and np.abs(b2[:, 0] - b1).max() <= 1e-15


def test_abr2_applies_le_roux_convention():
    rf, g = _pulse2d()
    x, y = np.linspace(-3, 3, 9), np.linspace(-200, 200, 5)
    a, b = mbfir.abr(rf, g, x, y)
    am, bm = mbfir.abrm(rf, g, x, y)
    assert np.array_equal(a, am) and np.array_equal(b, -np.conj(bm))


@pytest.fixture(scope="module")
def fixtures():
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        meta = json.load(fh)["dzepse"]
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        for name, v in meta.items():
            v["gx"] = z["dzepse/%s/gx" % name]
            v["rf"] = z["dzepse/%s/rf" % name]
    return meta


def _args(v):
    return (v["ang"], v["gx"], v["tbx"], v["tgx"], v["ngx"], v["sbw"], v["srip1"], v["srip2"], v["stype"])


DZEPSE_TOL = 5e-10           # relative to max|rf|; measured worst 1.8e-10


def test_dzepse_matches_fixtures(fixtures):
    assert {v["stype"] for v in fixtures.values()} == {"pm", "ls", "min"}
    worst = 0.0
    for name, v in fixtures.items():
        rf = mbfir.dzepse(*_args(v))
        assert rf.shape == v["rf"].shape
        err = float(np.abs(rf - v["rf"]).max() / np.abs(v["rf"]).max())
        print("dzepse %s: rel err %.2e" % (name, err))
        worst = max(worst, err)
        assert err <= DZEPSE_TOL, (name, err)
    print("dzepse worst rel err %.2e" % worst)


def test_dzepse_batch_is_bit_identical_to_single_calls(fixtures):
    specs = [_args(v) for v in fixtures.values()]
    specs += [dict(ang=math.pi, gx=fixtures["pm_sin64_n16_180"]["gx"], tbx=4.0, tgx=0.6, ngx=16, sbw=0.3, stype=s)
              for s in ("pm", "ls", "min", "max", "ms")]
    batch = mbfir.dzepse_batch(specs)
    assert len(batch) == len(specs)
    for s, rf in zip(specs, batch):
        one = mbfir.dzepse(**s) if isinstance(s, dict) else mbfir.dzepse(*s)
        assert np.array_equal(rf, one)


# Spin-echo profile of the 180 degree fixture ls_trap64_n13_180 (tbx 6, 13 lobes of 0.5 ms, sbw 0.4 kHz), simulated with the 2D
# abr: Re g = the versed lobes with alternating sign (2 pi per lobe, x in cycles of the spatial profile), Im g = 2 pi dt (y in Hz).
# Thresholds set from the CPU restatement on this grid: 0.996 at the centre, 0.995 at x = +-0.5, at most
# 7.0e-4 in the spectral stop band 450 .. 900 Hz at x = 0.
SE_CENTRE_MIN = 0.98
SE_STOP_MAX = 5e-3


def test_dzepse_180_spin_echo_profile(fixtures):
    v = fixtures["ls_trap64_n13_180"]
    rf = mbfir.dzepse(*_args(v))
    lgx, ngx = v["lgx"], v["ngx"]
    dt = v["tgx"] / lgx * 1e-3
    lobe = v["gx"] * 2 * np.pi / v["gx"].sum()
    g = np.concatenate([lobe * (-1) ** k for k in range(ngx)]) + 1j * 2 * np.pi * dt
    x = np.array([0.0, 0.5, -0.5])
    ys = np.concatenate([[0.0], np.linspace(450, 900, 46), -np.linspace(450, 900, 46)])
    a, b = mbfir.abr(rf, g, x, ys)
    se = np.abs(mbfir.ab2se(a, b))
    print("spin echo: centre %.4f, stop band max %.2e" % (se[0, 0], se[0, 1:].max()))
    assert se[:, 0].min() >= SE_CENTRE_MIN
    assert se[0, 1:].max() <= SE_STOP_MAX
    ar, br = abrm2_np(rf, g, x, ys)
    assert np.abs(b - (-np.conj(br))).max() <= 1e-11
