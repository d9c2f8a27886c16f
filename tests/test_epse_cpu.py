"""Spectral-spatial designer, host side (no GPU): the centred FFTs, verse / versec, dzbeta's mapping, the ab2* profiles, dzepse's
argument errors and its host logic with the device inverse SLR replaced by the oracle, and the fixture generator."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import scipy.interpolate as si

import mbfir
from mbfir import epse, slrclassic
from oracle import slr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_epse", os.path.join(GOLDEN, "make_golden_epse.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("l,n", [(5, 16), (6, 16), (5, 15), (6, 15), (1, 4), (8, 8), (7, 7)])
def test_fftcp_matches_literal_restatement(l, n):
    h = np.random.default_rng(l * 100 + n).standard_normal(l) + 1j * np.random.default_rng(n).standard_normal(l)
    pad = np.concatenate([np.zeros(math.ceil(n / 2 - l / 2)), h, np.zeros(math.floor(n / 2 - l / 2))])   # fftcp.m:17
    want = np.fft.fftshift(np.fft.fft(np.fft.fftshift(pad)))                                              # fftc.m:10
    got = mbfir.fftcp(h, n)
    assert len(got) == n and np.array_equal(got, want)
    assert np.array_equal(mbfir.fftc(pad), want)


def _lobe(n):
    r = n // 4
    t = np.ones(n)
    t[:r] = (np.arange(r) + 0.5) / r
    t[n - r:] = t[:r][::-1]
    return t


@pytest.mark.parametrize("lg,m,ncol", [(40, 24, 3), (17, 30, 1), (64, 5, 2), (12, 3, 1), (9, 2, 1)])
def test_verse_matches_scipy_not_a_knot(lg, m, ncol):
    g = _lobe(lg) + 0.1
    rng = np.random.default_rng(lg + m)
    rf = rng.standard_normal((m, ncol)) + 1j * rng.standard_normal((m, ncol))
    k = np.cumsum(g)
    k = (m - 1) * k / k.max()
    assert k[0] < 1                                        # verse.m samples below its grid's first point: extrapolation
    want = (m * g / g.sum())[:, None] * si.CubicSpline(np.arange(1, m + 1), rf, bc_type="not-a-knot", extrapolate=True)(k)
    got = mbfir.verse(g, rf)
    assert got.shape == (lg, ncol)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_verse_row_vector_is_transposed():
    g = _lobe(20)
    rf = np.random.default_rng(3).standard_normal(15)
    assert np.array_equal(mbfir.verse(g, rf), mbfir.verse(g, rf[:, None]))
    assert np.array_equal(mbfir.versec(g, rf), mbfir.versec(g, rf[:, None]))


@pytest.mark.parametrize("neg", [False, True])
def test_versec_matches_interp_with_nan_outside(neg):
    g = _lobe(30)
    if neg:
        g[0] = -0.5                                         # k starts below 0: NaN there
    m = 22
    rf = np.random.default_rng(5).standard_normal((m, 4)) + 1j
    k = np.cumsum(g)
    k = (m - 1) * k / k.max()
    gs = m * g / g.sum()
    want = np.stack([gs * np.interp(k, np.arange(m), rf[:, j], left=np.nan, right=np.nan) for j in range(4)], axis=1)
    got = mbfir.versec(g, rf)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() == neg
    assert np.allclose(got, want, rtol=0, atol=1e-14, equal_nan=True)


def test_verse_fixtures():
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        meta = json.load(fh)["verse"]
    gen = _generator()
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        for name, v in meta.items():
            g = gen.GRADS[v["shape"]](v["lg"])
            rf = z["verse/%s/rf" % name]
            want = z["verse/%s/verse" % name]
            assert np.abs(mbfir.verse(g, rf) - want).max() <= 1e-12 * np.abs(want).max()
            assert np.allclose(mbfir.versec(g, rf), z["verse/%s/versec" % name], rtol=0, atol=1e-14, equal_nan=True)


def test_dzbeta_se_ls_is_dzls_with_the_se_ripples():
    for n, tb, d1, d2 in [(64, 6.0, 0.01, 0.01), (33, 4.0, 0.02, 0.005)]:
        r1, r2, bsf = slrclassic.ptype_ripples("se", d1, d2)
        assert (r1, r2, bsf) == (d1 / 4, math.sqrt(d2), 1.0)
        assert np.array_equal(mbfir.dzbeta(n, tb, "se", "ls", d1, d2), bsf * slrclassic.dzls(n, tb, r1, r2))
    # 'ex' scales by bsf = sqrt(1/2); 'st' returns the filter itself; 'ms' ignores the ripples
    assert np.array_equal(mbfir.dzbeta(40, 4.0, "ex", "ms"), math.sqrt(0.5) * slrclassic.msinc(40, 1.0))
    assert np.array_equal(mbfir.dzbeta(40, 4.0), slrclassic.dzls(40, 4.0, 0.01, 0.01))
    with pytest.raises(ValueError):
        mbfir.dzbeta(40, 4.0, "se", "bogus")
    with pytest.raises(ValueError):
        mbfir.dzbeta(40, 4.0, "bogus")


def test_ab2_profiles():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((5, 3)) + 1j * rng.standard_normal((5, 3))
    b = rng.standard_normal((5, 3)) + 1j * rng.standard_normal((5, 3))
    ab = np.concatenate([a, b], axis=1)
    assert np.array_equal(mbfir.ab2ex(a, b), 2 * np.conj(a) * b)
    assert np.array_equal(mbfir.ab2se(a, b), 1j * b * b)
    assert np.allclose(mbfir.ab2inv(a, b), 1 - 2 * np.abs(b) ** 2, rtol=0, atol=1e-14)
    assert np.array_equal(mbfir.ab2sat(a, b), mbfir.ab2inv(a, b)) and np.isrealobj(mbfir.ab2inv(a, b))
    assert np.array_equal(mbfir.ab2st(a, b), 1j * a * a)
    for f in (mbfir.ab2ex, mbfir.ab2se, mbfir.ab2inv, mbfir.ab2sat):     # the one-argument [a b] form splits the columns
        assert np.array_equal(f(ab), f(a, b))
    assert np.array_equal(mbfir.ab2st(ab), 1j * a[:, 0] * a[:, 0])        # ab2st.m:12: the first column only
    # a unit-norm rotation: |a|^2 + |b|^2 = 1 -> |ab2se| = |b|^2 = (1 - ab2inv) / 2
    th = rng.uniform(0, np.pi, 7)
    a1, b1 = np.cos(th / 2) + 0j, 1j * np.sin(th / 2)
    assert np.allclose(np.abs(mbfir.ab2se(a1, b1)), (1 - mbfir.ab2inv(a1, b1)) / 2, atol=1e-15)


def test_dzepse_argument_errors():
    g = _lobe(32)
    with pytest.raises(ValueError, match="even"):
        mbfir.dzepse(np.pi, _lobe(33), 4, 0.5, 8, 0.5)              # odd lgx: dzepse.m cannot index 0.5 lgx + 1
    with pytest.raises(ValueError):
        mbfir.dzepse(np.pi, g, 4, 0.5, 8, 0.5, 0.01, 0.01, "bogus")
    with pytest.raises(ValueError):
        mbfir.dzepse(np.pi, g, 4, 0.5, 1, 0.5)                      # one lobe: no spectral polynomial
    with pytest.raises(ValueError):
        mbfir.dzepse(np.pi, g, 4, 0.5, 8.5, 0.5)
    with pytest.raises(ValueError):
        mbfir.dzepse(np.pi, np.zeros(32), 4, 0.5, 8, 0.5)
    with pytest.raises(ValueError):
        mbfir.dzepse_batch([dict(ang=np.pi, gx=g, tbx=4, tgx=0.5, ngx=8)])       # sbw missing
    with pytest.raises(ValueError):
        mbfir.dzepse_batch([(np.pi, g, 4, 0.5, 8)])
    assert mbfir.dzepse_batch([]) == []


def test_b2rf_batch_argument_errors():
    with pytest.raises(ValueError):
        mbfir.b2rf_batch(np.ones(8))
    with pytest.raises(ValueError):
        mbfir.b2rf_batch(np.ones((3, 1)))
    with pytest.raises(ValueError):
        mbfir.b2rf_batch(np.ones((3, 2049)))
    with pytest.raises(ValueError):
        mbfir.b2rf_batch(np.ones((0, 16)))


def test_dzepse_host_logic_with_oracle_inverse_slr(monkeypatch):
    """dzepse's host steps (profiles, slices, conjugating transposes, versec, column-major output) against the fixture, with
    the device inverse SLR replaced by oracle.slr.b2rf row by row: the 'ls' designs need no other device call."""
    calls = []

    def fake_batch(B, ctx=None):
        calls.append(np.shape(B))
        return np.stack([slr.b2rf(r) for r in np.asarray(B)])
    monkeypatch.setattr(mbfir, "b2rf_batch", fake_batch)
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: None)
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        meta = json.load(fh)["dzepse"]
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        ls = [(k, v) for k, v in meta.items() if v["stype"] == "ls"]
        assert len(ls) >= 2
        for name, v in ls:
            calls.clear()
            rf = mbfir.dzepse(v["ang"], z["dzepse/%s/gx" % name], v["tbx"], v["tgx"], v["ngx"], v["sbw"], v["srip1"], v["srip2"],
                              v["stype"])
            want = z["dzepse/%s/rf" % name]
            assert calls == [(v["lgx"], v["ngx"]), (v["ngx"], v["lgx"])]          # one batch per stage
            assert rf.shape == (v["lgx"] * v["ngx"],)
            assert np.abs(rf - want).max() <= 1e-9 * np.abs(want).max(), name


def test_fixture_generator_reproduces_committed_fixture():
    meta, vec = _generator().build()
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        assert json.load(fh) == json.loads(json.dumps(meta))
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        assert sorted(z.files) == sorted(vec)
        for k, v in vec.items():
            w = z[k]
            assert w.shape == v.shape, k
            assert np.allclose(v, w, rtol=0, atol=1e-12 * np.abs(w).max(), equal_nan=True), k


def test_new_symbols_are_bound():
    for sym in ("mbfir_b2rf_batch", "mbfir_abr2"):
        assert sym in mbfir.SYMBOLS
