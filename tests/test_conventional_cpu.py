"""Conventional SLR designers, host side (no GPU): dzrf.m's ptype rules, the dz* band vectors, msinc, the least-squares
design, argument errors, the C ABI binding, the mbfir.dzrf name, and sim_rf_scale's frequency axis."""
import math
import os
import re

import numpy as np
import pytest
import scipy.signal as ss

import mbfir
from mbfir import slrclassic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ptype,expect", [
    # dzrf.m:38-60 worked by hand for d1 = 0.01, d2 = 0.04
    ("st", (0.01, 0.04, 1.0)),
    ("ex", (math.sqrt(0.005), 0.04 / math.sqrt(2), math.sqrt(0.5))),     # sqrt(d1/2), d2/sqrt(2)
    ("se", (0.0025, 0.2, 1.0)),                                          # d1/4, sqrt(d2)
    ("inv", (0.00125, math.sqrt(0.02), 1.0)),                            # d1/8, sqrt(d2/2)
    ("sat", (0.005, 0.2, math.sqrt(0.5))),                               # d1/2, sqrt(d2)
])
def test_ptype_ripples(ptype, expect):
    got = slrclassic.ptype_ripples(ptype, 0.01, 0.04)
    assert np.allclose(got, expect, rtol=1e-15, atol=0)


def test_band_vectors():
    n, tb, d1, d2 = 128, 8.0, 0.01, 0.001
    di = mbfir.spec.dinf(d1, d2)
    w = di / tb
    f = [0, (1 - w) * 4 / 64, (1 + w) * 4 / 64, 1]
    nt, e, d, wt = slrclassic.dzlp_spec(n, tb, d1, d2)
    assert nt == n and np.allclose(e, f, rtol=1e-15) and d == [1, 1, 0, 0] and np.allclose(wt, [1, 10])
    nt, e, d, wt = slrclassic.dzls_spec(n, tb, d1, d2)
    assert nt == n and np.allclose(e, f, rtol=1e-15) and np.allclose(wt, [1, 10])
    nt, e, d, wt = slrclassic.dzmp_spec(n, tb, d1, d2)                 # dzmp.m: 2n - 1 taps, di = dinf(2 d1, d2^2 / 2) / 2
    wm = 0.5 * mbfir.spec.dinf(0.02, 0.5e-6) / tb
    assert nt == 2 * n - 1 and np.allclose(e, [0, (1 - wm) * 4 / 64, (1 + wm) * 4 / 64, 1], rtol=1e-15)
    assert np.allclose(wt, [1, 0.02 / 0.5e-6], rtol=1e-15)


@pytest.mark.parametrize("n,m", [(64, 1.0), (65, 1.5), (100, 0.5)])
def test_msinc_closed_form(n, m):
    h = mbfir.msinc(n, m)
    k = np.arange(n)
    x = (k - n / 2) / (n / 2)
    a = 2 * np.pi * m * x + 1e-5
    ref = np.sin(a) / a * (0.54 + 0.46 * np.cos(np.pi * x)) * 4 * m / n
    assert len(h) == n and np.allclose(h, ref, rtol=1e-14, atol=0)


@pytest.mark.parametrize("numtaps,edges,desired,weight", [
    (21, [0, 0.2, 0.3, 1], [1, 1, 0, 0], [1, 10]),
    (101, [0, 0.1, 0.15, 0.5, 0.55, 1], [0, 0, 1, 0.5, 0, 0], [3, 1, 2]),
    slrclassic.dzls_spec(129, 8, 0.01, 0.001),
])
def test_firls_matches_scipy(numtaps, edges, desired, weight):
    # scipy.signal.firls weights each band's squared-error integral by `weight`, as MATLAB's firls does: no conversion needed
    h = mbfir.firls_lp(numtaps, edges, desired, weight)
    hs = ss.firls(numtaps, edges, desired, weight=weight)
    assert np.abs(h - hs).max() <= 1e-10 * np.abs(hs).max()


def test_firls_even_length_is_the_least_squares_optimum():
    # type II (SciPy's firls takes odd lengths only): the normal equations against a dense quadrature least squares
    n, e, d, w = 64, [0, 0.2, 0.3, 1], [1, 1, 0, 0], [1, 4]
    h = mbfir.firls_lp(n, e, d, w)
    f = np.concatenate([np.linspace(0, 0.2, 4001), np.linspace(0.3, 1, 14001)])
    sw = np.sqrt(np.concatenate([np.full(4001, 1.0 * 0.2 / 4000), np.full(14001, 4.0 * 0.7 / 14000)]))
    L = n // 2
    C = np.cos(np.pi * np.outer(f, np.arange(L) + 0.5))
    c = np.linalg.lstsq(C * sw[:, None], np.r_[np.ones(4001), np.zeros(14001)] * sw, rcond=None)[0]
    ref = np.r_[c[::-1], c] / 2
    assert np.abs(h - ref).max() <= 2e-3 * np.abs(ref).max()           # trapezoid-free quadrature: a coarse check
    assert np.allclose(h, h[::-1])


def test_argument_errors():
    with pytest.raises(ValueError):
        mbfir.dzrf(64, 4, "xx")
    with pytest.raises(ValueError):
        mbfir.dzrf(64, 4, "ex", "foo")
    with pytest.raises(ValueError):
        mbfir.dzrf_batch([(64, 4, "ex", "foo")])
    with pytest.raises(ValueError):
        mbfir.remez(31, [0, 0.2, 0.3, 1.2], [1, 1, 0, 0], [1, 1])          # band outside [0, 1]
    with pytest.raises(ValueError):
        mbfir.remez(31, [-0.1, 0.2, 0.3, 1], [1, 1, 0, 0], [1, 1])
    with pytest.raises(ValueError):
        mbfir.remez(2048, [0, 0.2, 0.3, 1], [1, 1, 0, 0], [1, 1])          # numtaps > 2047
    with pytest.raises(ValueError):
        mbfir.remez_batch([(31, [0, 0.2, 0.3, 1], [0, 0, 1, 1], [1, 1], "hilbert")])   # antisymmetric
    with pytest.raises(ValueError):
        mbfir.remez_batch([(31, [0, 0.2, 0.3, 1], [0, 0, 1, 1], [1, 1], "differentiator")])
    with pytest.raises(ValueError):
        mbfir.fmp(np.ones(20))                                             # even length
    with pytest.raises(ValueError):
        mbfir.fmp(np.ones(2049))
    with pytest.raises(ValueError):
        mbfir.firls_lp(21, [0, 0.5, 0.4, 1], [1, 1, 0, 0], [1, 1])
    with pytest.raises(ValueError):
        mbfir.sim_rf_scale(np.ones(8), 0.1, bw=1.0, nucleus="P-31")


def test_abi_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym in ("mbfir_remez_batch", "mbfir_fmp"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in mbfir.SYMBOLS
    assert "mbfir_remez_job" in hdr and "mbfir_remez_opts" in hdr
    names = [f[0] for f in mbfir.RemezJob._fields_]
    assert names == ["numtaps", "nband", "type", "edges", "desired", "weight", "h", "ext", "status", "iterations", "delta"]
    assert [f[0] for f in mbfir.RemezOpts._fields_] == ["grid_density", "maxiter"]


def test_dzrf_name_keeps_dzrf_mb_importable():
    from mbfir.dzrf import dzrf_mb
    import sys
    assert callable(mbfir.dzrf) and mbfir.dzrf is slrclassic.dzrf
    assert mbfir.dzrf_mb is dzrf_mb and sys.modules["mbfir.dzrf"].dzrf_mb is dzrf_mb
    import mbfir.dzrf as m
    assert m.dzrf_mb is dzrf_mb
    for name in ("remez", "remez_batch", "fmp", "msinc", "firls_lp", "dzlp", "dzls", "dzmp", "dzrf_batch", "sim_rf_scale"):
        assert callable(getattr(mbfir, name)), name


def test_sim_rf_scale_axis_and_calls(monkeypatch):
    calls = []

    def fake_bloch(b1, gr, tp, t1, t2, df, dp, mode=0, **kw):
        calls.append(dict(b1=np.asarray(b1), tp=tp, t1=t1, t2=t2, df=np.asarray(df), dp=dp, nucleus=kw.get("nucleus")))
        n = len(df)
        return np.full((n, 1), 0.1), np.full((n, 1), 0.2), np.full((n, 1), 0.9)
    monkeypatch.setattr(mbfir, "bloch", fake_bloch)
    rf = np.linspace(0, 1, 10) * 0.01
    # the 7-argument form: bw in kHz -> [-3 BW, 3 BW] Hz
    df, mxy, mz = mbfir.sim_rf_scale(rf, 0.04, None, "C-13", bw=0.25)
    assert len(df) == 2048 and df[0] == -750.0 and df[-1] == 750.0 and np.allclose(np.diff(df), 1500 / 2047)
    assert len(calls) == 5 and [float((c["b1"][-1] / rf[-1]).real) for c in calls] == pytest.approx([0.8, 0.9, 1.0, 1.1, 1.2])
    assert calls[0]["tp"] == pytest.approx(0.04e-3) and calls[0]["t1"] == 1e3 and calls[0]["t2"] == 1e3
    assert calls[0]["nucleus"] == "C-13" and mxy.shape == (5, 2048) and np.all(mxy == 0.1 + 0.2j) and np.all(mz == 0.9)
    # the 9-argument form: band edges in kHz -> [f(1) - 300, f(end) + 300] Hz
    calls.clear()
    df, mxy, mz = mbfir.sim_rf_scale(rf, 0.04, [1.0], "H-1", f=[-0.5, -0.2, 0.1, 0.4])
    assert df[0] == -800.0 and df[-1] == 700.0 and len(calls) == 1 and calls[0]["nucleus"] == "H-1" and mxy.shape == (1, 2048)
    with pytest.raises(ValueError):
        mbfir.sim_rf_scale(rf, 0.04, bw=1.0, f=[0, 1])
