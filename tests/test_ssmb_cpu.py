"""Multiband spectral-spatial designer, host side (no GPU): band folding, argument checks, a NumPy restatement of the 2D inverse
SLR (oracle.slr.b2rf and FFTs) against dzepse's fixtures, and dzss_mb's host logic and physics with the device steps replaced by
the oracle (oracle.designers for the spectral beta, the restatement for the 2D SLR, oracle.bloch.blochsimfz for the simulation)."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import mbfir
from mbfir import epse, ssmb
from oracle import bloch, designers, slr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DZEPSE_TOL = 5e-10           # relative to max|rf|, as tests/test_epse_gpu.py


def slr2d_np(R, literal=False):
    """The 2D inverse SLR of mbfir.slr2d_batch restated (dzepse.m:39-49): b2rf of every row, the hard-pulse beta of every stage-1
    angle (literal: dzepse's sin(conj(theta) / 2)), fftcp over 2m, the middle m samples, b2rf of every column, conjugated."""
    out = []
    for r in np.asarray(R, dtype=np.complex128):
        m, n = r.shape
        rn1 = np.stack([slr.b2rf(r[q]) for q in range(m)])
        s = np.sin(np.conj(rn1) / 2) if literal else np.sin(np.abs(rn1) / 2) * np.exp(-1j * np.angle(rn1))
        cols = []
        for j in range(n):
            p2 = epse.fftcp(s[:, j], 2 * m) / (2 * m)
            cols.append(np.conj(slr.b2rf(p2[m // 2:m // 2 + m])))
        out.append(np.stack(cols, axis=1))
    return np.stack(out)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_epse", os.path.join(GOLDEN, "make_golden_epse.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dzepse_r(gen, name):
    """dzepse's own r = pwx' * kws * sin(ang / 2) (dzepse.m:24-36) of a fixture design, from the generator's CPU filters."""
    ang, shape, lgx, tbx, tgx, ngx, sbw, d1, d2, stype = gen.DESIGNS[name]
    pwx = gen.fftcp(gen.dzbeta_se(lgx, tbx, "ls", 0.01, 0.01), 2 * lgx)[lgx // 2:lgx // 2 + lgx]
    kws = gen.dzbeta_se(ngx, (ngx - 1) * tgx * sbw, stype, d1, d2)
    return np.outer(np.conj(pwx), kws) * math.sin(ang / 2), gen.GRADS[shape](lgx)


def test_restatement_literal_form_reproduces_dzepse_fixtures():
    """With dzepse's sin(conj(theta) / 2) the restatement is dzepse's host chain; the hard-pulse axis form differs measurably on
    these designs, whose stage-1 angles are not real (the spatial profile's half-sample phase ramp): hence the literal flag."""
    gen = _generator()
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        names = list(json.load(fh)["dzepse"])
    worst_axis = 0.0
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        for name in names:
            r, gx = dzepse_r(gen, name)
            want = z["dzepse/%s/rf" % name]
            lit = epse.versec(gx, slr2d_np(r[None], literal=True)[0]).ravel(order="F")
            axis = epse.versec(gx, slr2d_np(r[None])[0]).ravel(order="F")
            err = float(np.abs(lit - want).max() / np.abs(want).max())
            assert err <= DZEPSE_TOL, (name, err)
            worst_axis = max(worst_axis, float(np.abs(axis - want).max() / np.abs(want).max()))
    print("axis form against dzepse: worst rel diff %.2e" % worst_axis)
    assert worst_axis > 100 * DZEPSE_TOL


def test_restatement_forms_agree_for_real_angles():
    """For a real angle the hard-pulse axis form is dzepse's sin(conj(theta) / 2), to rounding (exp(-i pi) is not exactly -1)."""
    th = np.random.default_rng(4).uniform(-3, 3, 50)
    assert np.abs(np.sin(np.abs(th) / 2) * np.exp(-1j * np.angle(th)) - np.sin(np.conj(th + 0j) / 2)).max() <= 2e-16


# ---- band folding ------------------------------------------------------------------------------------------------------
def test_fold_bands_wraps_into_the_window_and_sorts():
    fs = 2.0
    out = mbfir.fold_bands([0.1, (2.3, 2.5), -4.6], [0.05, 0.1, 0.02], [10, 20, 30], [0.01, 0.02, 0.03], fs)
    # 0.1 stays, (2.3, 2.5) -> (0.3, 0.5), -4.6 -> -0.6; sorted: -0.6, 0.1, (0.3, 0.5)
    assert out["order"] == [2, 0, 1]
    assert np.allclose(out["mb_cf"][0], -0.6) and np.allclose(out["mb_cf"][1], 0.1) and np.allclose(out["mb_cf"][2], (0.3, 0.5))
    assert out["mb_FA"] == [30, 10, 20] and out["mb_ripple"] == [0.03, 0.01, 0.02] and out["mb_range"] == [0.02, 0.05, 0.1]
    same = mbfir.fold_bands([0.1, -0.3], None, [5, 6], [0.1, 0.2], fs)
    assert same["order"] == [1, 0] and same["mb_range"] is None and same["mb_FA"] == [6, 5]


def test_fold_bands_names_straddling_and_overlapping_bands():
    with pytest.raises(ValueError, match=r"band\(s\) 1 straddle"):
        mbfir.fold_bands([0.0, 0.98], [0.1, 0.1], [10, 20], [0.01, 0.01], 2.0)             # 0.98 +- 0.05 crosses fs/2 = 1
    with pytest.raises(ValueError, match=r"band\(s\) 0 straddle"):
        mbfir.fold_bands([(0.8, 1.3)], None, [10], [0.01], 2.0)                              # -> (-1.2, -0.7): crosses -fs/2
    with pytest.raises(ValueError, match="overlap: 0 and 2"):
        mbfir.fold_bands([0.1, 0.5, 2.15], [0.1, 0.1, 0.1], [10, 0, 20], [0.01] * 3, 2.0)    # 2.15 folds onto 0.15
    with pytest.raises(ValueError):
        mbfir.fold_bands([0.1, 0.5], [0.1], [10, 0], [0.01, 0.01], 2.0)
    with pytest.raises(ValueError):
        mbfir.fold_bands([0.1], None, [10], [0.01], 0.0)


# ---- argument checks ---------------------------------------------------------------------------------------------------
def _trap(n, ramp, amp):
    t = np.full(n, float(amp))
    t[:ramp] = amp * (np.arange(ramp) + 0.5) / ramp
    t[n - ramp:] = t[:ramp][::-1]
    return t


CS = mbfir.spec.spectrum_c13(3.0) * 1e-3                   # kHz: pyruvate, lactate, alanine, hydrate, bicarbonate, urea
# C-13 metabolite-specific excitations at 3 T: pyruvate 10 degrees, lactate 30, alanine (and bicarbonate) held at 0
SYM = dict(gx=_trap(100, 20, 4.0), dt=0.004, ngx=25, mb_cf=[CS[0], CS[2], CS[1]], mb_range=[0.06] * 3, mb_FA=[10, 0, 30],
           mb_ripple=[0.01] * 3)
FLY = dict(gx=_trap(80, 16, 4.0), dt=0.004, ngx=25, mb_cf=[CS[0], CS[2], CS[1], CS[4]], mb_range=[0.06] * 4, mb_FA=[10, 0, 30, 0],
           mb_ripple=[0.01] * 4, gfb=-_trap(40, 8, 8.0))             # the rewinder's area cancels the lobe's


@pytest.mark.parametrize("bad", [dict(gx=_trap(99, 20, 4.0)), dict(gx=np.ones(2050)), dict(gx=-_trap(100, 20, 4.0)),
                                 dict(gx=np.zeros(100)), dict(dt=0.0), dict(ngx=1), dict(ngx=2049), dict(ngx=12.5),
                                 dict(ftype="ms"), dict(ftype="bogus"), dict(ptype="st"), dict(nucleus="N-15"),
                                 dict(downsampling=2), dict(shift_f=1), dict(gfb=[]), dict(bogus=1),
                                 dict(mb_cf=[CS[0], CS[0] + 0.03, CS[1]])])
def test_dzss_mb_argument_errors(bad):
    with pytest.raises(ValueError):
        mbfir.dzss_mb_batch([dict(SYM, **bad)])


def test_dzss_mb_missing_arguments_and_empty_batch():
    with pytest.raises(ValueError, match="missing"):
        mbfir.dzss_mb_batch([{k: v for k, v in SYM.items() if k != "mb_FA"}])
    with pytest.raises(ValueError):
        mbfir.dzss_mb_batch([(SYM["gx"], 0.004, 25)])
    assert mbfir.dzss_mb_batch([]) == []


def test_slr2d_batch_argument_errors():
    for shape in [(8, 8), (1, 9, 8), (1, 8, 1), (1, 8, 2049), (1, 2050, 8), (0, 8, 8)]:
        with pytest.raises(ValueError):
            mbfir.slr2d_batch(np.ones(shape))


def test_new_symbols_are_bound():
    assert "mbfir_slr2d_batch" in mbfir.SYMBOLS
    assert mbfir.dzss_mb is ssmb.dzss_mb and mbfir.dzss_mb_batch is ssmb.dzss_mb_batch


# ---- dzss_mb with the device steps replaced by the oracle --------------------------------------------------------------
@pytest.fixture
def host_only(monkeypatch):
    calls = {"solve": [], "slr2d": []}

    def solve_batch(jobs, opts=None, **kw):
        calls["solve"].append(len(jobs))
        return [getattr(designers, name)(*args)[:2] for name, args in jobs]

    def slr2d_batch(R, literal=False, ctx=None):
        calls["slr2d"].append(np.shape(R))
        return slr2d_np(R, literal)
    monkeypatch.setattr(mbfir, "solve_batch", solve_batch)
    monkeypatch.setattr(mbfir, "slr2d_batch", slr2d_batch)
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: None)
    return calls


def test_dzss_mb_host_logic(host_only):
    (rf, g, info), (rf2, g2, info2) = mbfir.dzss_mb_batch([SYM, FLY])
    assert host_only["solve"] == [2] and sorted(host_only["slr2d"]) == [(1, 80, 25), (1, 100, 25)]   # one launch per shape
    assert info["status"] == info2["status"] == "Solved"
    # symmetric EPI: 25 lobes of alternating sign, a subpulse on each
    assert len(rf) == len(g) == 25 * 100 and np.array_equal(g[:100], SYM["gx"]) and np.array_equal(g[100:200], -SYM["gx"])
    assert info["Ts"] == pytest.approx(0.4) and info["fs"] == pytest.approx(2.5) and info["ngx"] == 25
    # flyback: the rewinder between the lobes, RF off there, none after the last lobe
    assert len(rf2) == len(g2) == 25 * 80 + 24 * 40 and info2["Ts"] == pytest.approx(0.48)
    assert np.array_equal(g2[80:120], FLY["gfb"]) and np.array_equal(g2[-80:], FLY["gx"])
    assert not np.any(rf2[80:120]) and np.all(np.abs(rf2[:80]) > 0)
    # units: radians per sample -> Gauss, gamma of C-13; slice thickness tbx / (gamma * lobe area)
    assert info["thk"] == pytest.approx(4.0 / (1.0705 * SYM["gx"].sum() * 0.004))
    rad = np.conj(rf[:100]) * 2 * np.pi * 1.0705 * 0.004
    r = np.outer(np.conj(info["pwx"]), info["beta"])
    assert np.allclose(rad, epse.versec(SYM["gx"], slr2d_np(r[None])[0])[:, 0], rtol=0, atol=1e-15)
    # the spectral beta is dzrf_mb's: the ap_cvx taps reversed, on the folded spec
    h, _ = designers.fir_ap_cvx(25, info["b_spec"]["f"], info["b_spec"]["a"], info["b_spec"]["d"], 1.0, 1e-3)
    assert np.array_equal(info["beta"], h[::-1])
    f, a, d = mbfir.spec.band_spec(25, 0.4, SYM["mb_cf"], SYM["mb_range"], SYM["mb_FA"], SYM["mb_ripple"], "ex")
    assert np.array_equal(info["b_spec"]["f"], f) and np.array_equal(info["b_spec"]["a"], a)


def test_dzss_mb_failed_design_returns_empty(host_only):
    rf, g, info = mbfir.dzss_mb(**dict(SYM, ngx=4))                      # four taps cannot separate the bands
    assert info["status"] == "Failed" and len(rf) == 0 and len(g) == 0 and len(info["beta"]) == 0


# Physics of the two C-13 excitations, simulated by the CPU Bloch restatement in physical units (DESIGN.md section 8g has the
# measured figures; tests/test_ssmb_gpu.py holds the device pulses to the same thresholds).
CENTRE_TOL = 0.005           # max | |Mxy| of the pulse at x = 0 - |Mxy| of the hard-pulse train |, over every band (0.0019 / 0.0028)
PASS_LO, PASS_HI = 0.80, 1.05  # |Mxy| within +-0.35 thk over |Mxy| at x = 0, excited bands (0.837 .. 1.018)
STOP_MAX = 0.005             # |Mxy| beyond 1.5 thk, every band (0.0018)
NULL_MAX = 0.02              # |Mxy| at x = 0 in the 0 degree bands (0.0089)


def hard_pulse_train(beta, starts, lgx, nsamp, dt, gamma):
    """The spectral beta's own pulse b2rf(beta) as hard pulses: one dt-long sample at every subpulse's centre, no gradient (Gauss)."""
    b1 = np.zeros(nsamp, dtype=np.complex128)
    b1[np.asarray(starts) + lgx // 2] = slr.b2rf(beta) / (2 * np.pi * gamma * dt)
    return b1


def physics_grids(spec, info):
    fr = np.concatenate([np.linspace(c - 0.03, c + 0.03, 7) for c in spec["mb_cf"]]) * 1e3           # Hz, every band
    x = np.linspace(-3, 3, 241) * info["thk"]                                                         # cm
    return fr, x


def check_physics(spec, rf, g, info, sim):
    """sim(b1, g, df, x) -> |Mxy| (len(df), len(x)) with dt = spec['dt'] ms per sample."""
    p = ssmb._norm_spec(spec)
    _, starts = ssmb._gradient(p, info["ngx"])
    fr, x = physics_grids(spec, info)
    centre = sim(rf, g, fr, np.zeros(1))[:, 0]
    train = sim(hard_pulse_train(info["beta"], starts, p["lgx"], len(rf), spec["dt"], p["gamma"]), np.zeros(len(rf)), fr,
                np.zeros(1))[:, 0]
    dev = float(np.abs(centre - train).max())
    cf = np.asarray(spec["mb_cf"]) * 1e3
    prof = sim(rf, g, cf, x)
    inner, outer = np.abs(x) <= 0.35 * info["thk"], np.abs(x) >= 1.5 * info["thk"]
    rep = dict(centre_dev=dev, stop=float(prof[:, outer].max()), null=0.0, pass_lo=1.0, pass_hi=1.0)
    for k, fa in enumerate(spec["mb_FA"]):
        c0 = prof[k, len(x) // 2]
        if fa > 0:
            assert c0 == pytest.approx(math.sin(math.radians(fa)), abs=0.03)
            rep["pass_lo"] = min(rep["pass_lo"], float(prof[k, inner].min() / c0))
            rep["pass_hi"] = max(rep["pass_hi"], float(prof[k, inner].max() / c0))
        else:
            rep["null"] = max(rep["null"], float(c0))
    print("physics: %s" % ", ".join("%s %.4f" % kv for kv in rep.items()))
    assert rep["centre_dev"] <= CENTRE_TOL
    assert PASS_LO <= rep["pass_lo"] and rep["pass_hi"] <= PASS_HI
    assert rep["stop"] <= STOP_MAX and rep["null"] <= NULL_MAX


def sim_cpu(dt):
    def sim(b1, g, df, x):
        grad = np.zeros((len(b1), 3))
        grad[:, 0] = g
        pos = np.zeros((len(x), 3))
        pos[:, 0] = x
        m = bloch.blochsimfz(b1, grad, dt * 1e-3, 1e6, 1e6, df, pos)
        return np.abs(m[:, :, 0, 0] + 1j * m[:, :, 0, 1])
    return sim


@pytest.mark.parametrize("spec", [SYM, FLY], ids=["symmetric", "flyback"])
def test_dzss_mb_physics_with_oracle(host_only, spec):
    rf, g, info = mbfir.dzss_mb(**spec)
    assert info["status"] == "Solved"
    check_physics(spec, rf, g, info, sim_cpu(spec["dt"]))
