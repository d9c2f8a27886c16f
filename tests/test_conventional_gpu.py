"""Conventional SLR designers on the device: the batched Parks-McClellan exchange against SciPy's designs and against the
alternation certificate, fmp against its NumPy restatement, and the dzrf chain (tests/golden/conventional.json)."""
import json
import os

import numpy as np
import pytest

import mbfir
import remez_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def conv():
    """conventional.json (specs) with the vectors of conventional.npz put in place: remez / firls taps (stored as their first
    half), fmp["name"] (real part), dzrf rf."""
    g = os.path.join(ROOT, "tests", "golden", "conventional")
    with open(g + ".json") as fh:
        out = json.load(fh)
    with np.load(g + ".npz", allow_pickle=False) as z:
        for part in ("remez", "firls"):
            for k, v in out[part].items():
                hh = z["%s/%s" % (part, k)]
                v["h"] = np.concatenate([hh, hh[::-1][v["numtaps"] % 2:]])
        out["fmp"] = {k: z["fmp/" + k] for k in out["fmp"]}
        for k, v in out["dzrf"].items():
            v["rf"] = z["dzrf/" + k]
    return out


def spec(d):
    return d["numtaps"], d["edges"], d["desired"], d["weight"]


# ---- the certificate (tests/remez_ref.py), on the host restatement of the grid in the fixture generator ---------------
gold = remez_ref.gold
dense_grid, amplitude = remez_ref.dense_grid, remez_ref.amplitude
weighted_error, certify, CERT_TOL = remez_ref.weighted_error, remez_ref.certify, remez_ref.CERT_TOL


# ---- remez ----------------------------------------------------------------------------------------------------
def test_remez_matches_scipy_fixtures(conv):
    names = sorted(conv["remez"])
    res = mbfir.remez_batch([spec(conv["remez"][k]) for k in names])
    for k, (h, info) in zip(names, res):
        ref = conv["remez"][k]
        hs = np.asarray(ref["h"])
        assert info["status"] == "converged", (k, info)
        assert np.abs(h - hs).max() <= 1e-7 * np.abs(hs).max(), (k, np.abs(h - hs).max() / np.abs(hs).max())
        assert abs(abs(info["delta"]) - ref["delta"]) <= 1e-7 * ref["delta"], (k, info["delta"], ref["delta"])


def test_remez_certificate_every_fixture(conv):
    designs = dict((k, spec(v)) for k, v in conv["remez"].items())
    designs.update((k, spec(v)) for k, v in conv["certify_only"].items())
    assert any(v[0] == 2047 for v in designs.values()) and any(v[0] == 2046 for v in designs.values())
    names = sorted(designs)
    res = mbfir.remez_batch([designs[k] for k in names])
    for k, (h, info) in zip(names, res):
        assert info["status"] == "converged", (k, info["status"], info["iterations"])
        certify(h, info, *designs[k])


def test_remez_sloped_band_certificate():
    # a passband whose desired amplitude falls linearly from 1 to 0.5: outside what scipy.signal.remez can express
    s = (151, [0.0, 0.3, 0.38, 1.0], [1.0, 0.5, 0.0, 0.0], [1.0, 20.0])
    h, info = mbfir.remez(*s, info=True)
    assert info["status"] == "converged"
    certify(h, info, *s)


def test_remez_batch_bit_identical_to_single_and_repeatable(conv):
    rng = np.random.default_rng(7)
    base = [spec(v) for v in conv["remez"].values() if v["numtaps"] <= 519]
    jobs = []
    for i in range(64):
        n, e, d, w = base[i % len(base)]
        jobs.append((n, e, d, [w[0]] + [float(x) * (1 + 0.5 * rng.random()) for x in w[1:]]))
    r1 = mbfir.remez_batch(jobs)
    r2 = mbfir.remez_batch(jobs)
    for (h1, i1), (h2, i2) in zip(r1, r2):
        assert np.array_equal(h1, h2) and i1["delta"] == i2["delta"] and np.array_equal(i1["ext"], i2["ext"])
    for j in (0, 5, 17, 63):
        h, info = mbfir.remez(*jobs[j], info=True)
        assert np.array_equal(h, r1[j][0]) and info["delta"] == r1[j][1]["delta"] and info["iterations"] == r1[j][1]["iterations"]


def test_remez_maxiter_is_not_converged(conv):
    h, info = mbfir.remez(*spec(conv["remez"]["lp519_w300"]), maxiter=1, info=True)
    assert info["status"] == "not converged" and info["iterations"] == 1
    assert np.all(np.isfinite(h)) and np.isfinite(info["delta"])
    with pytest.raises(mbfir.MbfirError):
        mbfir.remez(*spec(conv["remez"]["lp519_w300"]), maxiter=1)


# ---- fmp ------------------------------------------------------------------------------------------------------
def fmp_spread(h):
    """How far the NumPy restatement of fmp.m itself moves when its spectrum takes one-ulp noise (1.1e-16 max|hpf|): the lift
    leaves the spectrum's troughs at 1e-6 |min real(hpf)|, so where the stopband ripple is small the log and the cepstrum amplify
    any FFT's rounding there.  Relative to max|h|."""
    return float(np.abs(gold.fmp_np(h, 1.1e-16) - gold.fmp_np(h)).max() / np.abs(h).max())


def test_fmp_matches_numpy(conv):
    """Device fmp against the NumPy fixture: 1e-9 of max|h| wherever the NumPy restatement is itself reproducible to 1e-9 under
    one-ulp spectrum noise; on the spectra where it is not (stopband troughs near 1e-12 after the lift),
    within that spread of its own."""
    assert max(conv["remez"][k]["numtaps"] for k in conv["fmp"]) == 2047
    strict = 0
    for k, ref in conv["fmp"].items():
        h = np.asarray(conv["remez"][k]["h"])
        err = float(np.abs(mbfir.fmp(h) - ref).max() / np.abs(h).max())
        spread = fmp_spread(h)
        if spread <= 1e-9:
            strict += 1
            assert err <= 1e-9, (k, err, spread)
        else:
            assert err <= spread, (k, err, spread)
    assert strict >= 5


# ---- dzrf -----------------------------------------------------------------------------------------------------
def test_dzrf_matches_fixture_chain(conv):
    for k, ref in conv["dzrf"].items():
        rf = mbfir.dzrf(ref["np"], ref["tb"], ref["ptype"], ref["ftype"], ref["d1"], ref["d2"])
        r = ref["rf"]
        assert np.abs(rf - r).max() <= 1e-7 * np.abs(r).max(), (k, np.abs(rf - r).max() / np.abs(r).max())


def test_dzrf_batch_equals_single_calls():
    specs = [(65, 6.0, p, f, 0.01, 0.01) for p in ("st", "ex", "se", "inv", "sat") for f in ("ms", "ls", "pm", "min", "max")]
    specs.append(dict(np=150, tb=2.5, ptype="sat", ftype="max", d1=0.05, d2=5e-4))
    out = mbfir.dzrf_batch(specs)
    for s, rf in zip(specs, out):
        a = (s["np"], s["tb"], s["ptype"], s["ftype"], s["d1"], s["d2"]) if isinstance(s, dict) else s
        single = mbfir.dzrf(*a)
        assert np.array_equal(np.asarray(single), np.asarray(rf)), s


def test_inverse_slr_round_trip():
    """b2rf(bsf b) simulated in the hard-pulse model ab2rf inverts (mbfir.abrm, hard_pulse=True) gives back |B| of the designed
    beta (abr's b is -conj of abrm's: the same magnitude).  ex and sat keep max|B| = sqrt(1/2) (1 + d1) < 1, below b2a's clip."""
    n, tb = 128, 6.0
    x = np.linspace(-n / 2, n / 2, 513)[:-1]
    w = -2 * np.pi * x / n
    for ptype, ftype in (("ex", "pm"), ("ex", "min"), ("sat", "max"), ("sat", "ls"), ("ex", "ms")):
        rf = mbfir.dzrf(n, tb, ptype, ftype, 0.01, 0.01)
        d1, d2, bsf = mbfir.slrclassic.ptype_ripples(ptype, 0.01, 0.01)
        b = {"pm": lambda: mbfir.dzlp(n, tb, d1, d2), "min": lambda: mbfir.dzmp(n, tb, d1, d2)[::-1],
             "max": lambda: mbfir.dzmp(n, tb, d1, d2), "ls": lambda: mbfir.dzls(n, tb, d1, d2),
             "ms": lambda: mbfir.msinc(n, tb / 4)}[ftype]() * bsf
        _, beta = mbfir.abrm(rf, x, hard_pulse=True)
        B = (np.asarray(b, dtype=complex)[None, :] * np.exp(1j * w[:, None] * np.arange(n)[None, :])).sum(1)
        err = np.abs(np.abs(beta) - np.abs(B)).max()
        assert err <= 1e-8, (ptype, ftype, err)


# ---- sim_rf_scale ---------------------------------------------------------------------------------------------
def test_sim_rf_scale_equals_bloch_calls():
    rf = mbfir.rfscaleg(mbfir.dzrf(100, 4.0, "ex", "pm"), 4.0, 1.0705)
    dt = 4.0 / 100
    scale = [0.9, 1.0, 1.1]
    df, mxy, mz = mbfir.sim_rf_scale(rf, dt, scale, "C-13", bw=0.5)
    assert mxy.shape == (3, 2048) and mz.shape == (3, 2048)
    for k, s in enumerate(scale):
        mx, my, m_z = mbfir.bloch(rf * s, np.zeros(len(rf)), dt * 1e-3, 1e3, 1e3, df, 0.0, 0, nucleus="C-13")
        assert np.array_equal(mxy[k], mx.ravel() + 1j * my.ravel()) and np.array_equal(mz[k], m_z.ravel())
