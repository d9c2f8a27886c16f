"""Device forward simulation (mbfir_abr, mbfir_abr2, mbfir_bloch) and the dzrf_mb driver end to end on the GPU."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

import mbfir
from oracle import bloch, slr

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "slr_golden.json")))


def cx(d):
    return np.array(d["re"]) + 1j * np.array(d["im"])


@pytest.mark.parametrize("name", ["ap_c13_64_p071", "sinc127_p026", "rand511_p071", "one_tap_p097", "lin_cplx31_p097"])
def test_device_abrm_against_the_oracle(name):
    b = cx(GOLD[name]["b"])
    rf = slr.b2rf(b)
    x = np.linspace(-len(b) / 2, len(b) / 2, 777)
    a0, b0 = bloch.abrm(rf, x)
    a1, b1 = mbfir.abrm(rf, x)
    assert np.max(np.abs(a1 - a0)) <= 1e-12 and np.max(np.abs(b1 - b0)) <= 1e-12
    g = np.linspace(0.5, 1.5, len(rf)) * 2 * np.pi / len(rf)          # explicit per-sample weights
    a0, b0 = bloch.abrm(rf, g, x)
    a1, b1 = mbfir.abrm(rf, g, x)
    assert np.max(np.abs(a1 - a0)) <= 1e-12 and np.max(np.abs(b1 - b0)) <= 1e-12
    a2, b2 = mbfir.abr(rf, x)
    ao, bo = bloch.abr(rf, x)
    assert np.max(np.abs(b2 - bo)) <= 1e-12 and np.max(np.abs(a2 - ao)) <= 1e-12


@pytest.mark.parametrize("name", ["ap_c13_64_p071", "sinc127_p026", "rand200_p071", "qp_modelA48_p026"])
def test_device_closed_loop_beta_to_rf_to_beta(name):
    """b -> mbfir.b2rf -> mbfir.abrm(hard_pulse) : |beta(x)| = |B(-2 pi x / n)| to rounding, all on the device."""
    b = cx(GOLD[name]["b"])
    n = len(b)
    rf = mbfir.b2rf(b)
    x = np.linspace(-n / 2, n / 2, 513)[:-1]
    a1, b1 = mbfir.abrm(rf, x, hard_pulse=True)
    ah, bh = bloch.hard_pulse_ab(rf, x)
    assert np.max(np.abs(a1 - ah)) <= 1e-12 and np.max(np.abs(b1 - bh)) <= 1e-12
    w = -2 * np.pi * x / n
    B = (b[None, :] * np.exp(1j * w[:, None] * np.arange(n)[None, :])).sum(1)
    assert np.max(np.abs(np.abs(b1) - np.abs(B))) < 1e-10
    assert np.max(np.abs(np.abs(a1) ** 2 + np.abs(b1) ** 2 - 1)) < 1e-12


def c13_args():
    cf = mbfir.spec.spectrum_c13(14.0)[[5, 0, 2, 3, 1]] * 1e-3
    cf = cf - cf[4]
    return list(cf), [0.1] * 5, [0, 0, 0, 0, 60], [.005] * 4 + [.01]


def check_profile(rf_pulse, dt, gamma, rf_spec, slack=1.1, hard_pulse=True):
    """|Mxy| over the bands of rf_spec.  hard_pulse: the model the SLR design is exact in -- the band limits then hold
    at the designer's grid points (fir_ap_cvx.m:44-52: 15 n samples, 3-4 per 100 Hz band here) and overshoot by a
    few per cent of the ripple between them, hence the slack; otherwise abrm.m's joint rotations, the reference's simulator, which differs from it
    by O(rf * om) per sample -- a few 1e-3 at these pulse lengths."""
    rf = rf_pulse * (2 * np.pi * gamma * dt)                              # Gauss -> radians per sample (rfscaleg.m)
    fs = 1 / dt
    fk = np.linspace(-fs / 2, fs / 2, 4001)[:-1]
    x = fk * len(rf) * dt
    a, b = mbfir.abrm(rf, -x, hard_pulse=True) if hard_pulse else mbfir.abrm(rf, x)
    mxy = np.abs(2 * np.conj(a) * b)
    f = np.asarray(rf_spec["f"]) * fs / 2
    for i in range(len(rf_spec["d"])):
        sel = (fk >= f[2 * i]) & (fk <= f[2 * i + 1])
        assert sel.sum() >= 5
        assert np.max(np.abs(mxy[sel] - rf_spec["a"][2 * i])) <= rf_spec["d"][i] * slack + 1e-6
    return mxy


def test_dzrf_mb_c13_bssfp_pulse_end_to_end():
    """bSSFP_pulse_sb_mb.m:54: dzrf_mb(100, 0.04, ..., 'ex', 'ap_minorder_cvx', 'C-13', 0, 1, [], dbg, 58) on the
    device, then the simulated |Mxy| against the returned rf_spec (what the script plots)."""
    cf, rng, FA, rp = c13_args()
    rf_pulse, b, rf_spec, b_spec = mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ap_minorder_cvx", "C-13", 0, 1, None, 0, 58)
    assert len(rf_pulse) == len(b) == 58
    assert np.allclose(rf_spec["a"], [0] * 8 + [np.sin(np.pi / 3)] * 2) and np.allclose(rf_spec["d"], rp)
    check_profile(rf_pulse, 0.04, 1.0705, rf_spec)
    check_profile(rf_pulse, 0.04, 1.0705, rf_spec, slack=1.15, hard_pulse=False)       # the reference's simulator
    # the same pulse through the oracle chain
    from oracle import designers
    f, a, d = b_spec["f"], b_spec["a"], b_spec["d"]
    ho, so = designers.fir_ap_cvx(58, f, a, d, 0.1, 1e-3)
    ref = slr.rfscaleg(slr.b2rf(ho[::-1]), 58 * 0.04, 1.0705)
    assert np.max(np.abs(rf_pulse - ref)) <= 1e-6 * np.max(np.abs(ref))
    assert 0.05 < np.max(np.abs(rf_pulse)) < 1.0                          # Gauss, a sane 60-degree C-13 pulse


def test_dzrf_mb_filter_types_and_options():
    cf, rng, FA, rp = c13_args()
    # plain ap_cvx at full length, minimum-order search (min_order = 0.9 default) and fixed transition widening
    for ftype, kw in (("ap_cvx", {}), ("ap_minstopripple_cvx", {}), ("ap_minorder_cvx", dict(probes=4)), ("ap_mintran_cvx", dict(probes=3))):
        rf_pulse, b, rf_spec, b_spec = mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", ftype, "C-13", **kw)
        assert len(rf_pulse) == len(b) and 50 <= len(b) <= 100, ftype
        # 1.4: the 62-tap design's S(w) dips to -8e-5 between grid points, fmp2 takes abs() (fir_ap_cvx.m:281) and
        # |H|^2 then misses S by 2.6e-3 -- in the oracle exactly as on the device (tools/gpu_dzrf.py)
        check_profile(rf_pulse, 0.04, 1.0705, rf_spec, slack=1.4)
        if ftype == "ap_minorder_cvx":
            assert len(b) == int(np.ceil(100 * 0.1 + 57 * 0.9))              # fir_ap.m:173, min order 57
        if ftype == "ap_mintran_cvx":
            assert np.all(np.diff(b_spec["f"])[0::2] > 0.1 / 12.5)            # bands widened
    # saturation pulse type and the frequency shift option (shift the 90-degree band to f = 0, design, shift back)
    rf_pulse, b, rf_spec, b_spec = mbfir.dzrf_mb(128, 0.05, [[-1.0], [1.5]], [0.4, 0.4], [0, 90], [0.01, 0.01], "sat", "ap_cvx", "H-1", 0, 1,
                                                 None, 0, None, None, 2)
    rf = rf_pulse * (2 * np.pi * 4.2576 * 0.05)
    fk = np.array([-1.1, -1.0, -0.9, 1.4, 1.5, 1.6])
    a, bb = mbfir.abrm(rf, fk * len(rf) * 0.05)
    mz = 1 - 2 * np.abs(bb) ** 2
    assert np.all(mz[:3] > 0.985) and np.all(np.abs(mz[3:]) < 0.035)       # abrm.m's model, O(rf om) off the SLR one
    a, bb = mbfir.abrm(rf, -fk * len(rf) * 0.05, hard_pulse=True)
    mz = 1 - 2 * np.abs(bb) ** 2
    assert np.all(mz[:3] > 0.99 - 1e-3) and np.all(np.abs(mz[3:]) < 0.0125)
    # errors and the failure return
    with pytest.raises(NameError):
        mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ms")
    with pytest.raises(ValueError):
        mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ap_cvx", "N-15")
    with pytest.raises(ValueError):
        mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ap_cvx", "C-13", 0, 3)
    # flip_zero = 1: pass-band zeros reflected for a lower peak of beta, same |B(w)| -- the profile still meets the spec
    rf0, b0, _, _ = mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ap_minorder_cvx", "C-13", 0, 1, None, 0, 58)
    rf1, b1, rf_spec, _ = mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ap_minorder_cvx", "C-13", 1, 1, None, 0, 58)
    assert len(b1) == 58 and np.max(np.abs(b1)) <= np.max(np.abs(b0)) * (1 + 1e-9)
    check_profile(rf1, 0.04, 1.0705, rf_spec, slack=1.15)
    rf_pulse, b, rf_spec, b_spec = mbfir.dzrf_mb(100, 0.04, cf, rng, FA, rp, "ex", "ap_minorder_cvx", "C-13", 0, 1, None, 0, 40)
    assert len(rf_pulse) == 0 and len(b) == 0 and len(rf_spec["d"]) == 5      # 40 taps: 'Filter design failed.'


def test_dzrf_mb_downsampled_design():
    """downsampling = 2: design at 80 taps / 0.08 ms (the spec still fits the halved bandwidth of 6.25 kHz),
    upsample to 160 / 0.04 ms (dzrf_mb.m:92-98,228-231)."""
    cf, rng, FA, rp = c13_args()
    rf_pulse, b, rf_spec, b_spec = mbfir.dzrf_mb(160, 0.04, cf, rng, FA, rp, "ex", "ap_cvx", "C-13", 0, 2)
    assert len(rf_pulse) == len(b) == 160
    check_profile(rf_pulse, 0.04, 1.0705, rf_spec, slack=1.5)                         # resample's pass-band droop


# ---- mbfir_bloch: the device twin of bloch_simulation/blochC.c (blochsimfz) --------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_device_bloch_matches_the_oracle_in_every_mode(mode):
    rng = np.random.default_rng(10 + mode)
    nt = 300                                                 # more than one LDS chunk of 256 samples
    b1 = (rng.standard_normal(nt) + 1j * rng.standard_normal(nt)) * 0.02
    gr = rng.standard_normal((nt, 3)) * 0.1
    ts = rng.uniform(0.5e-4, 2e-4, nt)
    df = np.linspace(-500, 500, 37)
    pos = rng.standard_normal((5, 3))
    m0 = rng.standard_normal((37, 5, 3)) * 0.3
    ref = bloch.blochsimfz(b1, gr, ts, 0.08, 0.03, df, pos, mode, m0)
    mx, my, mz = mbfir.bloch(b1, gr, ts, 0.08, 0.03, df, pos, mode, m0[..., 0], m0[..., 1], m0[..., 2])
    got = np.stack([mx, my, mz], -1).reshape(ref.shape)
    assert np.abs(got - ref).max() <= 1e-12
    # end times instead of intervals (blochC.c:669-681) and the H-1 constant (blochH.c:6)
    refh = bloch.blochsimfz(b1, gr[:, :1], ts, 0.5, 0.1, df, pos[:, :1], mode & 2, gamma=bloch.GAMMA_H1)
    mx, my, mz = mbfir.bloch(b1, gr[:, 0], np.cumsum(ts), 0.5, 0.1, df, pos[:, 0], mode & 2, nucleus="H-1")
    assert np.abs(np.stack([mx, my, mz], -1).reshape(refh.shape) - refh).max() <= 1e-12


def test_device_bloch_closes_the_loop_with_abr_as_sim_rf_spectral_runs_it():
    """sim_rf_spectral.m:63-78 simulates the designed pulse with T1 = T2 = 1e3 s over 2048 off-resonances.  Without
    relaxation blochsimfz applies the same rotation per sample as abrm.m, so |Mxy| = 2 |a b| and Mz = 1 - 2 |b|^2 of
    mbfir_abr; with T1 = T2 = 1e3 s and a 4 ms pulse the relaxation moves that by 4e-6."""
    n = 58
    f, a, d = mbfir.spec.spec_c13_bssfp(n) if hasattr(mbfir.spec, "spec_c13_bssfp") else (None, None, None)
    h, status = mbfir.fir_ap_cvx(n, f, a, d, 0.1, 1e-3)
    assert status == "Solved"
    rf = np.asarray(mbfir.b2rf(h[::-1])).ravel()                  # radians per sample (dzrf_mb.m:220,239-240)
    dt = 4e-3 / n
    b1 = rf / (mbfir.GAMMA_C13 * dt)                              # Gauss (rfscaleg)
    df = np.linspace(-3000, 3000, 2048)                           # N_simu = 256*8 (sim_rf_spectral.m:63)
    av, bv = mbfir.abrm(rf, np.ones(n) * dt * 6.283185, df)
    for T, tol in ((1e3, 1e-5), (1e12, 1e-10)):
        mx, my, mz = mbfir.bloch(b1, np.zeros(n), dt, T, T, df, 0.0, 0)
        assert mx.shape == (2048, 1)
        assert np.abs(mx[:, 0] + 1j * my[:, 0] - 2 * av * np.conj(bv)).max() <= tol
        assert np.abs(mz[:, 0] - (1 - 2 * np.abs(bv) ** 2)).max() <= tol


# ---- the single calls at the boundary shapes, against the CPU oracle ----------------------------------------------------------
# mbfir_bloch / mbfir_abr / mbfir_abr2 run as the batch of one pulse at scale 1.0, so the shapes at which a 256-sample LDS tile or
# a 256-point workgroup is exactly full, or one over, are pinned here against the oracle directly.
TOL = 1e-12                                  # the bound of every device simulator against oracle/bloch.py in this file
BLOCH_NT = [1, 256, 257]
BLOCH_SHAPES = [(1, 1), (16, 16), (257, 1)]                    # (nf, npos): 1, 256 and 257 pairs
BLOCH_SHAPES_RECORD = [(1, 1), (3, 2)]                         # the record modes: the output stays small


def bloch_case(mode, nt, nf, npos, h1=False):
    """b1, gr, intervals, t1, t2, df, pos, m0 of one mbfir.bloch call (H-1 case: one gradient and position axis)."""
    rng = np.random.default_rng(1000 * mode + 10 * nt + nf + npos + h1)
    b1 = (rng.standard_normal(nt) + 1j * rng.standard_normal(nt)) * 0.05      # G
    gr = rng.standard_normal((nt, 1 if h1 else 3)) * 0.2                      # G/cm
    ts = rng.uniform(2e-6, 6e-6, nt)                                          # s
    t1, t2 = (2e-3, 1e-3) if mode & 1 else (0.08, 0.03)
    df = np.linspace(-3000, 3000, nf) + rng.uniform(-10, 10)
    pos = rng.standard_normal((npos, 1 if h1 else 3))
    m0 = rng.standard_normal((nf, npos, 3)) * 0.3
    return b1, gr, ts, t1, t2, df, pos, m0


def bloch_cases():
    """(mode, nt, nf, npos) of every case of test_single_bloch_at_the_boundary_shapes"""
    return [(mode, nt, nf, npos) for mode in range(4) for nt in BLOCH_NT
            for nf, npos in (BLOCH_SHAPES_RECORD if mode & 2 else BLOCH_SHAPES)]


def steady_state_margin(b1, gr, ts, t1, t2, df, pos, gamma=bloch.GAMMA_C13):
    """Smallest singular value of I - A over every (frequency, position), with the oracle alone: the pulse maps M to A M + B, so
    B is the endpoint from M = 0 and the columns of A are the endpoints from the unit vectors, less B."""
    nf, npos = len(df), len(pos)
    end = [bloch.blochsimfz(b1, gr, ts, t1, t2, df, pos, 0, np.broadcast_to(v, (nf, npos, 3)), gamma=gamma)[:, :, 0, :]
           for v in np.concatenate([np.zeros((1, 3)), np.eye(3)])]
    A = np.stack([e - end[0] for e in end[1:]], -1)
    return float(np.linalg.svd(np.eye(3) - A, compute_uv=False).min())


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_single_bloch_at_the_boundary_shapes(mode):
    """mbfir.bloch with its in / out magnetisation against blochsimfz: pulse lengths 1, 256, 257 at 1, 256 and 257 pairs."""
    for _, nt, nf, npos in [c for c in bloch_cases() if c[0] == mode]:
        b1, gr, ts, t1, t2, df, pos, m0 = bloch_case(mode, nt, nf, npos)
        if mode & 1:
            assert steady_state_margin(b1, gr, ts, t1, t2, df, pos) > 1e-9
        ref = bloch.blochsimfz(b1, gr, ts, t1, t2, df, pos, mode, m0)
        mx, my, mz = mbfir.bloch(b1, gr, ts, t1, t2, df, pos, mode, m0[..., 0], m0[..., 1], m0[..., 2])
        assert mx.shape == ((nf, npos, nt) if mode & 2 and nt > 1 else (nf, npos))
        err = np.abs(np.stack([mx, my, mz], -1).reshape(ref.shape) - ref).max()
        print("bloch mode %d, nt %d, (%d, %d): %.3g" % (mode, nt, nf, npos, err))
        assert err <= TOL, (mode, nt, nf, npos)


def test_single_bloch_h1_with_end_times():
    b1, gr, ts, t1, t2, df, pos, m0 = bloch_case(0, 257, 16, 16, h1=True)
    ref = bloch.blochsimfz(b1, gr, ts, t1, t2, df, pos[:, 0], 0, m0, gamma=bloch.GAMMA_H1)
    mx, my, mz = mbfir.bloch(b1, gr[:, 0], np.cumsum(ts), t1, t2, df, pos[:, 0], 0, m0[..., 0], m0[..., 1], m0[..., 2], nucleus="H-1")
    assert np.abs(np.stack([mx, my, mz], -1).reshape(ref.shape) - ref).max() <= TOL


def _rf(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (np.pi / n)


@pytest.mark.parametrize("hard_pulse", [False, True])
def test_single_abrm_1d_at_the_boundary_shapes(hard_pulse):
    """mbfir.abrm against the oracle, n and nx each 1, 256, 257; the oracle's hard-pulse model has no form with g."""
    rng = np.random.default_rng(50 + hard_pulse)
    for n in (1, 256, 257):
        rf, g = _rf(rng, n), rng.uniform(0.5, 1.5, n) * 2 * np.pi / n
        for nx in (1, 256, 257):
            x = np.linspace(-n / 2 - 3, n / 2 + 3, nx)
            a1, b1 = mbfir.abrm(rf, x, hard_pulse=hard_pulse)
            a0, b0 = bloch.hard_pulse_ab(rf, x) if hard_pulse else bloch.abrm(rf, x)
            assert a1.shape == (nx,) and max(np.abs(a1 - a0).max(), np.abs(b1 - b0).max()) <= TOL, (n, nx)
            if not hard_pulse:
                a1, b1 = mbfir.abrm(rf, g, x)
                a0, b0 = bloch.abrm(rf, g, x)
                assert max(np.abs(a1 - a0).max(), np.abs(b1 - b0).max()) <= TOL, (n, nx)


def test_single_abrm_2d_at_the_boundary_shapes():
    """mbfir.abrm(rf, g, x, y) against the NumPy restatement of tests/test_abr2batch_gpu.py (itself checked against the oracle
    there), with g and without."""
    spec = importlib.util.spec_from_file_location("abr2batch_gpu", os.path.join(os.path.dirname(__file__), "test_abr2batch_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(60)
    for n in (1, 257):
        rf = _rf(rng, n)
        g = rng.uniform(0.5, 1.5, n) * 2 * np.pi / n + 1j * rng.uniform(-1.5, 1.5, n) * 2 * np.pi / n
        for nx, ny in ((1, 1), (16, 16), (257, 1), (1, 257)):
            x, y = np.linspace(-n / 2 - 3, n / 2 + 3, nx), np.linspace(-n / 3, n / 3 + 1, ny)
            for gv in (g, None):
                a1, b1 = mbfir.abrm(rf, gv, x, y)
                a0, b0 = mod.abr2_np(rf, gv, x, y)
                assert a1.shape == (nx, ny) and max(np.abs(a1 - a0).max(), np.abs(b1 - b0).max()) <= TOL, (n, nx, ny, gv is None)


def test_argument_errors_of_the_single_raw_calls_leave_the_context_usable():
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    nul = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
    v = np.full(8, 0.01)
    z, df, m = np.zeros(8), np.zeros(1), [np.array([0.0]), np.array([0.0]), np.array([1.0])]

    def raw_bloch(mode=0, t1=0.1, df=p(df)):
        return lib.mbfir_bloch(ctx._h, 8, p(v), p(z), nul, nul, nul, p(np.full(8, 4e-6)), t1, 0.1, 1, df, 1, nul, nul, nul, mode,
                               mbfir.GAMMA_C13, *[p(o) for o in m])

    assert raw_bloch(mode=4) == mbfir.E_ARG and raw_bloch(t1=0.0) == mbfir.E_ARG and raw_bloch(df=nul) == mbfir.E_ARG
    out = [np.zeros(2) for _ in range(4)]
    x = np.array([0.0, 1.0])
    assert lib.mbfir_abr(ctx._h, 8, p(v), p(z), nul, 2, p(x), 2, *[p(o) for o in out]) == mbfir.E_ARG
    assert lib.mbfir_abr2(ctx._h, 8, p(v), p(z), nul, nul, 2, p(x), 0, p(x), *[p(o) for o in out]) == mbfir.E_ARG
    assert ctx.last_error().startswith("abr2: need")
    assert raw_bloch() == 0 and m[2][0] < 1.0                                          # the context still works
    assert lib.mbfir_abr(ctx._h, 8, p(v), p(z), nul, 2, p(x), 0, *[p(o) for o in out]) == 0
    a0, b0 = bloch.abrm(v, x)
    assert np.abs(out[0] + 1j * out[1] - a0).max() <= TOL and np.abs(out[2] + 1j * out[3] - b0).max() <= TOL
