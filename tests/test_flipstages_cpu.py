"""tests/flip_ref.py, the reference of the root-flip search's stages, checked without a GPU: its transforms against plain sums and
mpmath, its chain against oracle.slr.b2rf, its float64 twin (NumPy's FFT, another summation order) within a QUARTER of every stage
bound at every case the device tests use, the conditions those cases must meet, and that it rejects six planted errors, each at
the stage that carries it.  A reference that cannot fail proves nothing."""
import os
import re

import mpmath
import numpy as np
import pytest

import flip_ref as fr
import mbfir
from oracle import slr

# mode-threshold sizes for a device LDS limit of 64 KB and of 160 KB (the device tests compute theirs from the limit they read)
SIZES = sorted({v for lim in (65536, 163840) for v in fr.mode_sizes(lim).values() if v} | {1024})


def test_twiddles_are_exact_to_long_double():
    mpmath.mp.dps = 40
    for N in (8, 24, 504, 1384, 8192):
        w = fr.tw_ld(N)
        for m in (0, 1, N // 8, N // 4, N // 3, N // 2, N - 1):
            want = mpmath.expjpi(-2 * mpmath.mpf(m) / N)
            err = abs(complex(w[m]) - complex(want))              # float64 view: only a gross error shows here ...
            assert err <= 2e-16
            d = mpmath.mpc(mpmath.mpf(str(w[m].real)), mpmath.mpf(str(w[m].imag))) - want       # ... long double digits here
            assert abs(d) <= 2e-19, (N, m)
        assert w[N // 4] == -1j and w[N // 2] == -1


@pytest.mark.parametrize("N", [504, 520, 1040, 1384])
def test_split_transform_equals_the_plain_sum(N):
    rng = np.random.default_rng(N)
    x = (rng.standard_normal((3, N)) + 1j * rng.standard_normal((3, N))).astype(fr.CLD)
    for sign in (-1, +1):
        d = np.abs(fr.dft_ld(x, sign) - fr.dft_direct(x, sign)).max()
        assert d <= 1e-17 * np.abs(x).sum(axis=1).max()
    assert np.abs(fr.dft_direct(x, -1).astype(np.complex128) - np.fft.fft(x.astype(np.complex128), axis=1)).max() <= 1e-11


@pytest.mark.parametrize("name", ["n8_nz7", "n63_nz31", "n64_nz32_clip", "n130_nz32"])
def test_chain_is_b2rf(name):
    """The reference restates the header of flip.hip; this ties it to the package's oracle of the same chain."""
    case, flips, _, sel = fr.stage_case(name)
    ch = fr.chain(case, flips[sel])
    tol = 1e-9 if "clip" not in name else 1e-6
    for q in range(len(sel)):
        beta = ch["beta"][q].astype(np.complex128)
        assert np.abs(ch["a"][q].astype(np.complex128) - slr.b2a(beta)).max() <= tol
        assert np.abs(2 * ch["theta"][q].astype(np.float64) - np.abs(slr.b2rf(beta))).max() <= tol


def _check_twin(case, flips):
    got = fr.twin(case, flips)
    fracs, cond = fr.stage_fractions(got, case, flips)
    assert set(fracs) == set(fr.STAGES)                               # no stage skipped
    assert fr.conditions_ok(cond), cond
    for k in fr.STAGES:
        assert fracs[k] <= 0.25, (k, fracs[k])
    return got, fracs


@pytest.mark.parametrize("name", sorted(fr.STAGE_CASES))
def test_twin_within_a_quarter_of_every_bound(name):
    case, flips, _, sel = fr.stage_case(name)
    got, _ = _check_twin(case, flips[sel])
    ch = fr.chain(case, flips[sel])
    assert np.all(np.abs(got["st_peak"] - ch["peak"]) <= 0.25 * ch["peak_bound"])
    n, nz, kind, rule, level, _ = fr.STAGE_CASES[name]
    m = ch["maxB"]
    if rule == 0:
        assert np.all(np.abs(m - level) <= 1e-9)                       # the DC rule puts every candidate's max|B| at the level
    assert np.all((m >= 1) == (level > 1))


@pytest.mark.parametrize("n", SIZES)
def test_twin_at_the_mode_threshold_sizes(n):
    case, flips = fr.size_case(n)
    _check_twin(case, flips)


def test_case_list_covers_what_it_must():
    rows = list(fr.STAGE_CASES.values())
    assert {2, 3, 8, 63, 64, 65, 130} <= {r[0] for r in rows}
    assert {0, 1, 31, 32, 33} <= {r[1] for r in rows} and any(r[1] == r[0] - 1 for r in rows)
    assert {"complex", "real"} <= {r[2] for r in rows} and {0, 1} == {r[3] for r in rows}
    assert {0.5, 0.985, 1.7} <= {r[4] for r in rows} and {"enum", "bits", "masks"} == {r[5] for r in rows}


def test_winner_is_decided_in_nine_cases_of_ten():
    undecided = []
    for name in sorted(fr.STAGE_CASES):
        case, flips, _, _ = fr.stage_case(name)
        ch = fr.chain(case, flips)
        assert np.all(np.isfinite(ch["peak"])) and ch["pivot"].min() >= fr.PIVOT_MIN
        if not fr.reference_winner(ch["peak"], ch["peak_bound"], flips)[1]:
            undecided.append(name)
    assert 10 * len(undecided) <= len(fr.STAGE_CASES), undecided


# plant -> the stage that must reject it, and cases where its effect is above the rounding level (the clip constant only acts on a
# clipped input, the order of the factors only where the intermediate coefficients differ in size: flip_ref.make_case)
PLANTED = {"window4n": ("xlfp", ["n8_nz7", "n63_nz31", "n64_nz32_clip"]), "kmax": ("afa", ["n8_nz7", "n63_nz31", "n130_nz32"]),
           "edge": ("theta", ["n3_nz1", "n8_nz7", "n65_nz64", "n130_nz32"]), "conj": ("theta", ["n8_nz7", "n63_nz31", "n130_nz32"]),
           "clip": ("bf", ["n3_nz2_real_clip", "n64_nz32_clip"]), "order": ("beta", ["n44_ordered"])}


@pytest.mark.parametrize("plant", fr.PLANTS)
def test_planted_errors_are_caught_at_their_stage(plant):
    stage, names = PLANTED[plant]
    for name in names:
        case, flips, _, sel = fr.stage_case(name)
        fracs, _ = fr.stage_fractions(fr.twin(case, flips[sel], plant=plant), case, flips[sel])
        assert fracs[stage] > 4.0, (name, fracs)
        for k in fr.STAGES:                                            # every stage takes its input as given: only this one is off
            if k != stage:
                assert fracs[k] <= 0.25, (name, k, fracs[k])


def test_mode_formula():
    assert fr.mode_sizes(163840) == dict(last0=441, first1=442, last1=730, first2=731)
    assert fr.mode_sizes(65536) == dict(last0=173, first1=174, last1=291, first2=292)


def test_hook_symbol_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbfir.h")).read()
    m = re.search(r"\bint\s+mbfir_test_flip_stages\s*\(([^;]*)\)\s*;", hdr)
    assert m
    res, args = mbfir.SYMBOLS["mbfir_test_flip_stages"]
    assert len(args) == len(m.group(1).split(","))


@pytest.mark.parametrize("n,level", [(3, 0.5), (33, 0.985), (64, 1.7), (257, 0.9)])
def test_slr_chain_reference(n, level):
    """The end-to-end reference the device's b2a / b2rf are held to: its own float64 twin within a quarter of its bounds, its inputs
    away from every decision, and the oracle's b2rf within the same bounds."""
    b = fr.slr_input(n, level, 300 + n)
    ch = fr.slr_chain(b)
    assert (ch["maxB"] <= fr.CLIP_LOW).all() or (ch["maxB"] >= fr.CLIP_HIGH).all()
    assert ch["pivot"].min() >= fr.PIVOT_MIN
    tw = fr.twin_chain(b)
    assert np.all(np.abs(tw["st_a"].astype(fr.CLD) - ch["a"]).astype(np.float64) <= 0.25 * ch["d_a"])
    assert np.all(np.abs(2 * tw["st_theta"] - np.abs(ch["rf"]).astype(np.float64)) <= 0.25 * ch["d_rf"])
    assert np.all(np.abs(slr.b2rf(b).astype(fr.CLD) - ch["rf"][0]).astype(np.float64) <= ch["d_rf"][0])
