"""tests/specfact_ref.py, the reference of the tap extraction's stages (csrc/specfact.hip), checked without a GPU: its chain against
oracle/specfact.py and the fmp fixtures, its float64 twin (the kernel's bit reversal and radix-2 levels in NumPy) below every stage
bound at every case the device test uses, the spread conditions those cases must meet, and that it rejects twelve planted errors,
each at the stage that carries it and on the smallest case that has the feature.  A reference that cannot fail proves nothing."""
import os
import re

import numpy as np
import pytest

import mbfir
import specfact_ref as sr
from oracle import specfact

CASES = sr.cases()


def worst(fracs):
    return {k: float(np.max(v)) for k, v in fracs.items()}


def test_case_list_covers_what_it_must():
    assert {1, 2, 3, 16, 17, 33, 64, 65, 257, 512, 2048} <= set(sr.SIZES)
    assert sr.lp_of(2 * sr.N_MAX - 1) == 65536 and sr.lp_of(2 * (sr.N_MAX + 1) - 1) > 65536
    assert sr.lp_of(2 * 512 - 1) == 8192 and sr.lp_of(33) == 8 * 64 and sr.lp_of(32) == 8 * 32
    names = set(CASES)
    for b in ("seed4", "seed16", "seed28", "seed2324", "headline"):
        assert "B_" + b in names and {"C_%s_%g" % (b, t) for t in sr.T_LEVELS} <= names
    assert {"F_%d_%s" % (l, c) for l in (3, 5, 31, 33, 129) for c in ("real", "cplx")} <= names
    assert CASES["F_dzlp2047"][2] == 2047 and not np.iscomplexobj(CASES["F_dzlp2047"][1])
    assert CASES["A_n33_tiny"][1][0] < 1e-10 and len(CASES["B_headline"][1]) == 1023


@pytest.mark.parametrize("name", ["A_n2", "A_n17", "A_n257", "B_seed16", "C_seed4_1e-06"])
def test_chain_is_the_oracles_fmp2(name):
    """The reference restates fir_ap_cvx.m from its text; this ties it to the package's oracle of the same chain."""
    _, x, n = CASES[name]
    sp, ch = sr.reference(name)
    ho = specfact.fmp2(specfact.x_to_r(x, n))
    hmax = np.abs(ho).max()
    assert np.abs(ch["h"][0].astype(np.complex128) - ho).max() <= 1e-9 * hmax + 2 * sp[0]
    hpf = np.fft.fft(sr.place(0, x, n)[0].astype(np.complex128))
    assert np.abs(ch["hpf"][0].astype(np.complex128) - hpf).max() <= 1e-12 * np.abs(hpf).max()


def test_chain_is_the_fmp_fixture():
    import json
    with open(os.path.join(sr.GOLDEN, "conventional.json")) as fh:
        conv = json.load(fh)
    with np.load(os.path.join(sr.GOLDEN, "conventional.npz")) as z:
        for k in conv["fmp"]:
            sp, ch = sr.reference("F_" + k)
            ref = z["fmp/" + k]
            assert np.abs(ch["h"][0].astype(np.complex128) - ref).max() <= 1e-9 * np.abs(ref).max() + 2 * sp[0], k


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "D_zero"))
def test_twin_below_every_bound(name):
    kind, inp, n = CASES[name]
    got = sr.twin(kind, inp, n)
    fracs, exact = sr.stage_fractions(got, kind, inp, n)
    assert set(fracs) == set(sr.STAGES) | ({"lift"} if kind == 1 else set())      # no stage skipped
    assert all(exact.values()), exact
    for k, v in worst(fracs).items():
        assert v < 1.0, (k, v)
    sp, ch = sr.reference(name)                                                  # and end to end
    err = np.abs(got["st_h"].astype(sr.CLD) - ch["h"]).astype(np.float64)
    assert np.all(err <= 2 * sp[:, None] + ch["h_bound"]), (name, err.max(), sp)


def test_twin_on_the_exact_zero():
    """(D): r = [-1, 2, -1] sums to exactly 0 at k = 0 in any order; the logarithm is -inf there and every tap comes back non-finite,
    in the twin as in the oracle."""
    kind, inp, n = CASES["D_zero"]
    with np.errstate(invalid="ignore"):
        got = sr.twin(kind, inp, n)
    assert got["st_hpf"][0, 0] == 0 and got["st_xl"][0, sr.lp_of(3) // 2] == -np.inf
    fracs, exact = sr.stage_fractions(got, kind, inp, n, stages=("hpf", "xl"))
    assert max(worst(fracs).values()) < 1.0 and all(exact.values())
    assert not np.isfinite(got["st_h"]).any()
    with np.errstate(all="ignore"):
        assert not np.isfinite(specfact.fmp2(specfact.x_to_r(inp, n))).any()


def test_spread_conditions():
    """What makes the end-to-end bound mean something: the strict cases exist and are strict, the loose regime is really present."""
    rel = {}
    for name in CASES:
        if sr.family(name) in "AC":
            sp, ch = sr.reference(name)
            rel[name] = float(sp[0] / np.abs(ch["h"]).max())
    strict = [k for k in rel if sr.strict(k)]
    assert len([k for k in strict if k[0] == "A"]) == len(sr.SIZES) + 1 and len([k for k in strict if k[0] == "C"]) == 5
    for k in strict:
        assert rel[k] <= sr.STRICT, (k, rel[k])
    assert any(v >= sr.LOOSE for k, v in rel.items() if k[0] == "C")


# plant -> (the stage that must reject it, the smallest case that has the feature).  n = 1 transforms a single non-zero sample and a
# constant xl: no twiddle other than 1 meets a non-zero operand there, and the bin at lp / 2 is 0.  A rotation recurrence from a
# correctly rounded seed drifts slowly (its twiddles are 250 u off after 4096 steps) and a correct transform uses 1 / (eta sqrt L) =
# 1 / 60 of its worst-case bound, so the recurrence shows from the size at which it is ~100 u off: lp = 4096 at the latest, and at
# the headline's lp = 8192.  Below that its twiddles are as good as the budget allows sincospi to be, and no bound can tell.
# min |hpf| differs from min real(hpf) only where the spectrum goes negative: the 21-tap equiripple filter is the shortest such case.
PLANTED = {"tw32": ("hpf", "A_n2"), "twrot": ("hpf", None), "nyq2": ("xlfp", "A_n2"), "dc2": ("xlfp", "A_n1"), "zero_hlp": ("xlfp", "A_n2"),
           "padfloor": ("hpf", "A_n1"), "noconj": ("h", "A_n2"), "nosqrt": ("xl", "A_n1"), "inv2": ("h", "A_n1"), "inv0": ("h", "A_n1"),
           "lift5": ("lift", "F_3_real"), "minabs": ("lift", "F_lp21")}


@pytest.mark.parametrize("plant", sr.PLANTS)
def test_planted_errors_are_caught(plant):
    stage, name = PLANTED[plant]
    if name is None:                                                  # the first size at which the planted error leaves the bound
        for n in sr.SIZES:
            kind, inp, _ = CASES["A_n%d" % n]
            if worst(sr.stage_fractions(sr.twin(kind, inp, n, plant=plant), kind, inp, n)[0])[stage] > 1.0:
                break
        assert n <= 257, n
        name = "A_n%d" % n
    kind, inp, n = CASES[name]
    fracs = worst(sr.stage_fractions(sr.twin(kind, inp, n, plant=plant), kind, inp, n)[0])
    assert fracs[stage] > 1.0, (name, fracs)
    single = ("nyq2", "dc2", "zero_hlp", "padfloor", "noconj", "nosqrt", "inv2", "inv0", "lift5", "minabs")
    if plant in single:                                               # every stage takes its input as given: only this one is off
        for k, v in fracs.items():
            assert k == stage or v < 1.0, (name, k, v)
    if plant in ("tw32", "twrot"):                                    # and on the size we ship
        kind, inp, n = CASES["A_n512"]
        big = worst(sr.stage_fractions(sr.twin(kind, inp, n, plant=plant), kind, inp, n)[0])
        assert big["hpf"] > 1.0, big
        if plant == "tw32":                                           # every transform carries it
            assert min(big[k] for k in ("hpf", "xlfp", "a", "h")) > 1.0, big


def test_hook_symbol_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbfir.h")).read()
    m = re.search(r"\bint\s+mbfir_test_specfact_stages\s*\(([^;]*)\)\s*;", hdr)
    assert m
    res, args = mbfir.SYMBOLS["mbfir_test_specfact_stages"]
    assert len(args) == len(m.group(1).split(",")) == 11
