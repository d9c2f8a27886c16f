"""tests/remez_ref.py checked on the host: the long-double replay converges on every spec of the table and its taps pass the
alternation certificate; it agrees with scipy.signal.remez where SciPy can express the spec and converges; an fp64 NumPy restatement
of the kernel's arithmetic (remez_ref.Kern64) passes the comparison the GPU test uses (remez_ref.check_sweep) with no near-tie
allowance; four of five planted changes to the restatement are each caught by a named assertion on the specs, and the fifth (`>`
for `>=` in pass 2, which no spec can show) on an E with planted equal maxima; and the fmp reference.

Measured here (pytest -s prints it per spec): the restatement's delta uses at most 0.08 of its envelope; the three-part envelope of
the taps lies a median of 120 times (up to 7000 times) above the restatement's distance from the reference, beyond the two decades
that would make it the bound, so the taps are held to the fallback bound (remez_ref.taps_bound).  No near-tie in 208 (spec,
iteration) pairs over the 28 specs.  SciPy expresses and converges on 22 of the 28 specs (replay within 3e-13 max|h| of it)."""
import warnings

import numpy as np
import pytest
import scipy.signal as ss

import remez_ref as rr

LD = rr.LD


@pytest.fixture(scope="module")
def sweeps():
    """The restatement's runs maxiter = 1 .. K of every spec, computed once."""
    return {n: rr.kern64(n).sweep() for n in rr.NAMES}


def test_spec_table_reaches_its_edges():
    G = {n: rr.spec_grid(n) for n in rr.NAMES}
    assert [G["tiny%d" % n].L for n in (3, 4, 5)] == [2, 2, 3] and all(G[n].G < 256 for n in rr.SMALL if n.startswith("tiny"))
    assert [G["frexp%d" % n].n1 for n in (29, 30, 31, 32)] == [16, 16, 17, 17]
    assert [G["nodes%d" % n].n1 for n in (509, 511, 512, 513)] == [256, 257, 257, 258]
    assert [G["G%d" % n].G for n in (255, 256, 257, 512, 513)] == [255, 256, 257, 512, 513]
    assert len(rr.SPECS["comb64"][3]) == 64 and rr.SPECS["comb64"][1][-1] < 1
    g = G["point45"]
    assert g.starts[2] - g.starts[1] == 1 and g.f[g.starts[1]] == 0.25
    # type II: f = 1 dropped only when the last edge is 1
    assert G["frexp32"].f[-1] < 1 and G["frexp32"].G == rr.grid(*rr.SPECS["frexp32"], keep_f1=True).G - 1
    assert G["tiny6_below1"].f[-1] == 0.9 and G["bp60_type2_below1"].f[-1] == 0.9 and G["bp60_type2_below1"].f[0] == 0.1
    assert sorted(set(s[4] for s in rr.SPECS.values())) == [8, 16, 32]


@pytest.mark.parametrize("name", rr.NAMES)
def test_replay_converges_and_certifies(name):
    sets, K = rr.replay(name)
    assert K is not None and K <= 25, name
    g = rr.spec_grid(name)
    s = rr.ref_solve(name, sets[-1])
    assert np.all(s.E[sets[-1]] == s.sg * s.delta)
    h = rr.ref_taps(name, sets[-1]).astype(np.float64)
    sp = rr.SPECS[name]
    rr.certify(h, dict(delta=float(s.delta), ext=g.f[sets[-1]]), *sp[:4], density=sp[4])


def test_replay_matches_scipy():
    """On every spec scipy.signal.remez can express (one desired value per band, no point band) and converges on (no error or
    warning, and its taps pass the alternation count on the dense grid) the replay's taps agree with SciPy's to 1e-9 max|h|."""
    compared, left = [], []
    for name in rr.NAMES:
        numtaps, edges, desired, weight, density = rr.SPECS[name]
        nb = len(weight)
        if any(desired[2 * b] != desired[2 * b + 1] or edges[2 * b] == edges[2 * b + 1] for b in range(nb)):
            left.append((name, "not expressible"))
            continue
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                hs = ss.remez(numtaps, np.asarray(edges) / 2, desired[::2], weight=weight, maxiter=25, grid_density=density)
        except Exception:                                       # noqa: BLE001  (SciPy's failure to converge)
            left.append((name, "SciPy does not converge"))
            continue
        L, f, D, W, B = rr.dense_grid(numtaps, edges, desired, weight, density)
        if rr.gold.alternation(W * (D - rr.amplitude(hs, f)), B, 1e-7)[0] < L + 1:
            left.append((name, "SciPy's taps fail the alternation count"))
            continue
        sets, _ = rr.replay(name)
        h = rr.ref_taps(name, sets[-1]).astype(np.float64)
        err = np.abs(h - hs).max() / np.abs(hs).max()
        compared.append((name, err))
        assert err <= 1e-9, (name, err)
    print("compared:", ", ".join("%s %.1e" % c for c in compared))
    print("left out:", left)
    assert len(compared) >= 18, (len(compared), left)


@pytest.mark.parametrize("name", rr.NAMES)
def test_restatement_inside_every_bound(name, sweeps):
    runs = sweeps[name]
    st = rr.check_sweep(name, runs, default_run=runs[max(runs)], allow_ties=False)
    assert st["ties"] == 0 and st["delta"] <= 0.25, st
    # the three-part envelope of the taps beside the restatement's distance from the reference (not asserted: the device's taps are
    # held to the fallback bound, and the first-order envelope is itself exceeded where delta is tiny: w1e4_101, iterations 1 and 2)
    g = rr.spec_grid(name)
    ratios = []
    for k in sorted(runs):
        idx = rr.index_of(g, runs[k]["ext"])
        _, d = rr.taps_bound(name, idx)
        hm = float(np.abs(rr.ref_taps(name, idx)).max())
        ratios.append(rr.taps_envelope(rr.ref_solve(name, idx)) / max(d, 1e-16 * hm))
    worst = max(ratios)
    print("%-18s K %2d  delta err/env %.3f (env %.1e rel, amplification %.1e)  taps envelope / max(restatement, 1e-16 max|h|), largest over k: %.0f"
          % (name, st["K"], st["delta"], st["env_rel"], st["amp"], worst))


def test_restatement_uses_no_near_tie(sweeps):
    pairs = sum(len(r) for r in sweeps.values())
    assert pairs >= 190
    for name, runs in sweeps.items():
        assert rr.check_sweep(name, runs, allow_ties=True)["ties"] == 0, name


# ---- the comparison can fail ------------------------------------------------------------------------------------------------
def _caught(mut, names):
    """{spec: name of the assertion} over the specs on which check_sweep catches the planted change."""
    out = {}
    for n in names:
        try:
            rr.check_sweep(n, rr.Kern64(*rr.SPECS[n], mut=mut).sweep(), allow_ties=True)
        except rr.Miss as e:
            out[n] = e.name
    return out


CHEAP = [n for n in rr.NAMES if rr.SPECS[n][0] <= 130]


@pytest.mark.parametrize("mut,expect", [
    ("start", ("start_set",)),                      # the start set off by one
    ("keep_f1", ("start_set", "ext")),              # the dropped f = 1 kept
    ("sign", ("delta",)),                           # (-1)^k flipped
    ("tapshift", ("taps",)),                        # a[n - 1] + a[n] shifted by one
])
def test_planted_change_is_caught(mut, expect):
    got = _caught(mut, CHEAP)
    print(mut, got)
    assert got and set(got.values()) & set(expect), (mut, got)


def test_pass2_tie_rule_on_planted_equal_maxima():
    """`>` for `>=` in pass 2 (the last of equal maxima instead of the first).  No spec of the table can show it: two candidates of
    one run with the same |E| to the last bit do not occur in any of the 208 (spec, iteration) pairs (two nodes of equal sign always
    have a candidate of the other sign between them: the node between them, or the extremum uphill from it), and the sweep of the
    changed restatement passes on every spec (the loop below runs those up to 130 taps).  The rule is therefore pinned on an E with
    planted equal maxima: the first one is kept, and the planted change keeps the last."""
    for n in CHEAP:
        rr.check_sweep(n, rr.Kern64(*rr.SPECS[n], mut="pass2").sweep(), allow_ties=False)
    g = rr.grid(5, [0, 1], [1, 1], [1])
    E = np.zeros(g.G, dtype=LD)
    E[:] = [0.1 * (-1) ** (j // 12) for j in range(g.G)]
    for j, v in ((2, 1.0), (6, 1.0), (15, -1.0), (19, -1.0), (28, 1.0), (40, -1.0)):
        E[j] = v
    assert list(rr.exchange(g, E, LD(0.5))) == [2, 15, 28, 40]
    assert list(rr.exchange(g, E, LD(0.5), first_of_equal=False)) == [6, 19, 28, 40]


# ---- fmp --------------------------------------------------------------------------------------------------------------------
FMP_LENGTHS, fmp_input = rr.FMP_LENGTHS, rr.fmp_input


@pytest.mark.parametrize("l", (3, 5) + FMP_LENGTHS)
def test_fmp_reference_and_conditioning(l):
    h = rr.replay_taps(*fmp_input(l))
    ref = rr.gold.fmp_np(h)
    spread = float(np.abs(rr.gold.fmp_np(h, 1.1e-16) - ref).max() / np.abs(h).max())
    assert spread <= 1e-9, (l, spread)
    for hh in (h, h * np.exp(0.7j * (np.arange(l) - (l - 1) / 2))):
        a, b = rr.fmp_ref(hh), rr.gold.fmp_np(hh)
        assert np.abs(a - b).max() <= 1e-10 * np.abs(h).max(), (l, np.abs(a - b).max())


def test_fmp_reference_single_tap():
    assert np.allclose(rr.fmp_ref([0.25]), rr.gold.fmp_np([0.25]), rtol=1e-12) and np.isfinite(rr.fmp_ref([0.25])).all()
