"""The root-flip search (csrc/flip.hip) stage by stage through mbfir.test_flip_stages against tests/flip_ref.py: the long-double
reference of every stage, each taken from the device's own output of the stage before and held to the bound counted for that stage
alone (flip_ref's docstring; tests/test_flipstages_cpu.py shows the reference rejects planted errors).  Also here: the three kernel
modes forced and chosen, both thread counts, working-set reuse under a workgroup cap, the arg-min over more than 256 workgroups,
the tie rules, non-finite candidates, the refusals, and sentinels behind every block.

Measured on an MI355X (LDS limit read: 163840 bytes, so a search runs mode 0 up to n = 441, mode 1 up to 730, mode 2 above), worst
|device - reference| / bound per stage over every case of this file (each must be <= 1):
    beta 0.165   bf 0.169   xl 0.524   xlfp 0.105   afa 0.101   a 0.074   theta 0.173
xl spends half of its bound everywhere (three roundings of 1 - a * a and an ulp of the logarithm).  The slr.hip calls, held end to
end, use under 1e-3 of their carried-forward bounds (ab2rf alone: 0.037 of its stage bound): DESIGN.md section 8d-1 has the numbers.
"""
import numpy as np
import pytest

import flip_ref as fr
import mbfir

pytestmark = pytest.mark.gpu
SENT = -7.25
BLOCKS = ("st_beta", "st_bf", "st_xl", "st_xlfp", "st_afa", "st_a", "st_theta", "st_peak")


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def run(case, kw, sel, **over):
    args, ckw = fr.call_args(case)
    ckw.update(kw)
    ckw.update(over)
    r = mbfir.test_flip_stages(*args, sel=sel, guard=5, fill=SENT, **ckw)
    for k, size in r["sizes"].items():                                  # nothing written past any block
        assert np.all(r["raw"][k][size:] == SENT), k
    assert np.all(r["raw"]["blk_i"][len(r["peaks"]):] == -7) and np.all(r["raw"]["report"][8:] == -7)
    nb = r["report"]["blocks"]
    assert np.all(r["raw"]["blk_p"][nb:] == SENT) and np.all(r["raw"]["blk_i"][nb:] == -7)
    return r


def check_stages(r, case, flips_sel, label):
    fracs, cond = fr.stage_fractions(r, case, flips_sel)
    print("fractions", label, {k: "%.3f" % fracs[k] for k in fr.STAGES})
    assert set(fracs) == set(fr.STAGES)
    assert fr.conditions_ok(cond), cond
    for k in fr.STAGES:
        assert fracs[k] <= 1.0, (label, k, fracs[k])
    assert same_bits(r["st_peak"], 2.0 * r["st_theta"].max(axis=1))
    return fracs


def check_report(r, n, nz, forced=-1):
    rep = r["report"]
    nn = 1
    while nn < n:
        nn <<= 1
    assert rep["threads"] == (64 if n <= 64 else 256)
    assert rep["nn"] == nn
    assert rep["words"] == (nz + 31) // 32 and rep["stride"] == 14 * n + 1
    mode = fr.mode_of(n, rep["lds_limit"]) if forced < 0 else forced
    assert rep["mode"] == mode
    assert rep["lds"] == 256 + (0 if mode == 2 else (14 * n + 1) * 16) + ((8 * n + nn) * 16 if mode == 0 else 0)
    assert rep["lds"] <= rep["lds_limit"]


def check_search(r, peaks_ref=None):
    """What one search must satisfy on its own: the winner is the arg-min of the peaks it reports, through the workgroups' bests."""
    pk = r["peaks"]
    w = r["winner"]
    fin = np.isfinite(pk)
    assert w >= 0 and fin[w] and same_bits(pk[w:w + 1], np.array([pk[fin].min()])) and same_bits(np.array([r["winner_peak"]]), pk[w:w + 1])
    bp, bi = r["blk_p"], r["blk_i"]
    nb = len(bp)
    for b in range(nb):                                                  # workgroup b scored candidates b, b + nb, ..
        mine = pk[b::nb]
        if np.isfinite(mine).any():
            assert bi[b] % nb == b and same_bits(bp[b:b + 1], np.array([mine[np.isfinite(mine)].min()])) and pk[bi[b]] == bp[b]
        else:
            assert bi[b] == -1
    assert same_bits(np.array([bp[bi >= 0].min()]), pk[w:w + 1])


@pytest.fixture(scope="module")
def lds_limit():
    case, flips, kw, sel = fr.stage_case("n2_nz0")
    return run(case, kw, sel)["report"]["lds_limit"]


@pytest.mark.parametrize("name", sorted(fr.STAGE_CASES))
def test_stages_against_the_reference(name):
    case, flips, kw, sel = fr.stage_case(name)
    n, nz = case["n"], case["nz"]
    ch = fr.chain(case, flips)
    wref, decided = fr.reference_winner(ch["peak"], ch["peak_bound"], flips)
    sel = np.unique(np.append(sel, wref))
    r = run(case, kw, sel)
    assert r["status"] == 0
    check_report(r, n, nz)
    check_stages(r, case, flips[sel], name)
    check_search(r)
    # the search launch against the stage launch, bit for bit; every candidate's peak against the chain from the reference's beta
    assert same_bits(r["peaks"][sel], r["st_peak"])
    assert np.all(np.abs(r["peaks"] - ch["peak"]) <= ch["peak_bound"])
    w = r["winner"]
    if decided:
        assert w == wref
    rw = r if w in sel else run(case, kw, [w])
    q = int(np.nonzero(np.asarray(sel if rw is r else [w]) == w)[0][0])
    assert same_bits(rw["beta"], rw["st_beta"][q])


@pytest.mark.parametrize("name", ["n8_nz7", "n64_nz33", "n130_nz32"])
def test_beta_criterion(name):
    case, flips, kw, sel = fr.stage_case(name)
    r = run(case, kw, sel, criterion="beta")
    beta, bound, _ = fr.build(case, flips[sel])
    assert np.all(np.abs(r["st_beta"].astype(fr.CLD) - beta).astype(np.float64) <= bound)
    mag = np.abs(r["st_beta"].astype(fr.CLD)).max(axis=1).astype(np.float64)
    assert np.all(np.abs(r["st_peak"] - mag) <= 4 * fr.U * mag)                     # hypot, at 2 u
    assert same_bits(r["peaks"][sel], r["st_peak"])
    check_search(r)
    for k in BLOCKS[1:-1]:                                               # the RF stages are not run: their blocks stay as given
        assert np.all(r["raw"][k] == SENT), k
    allb = fr.build(case, flips)[0]
    want = np.abs(allb).max(axis=1).astype(np.float64)
    assert np.all(np.abs(r["peaks"] - want) <= 4 * fr.U * want + fr.build(case, flips)[1].max(axis=1))


@pytest.mark.parametrize("name", ["n65_nz33", "n130_nz32"])
def test_forced_modes_give_the_same_bits(name):
    """The three instantiations differ in the address space of the working set and the twiddles, not in the arithmetic."""
    case, flips, kw, sel = fr.stage_case(name)
    runs = [run(case, kw, sel, force_mode=m) for m in (0, 1, 2)]
    for m, r in enumerate(runs):
        check_report(r, case["n"], case["nz"], forced=m)
        check_stages(r, case, flips[sel], "%s mode %d" % (name, m))
        check_search(r)
    for r in runs[1:]:
        for k in BLOCKS + ("peaks", "beta", "blk_p", "blk_i"):
            assert same_bits(r[k], runs[0][k]), k
        assert r["winner"] == runs[0]["winner"]


@pytest.mark.parametrize("which", ["last0", "first1", "last1", "first2", "n1024"])
def test_the_mode_a_search_chooses_at_its_thresholds(which, lds_limit):
    sizes = dict(fr.mode_sizes(lds_limit), n1024=1024)
    n = sizes[which]
    assert n is not None, "this device's LDS limit leaves a mode unused up to n = 1024: %r" % (sizes,)
    want = dict(last0=0, first1=1, last1=1, first2=2, n1024=fr.mode_of(1024, lds_limit))[which]
    case, flips = fr.size_case(n)
    sel = np.arange(8)
    r = run(case, dict(masks=flips.T.copy()), sel)
    print("report", which, n, r["report"])
    check_report(r, n, case["nz"])
    assert r["report"]["mode"] == want and r["report"]["threads"] == 256
    check_stages(r, case, flips, "%s n=%d" % (which, n))
    check_search(r)
    assert same_bits(r["peaks"], r["st_peak"])
    assert same_bits(r["beta"], r["st_beta"][r["winner"]])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_working_set_reuse_under_a_workgroup_cap(mode):
    """Ten candidates on three workgroups: each workgroup scores three or four candidates on one working set (mode 2: one scratch
    slice), in the search launch and in the stage launch alike."""
    case, _, _, _ = fr.stage_case("n65_nz33")
    flips = fr.pick_flips(case, 10, 41)
    kw = dict(masks=flips.T.copy())
    sel = np.arange(10)
    free = run(case, kw, sel, force_mode=mode)
    capped = run(case, kw, sel, force_mode=mode, max_blocks=3)
    assert capped["report"]["blocks"] == 3 and free["report"]["blocks"] == 10
    for k in BLOCKS + ("peaks", "beta"):
        assert same_bits(capped[k], free[k]), k
    assert capped["winner"] == free["winner"]
    check_search(capped)
    check_stages(capped, case, flips, "capped mode %d" % mode)
    assert same_bits(capped["peaks"], capped["st_peak"])


def test_argmin_over_more_than_256_workgroups():
    """1024 enumerated candidates at n = 8 through 6 source bits: 64 different polynomials, each sixteen times."""
    case = fr.make_case(8, 6, "complex", 0, 0.5, 77)
    eb = [(j << 1) | (j & 1) for j in range(6)]
    kw = dict(enum_bits=eb, ncand=1024)
    flips = fr.enum_flips(6, 1024, eb)
    sel = np.array([0, 63, 64, 1023])
    lo, hi = run(case, kw, sel), run(case, kw, sel, tie_high=True)
    assert lo["report"]["blocks"] > 256
    for r in (lo, hi):
        check_search(r)
        check_stages(r, case, flips[sel], "n8 x 1024")
        assert same_bits(r["peaks"], np.tile(r["peaks"][:64], 16))
    assert same_bits(lo["peaks"], hi["peaks"])
    best = np.nonzero(lo["peaks"] == lo["peaks"].min())[0]
    assert len(best) >= 16 and lo["winner"] == best.min() and hi["winner"] == best.max()
    ch = fr.chain(case, flips[:64])
    wref, decided = fr.reference_winner(ch["peak"], ch["peak_bound"], flips[:64])
    assert decided and lo["winner"] == wref and hi["winner"] == wref + 960


def test_ties_between_identical_masks():
    case, flips, _, _ = fr.stage_case("n63_nz31")
    ch = fr.chain(case, flips)
    order = np.argsort(ch["peak"])
    cols = flips[[order[3], order[0], order[5], order[0], order[1], order[0], order[7]]]       # the best one three times
    kw = dict(masks=cols.T.copy())
    lo, hi = run(case, kw, [1, 3, 5]), run(case, kw, [1, 3, 5], tie_high=True)
    assert lo["winner"] == 1 and hi["winner"] == 5
    for r in (lo, hi):
        check_search(r)
        assert same_bits(r["st_peak"], np.repeat(r["st_peak"][:1], 3)) and same_bits(r["st_beta"][0], r["st_beta"][2])
        assert same_bits(r["beta"], r["st_beta"][0])
        assert r["peaks"][r["winner"]] == r["peaks"].min()


ZERO_DC = dict(n=4, nz=2, c0=np.array([1.0, 2.0], dtype=complex), z=np.array([1.0, 0.5], dtype=complex),
               zf=np.array([4.0, 2.0], dtype=complex), rule=0, target=0.25 + 0j, criterion="rf")


@pytest.mark.parametrize("criterion", ["rf", "beta"])
def test_a_candidate_without_a_finite_peak_never_wins(criterion):
    """(x + 2)(x - 1)(x - 1/2) in small dyadic numbers: every product and sum of the build is exact, so with the factor (x - 1)
    unflipped the DC sum is exactly 0 and the DC rule divides by it."""
    flips = np.array([[0, 0], [1, 0], [0, 1], [1, 1]])
    assert np.all(fr.build(ZERO_DC, flips[[0, 2]])[2] == 0) and np.all(fr.build(ZERO_DC, flips[[1, 3]])[2] > 0.05)
    r = run(ZERO_DC, dict(masks=flips.T.copy()), [0, 1, 2, 3], criterion=criterion)
    assert r["status"] == 0 and r["winner"] in (1, 3)
    assert np.all(np.isinf(r["peaks"][[0, 2]])) and np.all(np.isfinite(r["peaks"][[1, 3]]))
    assert np.all(np.isinf(r["st_peak"][[0, 2]])) and same_bits(r["st_peak"][[1, 3]], r["peaks"][[1, 3]])
    check_search(r)
    if criterion == "rf":
        good = {k: r[k][[1, 3]] for k in BLOCKS}
        fr_case = dict(ZERO_DC)
        fracs, _ = fr.stage_fractions(good, fr_case, flips[[1, 3]])
        assert max(fracs.values()) <= 1.0, fracs


def test_no_finite_candidate_is_a_numerical_status():
    ctx = mbfir.get_context()
    flips = np.array([[0, 0], [0, 1], [0, 0]])
    r = run(ZERO_DC, dict(masks=flips.T.copy()), [0, 1])
    assert r["status"] == mbfir.NUMERICAL and r["winner"] == -1 and np.all(np.isinf(r["peaks"])) and np.all(r["blk_i"] == -1)
    assert "no candidate has a finite peak" in ctx.last_error()
    with pytest.raises(mbfir.MbfirError, match="no candidate has a finite peak"):
        mbfir.flip_search(ZERO_DC["c0"], ZERO_DC["z"], ZERO_DC["zf"], masks=flips.T, target=ZERO_DC["target"], criterion="rf")
    case, fl, kw, sel = fr.stage_case("n8_nz3")                          # the context goes on working
    again = run(case, kw, sel)
    assert again["status"] == 0
    check_stages(again, case, fl[sel], "after the numerical status")
    f = [-0.6, -0.35, -0.1, 0.15, 0.45, 0.8]
    h, status = mbfir.fir_ap_cvx(33, f, [0, 0, 0.7, 0.7, 0, 0], [0.01, 0.02, 0.01], 0.1, 1e-2, ctx=ctx)
    assert status == "Solved"


def test_refusals(lds_limit):
    n = fr.mode_sizes(lds_limit)["first1"]
    case, flips = fr.size_case(n)
    kw = dict(masks=flips.T.copy())
    with pytest.raises(ValueError, match="forced mode 0 needs"):
        run(case, kw, [0], force_mode=0)
    n2 = fr.mode_sizes(lds_limit)["first2"]
    case2, flips2 = fr.size_case(n2)
    with pytest.raises(ValueError, match="forced mode 1 needs"):
        run(case2, dict(masks=flips2.T.copy()), [0], force_mode=1)
    small, fl, skw, sel = fr.stage_case("n8_nz3")
    with pytest.raises(ValueError, match="nsel"):
        run(small, skw, np.zeros(1025, dtype=int))
    with pytest.raises(ValueError, match=r"sel\[1\]"):
        run(small, skw, [0, 8])
    with pytest.raises(ValueError, match=r"sel\[0\]"):
        run(small, skw, [-1])
    with pytest.raises(ValueError, match="force_mode"):
        run(small, skw, [0], force_mode=3)
    ok = run(small, skw, sel)                                            # and a refused call leaves the context usable
    check_stages(ok, small, fl[sel], "after the refusals")


# ---- the same reference on slr.hip's calls (no hook: end to end from the caller's beta, flip_ref.slr_chain) ------------------------
# 31 .. 33: N = 8n crosses k_dft_any's 256-term tile; 128 / 129: N = 1024, the width of k_slr_logmag; the k_b2rf_batch tiers hold
# n <= 128, <= 512, <= 1024 and <= 2048 (with_b2rf_tier), so 2 / 128, 129 / 512, 513 / 1024 and 1025 / 2048 are their ends
SLR_CASES = [(n, 0.9) for n in (2, 3, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1024, 1025, 2048)] + [(64, 1.7)]


@pytest.mark.parametrize("n,level", SLR_CASES)
def test_slr_calls_against_the_reference(n, level):
    b = fr.slr_input(n, level, 300 + n)
    br = fr.slr_input(n, level, 700 + n, real=True)
    assert np.all(br.imag == 0) and np.any(b.imag != 0)
    ch, chr_ = fr.slr_chain(b), fr.slr_chain(br)
    for c in (ch, chr_):
        assert ((c["maxB"] <= fr.CLIP_LOW) | (c["maxB"] >= fr.CLIP_HIGH)).all() and c["pivot"].min() >= fr.PIVOT_MIN
        assert (c["maxB"] >= 1).all() == (level > 1)
    err = lambda got, ref, bound: float(np.max(np.abs(np.asarray(got).astype(fr.CLD) - ref).astype(np.float64) / bound))   # noqa: E731
    a = mbfir.b2a(b)
    rf = mbfir.b2rf(b)
    lrf, lbound, _ = fr.ref_theta(a, b, want_rf=True)                    # ab2rf alone: the device's own a taken as exact
    fa, frf, fab = err(a, ch["a"][0], ch["d_a"][0]), err(rf, ch["rf"][0], ch["d_rf"][0]), err(mbfir.ab2rf(a, b), lrf[0], lbound[0])
    batch = mbfir.b2rf_batch(np.stack([b, br, b]))
    fb, fbr = err(batch[0], ch["rf"][0], ch["d_rf"][0]), err(batch[1], chr_["rf"][0], chr_["d_rf"][0])
    print("slr fractions n=%d level=%g: b2a %.3f b2rf %.3f ab2rf %.3f batch %.3f batch(real) %.3f" % (n, level, fa, frf, fab, fb, fbr))
    assert max(fa, frf, fab, fb, fbr) <= 1.0
    assert same_bits(batch[0], batch[2])                                 # a row's bits do not depend on its place in the batch
    assert np.all(batch[1].imag == 0) or np.max(np.abs(batch[1].imag)) <= chr_["d_rf"].max()
