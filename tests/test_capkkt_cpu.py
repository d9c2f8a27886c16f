"""tests/capkkt_ref.py can fail: its stage checks pass the float64 NumPy restatement of the capacitance-form solve at the shapes
tests/test_capkkt_gpu.py runs, and reject each of the defects a matrix-core kernel of this kind can have -- a dropped k-slice, a
dropped split part, an unmasked diagonal tile, a padding row that is not quite unit or zero -- at the stage where it was planted.
Also here: the conditions the input family must meet for the end-to-end reference (oracle/ddlin.c) to mean anything."""
import numpy as np
import pytest

import capkkt_ref as ref

# (n, k) of tests/test_capkkt_gpu.py, without (1030, 70): the long-double products of that size belong to the device test alone
SHAPES = [(64, 1), (60, 3), (100, 7), (191, 65), (320, 129), (449, 64)]
# n < np and k < kp: every mutation below has a padding row / entry to work on; one tile and several
MUTATION_SHAPES = [(60, 3), (191, 65)]


def _kp(k):
    return ref.pad64(k)


@pytest.fixture(scope="module")
def problems():
    return {(n, k): ref.family(n, k, 2, "scaled") for n, k in SHAPES}


@pytest.mark.parametrize("n,k", SHAPES)
def test_the_restatement_passes_every_stage(problems, n, k):
    p = problems[n, k]
    rep = ref.stage_checks(p, _kp(k), ref.restate(p, _kp(k)))
    print({s: "%.3g" % f for s, f in rep.fractions.items()})
    assert not rep.failures, rep.failures
    assert set(rep.fractions) == set(ref.STAGES)


def test_the_restatement_passes_when_padded_further(problems):
    p = problems[191, 65]
    assert not ref.stage_checks(p, 512, ref.restate(p, 512)).failures


def _run(p, mutate):
    kp = _kp(p["k"])
    return ref.stage_checks(p, kp, ref.restate(p, kp, mutate))


def _at(stage, change):
    def mutate(name, out, inputs):
        if name == stage:
            change(out, inputs)
    return mutate


@pytest.mark.parametrize("n,k", MUTATION_SHAPES)
def test_a_dropped_k_slice_of_one_entry_of_Yt_fails_Yt(problems, n, k):
    """Yt[r][i] = sum_j U[r][j] M[i][j]: one MFMA step (4 consecutive j) left out of a single entry."""
    p = problems[n, k]
    r, i = k - 1, n - 3

    def change(out, inputs):
        U, M = inputs[1], np.tril(out["M"])
        j0 = 4 * ((i // 2) // 4)
        out["Yt"][r, i] -= U[r, j0:j0 + 4] @ M[i, j0:j0 + 4]
    rep = _run(p, _at("Yt", change))
    assert rep.failed_stages() == ["Yt"], rep.failures


@pytest.mark.parametrize("n,k", MUTATION_SHAPES)
def test_a_dropped_split_part_of_one_tile_of_Zt_fails_Zt(problems, n, k):
    """Zt = Yt M, tile (rb, cb) sums the tiles jb = cb .. nblk-1 of K in four contiguous parts: the last part (never empty) lost."""
    p = problems[n, k]

    def change(out, inputs):
        M, nblk = np.tril(out["M"]), len(out["M"]) // 64
        rb, cb, z = 0, 0, 3
        span = nblk - cb
        lo, hi = cb + span * z // 4, cb + span * (z + 1) // 4
        assert hi > lo
        rows, cols, ks = slice(64 * rb, 64 * rb + 64), slice(64 * cb, 64 * cb + 64), slice(64 * lo, 64 * hi)
        out["Zt"][rows, cols] -= out["Yt"][rows, ks] @ M[ks, cols]
    rep = _run(p, _at("Zt", change))
    assert rep.failed_stages() == ["Zt"], rep.failures


@pytest.mark.parametrize("n,k", MUTATION_SHAPES)
def test_an_unmasked_diagonal_tile_of_M_fails_Yt(problems, n, k):
    """A nonzero above the diagonal inside a diagonal tile of M, and a product that reads the tile as it is stored.  (The nonzero
    itself fails "M" too: the one-pass M'(M b) relies on exact zeros there.)  The control -- the same M, the product masked --
    fails "M" alone: the reference of Yt reads the lower triangle."""
    p = problems[n, k]
    i, j = n - 9, n - 2                                           # the same diagonal tile, j > i

    def dirty(out, inputs):
        assert i // 64 == j // 64
        out["M"][i, j] = 0.37

    def unmasked(name, out, inputs):
        _at("M", dirty)(name, out, inputs)
        if name == "Yt":
            out["Yt"] = inputs[1] @ out["M"].T
    rep = _run(p, unmasked)
    assert rep.failed_stages() == ["M", "Yt"], rep.failures
    assert _run(p, _at("M", dirty)).failed_stages() == ["M"]


@pytest.mark.parametrize("n,k", MUTATION_SHAPES)
def test_a_padding_row_of_S_with_a_diagonal_of_one_plus_1e_12_fails_S(problems, n, k):
    p = problems[n, k]

    def change(out, inputs):
        out["S"][k, k] = 1.0 + 1e-12
    rep = _run(p, _at("S", change))
    assert rep.failed_stages() == ["S"], rep.failures

    def offdiag(out, inputs):
        out["S"][k + 1, 0] = 1e-300
    assert _run(p, _at("S", offdiag)).failed_stages() == ["S"]


@pytest.mark.parametrize("n,k", MUTATION_SHAPES)
def test_a_nonzero_padding_entry_of_w_fails_w(problems, n, k):
    p = problems[n, k]

    def change(out, inputs):
        out["w"][1, k] = 1e-300
    rep = _run(p, _at("w", change))
    assert rep.failed_stages() == ["w"], rep.failures


@pytest.mark.parametrize("n,k", MUTATION_SHAPES)
def test_a_nonzero_padding_entry_of_dx_fails_dx(problems, n, k):
    p = problems[n, k]

    def change(out, inputs):
        out["dx"][0, n] = 1e-300
    rep = _run(p, _at("dx", change))
    assert rep.failed_stages() == ["dx"], rep.failures


def test_a_nan_in_a_lower_triangle_or_a_vector_fails_its_stage(problems):
    p = problems[100, 7]

    def nan_in(stage, idx):
        def change(out, inputs):
            out[stage][idx] = np.nan
        return _run(p, _at(stage, change)).failed_stages()
    assert nan_in("Ms", (5, 2))[0] == "Ms"
    assert nan_in("zeta", (0, 3))[0] == "zeta"
    assert nan_in("Zt", (2, 70))[0] == "Zt"


@pytest.mark.parametrize("n,k", SHAPES + [(700, 300)])
@pytest.mark.parametrize("t_mode", ["zero", "scaled"])
def test_the_input_family_suits_the_end_to_end_reference(n, k, t_mode):
    """What the reference alone must meet: the restatement's S is positive definite with cond(S) <= 1e6, and the restatement is
    within 1e-12 of the double-double solution (so that 16 x its error is a tolerance worth the name)."""
    p = ref.family(n, k, 2, t_mode)
    rs, _ = ref.restate_solve(p)
    err_self, err_restate, cond_s, spd = ref.end_to_end(p, rs)
    print("n %d k %d t %s: restatement %.3g of the dd solution, cond(S) %.3g" % (n, k, t_mode, err_restate, cond_s))
    assert spd and cond_s <= ref.COND_S_MAX
    assert err_self == err_restate <= ref.RESTATE_TOL
