"""The one-pass H-build runs its border operands only over the moment points k_assemble_H_lat reads (m < D1): the blocks of the
moment kernels whose 256 points all lie past D1 leave them out.  H as a unit has it in front of the factorisation
(mbfir_test_unit_ops, the hook of tests/test_latticeops_gpu.py) must be what MBFIR_FUSE=0 -- every block on every operand -- gives,
bit for bit, padding included: as one design (the unpaired kernel), as a unit of 2 (one pair) and of 3 lanes (a pair and a lone lane),
for fir_ap_cvx at
    n = 24                 D1 = 24, 71 points: one block, which straddles D1 -- nothing is trimmed
    n = 260                D1 = 260, 779 points: block 0 full-length, block 1 straddles, blocks 2 and 3 trimmed
    n = 512, grid 1024     D1 = 512, 1535 points: D1 on a block edge -- blocks 0 and 1 full-length, blocks 2 .. 5 trimmed, none straddles
and for a program that does not take the one-pass branch (fir_qp_cvx, n = 25), which the change must not touch."""
import numpy as np
import pytest

import lattice_ref as lr
import mbfir

pytestmark = pytest.mark.gpu
SWITCHES = ("MBFIR_LANEPAIR", "MBFIR_FUSE", "MBFIR_CGRP", "MBFIR_FOLD")
AP = {24: 512, 260: 1024, 512: 1024}          # n -> grid_m
_P, _H = {}, {}


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def case(key):
    if key == "qp25":
        c = lr.unit_cases()["c6_qp25"]
        return c["job"], c["grid_m"], c.get("ddkkt", 0)
    return lr._c13(key), AP[key], 0


def prog(key):
    if key not in _P:
        job, grid_m, _ = case(key)
        _P[key] = lr.program(job[0], job[1], grid_m)
    return _P[key]


def build(key, nl):
    """H of a unit of nl lanes of design `key` (lane b at its own iterate: lane 1 with orthant weights spread over 1e8) and the report"""
    job, grid_m, ddkkt = case(key)
    P = prog(key)
    N, R = P["N"], P["R"]
    sz = [lr.draw_sz(P, np.random.default_rng([7, b]), wide=(b == 1)) for b in range(nl)]
    rng = np.random.default_rng(11)
    v, u = rng.standard_normal((nl, 1, N)), rng.standard_normal((nl, 1, R))
    out = mbfir.test_unit_ops([job] * nl, v, u, np.stack([a for a, _ in sz]), np.stack([b for _, b in sz]),
                              opts=mbfir.make_opts(grid_m=grid_m, ddkkt=ddkkt))
    return out[3], out[4]


def default(key, nl):
    if (key, nl) not in _H:
        _H[(key, nl)] = build(key, nl)
    return _H[(key, nl)]


@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("n", sorted(AP))
def test_h_is_the_untrimmed_bit_for_bit(n, nl, monkeypatch):
    H, rep = default(n, nl)
    assert rep["one_pass"] == 1 and rep["lattice"] == 1 and rep["D1"] == n and rep["tmin"] == 0.0 and rep["lanes"] == nl
    assert (rep["pair_passes"] > 0) == (nl > 1)
    monkeypatch.setenv("MBFIR_FUSE", "0")
    H0, rep0 = build(n, nl)
    assert rep0["one_pass"] == 1 and (rep0["pair_passes"] > 0) == (nl > 1)
    assert not np.any(np.isnan(np.tril(H0))) and np.array_equal(H, H0, equal_nan=True)
    # a lane of the unit is its single design (lanes 0 and 1 draw their own iterates; lane 0's is the single design's)
    if nl > 1:
        assert np.array_equal(H[0], default(n, 1)[0][0], equal_nan=True)


def test_blocks_at_the_sizes():
    """what the three sizes are there for: the blocks of 256 moment points against D1"""
    for n, (full, straddle, trimmed) in {24: (0, 1, 0), 260: (1, 1, 2), 512: (2, 0, 4)}.items():
        D1 = n
        blocks = -(-(3 * D1 - 1) // 256)
        lo = [b * 256 for b in range(blocks)]
        assert (sum(1 for s in lo if s + 256 <= D1), sum(1 for s in lo if s < D1 < s + 256), sum(1 for s in lo if s >= D1)) == (full, straddle, trimmed)


@pytest.mark.parametrize("nl", [1, 2])
def test_two_pass_program_is_untouched(nl, monkeypatch):
    H, rep = default("qp25", nl)
    assert rep["one_pass"] == 0 and rep["lattice"] == 1
    monkeypatch.setenv("MBFIR_FUSE", "0")
    H0, rep0 = build("qp25", nl)
    assert rep0["one_pass"] == 0 and np.array_equal(H, H0, equal_nan=True)
