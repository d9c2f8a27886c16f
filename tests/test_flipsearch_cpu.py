"""Root-flip search, host side (no GPU): minpeakrf's flip-matrix translation, the npoly normalisation, argument limits,
the C ABI binding, and the default fir_flip_zero staying on the host."""
import os
import re

import numpy as np
import pytest

import mbfir
from mbfir.flipzero import _poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorded(Exception):
    pass


def record_flip_search(monkeypatch):
    """Replace the device search by a recorder: the calls minpeakrf makes, without a GPU."""
    calls = []

    def fake(c0, z, zf, **kw):
        calls.append(dict(c0=np.asarray(c0), z=np.asarray(z), zf=np.asarray(zf), **kw))
        nc = kw.get("ncand") or 1
        pk = np.full(nc, 1.0)
        return np.zeros(len(c0) + len(np.atleast_1d(z))), 0, pk
    monkeypatch.setattr(mbfir, "flip_search", fake)
    return calls


def test_minpeakrf_translates_singles_and_pairs(monkeypatch):
    calls = record_flip_search(monkeypatch)
    z = np.array([0.5 + 0.2j, 2.0 - 0.5j, 0.3j, 1.5 + 0j, 0.8 - 0.1j, -0.4 + 0j])
    # rows: single root 2, pair (4, 3) on opposite sides of the circle, single root 6, pair (1, 5) on the same side
    flip = np.array([[2, 0], [4, 3], [6, 0], [1, 5]])
    zmin = mbfir.minpeakrf(z, flip, 0.9)
    z0_call, search = calls
    # the unflipped start (z0: the opposite-side pair has its first root, index 4, flipped) is scored on its own
    z0 = z.copy()
    z0[3] = z[3] / abs(z[3]) ** 2
    assert np.allclose(z0_call["c0"], _poly(z0)) and len(z0_call["z"]) == 0 and z0_call["bsf"] == 0.9
    # singles take the low bits (units 0, 1), pairs the next (units 2, 3); a pair's first root flips on bit 1, its second on bit 0
    assert search["enum_bits"] == [(0 << 1) | 1, (1 << 1) | 1, (2 << 1) | 1, (2 << 1) | 0, (3 << 1) | 1, (3 << 1) | 0]
    assert search["ncand"] == 16 and search["tie_high"] and search["criterion"] == "rf"
    assert np.allclose(search["z"], z0[[1, 5, 3, 2, 0, 4]])
    assert np.allclose(search["zf"], 1 / np.conj(z0[[1, 5, 3, 2, 0, 4]]))
    assert np.allclose(search["c0"], [1.0])                      # every root flips
    # winner 0 with equal peaks: no single flipped, every pair's second root flipped
    want = z0.copy()
    for r in (2, 4):
        want[r] = 1 / np.conj(z0[r])
    assert np.allclose(zmin, want)


def test_minpeakrf_keeps_the_start_when_no_candidate_is_lower(monkeypatch):
    """The running minimum starts at z0's peak with index 0: a set whose every peak is higher returns candidate 0."""
    def fake(c0, z, zf, **kw):
        nc = kw.get("ncand") or 1
        return np.zeros(1), nc - 1, np.full(nc, 0.5 if nc == 1 else 0.7)
    monkeypatch.setattr(mbfir, "flip_search", fake)
    z = np.array([0.5 + 0j, 0.4j])
    assert np.allclose(mbfir.minpeakrf(z, [[1, 0], [2, 0]], 0.5), z)      # index 0 flips nothing


@pytest.mark.parametrize("flip,bsf", [([[0, 0]], 0.5), ([[4, 0]], 0.5), ([[1.5, 0]], 0.5), ([[1, 0], [1, 0]], 0.5),
                                      ([[1, 0]], 1.5), ([[1, 0]], -0.1), ([1, 2, 3], 0.5)])
def test_minpeakrf_argument_errors(flip, bsf):
    with pytest.raises(ValueError):
        mbfir.minpeakrf(np.array([0.5, 0.3j, 2.0]), flip, bsf)


def test_minpeakrf_rejects_more_than_1023_roots():
    with pytest.raises(ValueError):
        mbfir.minpeakrf(np.full(1024, 0.5), [[1, 0]], 0.5)


def test_npoly_normalisation_matches_the_host_rule():
    """npoly.code.c: max|FFT_nn(b)| = 1 on the next power of two nn >= n, either transform sign."""
    rng = np.random.default_rng(3)
    for n in (7, 16, 33):
        b = _poly(rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1))
        nn = 1 << int(np.ceil(np.log2(n)))
        m = np.abs(np.fft.fft(b, nn)).max()
        assert np.isclose(np.abs(np.fft.ifft(b, nn) * nn).max(), m, rtol=1e-13)   # four1's +i convention gives the same max
        assert np.isclose(np.abs(np.fft.fft(b / m, nn)).max(), 1.0, rtol=1e-14)


def test_all_candidates_above_24_zeros_raise():
    z = 0.5 * np.exp(2j * np.pi * np.arange(26) / 26)
    h = np.poly(z)
    with pytest.raises(ValueError, match="24"):
        mbfir.fir_flip_zero(h, candidates="all")


def test_pack_masks_bit_order():
    m = np.zeros((40, 3), dtype=int)
    m[0, 0] = m[31, 1] = m[32, 2] = m[39, 2] = 1
    w = mbfir._pack_masks(m)
    assert w.shape == (3, 2) and w.dtype == np.uint32
    assert w.tolist() == [[1, 0], [1 << 31, 0], [0, 1 | (1 << 7)]]


def test_flip_search_symbol_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bint\s+mbfir_flip_search\s*\(", hdr)
    assert "mbfir_flip_search" in mbfir.SYMBOLS
    res, args = mbfir.SYMBOLS["mbfir_flip_search"]
    assert len(args) == 22


def test_default_flip_zero_never_touches_the_library(monkeypatch):
    def boom():
        raise AssertionError("the default fir_flip_zero must stay on the host")
    monkeypatch.setattr(mbfir, "load_library", boom)
    monkeypatch.setattr(mbfir, "get_context", boom)
    rng = np.random.default_rng(0)
    zi = 0.7 * np.exp(1j * rng.uniform(-0.6, 0.6, 6))
    zo = np.exp(1j * rng.uniform(1.0, 2 * np.pi - 1.0, 12))
    h = np.poly(np.concatenate([zi, zo])) * 0.01
    hn, info = mbfir.fir_flip_zero(h, seed=1, return_info=True)
    assert info["candidates"] == 64 and "rf_peak_after" not in info
    with pytest.raises(ValueError):
        mbfir.fir_flip_zero(h, criterion="rf", device=False)
