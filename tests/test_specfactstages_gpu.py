"""The tap extraction (csrc/specfact.hip: k_specfact of fir_ap_cvx, k_fmp of dzrf's minimum-phase pulses) stage by stage through
mbfir.test_specfact_stages against tests/specfact_ref.py: the long-double reference of every stage, each taken from the device's own
output of the stage before and held to the bound counted for that stage alone (specfact_ref's docstring;
tests/test_specfactstages_cpu.py shows the reference rejects planted errors).  Also here: the lane-strided launch of a lock-step
unit (3 lanes, the bench's 16, a stride larger than the blocks need), every lane against its own reference and bit for bit against
its single-lane run; the taps bit for bit against mbfir.test_specfact / mbfir.fmp (the production instantiations); the exact zero
of r = [-1, 2, -1]; sentinels behind every device block; and, end to end, the taps against the long-double chain from the input
within 2 spread + the carried-forward bounds of stages 2 .. 5.

Measured on an MI355X, worst |device - reference| / bound per stage over every case and lane of this file (each must be <= 1; the
larger of the entry-wise and the norm ratio):
    hpf 0.035   lift 0.765   xl 0.596   xlfp 0.037   a 0.050   h 0.036
Every stage is within its counted bound on every input, the zero-touching ones included.  The transforms sit where independent
roundings put them against a worst-case norm bound (1 / (eta sqrt L), 0.01 .. 0.04); xl spends half of its bound (the budgets of
hypot, sqrt and log), lift is a single rounding.  The float64 twin of the CPU test gives figures of the same size.

Device, NumPy (oracle/specfact.py) and the long-double chain end to end on the zero-touching family (C), max |h - h_longdouble| /
max|h|, with the smallest |real hpf| put at t max|hpf| (`spread` is the long-double chain's own movement under the stage-1 bound):
    t        device (five inputs)      NumPy                     spread
    1e-6     3.0e-14 .. 1.1e-13        3.7e-14 .. 1.2e-13        2.4e-11 .. 2.5e-10
    1e-9     1.3e-12 .. 8.6e-12        3.6e-13 .. 3.0e-11        2.0e-9  .. 1.6e-8
    1e-12    7.3e-11 .. 9.2e-9         8.9e-11 .. 1.8e-8         1.8e-6  .. 8.3e-6
    1e-15    1.6e-8  .. 3.1e-5         7.0e-8  .. 3.1e-5         4.9e-6  .. 1.6e-3
    0        5.4e-6  .. 9.9e-4         1.6e-5  .. 9.9e-4         2.8e-5  .. 4.6e-3
Unshifted (B): 6.5e-13 .. 8.2e-10, except make_case seed 2324 (its natural trough is 6.6e-15 max|hpf|): device 3.04e-6, NumPy
3.04e-6, spread 6.8e-4.  Device and NumPy are equally far from long double at every depth; the distance is the input's
conditioning (it grows as 1 / t and stays below the spread), not a stage's error.  The long-double taps' autocorrelation misses r by
1.5e-4 .. 1.5e-3 of r[0] on (B) and (C): the spectrum goes negative (to -2e-4 max) and the chain factors |hpf|, not hpf.
"""
import numpy as np
import pytest

import mbfir
import specfact_ref as sr
from oracle import specfact

pytestmark = pytest.mark.gpu
SENT = -7.25
GUARD = 5
CASES = sr.cases()
BLOCKS = ("st_hpf", "st_xl", "st_xlfp", "st_a", "st_h", "lift")


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def run(kind, inp, n, extra=0):
    r = mbfir.test_specfact_stages(inp, n if kind == 0 else None, kind=kind, guard=GUARD, fill=SENT, extra=extra)
    raw, off, size = r["raw"], r["offsets"], r["sizes"]
    outside = np.ones(raw.shape[1], dtype=bool)
    for k in off:
        outside[off[k]:off[k] + size[k]] = False
        assert np.all(raw[:, off[k] + size[k]:off[k] + size[k] + GUARD] == SENT), k      # nothing written past the block
    assert outside.sum() >= 8 * GUARD + extra and np.all(raw[:, outside] == SENT)         # nor into the gap between two lanes
    src = np.atleast_2d(np.asarray(inp))                                                 # and the input is as it was given
    if kind == 1:
        src = np.stack([src.real, src.imag], axis=-1).reshape(1, -1)
    assert same_bits(raw[:, off["in"]:off["in"] + size["in"]], src.astype(np.float64))
    assert r["lp"] == sr.lp_of(sr.taps_of(kind, n)[0])
    return r


def check_stages(r, kind, inp, n, label, stages=None):
    fracs, exact = sr.stage_fractions(r, kind, inp, n, stages)
    print("fractions", label, {k: "%.3f" % np.max(v) for k, v in fracs.items()})
    if stages is None:
        assert set(fracs) == set(sr.STAGES) | ({"lift"} if kind == 1 else set())
    assert all(exact.values()), (label, exact)
    for k, v in fracs.items():
        assert np.all(v <= 1.0), (label, k, v)                                           # every lane, every stage
    return fracs


def check_taps(r, name, lane=0):
    """End to end: the device's taps against the long-double chain from the input."""
    sp, ch = sr.reference(name)
    err = np.abs(r["st_h"][lane].astype(sr.CLD) - ch["h"][0]).astype(np.float64)
    hmax = float(np.abs(ch["h"]).max())
    print("taps", name, "device-vs-longdouble %.3g  spread %.3g  carried %.3g  (of max|h|)" % (
        err.max() / hmax, sp[0] / hmax, float(ch["h_bound"].max()) / hmax))
    assert np.all(err <= 2 * sp[0] + ch["h_bound"][0]), (name, err.max() / hmax, sp[0] / hmax)
    if sr.strict(name):
        assert sp[0] <= sr.STRICT * hmax
    return err.max() / hmax, ch


@pytest.mark.parametrize("name", sorted(k for k in CASES if k != "D_zero"))
def test_stages_against_the_reference(name):
    kind, inp, n = CASES[name]
    r = run(kind, inp, n)
    check_stages(r, kind, inp, n, name)
    prod = mbfir.test_specfact(inp, n) if kind == 0 else mbfir.fmp(inp)                  # the instantiation production launches
    assert same_bits(r["st_h"][0], np.asarray(prod, dtype=np.complex128))
    dev, ch = check_taps(r, name)
    if sr.family(name) in "BC":                                                          # for the write-up; nothing asserted on it
        with np.errstate(all="ignore"):
            ho = specfact.fmp2(specfact.x_to_r(inp, n))
        h = ch["h"][0]
        hmax = float(np.abs(h).max())
        rr = np.correlate(h, h, mode="full")[n - 1:]
        rx = sr.place(0, inp, n)[0][:n]
        print("compare", name, "device %.3g  numpy %.3g  of max|h| from long double; long double's autocorrelation residual %.3g of r[0]" % (
            dev, float(np.abs(ho.astype(sr.CLD) - h).max()) / hmax, float(np.abs(rr - rx).max() / np.abs(rx[0]))))


def lanes_against_single(kind, xs, n, names, label, extra=0):
    r = run(kind, xs, n, extra=extra)
    check_stages(r, kind, xs, n, label)
    for q in range(len(xs)):
        one = run(kind, xs[q], n)
        for k in BLOCKS:
            assert same_bits(r[k][q], one[k][0]), (label, q, k)
        if names[q]:
            check_taps(r, names[q], lane=q)
    return r


def test_three_lanes_of_n33():
    xs = np.stack([sr.autocorr_x(33), sr.autocorr_x(33, seed=1033), CASES["A_n33_tiny"][1]])
    lanes_against_single(0, xs, 33, ["A_n33", None, "A_n33_tiny"], "3 x n33")


def test_sixteen_lanes_of_the_headline_order():
    """The bench's unit: 16 designs of n = 512 in one launch -- the headline solution, its five zero-touching variants, ten random."""
    names = ["B_headline"] + ["C_headline_%g" % t for t in sr.T_LEVELS] + [None] * 10
    xs = np.stack([CASES[k][1] for k in names[:6]] + [sr.autocorr_x(512, seed=5000 + q) for q in range(9)] + [CASES["A_n512"][1]])
    names[15] = "A_n512"
    lanes_against_single(0, xs, 512, names, "16 x n512")


def test_a_lane_stride_larger_than_the_blocks():
    xs = np.stack([CASES["A_n17"][1], sr.autocorr_x(17, seed=1017)])
    r = lanes_against_single(0, xs, 17, ["A_n17", None], "2 x n17, stride + 1001", extra=1001)
    tight = run(0, xs, 17)
    assert r["raw"].shape[1] == tight["raw"].shape[1] + 1002                              # (rounded up to 16 bytes)


def test_an_exact_zero_of_the_spectrum():
    """(D): r = [-1, 2, -1] between two ordinary lanes.  Its sample at k = 0 is an exact zero (every twiddle there is exactly 1), the
    logarithm is -inf, every tap of that lane comes back non-finite as the oracle's do, nothing is written past a block (run), and
    the lanes around it are what they are on their own."""
    xs = np.stack([CASES["A_n2"][1], sr.ZERO_X, sr.autocorr_x(2, seed=1002)])
    r = run(0, xs, 2)
    assert r["st_hpf"][1, 0] == 0 and r["st_xl"][1, r["lp"] // 2] == -np.inf
    assert not np.isfinite(r["st_h"][1]).any()
    with np.errstate(all="ignore"):
        assert not np.isfinite(specfact.fmp2(specfact.x_to_r(sr.ZERO_X, 2))).any()
    check_stages(r, 0, xs, 2, "D_zero: hpf, xl", stages=("hpf", "xl"))
    assert not np.isfinite(mbfir.test_specfact(sr.ZERO_X, 2)).any()
    for q in (0, 2):
        one = run(0, xs[q], 2)
        check_stages(one, 0, xs[q], 2, "D_zero: lane %d alone" % q)
        for k in BLOCKS:
            assert same_bits(r[k][q], one[k][0]), (q, k)
    alone = run(0, sr.ZERO_X, 2)
    for k in BLOCKS:
        assert same_bits(r[k][1], alone[k][0]), k


def test_refusals():
    x = CASES["A_n2"][1]
    for kw, inp, n in ((dict(kind=0), np.zeros((1, 2 * 4097 - 1)), 4097), (dict(kind=1), np.zeros(4), None),
                       (dict(kind=1), np.zeros(2049), None), (dict(kind=0), np.zeros((65, 3)), 2), (dict(kind=2), x, 2),
                       (dict(kind=0, guard=-1), x, 2), (dict(kind=0, extra=-1), x, 2)):
        with pytest.raises(ValueError, match="mbfir_test_specfact_stages"):
            mbfir.test_specfact_stages(inp, n, **kw)
    check_stages(run(0, x, 2), 0, x, 2, "after the refusals")                             # a refused call leaves the context usable
