"""Host side of the spiral 2D pulses and of the batched 2D simulation (no GPU): mbfir.dz2d / csg against tests/golden/spiral.json,
their properties, the k-space helpers, and the argument errors that dz2d, csg and mbfir.abr2_batch raise before any device work."""
import json
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Relative to the largest entry of each array.  Two independent fp64 restatements (mbfir.spiral: np.interp, jv; the generator: the
# interpolation written out on the bracketing knots, j1) differ on these five fixtures by at most 4.6e-15 in k, 4.7e-15 in rf,
# 4.9e-14 in g (differences of k: the rounding of k over a step of k) and 2.4e-16 in the duration.  The
# bounds are ten times the worst array figure, and forty times the duration's.
TOL = 5e-13
TOL_DURATION = 1e-14


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "spiral.json")) as fh:
        raw = json.load(fh)
    out = {}
    for name, d in raw.items():
        out[name] = dict(args=tuple(d["args"]), dur=d["duration_ms"], k=np.array(d["k_re"]) + 1j * np.array(d["k_im"]),
                         rf=np.array(d["rf"]), g=np.array(d["g_re"]) + 1j * np.array(d["g_im"]))
    return out


def _linear_spiral(nt, bw, ns):
    t = np.arange(1, int(ns) + 1) / int(ns)
    return t * np.exp(1j * 2 * np.pi * t * nt) * bw / 2


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_dz2d_and_csg_match_the_golden_file(golden):
    assert len(golden) == 5
    for name, d in golden.items():
        nt, bw, tbp, ns, mxg, mxs = d["args"]
        rf, g, dur = mbfir.dz2d(*d["args"])
        k, kdur = mbfir.csg(_linear_spiral(nt, bw, ns), mxg, mxs)
        assert rf.shape == d["rf"].shape == (ns,) and g.shape == (ns,) and np.isrealobj(rf) and np.iscomplexobj(g)
        errs = (_rel(k, d["k"]), _rel(rf, d["rf"]), _rel(g, d["g"]), abs(dur - d["dur"]) / d["dur"])
        print("%s: rel err k %.2e, rf %.2e, g %.2e, duration %.2e" % ((name,) + errs))
        assert max(errs[:3]) <= TOL and errs[3] <= TOL_DURATION, (name, errs)
        assert kdur == dur


def test_dz2d_properties(golden):
    for name, d in golden.items():
        nt, bw, tbp, ns, mxg, mxs = d["args"]
        rf, g, dur = mbfir.dz2d(*d["args"])
        k, _ = mbfir.csg(_linear_spiral(nt, bw, ns), mxg, mxs)
        assert np.all(np.isfinite(rf)) and np.all(np.isfinite(g)), name
        assert abs(rf.sum() - 1.0) <= 4 * np.finfo(float).eps * np.abs(rf).sum(), name
        # cumsum(g) over the reversed pulse walks the trajectory outwards again; ns additions of at most bw / 2 each
        assert np.abs(np.cumsum(g[::-1]) / (2 * np.pi) - k).max() <= ns * np.finfo(float).eps * bw / 2, name
        assert abs(abs(k[-1]) - bw / 2) <= 4 * np.finfo(float).eps * bw, name


def test_the_reference_example_is_an_eight_ms_spiral_without_nan(golden):
    rf, g, dur = mbfir.dz2d(8, 1, 4, 512, 1, 2)
    assert 8.0 <= dur <= 8.5                                        # dz2d.m:18 "an 8 ms 8 turn spiral"; 8.2049 ms
    assert abs(dur - golden["example_8turn_512"]["dur"]) <= TOL_DURATION * dur
    assert not np.isnan(rf).any() and not np.isnan(g).any()


def test_csg_interp_rule_at_the_first_knot():
    # stage 2's first query equals its first knot to rounding when the amplitude limit is not active: no NaN (the rule of csg)
    k, dur = mbfir.csg(_linear_spiral(8, 1.0, 512), 1.0, 2.0)
    assert np.isfinite(k[0])
    # a trajectory that starts with more than its mean slew step: stage 1's first query lies below the first knot, NaN as interp1
    kk = _linear_spiral(4, 1.0, 64)[::-1].copy()
    out, _ = mbfir.csg(kk, 1.0, 2.0)
    assert np.isnan(out[0])


def test_dz2d_batch_equals_single_calls_bit_for_bit(golden):
    specs = [d["args"] for d in golden.values()]
    specs.append(dict(nt=3, bw=2.0, tbp=4.0, ns=100, mxg=2.0, mxs=10.0))
    res = mbfir.dz2d_batch(specs)
    assert len(res) == len(specs)
    for s, (rf, g, dur) in zip(specs, res):
        rf1, g1, dur1 = mbfir.dz2d(**s) if isinstance(s, dict) else mbfir.dz2d(*s)
        assert np.array_equal(rf, rf1) and np.array_equal(g, g1) and dur == dur1
    assert mbfir.dz2d_batch([]) == []
    assert mbfir.spiral.dz2d is mbfir.dz2d and mbfir.spiral.csg is mbfir.csg


def test_ktog_ktos_gt2cm():
    rng = np.random.default_rng(3)
    k = np.cumsum(rng.standard_normal(40) + 1j * rng.standard_normal(40)) * 0.01
    dt = 0.004
    g, s = mbfir.ktog(k, dt), mbfir.ktos(k, dt)
    assert g.shape == (39,) and s.shape == (38,)
    assert np.allclose(s, np.diff(g) / dt, rtol=1e-13, atol=0)
    assert np.allclose(np.cumsum(g) * 4.257 * dt, k[1:] - k[0], rtol=1e-12, atol=1e-15)
    line = 0.5 * np.arange(10)                                      # a straight line: constant gradient, no slew
    assert np.allclose(mbfir.ktog(line, 0.1), 0.5 / 0.4257) and np.abs(mbfir.ktos(line, 0.1)).max() <= 1e-12
    x = np.linspace(-4, 4, 9)
    assert np.array_equal(mbfir.gt2cm(x, 0.5, 2.0), x / 4.257)      # 4.257 g t = 4.257
    assert np.allclose(mbfir.gt2cm(x, 1.0, 1.0) * 4.257, x)


def test_designer_argument_errors():
    for bad in ((0, 1, 4, 64, 1, 2), (8, -1, 4, 64, 1, 2), (8, 1, 0, 64, 1, 2), (8, 1, 4, 2, 1, 2), (8, 1, 4, 64.5, 1, 2),
                (8, 1, 4, 64, 0, 2), (8, 1, 4, 64, 1, -2), (8, 1, 4, 64, np.inf, 2)):
        with pytest.raises(ValueError):
            mbfir.dz2d(*bad)
    with pytest.raises(ValueError, match="at least 3"):
        mbfir.csg([0, 1], 1, 2)
    with pytest.raises(ValueError, match="zero slew"):
        mbfir.csg(np.arange(8.0), 1, 2)                             # a straight line: interp1 has no distinct knots
    with pytest.raises(ValueError, match="finite"):
        mbfir.csg([0, 1, np.nan, 2], 1, 2)
    with pytest.raises(ValueError, match="arguments"):
        mbfir.dz2d_batch([(8, 1, 4, 64, 1)])
    with pytest.raises(ValueError, match="arguments"):
        mbfir.dz2d_batch([dict(nt=8, bw=1, tbp=4, ns=64, mxg=1)])


def test_abr2_batch_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    assert re.search(r"\bmbfir_abr2_batch\s*\(", hdr)
    assert len(mbfir.SYMBOLS["mbfir_abr2_batch"][1]) == 20
    assert mbfir.load_library().mbfir_abr2_batch is not None        # the library exports it
    assert callable(mbfir.abr2_batch)
    # the workgroup table is the other batched simulators', with nx ny points per pulse
    tab = mbfir.sim_block_table([10, 600], [65 * 65, 3 * 5], 2)
    assert tab.shape == (2 * (17 + 1), 3) and tab[0, 0] == 1 and tab[2, 0] == 0


def test_abr2_batch_argument_errors_come_before_any_device_work():
    x, y = np.linspace(-1, 1, 5), np.linspace(-2, 2, 3)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr2_batch([], x, y)
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr2_batch([np.ones(4)], x, y, scales=())
    with pytest.raises(ValueError, match="no samples"):
        mbfir.abr2_batch([np.ones(4), np.zeros(0)], x, y)
    with pytest.raises(ValueError, match="empty x"):
        mbfir.abr2_batch([np.ones(4)], np.zeros(0), y)
    with pytest.raises(ValueError, match="empty y"):
        mbfir.abr2_batch([np.ones(4), np.ones(4)], x, [y, np.zeros(0)])
    with pytest.raises(ValueError, match="one entry per rf sample"):
        mbfir.abr2_batch([(np.ones(4), np.ones(3) + 0j)], x, y)
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr2_batch([np.ones(4)], x, y, convention="abx")
    with pytest.raises(ValueError, match="x has 3 grids for 2 pulses"):
        mbfir.abr2_batch([np.ones(4), np.ones(4)], [x, x, x], y)
    with pytest.raises(ValueError, match="y has 1 grids for 2 pulses"):
        mbfir.abr2_batch([np.ones(4), np.ones(4)], x, [y])
