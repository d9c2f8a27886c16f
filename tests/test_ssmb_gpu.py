"""Multiband spectral-spatial designer on the device: the 2D inverse SLR (mbfir.slr2d_batch) against its NumPy restatement, its
batch independence, its literal form against dzepse's fixtures, dzss_mb_batch against single calls, and the physics of two C-13
excitations simulated by mbfir.bloch, held to the thresholds of tests/test_ssmb_cpu.py."""
import importlib.util
import json
import os

import numpy as np
import pytest

import mbfir
from mbfir import epse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cpu():
    spec = importlib.util.spec_from_file_location("ssmb_cpu", os.path.join(ROOT, "tests", "test_ssmb_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _cpu()
SLR2D_TOL = 1e-12            # relative to max|rn2|; measured worst 1.1e-14


def _mats(count, m, n, seed):
    """count complex m x n matrices of physical rows: every row scaled to max|B| = U(0.2, 0.9) on b2a's 8 n grid.  (Rows with
    max|B| near or above 1 make log sqrt(1 - |B|^2) ill-conditioned: there device and oracle part by up to 4e-10 of max|rn2|.)"""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((count, m, n)) + 1j * rng.standard_normal((count, m, n))
    peak = np.abs(np.fft.fft(R, 8 * n, axis=2)).max(axis=2, keepdims=True)
    return R * (rng.uniform(0.2, 0.9, (count, m, 1)) / peak)


@pytest.mark.parametrize("m,n", [(2, 2), (2, 16), (16, 2), (16, 64), (64, 16), (64, 256), (256, 64), (256, 2), (2, 256),
                                 (2048, 2), (2, 2048), (16, 2048)])
def test_slr2d_batch_matches_restatement(m, n):
    R = _mats(2, m, n, m * 7 + n)
    got = mbfir.slr2d_batch(R)
    assert got.shape == (2, m, n)
    want = cpu.slr2d_np(R)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("slr2d %d x %d: rel err %.2e" % (m, n, err))
    assert err <= SLR2D_TOL, (m, n, err)
    lit = mbfir.slr2d_batch(R[:1], literal=True)[0]
    want = cpu.slr2d_np(R[:1], literal=True)[0]
    assert float(np.abs(lit - want).max() / np.abs(want).max()) <= SLR2D_TOL


def test_slr2d_batch_is_position_independent_and_repeatable():
    for m, n in ((16, 64), (256, 16), (64, 2048)):
        R = _mats(5, m, n, 11)
        ref = mbfir.slr2d_batch(R)
        assert np.array_equal(mbfir.slr2d_batch(R), ref)
        for q in (0, 4):
            assert np.array_equal(mbfir.slr2d_batch(R[q:q + 1])[0], ref[q])
        assert np.array_equal(mbfir.slr2d_batch(R[::-1])[::-1], ref)


def test_slr2d_batch_rejects_bad_sizes():
    ctx = mbfir.get_context()
    lib = mbfir.load_library()
    r = np.ones(4096)
    o = np.zeros(4096)
    p = mbfir._ptr
    for m, n, count, lit in ((3, 8, 1, 0), (8, 2049, 1, 0), (2050, 2, 1, 0), (8, 1, 1, 0), (8, 8, 0, 0), (8, 8, 1, 2)):
        assert lib.mbfir_slr2d_batch(ctx._h, m, n, count, p(r), None, p(o), p(o), lit) == mbfir.E_ARG


def test_slr2d_batch_literal_form_matches_dzepse_fixtures():
    """On dzepse's own r, then versec, the literal form reproduces the fixtures (the axis form does not: test_ssmb_cpu.py)."""
    gen = cpu._generator()
    with open(os.path.join(GOLDEN, "epse.json")) as fh:
        names = list(json.load(fh)["dzepse"])
    worst = 0.0
    with np.load(os.path.join(GOLDEN, "epse.npz")) as z:
        for name in names:
            r, gx = cpu.dzepse_r(gen, name)
            rf = epse.versec(gx, mbfir.slr2d_batch(r[None], literal=True)[0]).ravel(order="F")
            want = z["dzepse/%s/rf" % name]
            err = float(np.abs(rf - want).max() / np.abs(want).max())
            worst = max(worst, err)
            assert err <= cpu.DZEPSE_TOL, (name, err)
    print("slr2d literal against dzepse fixtures: worst rel err %.2e" % worst)


def test_dzss_mb_batch_is_bit_identical_to_single_calls():
    specs = [cpu.SYM, cpu.FLY, dict(cpu.SYM, ftype="qp_cvx"), dict(cpu.FLY, ftype="ap_minstopripple_cvx"),
             dict(cpu.SYM, ftype="ap_minorder_cvx", ngx=31), dict(cpu.FLY, ngx=4), dict(cpu.SYM, tbx=3.0, xftype="ms")]
    batch = mbfir.dzss_mb_batch(specs)
    assert [b[2]["status"] for b in batch].count("Solved") >= 5 and batch[5][2]["status"] == "Failed"
    assert batch[4][2]["ngx"] <= 31
    for s, (rf, g, info) in zip(specs, batch):
        rf1, g1, info1 = mbfir.dzss_mb(**s)
        assert np.array_equal(rf, rf1) and np.array_equal(g, g1) and np.array_equal(info["beta"], info1["beta"])
    # the spectral beta is the one dzrf_mb hands to b2rf on the folded spec
    rf, g, info = batch[0]
    fold = mbfir.fold_bands(cpu.SYM["mb_cf"], cpu.SYM["mb_range"], cpu.SYM["mb_FA"], cpu.SYM["mb_ripple"], info["fs"])
    _, b, _, _ = mbfir.dzrf_mb(25, info["Ts"], fold["mb_cf"], fold["mb_range"], fold["mb_FA"], fold["mb_ripple"], "ex", "ap_cvx")
    assert np.array_equal(info["beta"], b)


def sim_device(dt):
    def sim(b1, g, df, x):
        mx, my, _ = mbfir.bloch(b1, g, dt * 1e-3, 1e6, 1e6, df, x)
        return np.abs(mx + 1j * my)
    return sim


@pytest.mark.parametrize("name", ["SYM", "FLY"])
def test_dzss_mb_c13_physics(name):
    """At the slice centre |Mxy(f)| follows the hard-pulse train of the spectral beta over every band; the slice profile at every
    band centre has its pass band within +-0.35 thk and its stop band beyond 1.5 thk (thresholds: test_ssmb_cpu.py)."""
    spec = getattr(cpu, name)
    rf, g, info = mbfir.dzss_mb(**spec)
    assert info["status"] == "Solved" and len(spec["mb_FA"]) >= 3 and len(set(spec["mb_FA"]) - {0}) >= 2
    cpu.check_physics(spec, rf, g, info, sim_device(spec["dt"]))
    # the device simulation is the CPU restatement's
    fr, x = cpu.physics_grids(spec, info)
    dev = sim_device(spec["dt"])(rf, g, fr[::7], x[::20])
    ref = cpu.sim_cpu(spec["dt"])(rf, g, fr[::7], x[::20])
    assert np.abs(dev - ref).max() <= 1e-9
