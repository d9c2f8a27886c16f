"""Root-flip search on the device (mbfir.flip_search / fir_flip_zero(criterion="rf") / minpeakrf) against host restatements.
Every comparison with a host result is by peak value: mirror-image candidates tie to 1e-11 .. 1e-15 in these sets, so an index
is asserted only where the runner-up is more than 1e-8 away."""
import json
import os

import numpy as np
import pytest

import mbfir
from mbfir.flipzero import _flip, _masks, _poly
from oracle import slr

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


def golden(name, bmax):
    """Golden taps scaled to max|B(w)| = bmax."""
    h = np.array(GOLD[name]["h"]["re"]) + 1j * np.array(GOLD[name]["h"]["im"])
    return h * (bmax / np.abs(np.fft.fft(h, 8192)).max())


def split(h):
    """fir_flip_zero's decomposition: roots, pass-band indices, the common polynomial, the pass-band zeros."""
    Z = np.roots(h)
    pb = np.nonzero((np.abs(Z) > 1 + 1e-2) | (np.abs(Z) < 1 - 1e-2))[0]
    fixed = np.ones(len(Z), dtype=bool)
    fixed[pb] = False
    return _poly(Z[fixed]), Z[pb]


def all_masks(nz):
    """combination_2power(nz): every 2^nz combination, column c flips zero j iff bit (nz - 1 - j) of c is 0."""
    rows = np.arange(nz)[:, None]
    return 1 - ((np.arange(2 ** nz)[None, :] >> (nz - 1 - rows)) & 1)


def host_candidates(h, mask):
    """The candidates of mask (nz x num) as fir_flip_zero builds them, DC rule applied: num x n."""
    c0, zp = split(h)
    zsel = np.where(mask == 1, _flip(zp)[:, None], zp[:, None])
    coef = np.zeros((mask.shape[1], len(h)), dtype=np.complex128)
    coef[:, :len(c0)] = c0
    deg = len(c0) - 1
    for j in range(len(zp)):
        coef[:, 1:deg + 2] -= zsel[j][:, None] * coef[:, :deg + 1]
        deg += 1
    return coef * (np.sum(h) / np.sum(coef, axis=1))[:, None]


def host_rf_peaks(B):
    """max|rf| of b2a.m + ab2rf.m, vectorised over the rows of B."""
    B = np.atleast_2d(B)
    num, n = B.shape
    N = 8 * n
    bf = np.fft.fft(B, N, axis=1)
    m = np.abs(bf).max(axis=1, keepdims=True)
    bf = np.where(m >= 1.0, bf / (1e-8 + m), bf)
    xlf = np.fft.fft(np.log(np.sqrt(1 - (bf * np.conj(bf)).real)), axis=1)
    xlfp = np.zeros_like(xlf)
    xlfp[:, 0] = xlf[:, 0]
    xlfp[:, 1:N // 2] = 2 * xlf[:, 1:N // 2]
    xlfp[:, N // 2] = xlf[:, N // 2]
    aca = np.fft.fft(np.exp(np.fft.ifft(xlfp, axis=1)), axis=1) / N
    a = aca[:, :n][:, ::-1].copy()
    b = B.copy()
    peak = np.zeros(num)
    for i in range(n, 0, -1):
        q = b[:, i - 1] / a[:, i - 1]
        c = np.sqrt(1 / (1 + np.abs(q) ** 2))
        s = np.conj(c * q)
        peak = np.maximum(peak, np.abs(2 * np.arctan2(np.abs(s), c)))
        an = c[:, None] * a + s[:, None] * b
        bn = -np.conj(s)[:, None] * a + c[:, None] * b
        a, b = an[:, 1:i], bn[:, :i - 1]
    return peak


def test_host_chain_is_the_oracle_b2rf():
    h = golden("lin_real33", 0.99)
    B = host_candidates(h, all_masks(10)[:, ::61])
    assert len(B) >= 16
    want = np.array([np.abs(slr.b2rf(b)).max() for b in B])
    assert np.max(np.abs(host_rf_peaks(B) - want)) <= 1e-12 * want.max()


# Rebuilding beta from its roots is ill-conditioned for lin_real64 (the common polynomial's coefficients reach 2e7 against taps of
# 0.2): the host's own peaks move by 2e-3 when the factors are multiplied on in another order.  The device keeps the host's order;
# what is left is the rounding of its fused multiply-adds, measured at 8e-9 on that set.  The chain itself is checked to 1e-10 on
# identical input: the winner's beta through the host chain.
@pytest.mark.parametrize("name,nz,tol", [("lin_cplx31", 8, 1e-10), ("lin_real33", 10, 1e-10), ("lin_real64", 14, 1e-7)])
def test_per_candidate_rf_peaks(name, nz, tol):
    h = golden(name, 0.99)
    c0, zp = split(h)
    assert len(zp) == nz
    b, best, pk = mbfir.flip_search(c0, zp, _flip(zp), target=np.sum(h), criterion="rf", return_peaks=True)
    want = host_rf_peaks(host_candidates(h, all_masks(nz)))
    assert len(pk) == 2 ** nz
    assert np.max(np.abs(pk - want) / want) <= tol
    assert abs(pk[best] - want.min()) <= tol * want.min()
    assert abs(host_rf_peaks(b)[0] - pk[best]) <= 1e-10 * pk[best]


# tol: the rebuild's conditioning (see above) -- lin_real33 is well conditioned, the others differ by the device's fused rounding
@pytest.mark.parametrize("name,bmax,seed,tol", [("lin_real33", 0.707, 1, 1e-12), ("lin_real64", 0.707, 2, 1e-7),
                                                ("qp_modelA48", 0.99, 3, 1e-8), ("qp_modelB25", 0.99, 4, 1e-10)])
def test_beta_criterion_on_the_device_equals_the_host(name, bmax, seed, tol):
    """nz <= 12 (all), 12 < nz <= 19 (4096 sampled), nz > 19 (Monte-Carlo masks; a synthetic case below)."""
    h = golden(name, bmax)
    hh, ih = mbfir.fir_flip_zero(h, seed=seed, return_info=True)
    hd, idv = mbfir.fir_flip_zero(h, seed=seed, return_info=True, device=True)
    assert ih["candidates"] == idv["candidates"]
    assert abs(ih["peak_after"] - idv["peak_after"]) <= tol * ih["peak_after"]
    pk = np.abs(host_candidates(h, _masks(ih["n_passband_zeros"], np.random.default_rng(seed)))).max(axis=1)
    srt = np.sort(pk)
    if srt[1] - srt[0] > 1e-8 * srt[0]:
        assert np.max(np.abs(hh - hd)) <= tol * np.abs(hh).max()


def test_beta_criterion_monte_carlo_masks():
    rng = np.random.default_rng(5)
    zi = 0.75 * np.exp(1j * rng.uniform(-0.8, 0.8, 22))
    zo = np.exp(1j * rng.uniform(1.2, 2 * np.pi - 1.2, 17))
    h = np.poly(np.concatenate([zi, zo])) * 0.01
    hh, ih = mbfir.fir_flip_zero(h, seed=9, return_info=True)
    hd, idv = mbfir.fir_flip_zero(h, seed=9, return_info=True, device=True)
    assert ih["n_passband_zeros"] == 22 and idv["candidates"] == 4096
    assert abs(ih["peak_after"] - idv["peak_after"]) <= 1e-7 * ih["peak_after"]          # a 39-root rebuild: measured 4e-8


@pytest.mark.parametrize("name,bmax", [("lin_real33", 0.99), ("lin_cplx31", 0.99), ("lin_cplx32", 0.99)])
def test_rf_criterion_never_loses(name, bmax):
    h = golden(name, bmax)
    hb = mbfir.fir_flip_zero(h, seed=0, candidates="all")                        # beta criterion, same (full) set
    hr, info = mbfir.fir_flip_zero(h, seed=0, criterion="rf", candidates="all", return_info=True)
    rb, rr, r0 = host_rf_peaks(np.stack([hb, hr, h]))
    assert rr <= rb * (1 + 1e-12)
    assert rr <= r0 * (1 + 1e-12)                                                # the full set holds the unflipped candidate
    assert abs(info["rf_peak_after"] - rr) <= 1e-10 * rr and abs(info["rf_peak_before"] - r0) <= 1e-10 * r0
    if name == "lin_real33":
        assert rr < 0.9 * rb                                                    # 0.4831 against 0.5613
    H, Hr = np.abs(np.fft.fft(h, 1024)), np.abs(np.fft.fft(hr, 1024))
    assert np.max(np.abs(Hr - H)) <= 1e-8 * H.max()
    assert abs(np.sum(hr) - np.sum(h)) <= 1e-12 * abs(np.sum(h))


def test_exhaustive_beyond_the_reference_sample():
    h = golden("qp_modelA48", 0.99)
    c0, zp = split(h)
    assert len(zp) == 18
    b, best, pk = mbfir.flip_search(c0, zp, _flip(zp), target=np.sum(h), criterion="rf", return_peaks=True)
    assert len(pk) == 2 ** 18
    ref = host_rf_peaks(host_candidates(h, _masks(18, np.random.default_rng(0))))   # the reference's seeded 4096
    assert pk[best] <= ref.min() * (1 + 1e-12)
    assert abs(host_rf_peaks(b)[0] - pk[best]) <= 1e-10 * pk[best]
    rng = np.random.default_rng(1)
    idx = rng.choice(2 ** 18, 20000, replace=False)
    rows = np.arange(18)[:, None]
    sub = host_rf_peaks(host_candidates(h, 1 - ((idx[None, :] >> (17 - rows)) & 1)))
    assert sub.min() >= pk[best] * (1 - 1e-12)
    assert np.max(np.abs(sub - pk[idx]) / sub) <= 1e-8                             # rebuild conditioning: measured 3.7e-9


def host_minpeakrf(z, flip, bsf):
    """minpeakrf.c restated on the host: scored by oracle.slr.b2rf of the npoly-normalised beta."""
    def score(r):
        b = np.poly(r)
        nn = 1 << int(np.ceil(np.log2(len(b))))
        b = b / np.abs(np.fft.fft(b, nn)).max() * bsf
        return np.abs(slr.b2rf(b)).max()
    fr = lambda v: v / abs(v) ** 2                                                  # noqa: E731
    singles = [r - 1 for r, s in flip if s == 0]
    pairs = [(r - 1, s - 1) for r, s in flip if s != 0]
    z0 = z.copy()
    for r1, r2 in pairs:
        if (abs(z[r1]) - 1) / (abs(z[r2]) - 1) < 0:
            z0[r1] = fr(z[r1])

    def cand(i):
        zm, bit = z0.copy(), 1
        for r in singles:
            if i & bit:
                zm[r] = fr(z0[r])
            bit <<= 1
        for r1, r2 in pairs:
            if i & bit:
                zm[r1] = fr(z0[r1])
            else:
                zm[r2] = fr(z0[r2])
            bit <<= 1
        return zm
    best, bi = score(z0), 0
    peaks = []
    for i in range(2 ** (len(singles) + len(pairs))):
        p = score(cand(i))
        peaks.append(p)
        if p <= best:
            best, bi = p, i
    return cand(bi), best, np.array(peaks)


@pytest.mark.parametrize("bsf,seed", [(0.5, 0), (0.9, 1), (0.9, 2)])
def test_minpeakrf_semantics(bsf, seed):
    rng = np.random.default_rng(seed)
    zc = rng.uniform(0.5, 1.6, 3) * np.exp(1j * rng.uniform(0.3, 2.5, 3))
    z = np.concatenate([zc, np.conj(zc), rng.uniform(0.3, 1.8, 4) * np.exp(1j * rng.uniform(-3, 3, 4)),
                        np.exp(1j * rng.uniform(-3, 3, 8))])
    z[4] = 1 / np.conj(z[4]) if abs(z[1]) > 1 else z[4]                           # one pair on opposite sides of the circle
    flip = [[7, 0], [1, 4], [9, 0], [2, 5], [8, 0], [3, 6], [10, 0]]
    zmin = mbfir.minpeakrf(z, np.array(flip), bsf)
    zh, ph, peaks = host_minpeakrf(z, flip, bsf)
    def score(r):
        b = np.poly(r)
        nn = 1 << int(np.ceil(np.log2(len(b))))
        return np.abs(slr.b2rf(b / np.abs(np.fft.fft(b, nn)).max() * bsf)).max()
    assert abs(score(zmin) - score(zh)) <= 1e-10 * score(zh)
    assert score(zmin) <= max(ph, peaks[0]) * (1 + 1e-10)
    srt = np.sort(peaks)
    if srt[1] - srt[0] > 1e-8 * srt[0]:
        assert np.allclose(np.sort_complex(zmin), np.sort_complex(zh), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        mbfir.minpeakrf(z, [[30, 0]], bsf)
    with pytest.raises(ValueError):
        mbfir.minpeakrf(z, flip, 1.2)


def test_large_n_explicit_masks():
    """n = 512: a windowed-sinc common polynomial and 40 flip factors spread round the circle, npoly rule (max|B| = 0.7)."""
    rng = np.random.default_rng(7)
    n, nz, bsf = 512, 40, 0.7
    t = np.arange(n - nz) - (n - nz - 1) / 2
    c0 = (np.sinc(t / 8) * np.hamming(n - nz)).astype(np.complex128)
    zp = rng.uniform(0.85, 0.95, nz) * np.exp(2j * np.pi * (np.arange(nz) + rng.uniform(0, 1, nz)) / nz)
    masks = (rng.random((nz, 4096)) < 0.5).astype(int)
    b, best, pk = mbfir.flip_search(c0, zp, _flip(zp), masks=masks, bsf=bsf, criterion="rf", return_peaks=True)
    assert np.all(np.isfinite(pk)) and pk[best] == pk.min()
    samp = rng.choice(4096, 64, replace=False)
    zsel = np.where(masks[:, samp] == 1, _flip(zp)[:, None], zp[:, None])
    for col, c in enumerate(samp):
        bc = np.concatenate([c0, np.zeros(nz, dtype=np.complex128)])
        for j, deg in enumerate(range(n - nz - 1, n - 1)):                     # the device's order: c0, then factor 0, 1, ..
            bc[1:deg + 2] -= zsel[j, col] * bc[:deg + 1]
        bc = bc / np.abs(np.fft.fft(bc, 512)).max() * bsf
        want = np.abs(slr.b2rf(bc)).max()
        assert abs(pk[c] - want) <= 1e-9 * want, c                            # 4096-point direct sums: measured 1.7e-10


def test_determinism():
    h = golden("lin_real64", 0.99)
    c0, zp = split(h)
    r1 = mbfir.flip_search(c0, zp, _flip(zp), target=np.sum(h), criterion="rf", return_peaks=True)
    r2 = mbfir.flip_search(c0, zp, _flip(zp), target=np.sum(h), criterion="rf", return_peaks=True)
    assert r1[1] == r2[1] and np.array_equal(r1[0], r2[0]) and np.array_equal(r1[2], r2[2])


def test_dzrf_mb_rf_criterion():
    """C-13 multiband 60-degree qp_cvx design at 60 taps: 42 pass-band zeros (Monte-Carlo masks, seeded alike for both runs)."""
    from test_bloch_gpu import c13_args, check_profile
    cf, rng, FA, rp = c13_args()
    args = (60, 0.04, cf, rng, FA, rp, "ex", "qp_cvx", "C-13", 1)
    rf0, b0, spec0, _ = mbfir.dzrf_mb(*args, flip_seed=3)
    rf1, b1, spec1, _ = mbfir.dzrf_mb(*args, flip_seed=3, flip_criterion="rf")
    Z = np.roots(b0)
    assert np.sum((np.abs(Z) > 1.01) | (np.abs(Z) < 0.99)) >= 6
    assert np.abs(rf1).max() <= np.abs(rf0).max() * (1 + 1e-10)
    check_profile(rf1, 0.04, 1.0705, spec1, slack=1.4)
