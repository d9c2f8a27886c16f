"""The single-launch factorisation (k_chol_dag, form 4), whose inverse-row tasks run their 64-step substitutions on the matrix
cores' accumulator layout (subst16x4 on the transposed tile, minv_strip), against the per-step form (form 1, untouched code) bit
for bit and against an independent reference.  All cases go through mbfir.test_chol_lanes, which also checks Mt == M'.

Shapes: the smallest at which each branch of the two tasks runs -- n = 64 (one block: no row block), 150 (three blocks,
padding; inverse tiles j == r, j == r - 1 and one accumulated panel), 320 (several panels, left-looking trailing tiles), 1024 in
16 lanes (the bench's unit), 2112 (33 blocks: the inverse rows take R_rj from the inverse-update tasks).

Matrices: trig-Gram matrices A' D A with weights over ten decades, as test_cholesky_ill_conditioned_scaling builds them, and one
well-conditioned random SPD matrix per size.

Reference and bounds.  Up to n = 320 the reference is a Cholesky factorisation and triangular inverse in NumPy long double; at n
= 1024 and 2112 that takes 7 s and a minute per matrix, so there the reference is LAPACK's fp64 factor (what
tests/test_kernels_gpu.py::test_cholesky_and_inverse itself compares with) and its fp64 inverse.  Every lane of every case is
held against its reference, L and M both.  The well-conditioned matrices are held to that test's bounds for the same quantities:
relinf(L, Lref) <= 1e-12, max |M Lref - I| <= 1e-11, and relinf(M, Mref) <= 1e-11 (LAPACK's fp64 inverse is 5e-16 .. 1.2e-14
from the long double one on them, as close as its M Lref is to I: the same bound).  The trig-Gram matrices have cond(H) = 5e7 ..
3e9 and NO fp64 factorisation meets those: LAPACK's own fp64 factor is 5.7e-12 (n = 64), 1.7e-10 (150) and 2.8e-10 (320) away
from the long double one, its inverse 2e-11 .. 1.2e-9 from M L = I.  They are held to the bounds
test_cholesky_ill_conditioned_scaling sets for such a matrix: relinf(L L', H) <= 1e-12, relinf(L, Lref) <= 1e-6 and a solve
residual |H M'(M b) - b| <= 2e-4 |b|; M is held to the bound that test sets for L, max |M Lref - I| <= 1e-6 and relinf(M, Mref)
<= 1e-6 (LAPACK's fp64 inverse reaches 5e-12 .. 1.5e-9 and 2e-11 .. 1.7e-8 on them: the same conditioning, the same two to four
decades of room).  (Measured on an MI355X, maxima over the lanes: well-conditioned relinf(L, Lref) 6e-16 .. 3.7e-14, max |M Lref
- I| 1.5e-15 .. 3.4e-13, relinf(M, Mref) 2.3e-15 .. 5.7e-13; trig-Gram relinf(L L', H) <= 1.6e-15, relinf(L, Lref) 3e-11 ..
1.5e-9, max |M Lref - I| 1e-10 .. 1.1e-8, relinf(M, Mref) 4e-10 .. 1.2e-7, residual <= 8.2e-5.)"""
import functools

import numpy as np
import pytest
from conftest import relinf

import mbfir

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = [(64, 1), (64, 3), (150, 1), (150, 3), (320, 1), (320, 3), (1024, 16), (2112, 1)]
RUNS = [("trig", n, nl) for n, nl in CASES] + [("rand", n, 1) for n in sorted({n for n, _ in CASES})]
RUN_IDS = ["%s-%d-%d" % r for r in RUNS]


def _trig_gram(n, seed):
    rng = np.random.default_rng(seed)
    m = max(4000, 2 * n)
    A = np.cos(np.outer(rng.uniform(-3, 3, m), np.arange(n)))
    d = 10.0 ** rng.uniform(-5, 5, m)
    H = (A.T * d) @ A
    return H + 1e-9 * np.abs(H).max() * np.eye(n)


def _random_spd(n):
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n + 20, n))
    return B.T @ B + 0.1 * np.eye(n)


@functools.lru_cache(maxsize=None)
def _matrices(kind, n, nl):
    Hs = np.array([_trig_gram(n, 1000 * n + b) for b in range(nl)]) if kind == "trig" else _random_spd(n)[None]
    Hs.setflags(write=False)
    return Hs


@functools.lru_cache(maxsize=None)
def _factors(kind, n, nl, form):
    L, M = mbfir.test_chol_lanes(_matrices(kind, n, nl), form=form)
    L.setflags(write=False)
    M.setflags(write=False)
    return L, M


def _chol_inv_longdouble(H, bs=64):
    """Right-looking blocked Cholesky H = L L' and M = L^-1 by forward substitution on the identity, in long double."""
    n = H.shape[0]
    A = np.tril(H.astype(LD))
    for k in range(0, n, bs):
        e = min(k + bs, n)
        for c in range(k, e):
            A[c, c] = np.sqrt(A[c, c])
            A[c + 1:, c] /= A[c, c]
            if c + 1 < e:
                A[c + 1:, c + 1:e] -= np.outer(A[c + 1:, c], A[c + 1:e, c])
        if e < n:
            P = A[e:, k:e]
            A[e:, e:] -= P @ P.T
    L = np.tril(A)
    M = np.zeros_like(L)
    for k in range(0, n, bs):
        e = min(k + bs, n)
        R = np.concatenate([-(L[k:e, :k] @ M[:k, :k]), np.eye(e - k, dtype=LD)], axis=1)
        for c in range(k, e):
            i = c - k
            R[i] /= L[c, c]
            if c + 1 < e:
                R[i + 1:] -= np.outer(L[c + 1:e, c], R[i])
        M[k:e, :e] = R
    return L, M


@pytest.mark.parametrize("kind,n,nl", RUNS, ids=RUN_IDS)
def test_cholsubst_dag_equals_the_per_step_form(kind, n, nl):
    """Form 4 (one launch, the substitutions on the accumulator layout) against form 1 (per step): every lane's L and M
    bit for bit."""
    L4, M4 = _factors(kind, n, nl, 4)
    L1, M1 = _factors(kind, n, nl, 1)
    for b in range(nl):
        assert np.array_equal(L4[b], L1[b]), ("L", b)
        assert np.array_equal(M4[b], M1[b]), ("M", b)


@pytest.mark.parametrize("kind,n,nl", RUNS, ids=RUN_IDS)
def test_cholsubst_dag_against_an_independent_reference(kind, n, nl):
    """Form 4 against a long double Cholesky and inverse (n <= 320) or LAPACK's fp64 factor and inverse (beyond), every lane;
    bounds: see the module's docstring."""
    Hs = _matrices(kind, n, nl)
    L4, M4 = _factors(kind, n, nl, 4)
    rng = np.random.default_rng(7 * n + nl)
    for b in range(nl):
        H, L, M = Hs[b], L4[b], M4[b]
        assert np.abs(np.triu(L, 1)).max() == 0 and np.abs(np.triu(M, 1)).max() == 0
        if n <= 320:
            Lr, Mr = _chol_inv_longdouble(H)
        else:
            Lr = np.linalg.cholesky(H)
            Mr = np.linalg.inv(Lr)
        eL = relinf(L, Lr)
        eI = float(np.abs(M @ Lr - np.eye(n)).max())
        eM = relinf(M, Mr)
        eH = relinf(L @ L.T, H)
        rhs = rng.standard_normal(n)
        res = float(np.linalg.norm(H @ (M.T @ (M @ rhs)) - rhs) / np.linalg.norm(rhs))
        print("%s n %d lane %d: relinf(L, Lref) %.2e  max|M Lref - I| %.2e  relinf(M, Mref) %.2e  relinf(L L', H) %.2e  solve residual %.2e"
              % (kind, n, b, eL, eI, eM, eH, res))
        if kind == "rand":
            assert eL <= 1e-12
            assert eI <= 1e-11
            assert eM <= 1e-11
            assert res <= 1e-10
        else:
            assert eH <= 1e-12
            assert eL <= 1e-6
            assert eI <= 1e-6
            assert eM <= 1e-6
            assert res <= 2e-4


def test_cholsubst_masked_lane():
    """n = 150, three lanes, the middle one switched off: the live lanes equal their unmasked results bit for bit.  The masked
    lane's output is as it went in (zeros) -- which says that the hook hands nothing back for it, NOT what the kernel left in
    that lane's device buffers: mbfir_test_chol_lanes skips masked lanes at read-back, so this half witnesses the host side only."""
    Hs = _matrices("trig", 150, 3)
    L4, M4 = _factors("trig", 150, 3, 4)
    L, M = mbfir.test_chol_lanes(Hs, form=4, mask=[1, 0, 1])
    for b in (0, 2):
        assert np.array_equal(L[b], L4[b]) and np.array_equal(M[b], M4[b]), b
    assert not L[1].any() and not M[1].any()
