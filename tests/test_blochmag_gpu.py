"""The magnitude least-squares products of the Bloch simulator on the device (magnitude=True on mbfir.bloch_lsq_batch,
bloch_gn_batch, bloch_lm_step_batch, their steady-state twins and the refiners: k_bloch_lsq_batch_mag, k_bloch_gn_batch_mag,
k_bloch_lm_sweep_mag, k_bloch_ss_lsq_batch_mag, k_bloch_ss_gn_batch_mag, k_bloch_ss_lm_sweep_mag) against the long-double NumPy
recursion of tests/blochmag_ref.py, against the shipped calls (the component fit at the phase-projected target; jvp -> host seed ->
vjp), for the exact properties (zero loss at the call's own magnitude, rho = 0, zero weights and dead threads, the batch's
composition, a direction's place among K), the Levenberg-Marquardt step and the refiners.

Bounds (tests/blochmag_ref.py derives them): with gain = max|s| gamma dt_t (times kappa in the steady state), eps = 1e-12 (bound_m
(kappa) in the steady state), r = rho - t_xy, D = |dm_x| + |dm_y| and bj = bound_jvp,
    g within gain (1e-12 N + eps sum (w_xy (2 + 4 |r| / rho) + w_z)),  H v within gain (1e-12 N + bj sum (2 w_xy + w_z) + (2 sqrt 2
    + 4) eps sum w_xy D / rho),  L within eps (sqrt 2 sum w_xy |r| + sum w_z |mz - t_z|) + 1e-13 sum w (.)^2,
N = sum|c| of the reference's seed.  In the bounded comparisons w_xy = 0 where the long-double rho < 1e-3
(tests/test_blochmag_cpu.py asserts how many points that removes)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochmag_ref", os.path.join(ROOT, "tests", "blochmag_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
SCALES = ref.SCALES
KMAX = 3
MODELS = [False, True]                                                      # steady: the end point (mode 0), the steady state (mode 1)


def _fns(steady):
    """(forward, lsq, gn, jvp, vjp, lm step) of the model; the forward call returns (mx, my, mz) per pulse"""
    if steady:
        return (lambda *a, **k: mbfir.bloch_batch(*a, mode=1, **k), mbfir.bloch_ss_lsq_batch, mbfir.bloch_ss_gn_batch,
                mbfir.bloch_ss_jvp_batch, mbfir.bloch_ss_vjp_batch, mbfir.bloch_ss_lm_step_batch)
    return (mbfir.bloch_batch, mbfir.bloch_lsq_batch, mbfir.bloch_gn_batch, mbfir.bloch_jvp_batch, mbfir.bloch_vjp_batch,
            mbfir.bloch_lm_step_batch)


@functools.lru_cache(maxsize=None)
def _case(shared, steady):
    """The masked cases with three directions per pulse, their long-double references with the bounds, and the device's results"""
    if steady:
        pulses, dfs, dps, tgs, wts, vs, _, kept = ref.ss_cases(shared, KMAX)
        m0s = None
    else:
        pulses, dfs, dps, m0s, tgs, wts, vs, _ = ref.cases(shared, KMAX)
        kept = list(range(len(pulses)))
    want = {}
    for q in kept:
        a = (pulses[q], dfs[q], dps[q])
        if steady:
            L, g, li, h, hi = ref.ss_products(*a, tgs[q], wts[q], vs[q], SCALES, dtype=np.longdouble)
            k = li["kappa"]
            want[q] = (L, g, h, ref.ss_bound_L(li, k), ref.ss_bound_g(pulses[q], li, SCALES, k),
                       ref.ss_bound_h(pulses[q], vs[q], hi, SCALES, k))
        else:
            L, g, li = ref.lsq(*a, tgs[q], wts[q], SCALES, m0s[q], dtype=np.longdouble, parts=True)
            h, hi = ref.gn(*a, vs[q], wts[q], SCALES, m0s[q], dtype=np.longdouble, parts=True)
            want[q] = (L, g, h, ref.bound_L(li), ref.bound_g(pulses[q], li, SCALES), ref.bound_h(pulses[q], vs[q], hi, SCALES))
    D, P = (dfs[0], dps[0]) if shared else (dfs, dps)
    kw = dict(scales=SCALES) if steady else dict(scales=SCALES, m0=m0s)
    _, lsq_fn, gn_fn, _, _, _ = _fns(steady)
    lsq = lsq_fn(pulses, D, P, tgs, wts, magnitude=True, **kw)
    gn = gn_fn(pulses, D, P, vs, wts, magnitude=True, **kw)
    return pulses, dfs, dps, D, P, kw, tgs, wts, vs, want, lsq, gn


@pytest.mark.parametrize("steady", MODELS)
@pytest.mark.parametrize("shared", [False, True])
def test_device_loss_gradient_and_products_are_the_reference(shared, steady):
    """Eight pulses of 1 .. 600 samples on 1 .. 600 points, scales 1.0, 0.0, 0.9 (blochgn_ref.cases, blochssgn_ref.cases, as pairs):
    L, g and H v at K = 3 within the bounds of the long-double reference; K = 1 and 2 have K = 3's bits."""
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, want, lsq, gn = _case(shared, steady)
    gn_fn = _fns(steady)[2]
    by_k = {K: gn_fn(pulses, D, P, [v[:K] for v in vs], wts, magnitude=True, **kw) for K in (1, 2)}
    worst = [0.0, 0.0, 0.0]
    for q, (L, g, h, bl, bg, bh) in want.items():
        el = abs(float(lsq[q][0] - L))
        eg, eh = np.abs(lsq[q][1] - g).astype(np.float64), np.abs(gn[q] - h).astype(np.float64)
        share = (el / bl if bl else 0.0, float((eg / bg).max()), float((eh / bh).max()))
        worst = [max(a, b) for a, b in zip(worst, share)]
        print("steady %s shared %s n %d: L %.6g share of the bound %.3g; g share %.3g; H v share %.3g"
              % (steady, shared, len(pulses[q][0]), float(L), *share))
        assert el <= bl and np.all(eg <= bg) and np.all(eh <= bh), q
    print("steady %s shared %s: worst shares of the bounds L %.3g g %.3g H v %.3g" % (steady, shared, *worst))
    for q in range(len(pulses)):
        for K in (1, 2):
            assert np.array_equal(by_k[K][q], gn[q][:K]), (q, K)             # K does not change a direction's bits


@pytest.mark.parametrize("steady", MODELS)
@pytest.mark.parametrize("shared", [False, True])
def test_device_results_are_the_shipped_calls(shared, steady):
    """L and g against the forward call -> NumPy -> the component lsq call at t = (t_xy u_x, t_xy u_y, t_z), w = (w_xy, w_xy, w_z);
    H v against jvp -> host seed -> vjp; within the same bounds"""
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, want, lsq, gn = _case(shared, steady)
    fwd_fn, lsq_fn, _, jvp_fn, vjp_fn, _ = _fns(steady)
    fwd = fwd_fn(pulses, D, P, **kw)
    dirs = [ref.mag_dir(m[0], m[1]) for m in fwd]
    t3 = [(t[0] * ux, t[0] * uy, t[1]) for t, (_, ux, uy) in zip(tgs, dirs)]
    w3 = [(w[0], w[0], w[1]) for w in wts]
    comp = lsq_fn(pulses, D, P, t3, w3, **kw)
    tan = jvp_fn(pulses, D, P, vs, **kw)
    for q, (L, g, h, bl, bg, bh) in want.items():
        assert abs(lsq[q][0] - comp[q][0]) <= bl and np.all(np.abs(lsq[q][1] - comp[q][1]) <= bg), q
    for k in range(KMAX):
        seeds = []
        for w, (_, ux, uy), (_, dm) in zip(wts, dirs, tan):
            a = ux * dm[0][k] + uy * dm[1][k]
            seeds.append((w[0] * a * ux, w[0] * a * uy, w[1] * dm[2][k]))
        h2 = vjp_fn(pulses, D, P, seeds, **kw)
        for q, (L, g, h, bl, bg, bh) in want.items():
            got = h2[q][0] if isinstance(h2[q], tuple) else h2[q]
            assert np.all(np.abs(gn[q][k] - got) <= bh[k]), (q, k)


@pytest.mark.parametrize("steady", MODELS)
def test_the_calls_own_magnitude_as_target_gives_zero_loss_and_an_exactly_zero_gradient(steady):
    """t_xy = np.sqrt(mx * mx + my * my) and t_z = mz of the forward call's output: rho has those bits, so L == 0.0 and g == 0.
    For the end point this needs the kernel's sweep to end on k_bloch_batch's bits, which the component kernel's does not (the
    shipped bloch_lsq_batch at t = m of bloch_batch, unit weights, returns L = 1.2e-35 ... 1.2e-28 on these pulses, not 0: the
    compiler contracts R v differently in the two sweeps); k_bloch_lsq_batch_mag steps with bloch_fwd_step_batch (sim_dev.h), which
    states k_bloch_batch's rounding with explicit fma.  The steady state's pass 0 has mode 1's bits as it is."""
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, _, _, _ = _case(False, steady)
    fwd_fn, lsq_fn = _fns(steady)[:2]
    fwd = fwd_fn(pulses, D, P, **kw)
    own = [(np.sqrt(m[0] * m[0] + m[1] * m[1]), m[2]) for m in fwd]
    ones = [(1.0, 1.0)] * len(pulses)
    for q, res in enumerate(lsq_fn(pulses, D, P, own, ones, magnitude=True, **kw)):
        assert res[0] == 0.0 and np.array_equal(res[1], np.zeros(len(pulses[q][0]))), q
    if steady:
        res = lsq_fn(pulses, D, P, own, ones, magnitude=True, steady=True, **kw)
        for q, (L, g, M) in enumerate(res):
            assert L == 0.0 and all(np.array_equal(M[c], fwd[q][c]) for c in range(3)), q


@pytest.mark.parametrize("steady", MODELS)
def test_rho_exactly_zero_is_finite_and_adds_exact_zeros(steady):
    """b1 = 0 and m0 = (0, 0, 1): rho = 0 at every point.  L, g and H v are finite, g and H v have the bits of the call with
    w_xy = 0, and L is that call's loss plus 1/2 sum w_xy t_xy^2 within the loss bound (1e-13 of the sum of the terms)."""
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, _, _, _ = _case(False, steady)
    kw = dict(scales=SCALES)
    _, lsq_fn, gn_fn = _fns(steady)[:3]
    still = [(np.zeros_like(p[0]),) + tuple(p[1:]) for p in pulses]
    raw = ref.to_pairs(*(ref.ssg.cases(False, 1)[3:5] if steady else ref.gnref.cases(False, 1)[4:6]))[1]      # unmasked weights
    noxy = [(0.0, w[1]) for w in raw]
    a, b = lsq_fn(still, D, P, tgs, raw, magnitude=True, **kw), lsq_fn(still, D, P, tgs, noxy, magnitude=True, **kw)
    ha, hb = gn_fn(still, D, P, vs, raw, magnitude=True, **kw), gn_fn(still, D, P, vs, noxy, magnitude=True, **kw)
    for q in range(len(pulses)):
        extra = 0.5 * float((np.asarray(raw[q][0]) * np.asarray(tgs[q][0]) ** 2).sum())
        assert np.isfinite(a[q][0]) and np.all(np.isfinite(a[q][1])) and np.all(np.isfinite(ha[q])), q
        assert np.array_equal(a[q][1], b[q][1]) and np.array_equal(ha[q], hb[q]), q
        assert abs(a[q][0] - (b[q][0] + extra)) <= 1e-13 * 2 * a[q][0], q


@pytest.mark.parametrize("steady", MODELS)
def test_zero_direction_zero_weights_and_dead_threads_give_exact_zeros(steady):
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, _, lsq, gn = _case(False, steady)
    _, lsq_fn, gn_fn = _fns(steady)[:3]
    zero = [(0.0, 0.0)] * len(pulses)
    for h, v in zip(gn_fn(pulses, D, P, [np.zeros_like(v) for v in vs], wts, magnitude=True, **kw), vs):
        assert np.array_equal(h, np.zeros(v.shape))
    for res, v in zip(lsq_fn(pulses, D, P, tgs, zero, magnitude=True, **kw), vs):
        assert res[0] == 0.0 and np.array_equal(res[1], np.zeros(v.shape[1]))
    for h, v in zip(gn_fn(pulses, D, P, vs, zero, magnitude=True, **kw), vs):
        assert np.array_equal(h, np.zeros(v.shape))
    # the 1 x 257 grid: its second workgroup has one live thread.  With that point's weights zero the workgroup adds exact zeros,
    # so the results are those of the first 256 points alone
    q = next(i for i, (df, dp) in enumerate(zip(dfs, dps)) if len(df) * np.shape(dp)[0] == 257)
    cut = lambda tri: tuple(np.asarray(x)[..., :256] for x in tri)
    off = tuple(np.where(np.arange(257) == 256, 0.0, np.asarray(x)) for x in wts[q])
    kq = dict(scales=SCALES) if steady else dict(scales=SCALES, m0=[kw["m0"][q]])
    kc = dict(scales=SCALES) if steady else dict(scales=SCALES, m0=[cut(kw["m0"][q])])
    (full,), (part,) = (lsq_fn([pulses[q]], dfs[q], dps[q], [tgs[q]], [off], magnitude=True, **kq),
                        lsq_fn([pulses[q]], dfs[q], dps[q][:256], [cut(tgs[q])], [cut(off)], magnitude=True, **kc))
    assert full[0] == part[0] and np.array_equal(full[1], part[1])
    (hf,), (hp,) = (gn_fn([pulses[q]], dfs[q], dps[q], [vs[q]], [off], magnitude=True, **kq),
                    gn_fn([pulses[q]], dfs[q], dps[q][:256], [vs[q]], [cut(off)], magnitude=True, **kc))
    assert np.array_equal(hf, hp)


@pytest.mark.parametrize("steady", MODELS)
def test_a_pulse_alone_has_its_bits_in_the_batch_and_a_direction_its_bits_at_every_place(steady):
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, _, lsq, gn = _case(False, steady)
    _, lsq_fn, gn_fn = _fns(steady)[:3]
    for q in range(len(pulses)):
        kq = dict(scales=SCALES) if steady else dict(scales=SCALES, m0=[kw["m0"][q]])
        (one,) = lsq_fn([pulses[q]], dfs[q], dps[q], [tgs[q]], [wts[q]], magnitude=True, **kq)
        assert one[0] == lsq[q][0] and np.array_equal(one[1], lsq[q][1]), q
        for j in range(KMAX):
            (h,) = gn_fn([pulses[q]], dfs[q], dps[q], [np.roll(vs[q], j, 0)], [wts[q]], magnitude=True, **kq)
            assert np.array_equal(np.roll(h, -j, 0), gn[q]), (q, j)
    rev = lsq_fn(pulses[::-1], D[::-1], P[::-1], tgs[::-1], wts[::-1], magnitude=True,
                 **(kw if steady else dict(scales=SCALES, m0=kw["m0"][::-1])))
    for q in range(len(pulses)):
        assert rev[len(pulses) - 1 - q][0] == lsq[q][0] and np.array_equal(rev[len(pulses) - 1 - q][1], lsq[q][1]), q


def _rhs_and_mu(lsq, gn):
    """b = -g and mu = 1e-2 Re <g, H g> / <g, g> per pulse, as the refiners start"""
    bs = [-g for _, g in lsq]
    mus = [1e-2 * float((np.conj(b) * h).real.sum()) / float((np.abs(b) ** 2).sum()) if np.any(b) else 1.0 for b, h in zip(bs, gn)]
    return bs, mus


def _device_sum(v):
    """the step kernel's sum of one real per sample: thread t adds samples t, t + 256, ... in order, then the fixed tree over 256"""
    part = np.zeros(256)
    for t in range(min(256, len(v))):
        for m in range(t, len(v), 256):
            part[t] = part[t] + v[m]
    o = 128
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return float(part[0])


def _device_dot(u, v):
    return _device_sum(u.real * v.real + u.imag * v.imag)


@pytest.mark.parametrize("steady", MODELS)
def test_the_step_applies_the_magnitude_operator_and_tries_with_the_magnitude_loss(steady):
    """cg = 1, rtol = 0: H p of a running pulse is bloch_gn_batch(magnitude=True)'s on p = b, bit for bit, so gg, rr and d follow
    exactly from that product and the step kernel's arithmetic restated in NumPy, as tests/test_blochlm_gpu.py restates it for the
    component step (the step kernel is that one).  The trial's loss and gradient have the bits of the lsq call at b1 + d."""
    pulses, dfs, dps, D, P, kw, tgs, wts, vs, _, lsq, _ = _case(False, steady)
    _, lsq_fn, gn_fn, _, _, lm_fn = _fns(steady)
    bs = [-g for _, g in lsq]
    hb = gn_fn(pulses, D, P, bs, wts, magnitude=True, **kw)
    mus = _rhs_and_mu(lsq, hb)[1]
    got = lm_fn(pulses, D, P, bs, wts, mus, targets=tgs, cg=1, rtol=0.0, magnitude=True, **kw)
    moved = [(p[0] + d,) + tuple(p[1:]) for p, (d, _) in zip(pulses, got)]
    there = lsq_fn(moved, D, P, tgs, wts, magnitude=True, **kw)
    for q, ((d, i), b, h, mu) in enumerate(zip(got, bs, hb, mus)):
        assert i["loss"] == there[q][0] and np.array_equal(i["grad"], there[q][1]), q
        if not np.any(b):
            continue
        gg = _device_dot(b, b)
        ap = h + mu * b
        alpha = gg / _device_dot(b, ap)
        r = b + (-alpha) * ap
        assert i["gg"] == gg and i["ncg"] == 1, q
        assert np.array_equal(d, 0.0 + alpha * b) and i["rr"] == _device_dot(r, r), q


@pytest.mark.parametrize("steady", MODELS)
def test_refinements_lower_the_magnitude_loss_with_both_solvers(steady, monkeypatch):
    """tests/test_blochlm_gpu.py's case with a magnitude goal: 64 samples, 3 x 33 points, three gains, two outer iterations; |Mxy| = 1
    in the band, 0 outside, a transition band without weight, a tenth of the weight on mz.  What that file holds of the component
    refinements holds here: the device solver's losses fall, its calls are counted, a pulse alone has its bits in the batch, the
    last loss is the lsq call's at the result, and its first step is the host solver's to 1e-4."""
    sc, n, dur = (0.9, 1.0, 1.1), 64, 4e-3
    df, dp = ref._grid(3, 100.0), ref._grid(33, 3.0)
    probs = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        b1 = (np.hanning(n + 2)[1:-1] + 0.1 * rng.standard_normal(n)) * (np.pi / 2 / (ref.GAMMA_H1 * dur / n * np.hanning(n + 2).sum())) + 0j
        p = (b1, np.full(n, 0.05), dur / n, 0.1 if steady else 1.0, 10e-3, "H-1")
        txy = np.where(np.abs(dp) < 1.0, 0.5 if steady else 1.0, 0.0)[None, :] * np.ones((3, 1))
        w = np.where((np.abs(dp) > 0.8) & (np.abs(dp) < 1.2), 0.0, 1.0)[None, :] * np.ones((3, 1))
        probs.append((p, (txy, 1.0 - txy), (w, 0.1 * w)))
    refine = mbfir.refine_bloch_ss_batch if steady else mbfir.refine_bloch_batch
    lm_name, lsq_name = ("bloch_ss_lm_step_batch", "bloch_ss_lsq_batch") if steady else ("bloch_lm_step_batch", "bloch_lsq_batch")
    kw = dict(scales=sc, iters=2, cg=4, magnitude=True)
    args = ([p for p, _, _ in probs], df, dp, [t for _, t, _ in probs], [w for _, _, w in probs])
    steps, trials = [], []
    honest_lm, honest_lsq = getattr(mbfir, lm_name), getattr(mbfir, lsq_name)

    def lm(*a, **k):
        assert k.get("magnitude") is True
        res = honest_lm(*a, **k)
        steps.append([d for d, _ in res])
        return res

    def lsq(pulses, *a, **k):
        assert k.get("magnitude") is True
        trials.append([np.array(p[0]) for p in pulses])
        return honest_lsq(pulses, *a, **k)

    monkeypatch.setattr(mbfir, lm_name, lm)
    b1s, infos = refine(*args, solver="device", **kw)
    first = steps[0]
    for q, (p, t, w) in enumerate(probs):
        L = infos[q]["losses"]
        print("steady %s pulse %d: losses %s, refused %d, calls %s" % (steady, q, ["%.6g" % v for v in L], infos[q]["refused"],
                                                                       infos[q]["calls"]))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), q
        c = infos[q]["calls"]
        assert c["lsq"] == 1 and c["gn"] == 1 and c["lm"] == len(L) - 1 + infos[q]["refused"]
        (r1,), (i1,) = refine([p], df, dp, [t], [w], solver="device", **kw)
        assert np.array_equal(r1, b1s[q]) and i1 == infos[q], q
        (Lend, _), = honest_lsq([(b1s[q],) + p[1:]], df, dp, [t], [w], scales=sc, magnitude=True)
        assert Lend == L[-1]
    monkeypatch.setattr(mbfir, lm_name, honest_lm)
    monkeypatch.setattr(mbfir, lsq_name, lsq)
    _, host = refine(*args, **kw)
    for q, (p, _, _) in enumerate(probs):
        assert host[q]["losses"][-1] < host[q]["losses"][0], q
        d_host = trials[1][q] - p[0]                                # the host solver's second lsq call tries b1 + d
        err = np.abs(first[q] - d_host).max() / np.abs(d_host).max()
        print("steady %s pulse %d: first step of the device solver against the host solver's %.3g" % (steady, q, err))
        assert err <= 1e-4


def test_magnitude_false_is_the_call_without_the_keyword():
    pulses, dfs, dps, m0s, tgs, wts, vs = ref.gnref.cases(False, 1)
    a = mbfir.bloch_lsq_batch(pulses[:4], dfs[:4], dps[:4], tgs[:4], wts[:4], scales=SCALES, m0=m0s[:4])
    b = mbfir.bloch_lsq_batch(pulses[:4], dfs[:4], dps[:4], tgs[:4], wts[:4], scales=SCALES, m0=m0s[:4], magnitude=False)
    assert all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def test_errors_of_the_raw_calls_leave_the_context_usable():
    """The checks are the component calls' with their messages; the one new message is the pair's "only partly given"."""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr

    def L(*v):
        return np.array(v, dtype=np.int64)

    def lp(a):
        return a.ctypes.data_as(mbfir._lp)

    d, one, neg = np.full(64, 1e-5), np.ones(64), np.ones(64)
    neg[5] = -1.0
    outs = [np.zeros(64) for _ in range(3)]
    mu, ints = np.full(4, 0.1), [np.zeros(4, dtype=np.int32) for _ in range(2)]

    def q(t):
        return [p(a) if a is not None else None for a in t]

    def head():
        return [ctx._h, 1, lp(L(0, 3)), p(d), p(d), None, None, None, lp(L(0, 1)), p(d), p(one), p(one), p(one), 1, lp(L(0, 2)), p(d), 1,
                lp(L(0, 3)), p(d), None, None, 1, p(one)]

    def lsq(ss, w=(one, one), t=(d, d), out=outs):
        m0 = [] if ss else [None] * 3
        tail = [None] * 3 if ss else []
        fn = lib.mbfir_bloch_ss_lsq_mag_batch if ss else lib.mbfir_bloch_lsq_mag_batch
        return fn(*head(), *m0, *q(w), *q(t), *q(out), *tail)

    def gn(ss, w=(one, one), ndir=2, v=(d, d), out=outs[:2]):
        fn = lib.mbfir_bloch_ss_gn_mag_batch if ss else lib.mbfir_bloch_gn_mag_batch
        return fn(*head(), *([] if ss else [None] * 3), *q(w), ndir, *q(v), *q(out))

    def lm(ss, w=(one, one), t=(None, None), cg=2):
        fn = lib.mbfir_bloch_ss_lm_step_mag_batch if ss else lib.mbfir_bloch_lm_step_mag_batch
        i32 = [a.ctypes.data_as(mbfir._ip) for a in ints]
        return fn(*head(), *([] if ss else [None] * 3), *q(w), p(d), p(d), p(mu), cg, mbfir.C.c_double(1e-6), *q(t), p(outs[0]),
                  p(outs[1]), i32[0], p(mu.copy()), p(mu.copy()), i32[1], p(outs[2]), p(outs[0].copy()), p(outs[1].copy()))
    for ss, tag in ((False, "bloch_"), (True, "bloch_ss_")):
        for call, who, cases in (
                (lsq, tag + "lsq_mag_batch:", ((dict(w=(one, None)), "plane is null"), (dict(t=(None, d)), "plane is null"),
                                               (dict(w=(neg, one)), "negative or not finite"))),
                (gn, tag + "gn_mag_batch:", ((dict(w=(None, one)), "plane is null"), (dict(w=(one, neg)), "negative or not finite"),
                                             (dict(ndir=0), "ndir must be at least 1"))),
                (lm, tag + "lm_step_mag_batch:", ((dict(w=(one, None)), "plane is null"),
                                                  (dict(t=(d, None)), "txy and tz are given together or not at all"),
                                                  (dict(t=(None, d)), "txy and tz are given together or not at all"),
                                                  (dict(cg=-1), "cg must be at least 0")))):
            assert call(ss) == 0, who
            for kw, why in cases:
                assert call(ss, **kw) == mbfir.E_ARG, (who, kw)
                assert ctx.last_error().startswith(who) and why in ctx.last_error(), (who, kw, ctx.last_error())
            assert call(ss) == 0, who
    assert lm(False, t=(d, d)) == 0 and lm(True, t=(d, d)) == 0
