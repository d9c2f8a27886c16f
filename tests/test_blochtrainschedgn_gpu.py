"""The fused least-squares and Gauss-Newton products of the pulse train's schedule on the device
(mbfir.bloch_train_lsq_sched_batch, mbfir.bloch_train_gn_sched_batch, mbfir.bloch_train_normal_sched_batch:
k_bloch_train_run_sched_lsq, k_bloch_train_run_sched_gn, k_bloch_train_sched_gn_fold with the shipped k_bloch_train_prop and
k_bloch_train_prop_dgain) against the long-double reference of tests/blochtrainschedgn_ref.py, against the shipped two-call paths,
against central differences of the shipped mbfir.bloch_train_batch, for exact zeros and for the bit-invariance of a result under the
batch's composition, the number and place of the directions and the halves asked for; and mbfir.refine_bloch_train_sched_batch on
the device.

Every comparison with the reference is held to the bounds that blochtrainschedgn_ref composes through the seed and fixed on the CPU;
each test prints the share of its bound that the device takes, and DESIGN section 8af quotes the worst ones."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainschedgn_ref", os.path.join(ROOT, "tests", "blochtrainschedgn_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
sched, sj, gnr, tr = ref.sched, ref.sj, ref.gnr, ref.tr
CASES = list(ref.cases())


def _grids(c):
    shared = all(d is c["dfs"][0] for d in c["dfs"]) and len(c["dfs"]) > 1
    return (c["dfs"][0], c["dps"][0]) if shared else (list(c["dfs"]), list(c["dps"]))


def _opt(v):
    return None if v[0] is None else list(v)


def _train_kw(c):
    return dict(phases=list(c["phases"]), gains=list(c["gains"]), echo=list(c["echo"]), scales=c["scales"], m0=_opt(c["m0"]),
                meq=c["meq"], demod=c["demod"])


def _kw(c):
    return dict(_train_kw(c), rep_weights=None if c["rw"] is None else list(c["rw"]), weights_final=_opt(c["wf"]))


def _lsq(c, **over):
    df, dp = _grids(c)
    kw = dict(_kw(c), targets_final=_opt(c["tf"]), grad_m0=True)
    kw.update(over)
    return mbfir.bloch_train_lsq_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["t"]), _opt(c["w"]), **kw)


def _gn(c, dirs, **over):
    """dirs: per pulse (dg, dp), either None for every pulse"""
    df, dp = _grids(c)
    kw = _kw(c)
    kw.update(over)
    tg = None if dirs[0][0] is None else [d[0] for d in dirs]
    tp = None if dirs[0][1] is None else [d[1] for d in dirs]
    return mbfir.bloch_train_gn_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["w"]), tangents_gains=tg, tangents_phases=tp, **kw)


def _sub(c, idx):
    """the pulses idx of a case as a case"""
    d = dict(c)
    for k in ("pulses", "dfs", "dps", "ntr", "phases", "gains", "echo", "m0", "w", "t", "wf", "tf", "ce", "cf"):
        d[k] = [c[k][q] for q in idx]
    d["rw"] = None if c["rw"] is None else [c["rw"][q] for q in idx]
    return d


def _same(a, b):
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and all(np.array_equal(u, v) for u, v in zip(a[3], b[3])))


def _same_h(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _first(dirs, K):
    return [(dg[:K], dp[:K]) for dg, dp in dirs]


@pytest.mark.parametrize("name", CASES + ["small"])
def test_device_loss_gradients_and_products_are_the_longdouble_reference(name):
    c = ref.case_of(name)
    got, want = _lsq(c), ref.reference(name)
    dirs = ref.directions(name, 3)
    hs = {K: _gn(c, _first(dirs, K)) for K in (1, 2, 3)}
    assert len(got) == len(c["pulses"])
    for q, (L, gg, gp, gm) in enumerate(got):
        Lr, ggr, gpr, gmr = want[q]
        n = c["ntr"][q]
        assert gg.shape == gp.shape == (n,) and all(a.shape == b.shape for a, b in zip(gm, gmr)), q
        bg, bp = ref.bound_g(c, q)
        s = dict(L=ref.share(L - Lr, ref.bound_l(c, q)), gg=ref.share(gg - ggr, bg), gp=ref.share(gp - gpr, bp),
                 gm=max(ref.share(a - b, ref.bound_gm(c, q)) for a, b in zip(gm, gmr)))
        (Hg, Hp), (bhg, bhp) = ref.reference_gn(name, 3)[q], ref.bound_h(c, q, *dirs[q])
        assert all(hs[K][q][0].shape == hs[K][q][1].shape == (K, n) for K in (1, 2, 3))
        s["Hg"] = max(ref.share(hs[K][q][0] - Hg[:K], bhg[:K, None]) for K in (1, 2, 3))
        s["Hp"] = max(ref.share(hs[K][q][1] - Hp[:K], bhp[:K, None]) for K in (1, 2, 3))
        print("%s pulse %d: device against long double, shares: %s" % (name, q, ", ".join("%s %.3g" % kv for kv in s.items())))
        assert max(s.values()) <= 1, (q, s)


@pytest.mark.parametrize("name", CASES)
def test_fused_results_against_the_shipped_two_call_paths(name):
    """bloch_train_batch + NumPy + bloch_train_vjp_sched_batch, and bloch_train_jvp_sched_batch + NumPy + bloch_train_vjp_sched_batch"""
    c = ref.cases()[name]
    df, dp = _grids(c)
    P, ntr = len(c["pulses"]), list(c["ntr"])
    fwd = mbfir.bloch_train_batch(c["pulses"], df, dp, ntr, final=True, **_train_kw(c))
    W = [ref.full(c, q, c["w"][q]) for q in range(P)]
    T = [ref.full(c, q, c["t"][q]) for q in range(P)]
    rw = [ref.rw_of(c, q)[None, :, None, None] for q in range(P)]
    echo, final = c["w"][0] is not None, c["wf"][0] is not None
    ce = [tuple(rw[q] * W[q][i] * (fwd[q][0][i] - T[q][i]) for i in range(3)) for q in range(P)] if echo else None
    cf = [tuple(c["wf"][q][i] * (fwd[q][1][i] - c["tf"][q][i]) for i in range(3)) for q in range(P)] if final else None
    two = mbfir.bloch_train_vjp_sched_batch(c["pulses"], df, dp, ntr, ce, cot_final=cf, grad_m0=True, **_train_kw(c))
    got = _lsq(c)
    dirs = ref.directions(name, 2)
    tan = mbfir.bloch_train_jvp_sched_batch(c["pulses"], df, dp, ntr, tangents_gains=[d[0] for d in dirs],
                                            tangents_phases=[d[1] for d in dirs], final=True, **_train_kw(c))
    hv = _gn(c, dirs)
    for q in range(P):
        L2 = 0.0
        if echo:
            L2 += sum(0.5 * float((rw[q] * W[q][i] * (fwd[q][0][i] - T[q][i]) ** 2).sum()) for i in range(3))
        if final:
            L2 += sum(0.5 * float((c["wf"][q][i] * (fwd[q][1][i] - c["tf"][q][i]) ** 2).sum()) for i in range(3))
        bg, bp = ref.bound_g(c, q)
        s = dict(L=ref.share(got[q][0] - L2, ref.bound_l(c, q)), gg=ref.share(got[q][1] - two[q][0], bg),
                 gp=ref.share(got[q][2] - two[q][1], bp),
                 gm=max(ref.share(a - b, ref.bound_gm(c, q)) for a, b in zip(got[q][3], two[q][2])))
        (bhg, bhp), sh = ref.bound_h(c, q, *dirs[q]), 0.0
        s1 = _sub(c, [q])
        for k in range(2):
            cek = [tuple(rw[q] * W[q][i] * tan[q][0][i][k] for i in range(3))] if echo else None
            cfk = [tuple(c["wf"][q][i] * tan[q][1][i][k] for i in range(3))] if final else None
            (h2g, h2p), = mbfir.bloch_train_vjp_sched_batch(s1["pulses"], c["dfs"][q], c["dps"][q], [ntr[q]], cek, cot_final=cfk,
                                                            **_train_kw(s1))
            sh = max(sh, ref.share(hv[q][0][k] - h2g, bhg[k]), ref.share(hv[q][1][k] - h2p, bhp[k]))
        s["Hv"] = sh
        print("%s pulse %d: fused against the two-call paths, shares: %s" % (name, q, ", ".join("%s %.3g" % kv for kv in s.items())))
        assert max(s.values()) <= 1, (q, s)


@pytest.mark.parametrize("name", ["groups", "batch", "allgains", "h1_long", "repeat", "zerogain"])
def test_targets_equal_to_the_trains_own_output_give_a_zero_loss_and_exact_zero_gradients(name):
    c = ref.cases()[name]
    df, dp = _grids(c)
    fwd = mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), final=True, **_train_kw(c))
    over = dict(targets_final=[f for _, f in fwd] if c["wf"][0] is not None else None)
    kw = dict(_kw(c), grad_m0=True, **over)
    w = None if c["w"][0] is None else [ref.full(c, q, c["w"][q]) for q in range(len(c["pulses"]))]
    res = mbfir.bloch_train_lsq_sched_batch(c["pulses"], df, dp, list(c["ntr"]), [e for e, _ in fwd] if w is not None else None, w, **kw)
    for L, gg, gp, gm in res:
        assert L == 0.0 and np.all(gg == 0) and np.all(gp == 0) and all(np.all(v == 0) for v in gm)


@pytest.mark.parametrize("name", gnr.BCAST)
def test_the_broadcast_form_has_the_bits_of_the_full_form_with_the_planes_repeated(name):
    c = ref.cases()[name]
    P = len(c["pulses"])
    rep = dict(c, w=[ref.full(c, q, c["w"][q]) for q in range(P)], t=[ref.full(c, q, c["t"][q]) for q in range(P)])
    assert np.ndim(c["w"][0][0]) == 3 and np.ndim(rep["w"][0][0]) == 4
    dirs = ref.directions(name, 2)
    for a, b in zip(_lsq(c), _lsq(rep)):
        assert _same(a, b)
    for a, b in zip(_gn(c, dirs), _gn(rep, dirs)):
        assert _same_h(a, b)


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_central_difference_of_the_shipped_train_along_the_gradient(name):
    """L through mbfir.bloch_train_batch and NumPy at the schedule moved along the normalised gradient, no repetition turning or
    swinging by more than FD_ANGLE; in units of the scales of the entries moved"""
    c = ref.case_of(name)
    df, dp, n = c["dfs"][0], c["dps"][0], c["ntr"][0]
    (_, gg, gp, _), = _lsq(c)
    norm = np.sqrt((gg ** 2).sum() + (gp ** 2).sum())
    ug, up = gg / norm, gp / norm
    hg, hp = sched.fd_steps(c, 0)
    h = float(min((hg / np.maximum(np.abs(ug), 1e-300)).min(), (hp / np.maximum(np.abs(up), 1e-300)).min()))
    kw = dict(_train_kw(c), echo=c["echo"][0], m0=c["m0"][0])
    W, T, rw = ref.full(c, 0, c["w"][0]), ref.full(c, 0, c["t"][0]), ref.rw_of(c, 0)[None, :, None, None]
    Ls = []
    for s in (1, -1):
        kw.update(gains=c["gains"][0] + s * h * ug, phases=c["phases"][0] + s * h * up)
        (e, f), = mbfir.bloch_train_batch(c["pulses"], df, dp, n, final=True, **kw)
        Ls.append(sum(0.5 * float((rw * W[i] * (e[i] - T[i]) ** 2).sum()) + 0.5 * float((c["wf"][0][i] * (f[i] - c["tf"][0][i]) ** 2).sum())
                      for i in range(3)))
    fd, want = (Ls[0] - Ls[1]) / (2 * h), float((ug * gg).sum() + (up * gp).sum())
    sg, sp = ref.scale_fd(c, 0)
    scale = float(sg * np.abs(ug).sum() + sp * np.abs(up).sum())
    print("%s: central difference along the gradient: %.3g of the scale (FD_TOL %.0e)" % (name, abs(fd - want) / scale, ref.FD_TOL))
    assert abs(fd - want) <= ref.FD_TOL * scale


def test_exact_zeros():
    c = ref.cases()["groups"]
    dirs = ref.directions("groups", 2)
    P = len(c["pulses"])
    none = lambda h: np.all(h[0] == 0) and np.all(h[1] == 0)
    for h in _gn(c, [(np.zeros_like(dg), np.zeros_like(dp)) for dg, dp in dirs]):
        assert none(h)
    zero = lambda tri: tuple(np.zeros_like(v) for v in tri)
    z = dict(c, w=[zero(t) for t in c["w"]], wf=[zero(t) for t in c["wf"]])
    for L, gg, gp, gm in _lsq(z):
        assert L == 0.0 and np.all(gg == 0) and np.all(gp == 0) and all(np.all(v == 0) for v in gm)
    for h in _gn(z, dirs):
        assert none(h)
    norw = dict(c, rw=[np.zeros(n) for n in c["ntr"]], wf=[None] * P, tf=[None] * P)
    for L, gg, gp, gm in _lsq(norw):
        assert L == 0.0 and np.all(gg == 0) and np.all(gp == 0) and all(np.all(v == 0) for v in gm)
    for h in _gn(norw, dirs):
        assert none(h)


def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated():
    c = ref.cases()["groups"]
    dirs = ref.directions("groups", 3)
    alone = [(_lsq(_sub(c, [q]))[0], _gn(_sub(c, [q]), [dirs[q]])[0]) for q in range(3)]
    idx = [k % 3 for k in range(17)]
    for order in (idx, idx[::-1], [1, 1, 1]):
        s = _sub(c, order)
        for q, a, h in zip(order, _lsq(s), _gn(s, [dirs[q] for q in order])):
            assert _same(a, alone[q][0]) and _same_h(h, alone[q][1]), (order, q)


@pytest.mark.parametrize("name", ["allgains", "zerogain", "h1_long"])
def test_a_direction_has_the_same_bits_at_every_place_and_at_every_k(name):
    c = ref.cases()[name]
    dg, dp = ref.directions(name, 3)[0]
    one, = _gn(c, [(dg[2], dp[2])])
    assert one[0].shape == one[1].shape == dg[2].shape
    for K in (1, 2, 3):
        for place in range(K):
            order = [k for k in range(3) if k != 2][:K - 1]
            order.insert(place, 2)
            h, = _gn(c, [(dg[order], dp[order])])
            assert np.array_equal(h[0][place], one[0]) and np.array_equal(h[1][place], one[1]), (K, place)


@pytest.mark.parametrize("name", ["groups", "zerogain", "c13_ramp"])
def test_a_null_half_is_a_half_of_zeros_and_a_wanted_half_does_not_depend_on_the_other(name):
    c = ref.cases()[name]
    dirs = ref.directions(name, 3)
    z = lambda a: np.zeros_like(a)
    # directions: the unit gains direction (0) has a zero phases half, the unit phases direction (1) a zero gains half
    for k, null in ((0, "p"), (1, "g")):
        full = _gn(c, [(dg[k], dp[k]) for dg, dp in dirs], prod_gains=True, prod_phases=True)
        assert all(not (dp[k] if null == "p" else dg[k]).any() for dg, dp in dirs)
        part = _gn(c, [(dg[k], None) if null == "p" else (None, dp[k]) for dg, dp in dirs], prod_gains=True, prod_phases=True)
        for a, b in zip(full, part):
            assert _same_h(a, b), (k, null)
    both = _gn(c, dirs, prod_gains=True, prod_phases=True)
    only_g, only_p = _gn(c, dirs, prod_gains=True, prod_phases=False), _gn(c, dirs, prod_gains=False, prod_phases=True)
    for b, g, p in zip(both, only_g, only_p):
        assert g[1] is None and p[0] is None and np.array_equal(b[0], g[0]) and np.array_equal(b[1], p[1])
    # a phases direction with the phases half alone never launches the period's tangent, and has the same bits
    ph = [(None, dp) for _, dp in dirs]
    for b, p in zip(_gn(c, [(z(dg), dp) for dg, dp in dirs], prod_gains=True, prod_phases=True), _gn(c, ph)):
        assert p[0] is None and np.array_equal(b[1], p[1])
    whole = _lsq(c)
    lg, lp = _lsq(c, grad_phases=False, grad_m0=False), _lsq(c, grad_gains=False)
    for a, g, p in zip(whole, lg, lp):
        assert len(g) == 3 and g[2] is None and p[1] is None
        assert a[0] == g[0] == p[0] and np.array_equal(a[1], g[1]) and np.array_equal(a[2], p[2])
        assert all(np.array_equal(u, v) for u, v in zip(a[3], p[3]))


@pytest.mark.parametrize("name", [n for n in CASES if len(ref.cases()[n]["scales"]) > 1])
def test_each_scale_alone_sums_to_the_sweep_within_the_bound(name):
    c = ref.cases()[name]
    dirs = ref.directions(name, 1)
    whole, hw = _lsq(c), _gn(c, dirs)
    parts = []
    for k, s in enumerate(c["scales"]):
        at = lambda tris: [None if t is None else tuple(np.asarray(v)[k:k + 1] for v in t) for t in tris]
        d = dict(c, scales=(s,), w=at(c["w"]), t=at(c["t"]), wf=at(c["wf"]), tf=at(c["tf"]))
        parts.append((_lsq(d), _gn(d, dirs)))
    for q in range(len(c["pulses"])):
        L, gg, gp = [sum(p[0][q][i] for p in parts) for i in range(3)]
        hg, hp = [sum(p[1][q][i] for p in parts) for i in range(2)]
        (bg, bp), (bhg, bhp) = ref.bound_g(c, q), ref.bound_h(c, q, *dirs[q])
        s = [ref.share(L - whole[q][0], ref.bound_l(c, q)), ref.share(gg - whole[q][1], bg), ref.share(gp - whole[q][2], bp),
             ref.share(hg - hw[q][0], bhg[:, None]), ref.share(hp - hw[q][1], bhp[:, None])]
        print("%s pulse %d: the scales one by one against the sweep, shares: L %.3g, gg %.3g, gp %.3g, Hg %.3g, Hp %.3g" % ((name, q) + tuple(s)))
        assert max(s) <= 1


@pytest.mark.parametrize("name", ["small", "groups", "p65", "zerogain"])
def test_the_products_are_symmetric_and_positive_semidefinite(name):
    c = ref.case_of(name)
    dirs = ref.directions(name, 3)
    for q, (hg, hp) in enumerate(_gn(c, [(dg[1:], dp[1:]) for dg, dp in dirs])):
        u, v = (dirs[q][0][1], dirs[q][1][1]), (dirs[q][0][2], dirs[q][1][2])
        assert abs(ref.pair(u, (hg[1], hp[1])) - ref.pair(v, (hg[0], hp[0]))) <= ref.pair_tol(c, q, u, v)
        assert ref.pair(v, (hg[1], hp[1])) >= -ref.pair_tol(c, q, v, v) / 2
        assert ref.pair(u, (hg[0], hp[0])) >= -ref.pair_tol(c, q, u, u) / 2


@pytest.mark.parametrize("vary", [("gains", "phases"), ("gains",), ("phases",)])
def test_every_row_of_the_normal_matrix_is_its_own_gn_call(vary):
    c = ref.cases()["groups"]
    s = _sub(c, [1, 1])                                                  # two pulses that share ntr = 8
    s["pulses"] = [s["pulses"][0], (s["pulses"][1][0] * 0.9,) + tuple(s["pulses"][1][1:])]
    df, dp = _grids(s)
    n, vg, vp = s["ntr"][0], "gains" in vary, "phases" in vary
    res = mbfir.bloch_train_normal_sched_batch(s["pulses"], df, dp, n, _opt(s["t"]), _opt(s["w"]), vary=vary, targets_final=_opt(s["tf"]),
                                               **_kw(s))
    lsq = _lsq(s, grad_m0=False)
    N = n * len(vary)
    for q, (L, g, H) in enumerate(res):
        assert g.shape == (N,) and H.shape == (N, N)
        assert L == lsq[q][0] and np.array_equal(g, np.concatenate([v for v, on in ((lsq[q][1], vg), (lsq[q][2], vp)) if on]))
        bhg, bhp = ref.bound_h(s, q, *ref.unit_directions(n))
        for j in (0, n - 1, N - 1):
            e = np.zeros(N)
            e[j] = 1.0
            d = (e[:n] if vg else None, e[n:] if vg and vp else e if vp else None)
            (hg, hp), = _gn(_sub(s, [q]), [d], prod_gains=vg, prod_phases=vp)
            assert np.array_equal(H[j], np.concatenate([v for v in (hg, hp) if v is not None])), (q, j)
        if vg and vp:
            tol = np.concatenate([np.repeat(bhg[:, None], n, 1), np.repeat(bhp[:, None], n, 1)], 1)
            assert np.all(np.abs(H - H.T) <= tol + tol.T)
            assert np.linalg.eigvalsh((H + H.T) / 2).min() >= -float((tol + tol.T).sum())


def _raw_tables(ntr, gains, phi, echo, meq):
    uq, gi = np.unique(gains, return_inverse=True)
    tab = [np.array([ntr], dtype=np.int32), np.array([0, ntr], dtype=np.int64), np.cos(phi), np.sin(phi), gi.astype(np.int32),
           np.array([0, len(uq)], dtype=np.int64), uq, np.array([echo], dtype=np.int32), np.array([meq])]
    ip, lp, ptr = (lambda a: a.ctypes.data_as(mbfir._ip)), (lambda a: a.ctypes.data_as(mbfir._lp)), mbfir._ptr
    return tab, [ip(tab[0]), lp(tab[1]), ptr(tab[2]), ptr(tab[3]), ip(tab[4]), lp(tab[5]), ptr(tab[6]), ip(tab[7]), ptr(tab[8])]


def test_outputs_are_written_in_full_and_nowhere_else():
    """The raw calls with NaN sentinels: every entry of the wanted outputs is written, the 16 entries after them are not, unwanted
    halves and dL/dm0 planes are left alone, and the bits are the Python calls'"""
    c = ref.cases()["allgains"]
    p, df, dp, ntr = c["pulses"][0], c["dfs"][0], c["dps"][0], c["ntr"][0]
    S, O = 2, 2 * 6
    dg, dph = ref.directions("allgains", 3)[0]
    wf = tuple(np.full((S, 3, 2), 0.5 + i) for i in range(3))
    tf = tuple(np.full((S, 3, 2), 0.1 * i) for i in range(3))
    d = dict(c, wf=[wf], tf=[tf])
    (Lp, ggp, gpp, gmp), = _lsq(d)
    (hgp, hpp), = _gn(d, [(dg, dph)])
    ctx, lib, ptr = mbfir.get_context(), mbfir.load_library(), mbfir._ptr
    A = mbfir._BlochArgs("raw", [p], df, dp, c["scales"])
    keep, targs = _raw_tables(ntr, c["gains"][0], c["phases"][0], c["echo"][0], c["meq"])
    m0 = A.m0_planes(c["m0"][0], np.array([0, O]), [1])
    flat = lambda tri: [np.ascontiguousarray(np.ravel(v)) for v in tri]
    w, t, wfp, tfp = flat(c["w"][0]), flat(c["t"][0]), flat(wf), flat(tf)
    for want_g, want_p, want_m0 in ((True, True, True), (True, False, False), (False, True, True)):
        loss, gg, gp = np.full(1 + 16, np.nan), np.full(ntr + 16, np.nan), np.full(ntr + 16, np.nan)
        gm = [np.full(O + 16, np.nan) for _ in range(3)]
        rc = lib.mbfir_bloch_train_lsq_sched_batch(ctx._h, *A.head, *targs, int(c["demod"]), *[ptr(a) for a in m0], 0,
                                                   *[ptr(a) for a in w + t], None, *[ptr(a) for a in wfp + tfp], ptr(loss),
                                                   ptr(gg) if want_g else None, ptr(gp) if want_p else None,
                                                   *[ptr(a) if want_m0 else None for a in gm])
        assert rc == 0, ctx.last_error()
        assert loss[0] == Lp and np.all(np.isnan(loss[1:]))
        assert (np.array_equal(gg[:ntr], ggp) and np.all(np.isnan(gg[ntr:]))) if want_g else np.all(np.isnan(gg))
        assert (np.array_equal(gp[:ntr], gpp) and np.all(np.isnan(gp[ntr:]))) if want_p else np.all(np.isnan(gp))
        for a, b in zip(gm, gmp):
            assert (np.array_equal(a[:O], b.ravel()) and np.all(np.isnan(a[O:]))) if want_m0 else np.all(np.isnan(a))
    K = 3
    v = [np.ascontiguousarray(dg.ravel()), np.ascontiguousarray(dph.ravel())]
    for want_g, want_p in ((True, True), (True, False), (False, True)):
        hg, hp = np.full(K * ntr + 16, np.nan), np.full(K * ntr + 16, np.nan)
        rc = lib.mbfir_bloch_train_gn_sched_batch(ctx._h, *A.head, *targs, int(c["demod"]), *[ptr(a) for a in m0], 0,
                                                  *[ptr(a) for a in w], None, *[ptr(a) for a in wfp], K, ptr(v[0]), ptr(v[1]),
                                                  ptr(hg) if want_g else None, ptr(hp) if want_p else None)
        assert rc == 0, ctx.last_error()
        assert (np.array_equal(hg[:K * ntr].reshape(K, ntr), hgp) and np.all(np.isnan(hg[K * ntr:]))) if want_g else np.all(np.isnan(hg))
        assert (np.array_equal(hp[:K * ntr].reshape(K, ntr), hpp) and np.all(np.isnan(hp[K * ntr:]))) if want_p else np.all(np.isnan(hp))


def test_refine_on_the_device_lowers_the_loss_and_a_pulse_alone_has_its_bits_in_a_batch():
    """the 9-sample period, 3 x 2 points, 9 repetitions, three gains, two outer iterations"""
    c = ref.small()
    p = c["pulses"][0]
    rng = np.random.default_rng(5)
    ntr, gains = 9, np.tile([0.5, 0.75, 1.0], 3)
    pulses = [(p[0] * s,) + tuple(p[1:]) for s in (1.0, 0.9, 1.1)]
    w = (np.ones((3, 2)), np.ones((3, 2)), 0.5)
    tg = tuple(rng.uniform(-0.5, 0.5, (3, 2)) for _ in range(3))
    rw = np.r_[0.0, 0.0, np.ones(7)]
    kw = dict(rep_weights=rw, phases=np.pi, gains=gains, echo=c["echo"][0], m0=c["m0"][0], demod=True, iters=2)
    for vary in (("gains", "phases"), ("gains",)):
        sch, infos = mbfir.refine_bloch_train_sched_batch(pulses, c["dfs"][0], c["dps"][0], ntr, [tg] * 3, [w] * 3, vary=vary, **kw)
        for q in range(3):
            L = infos[q]["losses"]
            assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
            assert sch[q][0].shape == sch[q][1].shape == (ntr,)
            if "phases" not in vary:
                assert np.array_equal(sch[q][1], np.pi * np.arange(ntr))
            (one,), (info,) = mbfir.refine_bloch_train_sched_batch([pulses[q]], c["dfs"][0], c["dps"][0], ntr, [tg], [w], vary=vary, **kw)
            assert np.array_equal(one[0], sch[q][0]) and np.array_equal(one[1], sch[q][1]) and info["losses"] == L


def test_errors_of_the_raw_calls_leave_the_context_usable():
    """Every MBFIR_E_ARG case of the two raw calls with its message, a good call before and after; every case returns before any
    device work"""
    ctx = mbfir.get_context()
    lib, p = mbfir.load_library(), mbfir._ptr
    L = lambda *v: np.array(v, dtype=np.int64)
    I = lambda *v: np.array(v, dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(mbfir._lp)
    ip = lambda a: a.ctypes.data_as(mbfir._ip)
    d, one = np.full(64, 1e-5), np.ones(64)
    neg, nan = np.r_[one[:5], -1.0, one[:58]], np.r_[one[:5], np.nan, one[:58]]
    rneg, rnan = np.r_[1.0, -1.0, one[:62]], np.r_[1.0, 1.0, 1.0, np.inf, one[:60]]
    outs = [np.zeros(64) for _ in range(6)]
    N3, N6 = (None,) * 3, (None,) * 6

    def opt(a, f=p):
        return f(a) if a is not None else None

    def head(npulse, toff, tsoff, nfgrid, foff, npgrid, poff, nscale, ntr, roff, echo):
        return (ctx._h, npulse, lp(toff), p(d), p(d), None, None, None, lp(tsoff), p(d), p(one), p(one), p(one), nfgrid, lp(foff), p(d),
                npgrid, lp(poff), p(d), None, None, nscale, p(one), opt(ntr, ip), lp(roff), p(one), p(np.zeros(64)), ip(I(0, 1, 1, 0)),
                lp(L(0, 2)), p(np.array([0.5, 1.0])), opt(echo, ip), p(one), 0, None, None, None)

    def lsq(npulse=1, toff=L(0, 3), tsoff=L(0, 1), nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, ntr=I(4), roff=L(0, 4),
            echo=I(2), ebcast=0, wt=(one,) * 6, rw=None, wtf=(one,) * 6, loss=outs[0], g=(outs[1], outs[2]), gm=tuple(outs[3:6])):
        return lib.mbfir_bloch_train_lsq_sched_batch(*head(npulse, toff, tsoff, nfgrid, foff, npgrid, poff, nscale, ntr, roff, echo),
                                                     ebcast, *[opt(a) for a in wt], opt(rw), *[opt(a) for a in wtf], opt(loss),
                                                     *[opt(a) for a in g], *[opt(a) for a in gm])

    def gn(npulse=1, toff=L(0, 3), tsoff=L(0, 1), nfgrid=1, foff=L(0, 2), npgrid=1, poff=L(0, 3), nscale=1, ntr=I(4), roff=L(0, 4),
           echo=I(2), ebcast=0, w=(one,) * 3, rw=None, wf=(one,) * 3, ndir=2, v=(d, d), h=(outs[1], outs[2])):
        return lib.mbfir_bloch_train_gn_sched_batch(*head(npulse, toff, tsoff, nfgrid, foff, npgrid, poff, nscale, ntr, roff, echo),
                                                    ebcast, *[opt(a) for a in w], opt(rw), *[opt(a) for a in wf], ndir,
                                                    *[opt(a) for a in v], *[opt(a) for a in h])
    big = 2 ** 31 - 1
    shared = ((dict(npulse=0), "no pulses"), (dict(echo=I(4)), "echo of pulse 0 must lie in [0, ntime]"),
              (dict(ntr=I(0), roff=L(0, 0)), "ntr of pulse 0 must be at least 1"), (dict(ebcast=2), "ebcast must be 0 or 1"),
              (dict(ebcast=-1), "ebcast must be 0 or 1"), (dict(rw=rneg), "a repetition weight is negative or not finite"),
              (dict(rw=rnan), "a repetition weight is negative or not finite"))
    lsq_cases = shared + ((dict(wt=(one, None) + (one,) * 4), "the echo weights and targets are given together"),
                          (dict(wt=(one,) * 5 + (None,)), "the echo weights and targets are given together"),
                          (dict(wtf=(None,) + (one,) * 5), "the final weights and targets are given together"),
                          (dict(wt=N6, wtf=N6), "neither an echo term nor a final term"), (dict(loss=None), "the loss plane is null"),
                          (dict(g=(None, None)), "neither the gradient in the gains nor the gradient in the phases is wanted"),
                          (dict(gm=(outs[3], None, outs[5])), "gmx, gmy and gmz"), (dict(wt=(neg,) + (one,) * 5), "a weight is negative"),
                          (dict(wtf=(one, nan) + (one,) * 4), "a weight is negative or not finite"),
                          (dict(ebcast=1, wt=(one, one, neg) + (one,) * 3), "a weight is negative"))
    gn_cases = shared + ((dict(w=(one, None, one)), "the echo weights are given together"),
                         (dict(wf=(None, one, one)), "the final weights are given together"),
                         (dict(w=N3, wf=N3), "neither an echo term nor a final term"),
                         (dict(h=(None, None)), "neither the product's gains half nor its phases half is wanted"),
                         (dict(v=(None, None)), "no direction is given"), (dict(ndir=0), "ndir must be at least 1"),
                         (dict(ndir=-3), "ndir must be at least 1"), (dict(w=(one, neg, one)), "a weight is negative"),
                         (dict(wf=(nan, one, one)), "a weight is negative or not finite"),
                         # 2^30 points, 2^31 - 1 or 2^21 directions: the workgroups and the checkpoints overflow before a plane is read
                         (dict(ndir=big, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"),
                         (dict(ndir=2 ** 21, foff=L(0, 2 ** 15), poff=L(0, 2 ** 15)), "overflows"))
    for call, who, cases in ((lsq, "bloch_train_lsq_sched_batch:", lsq_cases), (gn, "bloch_train_gn_sched_batch:", gn_cases)):
        assert call() == 0, ctx.last_error()
        for kw, why in cases:
            assert call(**kw) == mbfir.E_ARG, kw
            assert ctx.last_error().startswith(who) and why in ctx.last_error(), (kw, ctx.last_error())
        assert call() == 0
    assert lsq(wt=N6) == 0 and lsq(wtf=N6) == 0 and lsq(gm=N3) == 0 and lsq(ebcast=1) == 0 and lsq(rw=one) == 0
    assert lsq(g=(outs[1], None)) == 0 and lsq(g=(None, outs[2])) == 0
    assert gn(w=N3) == 0 and gn(wf=N3) == 0 and gn(ebcast=1, rw=one) == 0
    assert gn(v=(d, None)) == 0 and gn(v=(None, d)) == 0 and gn(h=(outs[1], None)) == 0 and gn(h=(None, outs[2]), v=(None, d)) == 0
    hd = head(1, L(0, 3), L(0, 1), 1, L(0, 2), 1, L(0, 3), 1, I(4), L(0, 4), I(2))[1:]
    assert lib.mbfir_bloch_train_lsq_sched_batch(None, *hd, 0, *[p(one)] * 6, None, *[p(one)] * 6, p(outs[0]), p(outs[1]), p(outs[2]),
                                                 None, None, None) == mbfir.E_ARG
    assert lib.mbfir_bloch_train_gn_sched_batch(None, *hd, 0, *[p(one)] * 3, None, *[p(one)] * 3, 2, p(d), p(d), p(outs[1]),
                                                p(outs[2])) == mbfir.E_ARG
    # a good call after the refused ones is correct: the Python call on the same inputs gives the same bits
    pulse = (d[:3] * (1 + 1j), None, 1e-5, 1.0, 1.0, 1.0)
    kw = dict(phases=0.0, gains=np.array([0.5, 1.0, 1.0, 0.5]), echo=2)
    (Lw, ggw, gpw, gmw), = mbfir.bloch_train_lsq_sched_batch([pulse], d[:2], d[:3], 4, [(1.0, 1.0, 1.0)], [(1.0, 1.0, 1.0)],
                                                            targets_final=[(1.0,) * 3], weights_final=[(1.0,) * 3], grad_m0=True, **kw)
    assert lsq() == 0
    assert outs[0][0] == Lw and np.array_equal(outs[1][:4], ggw) and np.array_equal(outs[2][:4], gpw)
    assert all(np.array_equal(o[:6], m.ravel()) for o, m in zip(outs[3:6], gmw))
    v = np.stack([d[:4], d[4:8]])
    (hgw, hpw), = mbfir.bloch_train_gn_sched_batch([pulse], d[:2], d[:3], 4, [(1.0, 1.0, 1.0)], tangents_gains=[v], tangents_phases=[v],
                                                   weights_final=[(1.0,) * 3], **kw)
    assert gn() == 0
    assert np.array_equal(outs[1][:8].reshape(2, 4), hgw) and np.array_equal(outs[2][:8].reshape(2, 4), hpw)
