"""The magnitude fits of the pulse train on the device (magnitude=True of mbfir.bloch_train_lsq_batch, bloch_train_gn_batch,
bloch_train_lm_step_batch, their _sched twins, bloch_train_normal_sched_batch and the four train refiners: the kernels
k_bloch_train_run_lsq_mag, k_bloch_train_run_gn_mag, k_bloch_train_lm_run_mag and their _sched twins) against the
long-double reference of tests/blochtrainmag_ref.py, against the shipped component calls at the phase-projected target, against
the shipped two-call path jvp -> host seed -> vjp, and for the exact properties: zero loss at the train's own magnitudes, rho = 0,
exact zeros, and the bit-invariance of a result under the batch's composition, K, a direction's place and the halves asked for.

"b1" is the chain in the period's b1, "sched" the chain in the schedule.  Every comparison with
the reference is held to the bounds that blochtrainmag_ref composes through the seed and fixed on the CPU; each test prints the
share of its bound that the device takes, and DESIGN section 8ai quotes the worst ones."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("blochtrainmag_ref")
lmref = _load("blochtrainschedlm_ref")
gnr, sgr = ref.gnr, ref.sgr
ALL = [(ch, n) for ch in ref.CHAINS for n in ref.cases(ch)]
FULL = [(ch, n) for ch, n in ALL if not ref.cases(ch)[n]["bcast"]]


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


def _lsq(chain, c, magnitude=True, **over):
    """per pulse (L, [the gradients: g, or gg and gp], gm)"""
    df, dp = _grids(c)
    kw = dict(_kw(c), targets_final=_opt(c["tf"]), grad_m0=True, magnitude=magnitude)
    kw.update(over)
    fn = mbfir.bloch_train_lsq_batch if chain == "b1" else mbfir.bloch_train_lsq_sched_batch
    return [(r[0], list(r[1:-1]), r[-1]) for r in fn(c["pulses"], df, dp, list(c["ntr"]), _opt(c["t"]), _opt(c["w"]), **kw)]


def _gn(chain, c, dirs, magnitude=True, **over):
    """per pulse the list of the product's parts: [H v], or [Hg, Hp]"""
    df, dp = _grids(c)
    kw = dict(_kw(c), magnitude=magnitude)
    kw.update(over)
    if chain == "b1":
        return [[h] for h in mbfir.bloch_train_gn_batch(c["pulses"], df, dp, list(c["ntr"]), list(dirs), _opt(c["w"]), **kw)]
    tg = None if dirs[0][0] is None else [d[0] for d in dirs]
    tp = None if dirs[0][1] is None else [d[1] for d in dirs]
    return [list(h) for h in mbfir.bloch_train_gn_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["w"]), tangents_gains=tg,
                                                               tangents_phases=tp, **kw)]


def _first(chain, dirs, K):
    return [v[:K] for v in dirs] if chain == "b1" else [(dg[:K], dp[:K]) for dg, dp in dirs]


def _pick(chain, d, idx):
    """the directions idx of one pulse's directions"""
    return d[idx] if chain == "b1" else (d[0][idx], d[1][idx])


def _bg(chain, c, q):
    b = ref.bound_g(chain, c, q)
    return [b] if chain == "b1" else list(b)


def _bh(chain, c, q, v):
    b = ref.bound_h(chain, c, q, v)
    return [b] if chain == "b1" else [b[0][:, None], b[1][:, None]]


def _parts(chain, x):
    return [x] if chain == "b1" else list(x)


def _sub(c, idx):
    d = dict(c)
    for k in ("pulses", "dfs", "dps", "ntr", "phases", "gains", "echo", "m0", "w", "t", "wf", "tf", "ce", "cf"):
        d[k] = [c[k][q] for q in idx]
    d["rw"] = None if c["rw"] is None else [c["rw"][q] for q in idx]
    return d


def _same(a, b):
    return (a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))
            and all(np.array_equal(u, v) for u, v in zip(a[2], b[2])))


def _same_h(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


def _zero(res):
    L, gs, gm = res
    return L == 0.0 and all(np.all(g == 0) for g in gs) and all(np.all(v == 0) for v in gm)


def _forward(c):
    df, dp = _grids(c)
    return mbfir.bloch_train_batch(c["pulses"], df, dp, list(c["ntr"]), final=True, **_train_kw(c))


def _mags(tri):
    """(np.sqrt(ex * ex + ey * ey), ez) of a triple of the forward call's output"""
    return (np.sqrt(tri[0] * tri[0] + tri[1] * tri[1]), tri[2])


@pytest.mark.parametrize("chain,name", ALL + [(ch, "small") for ch in ref.CHAINS] + [("sched", "z0")])
def test_device_loss_gradients_and_products_are_the_longdouble_reference(chain, name):
    c = ref.bounded(chain, name)
    got, want = _lsq(chain, c), ref.reference(chain, name)
    dirs = ref.directions(chain, name, 3)
    hs = {K: _gn(chain, c, _first(chain, dirs, K)) for K in (1, 2, 3)}
    assert len(got) == len(c["pulses"])
    for q, (L, gs, gm) in enumerate(got):
        Lr, grs, gmr = want[q][0], list(want[q][1:-1]), want[q][-1]
        assert all(a.shape == b.shape for a, b in zip(gs + list(gm), grs + list(gmr))), q
        s = dict(L=ref.share(L - Lr, ref.bound_l(c, q)), gm=max(ref.share(a - b, ref.bound_gm(c, q)) for a, b in zip(gm, gmr)))
        s["g"] = max(ref.share(a - b, bd) for a, b, bd in zip(gs, grs, _bg(chain, c, q)))
        H, bh = _parts(chain, ref.reference_gn(chain, name, 3)[q]), _bh(chain, c, q, dirs[q])
        s["Hv"] = max(ref.share(h - Hr, b) for h, Hr, b in zip(hs[3][q], H, bh))
        for K in (1, 2):                                                        # K = 1 and 2 have K = 3's bits
            assert all(np.array_equal(a, b[:K]) for a, b in zip(hs[K][q], hs[3][q])), (q, K)
        print("%s %s pulse %d: device against long double, shares: %s" % (chain, name, q, ", ".join("%s %.3g" % kv for kv in s.items())))
        assert max(s.values()) <= 1, (q, s)
    if name == "z0":                                                            # the magnitude loss does not see a common phase
        gp, bp = got[0][1][1], ref.bound_g(chain, c, 0)[1]
        print("z0: sum of dL/dphases %.3g of %.3g" % (abs(gp.sum()), bp * len(gp)))
        assert abs(gp.sum()) <= bp * len(gp)


@pytest.mark.parametrize("chain,name", ALL)
def test_loss_and_gradient_are_the_component_calls_at_the_phase_projected_target(chain, name):
    """L and g against the shipped component call (magnitude=False) at t = (t_xy u_x, t_xy u_y, t_z), w = (w_xy, w_xy, w_z), u the
    direction of bloch_train_batch's own echoes and final state, in the full echo form.  Both calls form their residual from the same
    device echo, (rho - t_xy) u against e - t_xy u, so they differ by the two calls' own errors: the magnitude bound plus the
    component reference's bound at the projected case."""
    c = ref.bounded(chain, name)
    fwd = _forward(c)
    comp = c
    for q in range(len(c["pulses"])):
        comp = ref.projected(comp, q, *fwd[q])
    got, want = _lsq(chain, c), _lsq(chain, comp, magnitude=False)
    src = gnr if chain == "b1" else sgr
    for q, ((L, gs, gm), (Lc, gcs, gmc)) in enumerate(zip(got, want)):
        bc = src.bound_g(comp, q)
        bc = [bc] if chain == "b1" else list(bc)
        s = dict(L=ref.share(L - Lc, ref.bound_l(c, q) + src.bound_l(comp, q)),
                 g=max(ref.share(a - b, x + y) for a, b, x, y in zip(gs, gcs, _bg(chain, c, q), bc)),
                 gm=max(ref.share(a - b, ref.bound_gm(c, q) + src.bound_gm(comp, q)) for a, b in zip(gm, gmc)))
        print("%s %s pulse %d: magnitude against component at the projected target, shares: %s"
              % (chain, name, q, ", ".join("%s %.3g" % kv for kv in s.items())))
        assert max(s.values()) <= 1, (q, s)


@pytest.mark.parametrize("chain,name", ALL)
def test_products_against_the_shipped_tangent_a_host_seed_and_the_shipped_adjoint(chain, name):
    c = ref.bounded(chain, name)
    df, dp = _grids(c)
    P, ntr = len(c["pulses"]), list(c["ntr"])
    fwd = _forward(c)
    dirs = ref.directions(chain, name, 2)
    if chain == "b1":
        tan = mbfir.bloch_train_jvp_batch(c["pulses"], df, dp, ntr, list(dirs), final=True, **_train_kw(c))
    else:
        tan = mbfir.bloch_train_jvp_sched_batch(c["pulses"], df, dp, ntr, tangents_gains=[d[0] for d in dirs],
                                                tangents_phases=[d[1] for d in dirs], final=True, **_train_kw(c))
    hv = _gn(chain, c, dirs)
    echo, final = c["w"][0] is not None, c["wf"][0] is not None
    for q in range(P):
        W, rw = ref.full(c, q, c["w"][q]), ref.rw_of(c, q)[None, :, None, None]
        bh, sh = _bh(chain, c, q, dirs[q]), 0.0
        s1 = _sub(c, [q])
        for k in range(2):
            cek = cfk = None
            if echo:
                _, ux, uy = ref.mag_dir(fwd[q][0][0], fwd[q][0][1])
                a = ux * tan[q][0][0][k] + uy * tan[q][0][1][k]
                cek = [(rw * W[0] * a * ux, rw * W[0] * a * uy, rw * W[1] * tan[q][0][2][k])]
            if final:
                _, ux, uy = ref.mag_dir(fwd[q][1][0], fwd[q][1][1])
                a = ux * tan[q][1][0][k] + uy * tan[q][1][1][k]
                cfk = [(c["wf"][q][0] * a * ux, c["wf"][q][0] * a * uy, c["wf"][q][1] * tan[q][1][2][k])]
            fn = mbfir.bloch_train_vjp_batch if chain == "b1" else mbfir.bloch_train_vjp_sched_batch
            h2, = fn(s1["pulses"], c["dfs"][q], c["dps"][q], [ntr[q]], cek, cot_final=cfk, **_train_kw(s1))
            sh = max([sh] + [ref.share(h[k] - x, b[k]) for h, x, b in zip(hv[q], _parts(chain, h2), bh)])
        print("%s %s pulse %d: fused products against jvp, host seed, vjp: share %.3g" % (chain, name, q, sh))
        assert sh <= 1, (q, sh)


@pytest.mark.parametrize("chain,name", FULL)
def test_the_trains_own_magnitudes_give_a_zero_loss_and_exact_zero_gradients(chain, name):
    """t_xy = np.sqrt(ex * ex + ey * ey), t_z = e_z of bloch_train_batch's own output under the same demod, the full echo form"""
    c = ref.cases(chain)[name]
    fwd = _forward(c)
    own = dict(c, t=[_mags(e) if c["w"][0] is not None else None for e, _ in fwd],
               w=[None if w is None else ref.full(c, q, w) for q, w in enumerate(c["w"])],
               tf=[_mags(f) if c["wf"][0] is not None else None for _, f in fwd])
    for res in _lsq(chain, own):
        assert _zero(res)


@pytest.mark.parametrize("chain", ref.CHAINS)
@pytest.mark.parametrize("name", gnr.BCAST)
def test_the_broadcast_form_at_one_repetitions_own_magnitudes(chain, name):
    """The broadcast form: with rep_weights zero but for the last repetition, point-sized targets equal to that echo's own
    magnitudes give L == 0.0 and exact zeros; and the broadcast form has the bits of the full form with the planes repeated."""
    c = ref.cases(chain)[name]
    P = len(c["pulses"])
    assert c["bcast"] and np.ndim(c["w"][0][0]) == 3
    fwd = _forward(c)
    last = [np.r_[np.zeros(n - 1), 1.0] for n in c["ntr"]]
    own = dict(c, rw=last, t=[_mags([v[:, -1] for v in e]) for e, _ in fwd],
               tf=[_mags(f) if c["wf"][0] is not None else None for _, f in fwd])
    for res in _lsq(chain, own):
        assert _zero(res)
    rep = dict(c, w=[ref.full(c, q, c["w"][q]) for q in range(P)], t=[ref.full(c, q, c["t"][q]) for q in range(P)])
    assert np.ndim(rep["w"][0][0]) == 4
    dirs = ref.directions(chain, name, 2)
    assert all(_same(a, b) for a, b in zip(_lsq(chain, c), _lsq(chain, rep)))
    assert all(_same_h(a, b) for a, b in zip(_gn(chain, c, dirs), _gn(chain, rep, dirs)))


@pytest.mark.parametrize("chain,name", [("b1", "groups"), ("b1", "p65"), ("sched", "groups"), ("sched", "zerogain")])
def test_rho_zero_adds_half_w_t_squared_to_the_loss_and_exact_zeros_elsewhere(chain, name):
    """b1 = 0 and m0 = (0, 0, 1): rho = 0 at every echo and at the final state.  L is finite, g and H v have the bits of the same call
    with w_xy = 0, and L exceeds that call's by 1/2 sum rw w_xy t_xy^2 to rounding"""
    c = ref.cases(chain)[name]
    P = len(c["pulses"])
    rest = dict(c, pulses=[(np.zeros_like(p[0]),) + tuple(p[1:]) for p in c["pulses"]], m0=[None] * P)
    off = lambda pairs: [None if p is None else (np.zeros_like(p[0]), p[1]) for p in pairs]
    noxy = dict(rest, w=off(c["w"]), wf=off(c["wf"]))
    dirs = ref.directions(chain, name, 2)
    for q, (a, b) in enumerate(zip(_lsq(chain, rest), _lsq(chain, noxy))):
        extra, S = 0.0, len(c["scales"])
        if c["w"][q] is not None:
            W, T = ref.full(c, q, c["w"][q]), ref.full(c, q, c["t"][q])
            extra += 0.5 * float((ref.rw_of(c, q)[None, :, None, None] * W[0] * T[0] * T[0]).sum())
        if c["wf"][q] is not None:
            extra += 0.5 * float((c["wf"][q][0] * c["tf"][q][0] ** 2).sum())
        assert np.isfinite(a[0]) and extra > 0 and S >= 1
        assert all(np.array_equal(u, v) for u, v in zip(a[1] + list(a[2]), b[1] + list(b[2]))), q
        assert abs(a[0] - b[0] - extra) <= 1e-12 * (abs(a[0]) + extra), (q, a[0], b[0], extra)
    assert all(_same_h(a, b) for a, b in zip(_gn(chain, rest, dirs), _gn(chain, noxy, dirs)))


@pytest.mark.parametrize("chain,name", [("b1", "groups"), ("b1", "p65"), ("b1", "h1_long"), ("sched", "groups"), ("sched", "p65"),
                                        ("sched", "h1_long")])
def test_exact_zeros(chain, name):
    """zero weights, a zero direction and rep_weights of zeros; p65 and h1_long (300 points) have the dead threads of a 256-point chunk"""
    c = ref.cases(chain)[name]
    dirs = ref.directions(chain, name, 2)
    P = len(c["pulses"])
    none = lambda h: all(np.all(x == 0) for x in h)
    zdir = [np.zeros_like(v) for v in dirs] if chain == "b1" else [(np.zeros_like(dg), np.zeros_like(dp)) for dg, dp in dirs]
    assert all(none(h) for h in _gn(chain, c, zdir))
    zero = lambda pairs: [None if p is None else tuple(np.zeros_like(v) for v in p) for p in pairs]
    z = dict(c, w=zero(c["w"]), wf=zero(c["wf"]))
    assert all(_zero(r) for r in _lsq(chain, z)) and all(none(h) for h in _gn(chain, z, dirs))
    if c["w"][0] is not None:
        norw = dict(c, rw=[np.zeros(n) for n in c["ntr"]], wf=[None] * P, tf=[None] * P)
        assert all(_zero(r) for r in _lsq(chain, norw)) and all(none(h) for h in _gn(chain, norw, dirs))


@pytest.mark.parametrize("chain", ref.CHAINS)
def test_a_pulse_has_the_same_bits_alone_in_17_reversed_and_repeated(chain):
    c = ref.cases(chain)["groups"]
    dirs = ref.directions(chain, "groups", 3)
    alone = [(_lsq(chain, _sub(c, [q]))[0], _gn(chain, _sub(c, [q]), [dirs[q]])[0]) for q in range(3)]
    idx = [k % 3 for k in range(17)]
    for order in (idx, idx[::-1], [1, 1, 1]):
        s = _sub(c, order)
        for q, a, h in zip(order, _lsq(chain, s), _gn(chain, s, [dirs[q] for q in order])):
            assert _same(a, alone[q][0]) and _same_h(h, alone[q][1]), (order, q)


@pytest.mark.parametrize("chain,name", [("b1", "allgains"), ("b1", "h1_long"), ("sched", "allgains"), ("sched", "zerogain")])
def test_a_direction_has_the_same_bits_at_every_place_and_at_every_k(chain, name):
    c = ref.cases(chain)[name]
    d = ref.directions(chain, name, 3)[0]
    one, = _gn(chain, c, [_pick(chain, d, 2)])
    for K in (1, 2, 3):
        for place in range(K):
            order = [k for k in range(3) if k != 2][:K - 1]
            order.insert(place, 2)
            h, = _gn(chain, c, [_pick(chain, d, order)])
            assert all(np.array_equal(x[place], y) for x, y in zip(h, one)), (K, place)


@pytest.mark.parametrize("name", ["groups", "zerogain", "c13_ramp"])
def test_a_half_of_the_schedule_does_not_depend_on_the_other(name):
    c = ref.cases("sched")[name]
    dirs = ref.directions("sched", name, 3)
    for k, null in ((0, "p"), (1, "g")):                                        # unit directions: one half is zero
        both = _gn("sched", c, [(dg[k], dp[k]) for dg, dp in dirs], prod_gains=True, prod_phases=True)
        part = _gn("sched", c, [(dg[k], None) if null == "p" else (None, dp[k]) for dg, dp in dirs], prod_gains=True, prod_phases=True)
        assert all(_same_h(a, b) for a, b in zip(both, part)), (k, null)
    both = _gn("sched", c, dirs, prod_gains=True, prod_phases=True)
    only_g, only_p = _gn("sched", c, dirs, prod_gains=True, prod_phases=False), _gn("sched", c, dirs, prod_gains=False, prod_phases=True)
    for b, g, p in zip(both, only_g, only_p):
        assert g[1] is None and p[0] is None and np.array_equal(b[0], g[0]) and np.array_equal(b[1], p[1])
    whole = _lsq("sched", c)
    lg, lp = _lsq("sched", c, grad_phases=False), _lsq("sched", c, grad_gains=False)
    for a, g, p in zip(whole, lg, lp):
        assert g[1][1] is None and p[1][0] is None and a[0] == g[0] == p[0]
        assert np.array_equal(a[1][0], g[1][0]) and np.array_equal(a[1][1], p[1][1])
        assert all(np.array_equal(u, v) for u, v in zip(a[2], p[2]))


# ---- the device steps ---------------------------------------------------------------------------------------------------------
def _device_sum(v):
    """the step kernels' sum of one real per entry: thread t adds entries t, t + 256, ... in order, then the fixed tree over 256"""
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


def _lm(chain, c, bs, mus, targets=True, **over):
    """per pulse (d, info); sched: d, b and the gradient as gains + i phases"""
    df, dp = _grids(c)
    kw = dict(_kw(c), magnitude=True, targets=_opt(c["t"]) if targets else None, targets_final=_opt(c["tf"]) if targets else None)
    kw.update(over)
    if chain == "b1":
        return mbfir.bloch_train_lm_step_batch(c["pulses"], df, dp, list(c["ntr"]), bs, _opt(c["w"]), mus, **kw)
    res = mbfir.bloch_train_lm_step_sched_batch(c["pulses"], df, dp, list(c["ntr"]), _opt(c["w"]), mus,
                                                b=None if bs is None else [(b.real.copy(), b.imag.copy()) for b in bs], **kw)
    out = []
    for dg, dp_, info in res:
        if "loss" in info:
            info = dict(info, grad=info["grad_gains"] + 1j * info["grad_phases"])
        out.append((dg + 1j * dp_, info))
    return out


def _cx(chain, parts):
    return parts[0] if chain == "b1" else parts[0] + 1j * parts[1]


@pytest.mark.parametrize("chain,name", [("b1", "groups"), ("b1", "batch"), ("b1", "p65"), ("sched", "groups"), ("sched", "batch"),
                                        ("sched", "p65"), ("sched", "zerogain")])
def test_the_steps_first_product_and_its_trial_have_the_fused_calls_bits(chain, name):
    """cg = 1, rtol = 0, b = -g: H p of the step is the magnitude gn call's on p = b, bit for bit, so gg, d and rr follow from one
    product and the step kernel's arithmetic restated in NumPy.  The trial (b1: loss and gradient at b1 + d) or the evaluation (sched:
    at the call's schedule) has the magnitude lsq call's bits."""
    c = ref.cases(chain)[name]
    at = _lsq(chain, c)
    bs = [-_cx(chain, gs) for _, gs, _ in at]
    mus = [1e-3 * (1 + q) for q in range(len(bs))]
    dirs = bs if chain == "b1" else [(b.real.copy(), b.imag.copy()) for b in bs]
    got = _lm(chain, c, bs, mus, cg=1, rtol=0.0)
    for q, ((d, i), b, h, mu) in enumerate(zip(got, bs, _gn(chain, c, dirs), mus)):
        hb = _cx(chain, h)
        gg = _device_dot(b, b)
        ap = hb + mu * b
        alpha = gg / _device_dot(b, ap)
        r = b + (-alpha) * ap
        assert i["gg"] == gg and i["ncg"] == 1, q
        assert np.array_equal(d, 0.0 + alpha * b) and i["rr"] == _device_dot(r, r), q
    if chain == "b1":
        moved = dict(c, pulses=[(p[0] + d,) + tuple(p[1:]) for p, (d, _) in zip(c["pulses"], got)])
        there = _lsq(chain, moved)
    else:
        there = at
    for (d, i), (L, gs, _) in zip(got, there):
        assert i["loss"] == L and np.array_equal(i["grad"], _cx(chain, gs))


def _refine_case():
    """the refine shape of the component tests: the 9-sample period, 3 x 2 points, 9 repetitions, three gains, three pulses, with
    pairs: one constant |Mxy| per point over the echoes; also as a case of the reference (the broadcast form)"""
    c0 = gnr.small()
    p = c0["pulses"][0]
    rng = np.random.default_rng(5)
    ntr, gains = 9, np.tile([0.5, 0.75, 1.0], 3)
    pulses = [(p[0] * s,) + tuple(p[1:]) for s in (1.0, 0.9, 1.1)]
    w = (np.ones((3, 2)), 0.5)
    tg = (rng.uniform(0.1, 0.6, (3, 2)), rng.uniform(-0.5, 0.5, (3, 2)))
    rw = np.r_[0.0, 0.0, np.ones(7)]
    kw = dict(rep_weights=rw, phases=np.pi, gains=gains, echo=c0["echo"][0], m0=c0["m0"][0], demod=True, magnitude=True)
    args = (c0["dfs"][0], c0["dps"][0], ntr)
    plane = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (1, 3, 2)).copy()
    case = dict(pulses=pulses, dfs=[c0["dfs"][0]] * 3, dps=[c0["dps"][0]] * 3, ntr=[ntr] * 3, phases=[np.pi * np.arange(ntr)] * 3,
                gains=[gains] * 3, echo=[c0["echo"][0]] * 3, m0=[c0["m0"][0]] * 3, scales=(1.0,), cot="echo", demod=True, meq=1.0,
                bcast=True, w=[tuple(plane(v) for v in w)] * 3, t=[tuple(plane(v) for v in tg)] * 3, wf=[None] * 3, tf=[None] * 3,
                rw=[rw] * 3, ce=[None] * 3, cf=[None] * 3)
    return pulses, args, tg, w, kw, case


def test_refine_b1_with_magnitude_targets():
    """as tests/test_blochtrainlm_gpu.py holds the component refiner: the accepted losses fall, 'calls' counts the device steps under
    'lm', a pulse alone has its bits in the batch, the last loss is the magnitude lsq call's, and solver='host' of the LM entry point
    is refine_bloch_train_batch(magnitude=True)"""
    pulses, args, tg, w, kw, _ = _refine_case()
    kw = dict(kw, iters=2, cg=4)
    p = pulses[0]
    b1s, infos = mbfir.refine_bloch_train_lm_batch(pulses, *args, [tg] * 3, [w] * 3, solver="device", **kw)
    for q in range(3):
        L = infos[q]["losses"]
        print("b1 pulse %d: losses %s, refused %d, calls %s" % (q, ["%.6g" % v for v in L], infos[q]["refused"], infos[q]["calls"]))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
        cc = infos[q]["calls"]
        assert set(cc) == {"lsq", "gn", "lm"} and cc["lsq"] == 1 and cc["gn"] == 1 and cc["lm"] == len(L) - 1 + infos[q]["refused"]
        (b1,), (info,) = mbfir.refine_bloch_train_lm_batch([pulses[q]], *args, [tg], [w], solver="device", **kw)
        assert np.array_equal(b1, b1s[q]) and info == infos[q]
        lkw = {k: v for k, v in kw.items() if k not in ("iters", "cg")}
        (Lend, _), = mbfir.bloch_train_lsq_batch([(b1s[q],) + tuple(p[1:])], *args, [tg], [w], **lkw)
        assert Lend == L[-1]
    new = mbfir.refine_bloch_train_lm_batch(pulses, *args, [tg] * 3, [w] * 3, solver="host", **kw)
    old = mbfir.refine_bloch_train_batch(pulses, *args, [tg] * 3, [w] * 3, **kw)
    for q in range(3):
        L = old[1][q]["losses"]
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
        assert np.array_equal(new[0][q], old[0][q]) and new[1][q] == old[1][q] and set(new[1][q]["calls"]) == {"lsq", "gn"}
        (one,), (info,) = mbfir.refine_bloch_train_batch([pulses[q]], *args, [tg], [w], **kw)
        assert np.array_equal(one, old[0][q]) and info == old[1][q]


@pytest.mark.parametrize("vary", [("gains", "phases"), ("gains",)])
def test_refine_sched_with_magnitude_targets(vary):
    """as tests/test_blochtrainschedlm_gpu.py holds the component refiners: solver='host' of the LM entry point is
    refine_bloch_train_sched_batch(magnitude=True); solver='device' at cg = 4 n, rtol = 1e-24, two outer iterations: the losses
    fall, as many steps are accepted as by the host solver, a pulse alone has its bits in the batch, and the final loss is the host
    solver's within that test's margin: the host loop (dense Cholesky) on the float64 reference's H and gradient against the same
    loop on the device's, times 100"""
    pulses, args, tg, w, kw, case = _refine_case()
    n, vg, vp = 9 * len(vary), "gains" in vary, "phases" in vary
    host_s, host_i = mbfir.refine_bloch_train_sched_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, **kw)
    same_s, same_i = mbfir.refine_bloch_train_sched_lm_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, solver="host", **kw)
    sch, infos = mbfir.refine_bloch_train_sched_lm_batch(pulses, *args, [tg] * 3, [w] * 3, vary=vary, iters=2, solver="device", cg=4 * n,
                                                         rtol=1e-24, **kw)

    def lsq_fn(q):
        def f(x):
            L, gg, gp, _ = ref.lsq("sched", lmref.moved(case, q, x), q, np.float64)
            return float(L), lmref.mask(np.asarray(gg, dtype=np.float64) + 1j * np.asarray(gp, dtype=np.float64), vary)
        return f

    def dense_fn(q):
        on = np.r_[np.full(9, vg), np.full(9, vp)]

        def f(x):
            hg, hp = ref.gn("sched", lmref.moved(case, q, x), q, sgr.unit_directions(9), np.float64)
            return np.asarray(np.concatenate([hg, hp], 1), dtype=np.float64)[np.ix_(on, on)]
        return f

    for q in range(3):
        assert np.array_equal(same_s[q][0], host_s[q][0]) and np.array_equal(same_s[q][1], host_s[q][1]) and same_i[q] == host_i[q]
        L, Lh = infos[q]["losses"], host_i[q]["losses"]
        _, Lr, _ = lmref.refine_dense(case, q, 2, vary, lsq_fn=lsq_fn(q), dense_fn=dense_fn(q))
        margin = 100 * abs(Lr[-1] - Lh[-1])
        print("%s pulse %d: losses %s (host %s, reference loop %s), refused %d (host %d), calls %s; |L - L host| %.3g, margin %.3g"
              % (vary, q, ["%.9g" % v for v in L], ["%.9g" % v for v in Lh], ["%.9g" % v for v in Lr], infos[q]["refused"],
                 host_i[q]["refused"], infos[q]["calls"], abs(L[-1] - Lh[-1]), margin))
        assert len(L) >= 2 and all(b < a for a, b in zip(L, L[1:])), (q, L)
        assert all(b < a for a, b in zip(Lh, Lh[1:])), (q, Lh)
        assert len(L) == len(Lh) and len(Lr) == len(Lh), q
        if not vp:
            assert np.array_equal(sch[q][1], np.pi * np.arange(9))
        (one,), (info,) = mbfir.refine_bloch_train_sched_lm_batch([pulses[q]], *args, [tg], [w], vary=vary, iters=2, solver="device",
                                                                  cg=4 * n, rtol=1e-24, **kw)
        assert np.array_equal(one[0], sch[q][0]) and np.array_equal(one[1], sch[q][1]) and info == infos[q]
        assert abs(L[-1] - Lh[-1]) <= margin, (q, L[-1], Lh[-1], margin)


def test_a_triple_with_magnitude_and_a_pair_without_it_are_refused():
    pulses, args, tg, w, kw, _ = _refine_case()
    kw = {k: v for k, v in kw.items() if k != "magnitude"}
    tri_t, tri_w = (tg[0], tg[0], tg[1]), (w[0], w[0], w[1])
    b = [np.ones(len(pulses[0][0]), dtype=complex)]
    one = ([pulses[0]],) + args
    calls = [
        lambda t, w_, m: mbfir.bloch_train_lsq_batch(*one, [t], [w_], magnitude=m, **kw),
        lambda t, w_, m: mbfir.bloch_train_gn_batch(*one, b, [w_], magnitude=m, **kw),
        lambda t, w_, m: mbfir.bloch_train_lm_step_batch(*one, b, [w_], 1e-3, targets=[t], magnitude=m, **kw),
        lambda t, w_, m: mbfir.bloch_train_lsq_sched_batch(*one, [t], [w_], magnitude=m, **kw),
        lambda t, w_, m: mbfir.bloch_train_gn_sched_batch(*one, [w_], tangents_gains=[np.ones(9)], magnitude=m, **kw),
        lambda t, w_, m: mbfir.bloch_train_normal_sched_batch(*one, [t], [w_], magnitude=m, **kw),
        lambda t, w_, m: mbfir.bloch_train_lm_step_sched_batch(*one, [w_], 1e-3, targets=[t], magnitude=m, **kw),
        lambda t, w_, m: mbfir.refine_bloch_train_batch(*one, [t], [w_], iters=1, magnitude=m, **kw),
        lambda t, w_, m: mbfir.refine_bloch_train_lm_batch(*one, [t], [w_], iters=1, solver="device", magnitude=m, **kw),
        lambda t, w_, m: mbfir.refine_bloch_train_sched_batch(*one, [t], [w_], iters=1, magnitude=m, **kw),
        lambda t, w_, m: mbfir.refine_bloch_train_sched_lm_batch(*one, [t], [w_], iters=1, solver="device", magnitude=m, **kw),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError, match="pair"):
            call(tri_t, tri_w, True)
        with pytest.raises(ValueError, match="triple"):
            call(tg, w, False)
        assert call(tg, w, True) is not None, k
    fkw = dict(kw, weights_final=[tri_w], targets_final=[tri_t])
    with pytest.raises(ValueError, match="pair"):
        mbfir.bloch_train_lsq_batch(*one, None, None, magnitude=True, **fkw)
    with pytest.raises(ValueError, match="triple"):
        mbfir.bloch_train_lsq_batch(*one, None, None, **dict(kw, weights_final=[w], targets_final=[tg]))
