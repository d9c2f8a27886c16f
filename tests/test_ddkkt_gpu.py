"""The extended-precision KKT path of an iteration (mbfir_test_unit_ddkkt: the NT scaling, dd_prepare / dd_prepare_lanes, the mode masks,
build_H(dd_k), then solve_modes with an observer on kkt_solve_dd that reads every group of launches back) against the high-precision
reference of tests/ddkkt_ref.py, stage by stage, within the bounds derived there and validated on the CPU by
tests/test_ddkkt_ref_cpu.py.  Every stage is handed the device's own earlier outputs, so a wrong kernel fails alone; every entry of
every output of every live lane is checked; decisions (the strong set, its order, the slot maps, sX, dlc, every fl(a + b)) must match
exactly; what no launch of a lane writes must come back holding the sentinel it went in with.

Runs (ddkkt_ref.RUNS): iterates with a planned strong set, a decade from every cap they meet (asserted on the CPU) -- c8_dup12 with
k = 0 (the plain mode), 1, 63 / 64 / 65 (either side of a tile of the capacitance matrix; six cone directions) and 315; c6_qp25 (no
orthant rows: 3-row cones alone, with the big cone's e_p, with both its directions, the big cone alone); c3_lin64 with 1024 and 1025 rows
(the capacitance form raises the cap once and keeps 1000; the double-double form takes 1025); c4_qphs21 with 1102 (k_dd_order's second
strided trip), 3072 (fits exactly) and 3100 (one raise) in the double-double form, the last two without a solve; c2_ap150 (several
column workgroups of k_dd_rhs).  Each solving run with nv = 2, nv = 1 and an all-zero second column, in both forms where the form takes
it.  pytest -s prints the worst error / bound per stage.

Bit-identities asserted: a second call; every lane of a unit of four strong sets (one empty: ROW_PL next to ROW_DD) and a masked lane
against the same lane alone with MBFIR_TEST_CAP_KP at the unit's kp.

That the tests can fail -- eight arithmetic-only changes of ddkkt.inc, each built apart and this file run once on it (the 90 tests it
held before test_heterogeneous_unit, the partial rows and the plain lane's H against the reference were added;
fractions are error / bound at worst; every other test passed, none faulted):
  1 sX = d - cap -> d, k_dd_select (orthant rows)    54 fail: every run with a strong orthant row, both forms, and the unit: stage set,
                                                      "sX = fl(lam - cap)"; nothing else (every later stage takes the device's own sX)
  2 e_m -> -e_m in soc3_evec                          43 fail: every run with a 3-row cone strong in e_m (dup_k63 .. 315, qp_k33, qp_k22,
                                                      ap150_k70) and the unit: U rows (5e13), t = e'r2 (8e14), the spread in acc dz (4e14)
  3 slot3[3 idx + dir] -> slot3[3 idx], k_dd_order    45 fail: every run with a strong 3-row cone, the unit, two of the second-call
                                                      tests (sel_i moves with the atomic order): t lands in the wrong slots, the slots
                                                      nobody writes keep their sentinel, and NaN (fraction inf) runs through r2 cones,
                                                      rhs_w, w, G Bh, acc dz and the next pass's norm
  4 dz / dl -> dz * dl, k_dd_r2                       52 fail: every solving run with orthant rows and the unit: r2 orth (5e42)
  5 the uncapped e[0] in k_dd_winv2c                  49 fail: every solving run with 3-row cones (qp_p5 included) and the unit: wbz cones,
                                                      first and second application (2e22)
  6 (lp - l0) -> lp in k_H_big_dd                     27 fail: every solving run with the big cone (c6_qp25, qphs_k1102): H_w (3e12)
  7 (zm - zp) -> (zp - zm) in k_dd_accum_big          21 fail: every solving run with a strong direction of the big cone (qp_k33, qp_k22,
                                                      qp_big2, qphs_k1102): acc dz (7e14); max |bz - G dx + W^2 dz| at the end 8e7 against
                                                      the twin's 6e-6
  8 the padding rows of k_dd_rows left unwritten      31 fail: every capacitance-form run whose k is no multiple of 64, and the unit: the
                                                      sentinel stays in the padding rows of U, Ms is not finite (fraction inf), then
                                                      rhs_w, G Bh, acc dz; the double-double form (no padding) and k = 64, 1024 pass
(The bound fractions are reported ahead of the exact checks: where one of them is infinite the list of failed exact checks of the
same run -- slot3 in 3, the padding rows of U in 8 -- is not printed.)
"""
import numpy as np
import pytest

import ddkkt_ref as R
import kkt_ref as K
import mbfir

pytestmark = pytest.mark.gpu
CASES = ((2, "random"), (1, "random"), (2, "zero"))
BLOCKS = ("sel_r", "sel_q", "sel_sc", "sel_i", "strong_i", "strong_x", "H", "U", "M", "Hf", "Yt", "Zt", "S", "Ms", "out_x", "out_r", "out_k", "sc",
          "end_x", "end_r", "flag", "lane_rep")
_DEV, _TW = {}, {}


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    for k in ("MBFIR_DDFORM", "MBFIR_TEST_CAP_KP", "MBFIR_FUSE", "MBFIR_HSOLVE"):
        monkeypatch.delenv(k, raising=False)


def opts_of(name, **kw):
    return mbfir.make_opts(grid_m=K.designs()[R.RUNS[name]["design"]]["grid_m"], ddkkt=1, **kw)


def ldu_of(k):
    return min(R.DD_KMAX, max(64, -(-k // 64) * 64) + 64)


def call(monkeypatch, lanes, form, nv=2, rhs="random", mask=None, ldu=None, cap_kp=0, solve=None, **kw):
    """the hook on a unit whose lanes are (run, seed) pairs of one design"""
    if form == "dd":
        monkeypatch.setenv("MBFIR_DDFORM", "dd")
    if cap_kp:
        monkeypatch.setenv("MBFIR_TEST_CAP_KP", str(cap_kp))
    ins = [R.run_inputs(n, seed, nv, rhs) for n, seed in lanes]
    name = lanes[0][0]
    P = ins[0][0]
    job = K.designs()[R.RUNS[name]["design"]]["job"]
    o = mbfir.test_unit_ddkkt([job] * len(lanes), np.stack([i[1] for i in ins]), np.stack([i[2] for i in ins]), np.stack([i[4] for i in ins]),
                              np.stack([i[5] for i in ins]), P["nq3"], solve=R.RUNS[name]["solve"] if solve is None else solve,
                              ldu=ldu or ldu_of(max(R.RUNS[n]["k"] for n, _ in lanes)), cap_blocks=form == "cap", mask=mask,
                              opts=kw.pop("opts", None) or opts_of(name), **kw)
    monkeypatch.delenv("MBFIR_DDFORM", raising=False)
    monkeypatch.delenv("MBFIR_TEST_CAP_KP", raising=False)
    rep = o["report"]
    assert (rep["lanes"], rep["nv"], rep["cap_form"], rep["passes"]) == (len(lanes), nv, int(form == "cap"), 3 if form == "cap" else 2)
    assert (rep["N"], rep["R"], rep["l"], rep["nq3"], rep["big"]) == (P["N"], P["R"], P["l"], P["nq3"], P["big"])
    return o


def single(monkeypatch, name, form, nv=2, rhs="random", seed=0, cap_kp=0):
    key = (name, form, nv, rhs, seed, cap_kp)
    if key not in _DEV:
        _DEV[key] = call(monkeypatch, [(name, seed)], form, nv, rhs, cap_kp=cap_kp, ldu=ldu_of(max(cap_kp, R.RUNS[name]["k"])))
    return _DEV[key]


def twin_res(name, form, nv, rhs, seed, Dn):
    """the float64 twin of a run (nothing of the device's enters): its end residuals, and T, the twin itself"""
    key = (name, form, nv, rhs, seed)
    if key not in _TW:
        P, s, z, planned, bx, bz = R.run_inputs(name, seed, nv, rhs)
        T = R.twin(P, K.model_G(P), s, z, bx, bz, form)
        n1, n2, _, _ = R.residuals(P, Dn, R.Eig(P, T), bx, bz, T["dx_end"][:nv, :P["N"]], T["dz_end"][:nv])
        _TW[key] = dict(n1=n1, n2=n2, T=T)
    return _TW[key]


def held(o, b, name, form, nv=2, rhs="random", seed=0, tag="", solve=None, sentinel=np.nan):
    run = R.RUNS[name]
    P, s, z, planned, bx, bz = R.run_inputs(name, seed, nv, rhs)
    D = R.unpack(o, b, P)
    rec, facts = R.check_selection(P, D, s, z, sentinel=sentinel)
    k = facts["k"]
    solve = run["solve"] if solve is None else solve
    assert D["mode"] == (1 if k else 2)
    worse = []
    if k:
        Dn = R.design_of(run["design"])
        tw = twin_res(name, form, nv, rhs, seed, Dn)
        R.check_build(P, Dn, D, rec, sentinel=sentinel, rows_only=not solve, ref=tw["T"])
        if solve:
            _, pf = R.check_passes(P, Dn, D, bx, bz, nv, rec, sentinel=sentinel, slow=k <= 400 or nv == 1)
            worse = R.refines(pf, tw)
            tag += "  end %.1e / %.1e (twin %.1e / %.1e)" % (pf["n1"], pf["n2"], tw["n1"], tw["n2"])
            if rhs == "zero":          # the all-zero column comes back all zero wherever a launch writes: no NaN from 0 x a huge weight
                lim = {R.DD_KMAX: k, -(-P["N"] // 64) * 64: P["N"]}
                for pq in D["pass"][:D["passes"]]:
                    for key, v in pq.items():
                        if key != "sc" and not R.is_sent(v[1]):
                            assert np.all(v[1][:lim.get(len(v[1]), P["R"])] == 0.0), key
    else:
        # nothing above the cap: the plain mode; every slot -1 (check_selection), dlc = dl, no pass of the extended-precision solve ran
        assert np.array_equal(D["dlc"], D["dl"]) and D["kcnt"] == 0
        assert all(R.is_sent(v) for pq in D["pass"] for v in pq.values())
        assert np.all(np.isfinite(D["dx_end"][:nv, :P["N"]])) and np.all(np.isfinite(D["dz_end"][:nv, :P["R"]])) and D["flag"] == 0
        # its H against the reference of the plain solve G'W^-2 G at (s, z)
        R.check_plain_H(P, R.design_of(run["design"]), D, s, z, rec)
    print("\n%-12s %-4s nv %d %-6s%s k %4d  %s" % (name, form, nv, rhs, tag, k, "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.over(), rec.over()
    assert not rec.failed, rec.failed
    assert not worse, worse
    return D, facts


def same(a, la, b, lb, skip=()):
    return [k for k in BLOCKS if k in a and k in b and k not in skip and not np.array_equal(a[k][la], b[k][lb], equal_nan=True)]


# (a run without a solve checks selection, order and rows only: the right-hand sides do not enter, one case)
STAGE_RUNS = [(n, f, nv, rhs) for n in R.RUNS for f in R.RUNS[n]["forms"] for nv, rhs in (CASES if R.RUNS[n]["solve"] else CASES[:1])]


@pytest.mark.parametrize("name,form,nv,rhs", STAGE_RUNS, ids=lambda v: str(v))
def test_stages(name, form, nv, rhs, monkeypatch):
    run = R.RUNS[name]
    o = single(monkeypatch, name, form, nv, rhs)
    D, facts = held(o, 0, name, form, nv, rhs)
    att = facts["attempts"]
    fit = R.fit_of(form)
    assert o["report"]["attempts"] == len(att) == (2 if run["k"] > fit else 1)
    assert o["report"]["k_max"] == len(att[-1][1]) and D["theta"] == R.THETA * 100.0 ** (len(att) - 1)
    assert D["nbp"] == max(1, -(-(D["dl"].size + len(D["e3"])) // 256)) + (1 if len(D["wbb"]) else 0)
    assert o["report"]["kp"] == (0 if not facts["k"] else -(-facts["k"] // 64) * 64 if form == "cap" else facts["k"])


@pytest.mark.parametrize("name,form", [("dup_k65", "cap"), ("dup_k65", "dd"), ("qp_k22", "cap"), ("qphs_k1102", "dd"), ("lin_k1025", "cap")])
def test_a_second_call_returns_the_same_bits(name, form, monkeypatch):
    """the atomic counter hands the slots out in any order: k_dd_order makes the solve reproducible"""
    a = single(monkeypatch, name, form)
    b = call(monkeypatch, [(name, 0)], form)
    assert not same(a, 0, b, 0)


def test_lanes_in_different_modes_are_their_single_runs(monkeypatch):
    """four lanes of one design with different strong sets, one of them empty (ROW_PL next to ROW_DD), and a masked lane: every live lane
    is held to the reference and is bit-identical, stage for stage, to the same lane alone padded to the unit's kp.
    The empty lane: in the unit build_H runs with the capped weights (D.dlc, D.m3c) and the lane's kernels switch to dl and the
    uncapped block through DProg::plain_weights (dd_lane / dl_plain); alone, dd_k = 0 and build_H(0) reads dl and w3 with no switch at
    all (dd_lane = nullptr, m3c = nullptr) -- the plain solve's own build.  So H, M and the solution of that lane against its single run
    is the comparison that shows a capped weight on a plain lane: the single run does not share the switch.  (mbfir.test_unit_kkt with
    opts.ddkkt = -1 is no bit-for-bit partner: with ddkkt off lane_prep folds the +w / -w grid, with ddkkt on it does not, and the
    moment sums of H run in another order.)  The lane's H is also held to G'W^-2 G in longdouble (ddkkt_ref.check_plain_H)."""
    names = ["dup_k65", "dup_k0", "dup_k315", "dup_k1", "dup_k64"]
    mask = [1, 1, 1, 0, 1]
    kp = 320
    o = call(monkeypatch, [(n, 0) for n in names], "cap", mask=mask, ldu=kp + 64)
    assert o["report"]["kp"] == kp and o["report"]["k_max"] == 315
    assert o["lane_rep"][:, 0].tolist() == [1, 2, 1, 0, 1] and o["lane_rep"][:, 1].tolist() == [65, 0, 315, 0, 64]
    for k in BLOCKS:
        if k in ("flag", "lane_rep"):
            continue
        assert R.is_sent(o[k][3]) if o[k].dtype.kind == "f" else np.all(o[k][3] == -9), k
    assert o["flag"][3] == -1
    for b, n in enumerate(names):
        if not mask[b]:
            continue
        D, _ = held(o, b, n, "cap", tag=" lane %d" % b)
        alone = call(monkeypatch, [(n, 0)], "cap", ldu=kp + 64, cap_kp=kp)
        assert not same(o, b, alone, 0), (n, same(o, b, alone, 0))


def test_refusals_and_the_context_after(monkeypatch):
    name = "dup_k1"
    P, s, z, planned, bx, bz = R.run_inputs(name)
    job = K.designs()["c8_dup12"]["job"]
    a = (s[None], z[None], bx[None], bz[None], P["nq3"])
    with pytest.raises(ValueError, match="row-sharded"):
        mbfir.test_unit_ddkkt([job], *a, opts=opts_of(name, shard_size=2))
    with pytest.raises(ValueError, match="extended-precision"):
        mbfir.test_unit_ddkkt([job], *a, opts=mbfir.make_opts(ddkkt=-1))
    with pytest.raises(ValueError, match="lane count"):
        mbfir.test_unit_ddkkt([job] * 65, *[np.repeat(v, 65, axis=0) for v in a[:4]], P["nq3"], opts=opts_of(name))
    with pytest.raises(ValueError, match="right-hand sides"):
        mbfir.test_unit_ddkkt([job], s[None], z[None], np.zeros((1, 3, P["N"])), np.zeros((1, 3, P["R"])), P["nq3"], opts=opts_of(name))
    with pytest.raises(ValueError, match="do not fit"):
        mbfir.test_unit_ddkkt([job], s[None, :-1], z[None, :-1], bx[None], bz[None, :, :-1], P["nq3"], opts=opts_of(name))
    with pytest.raises(ValueError, match="ldu"):
        mbfir.test_unit_ddkkt([job], *a, ldu=32, opts=opts_of(name))
    monkeypatch.setenv("MBFIR_DDFORM", "dd")
    with pytest.raises(ValueError, match="one design at a time"):
        mbfir.test_unit_ddkkt([job] * 2, *[np.repeat(v, 2, axis=0) for v in a[:4]], P["nq3"], opts=opts_of(name))
    monkeypatch.delenv("MBFIR_DDFORM")
    # the context still solves, and the hook after a solve gives what it gave before
    fn, args = job
    h, status = getattr(mbfir, fn)(*args)
    assert status == "Solved" and len(h) == args[0]
    assert not same(call(monkeypatch, [(name, 0)], "cap"), 0, single(monkeypatch, name, "cap"), 0)


def test_heterogeneous_unit(monkeypatch):
    """two orders in one unit (lattice_ref.hetero_jobs): per-lane N, R and strong sets (24 and 68: kp = 128).  Each lane is held to the
    reference, returns the sentinel past its own N / R, and is bit-identical, stage for stage, to the same lane alone padded to the
    unit's kp.  A finite sentinel: the capacitance form's vector kernels run over the unit's largest N, where the shorter lane's G'v
    leaves the sentinel and its factor is the identity (0 x NaN would not be 0); ddkkt_ref takes the padded problem for that lane."""
    import lattice_ref as lr
    jobs, grid_m = lr.hetero_jobs()
    Ps = [lr.program(fn, args, grid_m) for fn, args in jobs]
    assert Ps[0]["R"] != Ps[1]["R"] and Ps[0]["N"] != Ps[1]["N"] and -(-Ps[0]["N"] // 64) == -(-Ps[1]["N"] // 64)
    assert min(P["nq3"] for P in Ps) >= 2 and min(P["l"] for P in Ps) >= 66
    plans = [dict(kl=20, q3=(("p", 1), ("p0m", 1))), dict(kl=66, q3=(("p0", 1),))]
    sent, kp = -7.25e77, 128
    ins = []
    for b, P in enumerate(Ps):
        s, z, planned = R.strong_iterate(P, 900 + b, plans[b])
        rng = np.random.default_rng(910 + b)
        ins.append(dict(s=s, z=z, planned=planned, bx=rng.standard_normal((2, P["N"])), bz=rng.standard_normal((2, P["R"]))))
        E = R.ref_eigs(P, s, z)
        assert R.ref_set(E, R.ref_cap(E, R.THETA)) == planned and R.margins(E, [R.ref_cap(E, R.THETA)]) >= 1
    assert [len(i["planned"]) for i in ins] == [24, 68]

    def pad(v, n):
        return np.concatenate([v, np.zeros(v.shape[:-1] + (n - v.shape[-1],))], axis=-1)

    def go(bs, cap_kp=0):
        if cap_kp:
            monkeypatch.setenv("MBFIR_TEST_CAP_KP", str(cap_kp))
        Rm, Nm, nq3 = max(Ps[b]["R"] for b in bs), max(Ps[b]["N"] for b in bs), max(Ps[b]["nq3"] for b in bs)
        o = mbfir.test_unit_ddkkt([jobs[b] for b in bs], np.stack([pad(ins[b]["s"], Rm) for b in bs]), np.stack([pad(ins[b]["z"], Rm) for b in bs]),
                                  np.stack([pad(ins[b]["bx"], Nm) for b in bs]), np.stack([pad(ins[b]["bz"], Rm) for b in bs]), nq3, ldu=kp + 64,
                                  opts=mbfir.make_opts(grid_m=grid_m, ddkkt=1), sentinel=sent)
        monkeypatch.delenv("MBFIR_TEST_CAP_KP", raising=False)
        return o
    o = go([0, 1])
    assert o["report"]["hetero"] == 1 and o["report"]["lanes"] == 2 and o["report"]["kp"] == kp and o["report"]["cap_form"] == 1
    n_unit = max(P["N"] for P in Ps)
    for b, P in enumerate(Ps):
        I = ins[b]
        D = R.unpack(o, b, P)
        D["n_unit"] = n_unit
        Dn = R.Design(P)
        T = R.twin(P, K.model_G(P), I["s"], I["z"], I["bx"], I["bz"], "cap")
        rec, facts = R.check_selection(P, D, I["s"], I["z"], sentinel=sent)
        assert facts["k"] == len(I["planned"]) and D["mode"] == 1
        R.check_build(P, Dn, D, rec, sentinel=sent, ref=T)
        _, pf = R.check_passes(P, Dn, D, I["bx"], I["bz"], 2, rec, sentinel=sent)
        print("\nhetero lane %d k %d  %s" % (b, facts["k"], "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
        assert not rec.over() and not rec.failed, (rec.over(), rec.failed)
        alone = go([b], cap_kp=kp)
        assert alone["report"]["hetero"] == 0 and alone["report"]["kp"] == kp
        A = R.unpack(alone, 0, P)
        n, r = P["N"], P["R"]
        for key in ("dl", "dlc", "w3", "e3", "m3c", "eb", "theta", "slotl", "slot3", "kcnt", "skind", "sidx", "sdir", "sX", "M", "U", "Yt", "Zt", "S", "Ms"):
            assert np.array_equal(D[key], A[key], equal_nan=True), key
        assert np.array_equal(np.tril(D["H"]), np.tril(A["H"])), "H"
        for q in range(3):
            for key, v in D["pass"][q].items():
                cut = slice(None) if key == "sc" or v.shape[-1] == R.DD_KMAX else slice(0, n) if v.shape[-1] == len(D["M"]) else slice(0, r)
                assert np.array_equal(v[..., cut], A["pass"][q][key][..., cut], equal_nan=True), (q, key)
        assert np.array_equal(D["dx_end"][:, :n], A["dx_end"][:, :n]) and np.array_equal(D["dz_end"][:, :r], A["dz_end"][:, :r])
        assert np.array_equal(D["sc_end"], A["sc_end"], equal_nan=True)
