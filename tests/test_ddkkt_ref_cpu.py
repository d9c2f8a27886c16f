"""tests/ddkkt_ref.py without a GPU: the inputs of the device tests have the planned strong sets with a decade to spare at every cap a
run meets; a float64 twin of the extended-precision path (oracle/conic_ipm.py's factor_dd / kkt_solve_dd restated with explicit factors,
on lattice_ref's model of the recurrences) stays within a quarter of every derived bound (within the bound itself where it only counts
the roundings of a short expression); the twin's own norms set the factor the device's residuals are held to; and the checker rejects
planted errors at the stage where they are planted."""
import numpy as np
import pytest

import ddkkt_ref as R
import kkt_ref as K

TWIN_RUNS = [("dup_k1", "cap"), ("dup_k65", "cap"), ("dup_k65", "dd"), ("qp_k22", "cap"), ("qp_k22", "dd"), ("qp_big2", "dd")]
_TW = {}


def twin_of(name, form, nv=2, order="device"):
    key = (name, form, nv, order)
    if key not in _TW:
        P, s, z, planned, bx, bz = R.run_inputs(name, nv=nv)
        _TW[key] = R.twin(P, K.model_G(P), s, z, bx, bz, form, order=order)
    return _TW[key]


@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_planned_sets_and_margins(name):
    """The strong set at the first cap is the planned one, every later attempt's is the plan's, and no eigenvalue a decision is taken on
    lies within a decade of a cap the run meets.  On the two retry runs (lin_k1025, qphs_k3100) the margin holds TO ROUNDING ONLY, hence
    the 1e-6 below: the rows that drop out at the raised cap all carry the same weight F = 1e7 -- with caps 1e6 and 1e8 no other value
    is a decade from both, so they are not drawn from a range -- and 1e7 / 1e6 is one decade up to the rounding of z / s and of the cap."""
    run = R.RUNS[name]
    P, s, z, planned, bx, bz = R.run_inputs(name)
    E = R.ref_eigs(P, s, z)
    assert abs(float(R.ref_cap(E, R.THETA)) / R.THETA - 1) < 1e-9
    assert R.ref_set(E, R.ref_cap(E, R.THETA)) == planned and len(planned) == run["k"]
    for form in run["forms"]:
        att = R.attempts_of(E, R.THETA, R.fit_of(form))
        caps = [R.ref_cap(E, th) for th, _ in att]
        m = R.margins(E, caps)
        print("%-12s %-4s attempts %d  sizes %s  margin %.3f decades" % (name, form, len(att), [len(st) for _, st in att], m))
        assert m >= 1 - 1e-6
        drop = run["plan"].get("drop", 0)
        assert [len(st) for _, st in att] == ([run["k"]] if run["k"] <= R.fit_of(form) else [run["k"], run["k"] - drop])
        assert att[-1][1] == [t for t in planned if not (len(att) > 1 and float(E["d"][t[1]] if t[0] == 0 else 1e30) < 1e8)]


def held(P, D, s, z, bx, bz, nv):
    rec, facts = R.check_selection(P, D, s, z)
    if D["k"]:
        Dn = R.Design(P)
        R.check_build(P, Dn, D, rec, ref=D)              # (D is the twin: the reference's own condition numbers)
        R.check_passes(P, Dn, D, bx, bz, nv, rec)
    return rec


@pytest.mark.parametrize("name,form", TWIN_RUNS)
def test_twin_within_a_quarter_of_the_bounds(name, form):
    P, s, z, planned, bx, bz = R.run_inputs(name)
    D = twin_of(name, form)
    rec = held(P, D, s, z, bx, bz, 2)
    print("\n%-10s %-4s %s" % (name, form, "  ".join("%s %.3f" % kv for kv in rec.worst().items())))
    assert not rec.failed, rec.failed
    over = [(k, v) for k, v in rec.frac.items() if not v <= (1.0 if k in R.COUNTED or k[0].startswith("cap ") else 0.25)]
    assert not over, over


def test_twin_spread_sets_the_factor():
    """The twin's own norms under two summation orders, and its end residuals under both forms, each as max(value, floor): the largest
    ratio is the spread; FACTOR = 4 x SPREAD_MEASURED covers it."""
    spread = 1.0
    for name in ("dup_k65", "qp_k22"):
        P, s, z, planned, bx, bz = R.run_inputs(name)
        Dn = R.Design(P)
        ends = {}
        for form in ("cap", "dd"):
            Da, Db = twin_of(name, form), twin_of(name, form, order="seq")
            Eg = R.Eig(P, Da)
            n1, n2, f1, f2 = R.residuals(P, Dn, Eg, bx, bz, Da["dx_end"][:2, :P["N"]], Da["dz_end"][:2])
            ends[form] = (max(n1, f1), max(n2, f2))
            for a, b in zip(Da["sc_end"][:Da["passes"]], Db["sc_end"][:Db["passes"]]):
                a, b = max(a, f1), max(b, f1)
                spread = max(spread, a / b, b / a)
            print("%-8s %-4s norms %s  end %.3e (floor %.3e)  %.3e (floor %.3e)" % (name, form, Da["sc_end"][:Da["passes"]], n1, f1, n2, f2))
        for i in range(2):
            spread = max(spread, ends["cap"][i] / ends["dd"][i], ends["dd"][i] / ends["cap"][i])
    print("measured spread %.4f" % spread)
    assert spread <= R.SPREAD_MEASURED * (1 + 1e-12) and R.FACTOR == 4.0 * R.SPREAD_MEASURED


def _copy(D):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in D.items()}
    out["pass"] = [{k: v.copy() for k, v in pq.items()} for pq in D["pass"]]
    return out


def _failed_stages(rec):
    return sorted({st for st, _ in rec.failed} | {k[0] for k, v in rec.frac.items() if not v <= 1.0})


def test_checker_rejects_planted_errors():
    """a dropped strong row, a swapped direction, unsorted slots, an unwritten padding row: each fails at its own stage and nowhere else"""
    name, form = "dup_k65", "cap"
    P, s, z, planned, bx, bz = R.run_inputs(name)
    Dn = R.Design(P)
    base = twin_of(name, form)
    k = base["k"]

    def stages(D):
        rec, _ = R.check_selection(P, D, s, z)
        R.check_build(P, Dn, D, rec, rows_only=True)
        return _failed_stages(rec)
    assert stages(_copy(base)) == []
    # a dropped strong row: the last slot goes, with its map entry
    D = _copy(base)
    kind, idx, d = int(D["skind"][k - 1]), int(D["sidx"][k - 1]), int(D["sdir"][k - 1])
    assert kind == 1
    D["slot3"][idx, d] = -1
    for key in ("skind", "sidx", "sdir"):
        D[key][k - 1] = -9
    D["sX"][k - 1] = np.nan
    D["U"][k - 1] = 0.0
    D["k"] = D["kcnt"] = k - 1
    assert stages(D) == ["set"]
    # a swapped direction: e_p of a 3-row cone stored as e_m (its row of U follows the stored direction)
    D = _copy(base)
    q = int(np.nonzero((D["skind"][:k] == 1) & (D["sdir"][:k] == 0))[0][0])
    D["sdir"][q] = 2
    assert "set" in stages(D)
    # unsorted slots: two neighbours exchanged consistently (maps, sX, rows of U)
    D = _copy(base)
    a, b = 3, 4
    for key in ("skind", "sidx", "sdir", "sX"):
        D[key][[a, b]] = D[key][[b, a]]
    D["U"][[a, b]] = D["U"][[b, a]]
    D["slotl"][D["sidx"][a]], D["slotl"][D["sidx"][b]] = a, b
    assert stages(D) == ["set"]
    rec, _ = R.check_selection(P, D, s, z)
    assert [w for st, w in rec.failed] == ["sorted by (kind, index, direction)"]
    # an unwritten padding row of U
    D = _copy(base)
    assert D["kp"] > k
    D["U"][k] = np.nan
    assert stages(D) == ["U"]
    # ... and an arithmetic one further on: the excess weight lam in place of lam - cap
    D = _copy(base)
    D["sX"][:k] = D["sX"][:k] + D["cap"]
    assert stages(D) == ["set"]
