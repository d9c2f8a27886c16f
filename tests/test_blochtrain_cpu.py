"""The NumPy reference of the pulse train (tests/blochtrain_ref.py, no GPU): its propagator form against its recursion over the tiled
waveform in long double (which pins the sense of the z rotations), its float64 form against the bound the device is held to, its
exact edge cases, and the declaration, the binding and the argument errors of mbfir.bloch_train_batch / mbfir.bloch_prop_batch, none
of which needs a device."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrain_ref", os.path.join(ROOT, "tests", "blochtrain_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

CASES = list(ref.cases())
LD_EPS = float(np.finfo(np.longdouble).eps)


def _args(c, q, s, meq):
    return (c["pulses"][q], c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], s, c["m0"][q], meq)


def test_cases_cover_what_they_claim():
    cs = ref.cases()
    nts = {len(p[0]) for c in cs.values() for p in c["pulses"]}
    ntrs = {n for c in cs.values() for n in c["ntr"]}
    assert nts == {1, 9, 257} and ntrs == {1, 2, 257}
    echoes = {(len(p[0]), e) for c in cs.values() for p, e in zip(c["pulses"], c["echo"])}
    assert {(9, 0), (9, 4), (9, 9), (257, 256), (257, 257), (1, 0), (1, 1)} <= echoes
    ngain = {len(np.unique(g)) for c in cs.values() for g in c["gains"]}
    assert ngain == {1, 2, 3}
    assert {c["scales"] for c in cs.values()} == {(1.0,), (0.9, 1.0, 1.1)}
    assert len(cs["h1_long"]["dfs"][0]) * len(cs["h1_long"]["dps"][0]) == 300
    assert cs["shared"]["dfs"][0] is cs["shared"]["dfs"][2] and cs["batch"]["dfs"][0] is not cs["batch"]["dfs"][1]
    for c in cs.values():
        for p in c["pulses"]:
            tp = ref.intervals(p)
            assert len(tp) == 1 or (tp[-1] > tp[:-1].max() and p[0][-1] == 0.0)
    assert any(p[1] is not None for c in cs.values() for p in c["pulses"])
    assert {(p[3], p[4]) for c in cs.values() for p in c["pulses"]} == {(30.0, 2.0), (1.0, 0.1)}


@pytest.mark.parametrize("name", CASES)
def test_longdouble_propagator_form_is_the_longdouble_tiled_recursion(name):
    """Both demod settings and meq in {1, 1e-4, 0} on every case.  Two long-double evaluations of the same rational function of
    the same inputs: they differ by their roundings, a few long-double eps per step, held to 8 eps ntr (ntime + 4) mu (measured:
    1.3e-17 at most, on c13_ramp, whose tolerance is 2.9e-15).  The opposite sense of Z misses by 0.1 and more."""
    c = ref.cases()[name]
    worst = 0.0
    for meq in ref.MEQS:
        want = ref.reference(name, meq)
        for q, p in enumerate(c["pulses"]):
            tol = 8 * LD_EPS * c["ntr"][q] * (len(p[0]) + 4) * ref.mu_of(c["m0"][q], meq, len(c["dfs"][q]), len(c["dps"][q]))
            for si, s in enumerate(c["scales"]):
                for demod in (False, True):
                    E, F = ref.train(*_args(c, q, s, meq), demod, np.longdouble)
                    wE = ref.demodulate(want[q][0][si], c["phases"][q], np.longdouble) if demod else want[q][0][si]
                    eE, eF = np.abs(E - wE).max(1), np.abs(F - want[q][1][si]).max(0)
                    worst = max(worst, float((eE / tol).max()), float((eF / tol).max()))
                    assert np.all(eE <= tol) and np.all(eF <= tol), (meq, q, s, demod)
    print("%s: worst |propagator form - tiled| / tolerance in long double %.3g" % (name, worst))


def test_the_opposite_sense_of_z_is_far_off():
    c = ref.cases()["c13_ramp"]
    a = list(_args(c, 0, 1.0, 1e-4))
    a[4] = -c["phases"][0] + 0.4 * np.arange(257)                       # not a multiple of pi: the two senses differ
    a = tuple(a)
    E, _ = ref.train(*a, False, np.longdouble)
    T, _ = ref.tiled(*a, np.longdouble)
    assert np.abs(E - T).max() < 1e-15
    a2 = a[:4] + (-a[4],) + a[5:]
    E2, _ = ref.train(*a2, False, np.longdouble)
    assert np.abs(E2 - T).max() > 0.1


@pytest.mark.parametrize("name", CASES)
def test_float64_propagator_form_is_within_a_hundredth_of_the_device_bound(name):
    """Measured worst shares of C u ntr (ntime + 4) mu with C = 200: c13_ramp 1.2e-3, h1_long 2.1e-4, one 9.4e-4, batch 1.1e-3,
    shared 1.1e-3."""
    c = ref.cases()[name]
    worst = 0.0
    for meq in ref.MEQS:
        want, bd = ref.reference(name, meq), ref.case_bounds(name, meq)
        for q in range(len(c["pulses"])):
            for si, s in enumerate(c["scales"]):
                E, F = ref.train(*_args(c, q, s, meq), False, np.float64)
                sh = max(float((np.abs(E - want[q][0][si]).astype(np.float64) / bd[q]).max()),
                         float((np.abs(F - want[q][1][si]).astype(np.float64) / bd[q]).max()))
                worst = max(worst, sh)
                assert sh <= 0.01, (meq, q, s, sh)
    print("%s: worst float64 share of the bound %.3g" % (name, worst))


def test_echo_edges_are_exact():
    """echo = 0 with demod returns Z(+phi_k) m_k, echo = ntime returns m_{k+1}, and the last of those is the final state"""
    c = ref.cases()["c13_ramp"]
    a = list(_args(c, 0, 1.1, 1e-4))
    a[3], a[4], a[5] = 6, c["phases"][0][:6] + 0.3 * np.arange(6), c["gains"][0][:6]
    n = len(c["pulses"][0][0])
    for dtype in (np.float64, np.longdouble):
        En, Fn = ref.train(*a[:6], n, *a[7:], False, dtype)
        assert np.array_equal(En[-1], Fn)
        E0, F0 = ref.train(*a[:6], 0, *a[7:], True, dtype)
        assert np.array_equal(F0, Fn)
        cs, sn = ref._table(a[4], dtype)
        m = [np.asarray(v) for v in ref._grad._m0(a[8], 3, 2, dtype)]
        for k in range(6):
            assert np.array_equal(E0[k], np.stack(ref._zp(cs[k], sn[k], m))), k
            m = list(En[k])
        Tn, TF = ref.tiled(*a[:6], n, *a[7:], dtype)
        T0, _ = ref.tiled(*a[:6], 0, *a[7:], dtype)
        assert np.array_equal(Tn[-1], TF) and np.array_equal(T0[1:], Tn[:-1])


def test_one_repetition_at_phase_0_and_gain_1_is_the_simulators_end_point():
    c = ref.cases()["one"]
    for p, df, dp in ((c["pulses"][0], c["dfs"][0], c["dps"][0]),) + tuple(
            (q, ref.cases()["batch"]["dfs"][0], ref.cases()["batch"]["dps"][0]) for q in ref.cases()["batch"]["pulses"][:2]):
        n = len(p[0])
        for dtype in (np.float64, np.longdouble):
            want = ref._grad.forward(p[0], p[1], p[2], p[3], p[4], df, dp, ref.gamma_of(p[5]), 1.0, None, dtype)
            E, F = ref.tiled(p, df, dp, 1, np.zeros(1), np.ones(1), n, 1.0, None, 1.0, dtype)
            assert np.array_equal(F, np.stack(want)) and np.array_equal(E[0], F)


def test_zero_b1_is_precession_and_decay():
    p = ref.cases()["c13_ramp"]["pulses"][0]
    z = (np.zeros_like(p[0]),) + p[1:]
    df, dp = ref.cases()["c13_ramp"]["dfs"][0], ref.cases()["c13_ramp"]["dps"][0]
    e1 = np.exp(-ref.intervals(p) / p[3])
    a22, b2 = 1.0, 0.0
    for e in e1:
        a22, b2 = e * a22, e * b2 + (1 - e)
    A, B, Ae, Be = ref.prop(z, df, dp, 1.0, 4)
    assert all(np.all(A[i][j] == 0) for i, j in ((0, 2), (1, 2), (2, 0), (2, 1))) and np.all(B[0] == 0) and np.all(B[1] == 0)
    # exact zeros above; the longitudinal entries to rounding (cos^2 + sin^2 of a sample's half angle rounds: 4 u per sample)
    assert np.allclose(A[2][2], a22, rtol=36 * ref.U, atol=0) and np.allclose(B[2], b2, rtol=36 * ref.U, atol=0)
    assert np.array_equal(A[0][0], A[1][1]) and np.array_equal(A[0][1], -A[1][0])
    e2 = np.exp(-ref.intervals(p) / p[4])
    assert np.allclose(A[0][0] ** 2 + A[0][1] ** 2, np.prod(e2) ** 2, rtol=1e-13, atol=0)
    # the phases and gains of a train do not matter then: the z component to the bit, the transverse one to rounding
    m0 = ref.cases()["c13_ramp"]["m0"][0]
    E1, F1 = ref.train(z, df, dp, 5, 0.7 * np.arange(5), np.linspace(0.5, 1, 5), 9, 1.0, m0, 0.0)
    E2, F2 = ref.train(z, df, dp, 5, np.zeros(5), np.ones(5), 9, 1.0, m0, 0.0)
    assert np.array_equal(F1[2], F2[2]) and np.abs(F1 - F2).max() <= 50 * ref.U


def test_the_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    head = len(mbfir.SYMBOLS["mbfir_bloch_batch"][1]) - 4                        # up to and including scales
    for name, extra in (("mbfir_bloch_train_batch", 19), ("mbfir_bloch_prop_batch", 5)):
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert len(mbfir.SYMBOLS[name][1]) == head + extra
        assert getattr(mbfir.load_library(), name) is not None                   # the library exports it
    assert callable(mbfir.bloch_train_batch) and callable(mbfir.bloch_prop_batch)
    # a null context is refused before anything else is read
    for name in ("mbfir_bloch_train_batch", "mbfir_bloch_prop_batch"):
        args = [None] + [0 if a is ctypes.c_int else None for a in mbfir.SYMBOLS[name][1][1:]]
        assert getattr(mbfir.load_library(), name)(*args) == mbfir.E_ARG


class _NoDevice:
    """Stands for the library: any call is device work that must not have been reached"""

    def __getattr__(self, name):
        raise AssertionError("the library call %s was reached" % name)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(mbfir, "load_library", lambda: _NoDevice())
    monkeypatch.setattr(mbfir, "get_context", lambda device=None: (_ for _ in ()).throw(AssertionError("a context was asked for")))
    df, dp = np.linspace(-10, 10, 3), np.linspace(-1, 1, 5)
    p = (np.ones(4), None, 4e-6, 1.0, 1.0, "C-13")
    call, prop = mbfir.bloch_train_batch, mbfir.bloch_prop_batch
    with pytest.raises(ValueError, match="bloch_train_batch: no pulses"):
        call([], df, dp, 4)
    with pytest.raises(ValueError, match="bloch_train_batch: the scale list is empty"):
        call([p], df, dp, 4, scales=())
    with pytest.raises(ValueError, match="bloch_train_batch: pulse 1 has no samples"):
        call([p, (np.zeros(0),) + p[1:]], df, dp, 4)
    with pytest.raises(ValueError, match="bloch_train_batch: pulse 0 has more than 3 gradient axes"):
        call([(p[0], np.zeros((4, 4))) + p[2:]], df, dp, 4)
    with pytest.raises(ValueError, match="bloch_train_batch: an empty grid"):
        call([p], np.zeros(0), dp, 4)
    with pytest.raises(ValueError, match="bloch_train_batch: ntr of pulse 0 must be at least 1"):
        call([p], df, dp, 0)
    with pytest.raises(ValueError, match="bloch_train_batch: ntr of pulse 1 must be at least 1"):
        call([p, p], df, dp, [3, -1])
    with pytest.raises(ValueError, match="bloch_train_batch: 3 values of ntr for 2 pulses"):
        call([p, p], df, dp, [3, 3, 3])
    with pytest.raises(ValueError, match="bloch_train_batch: ntr must be an integer"):
        call([p], df, dp, 2.5)
    with pytest.raises(ValueError, match=r"bloch_train_batch: echo of pulse 0 must lie in \[0, ntime\]"):
        call([p], df, dp, 4, echo=5)
    with pytest.raises(ValueError, match=r"bloch_train_batch: echo of pulse 1 must lie in \[0, ntime\]"):
        call([p, p], df, dp, 4, echo=[4, -1])
    with pytest.raises(ValueError, match="bloch_train_batch: phases of pulse 0 has 3 entries for its 4 repetitions"):
        call([p], df, dp, 4, phases=np.zeros(3))
    with pytest.raises(ValueError, match="bloch_train_batch: gains of pulse 1 has 4 entries for its 2 repetitions"):
        call([p, p], df, dp, [4, 2], gains=[np.ones(4), np.ones(4)])
    with pytest.raises(ValueError, match="bloch_train_batch: a gain is not finite"):
        call([p], df, dp, 4, gains=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match="bloch_train_batch: a cosine or sine of the phase table is not finite"):
        call([p], df, dp, 4, phases=np.nan)
    with pytest.raises(ValueError, match="bloch_train_batch: meq of pulse 0 is not finite"):
        call([p], df, dp, 4, meq=np.nan)
    with pytest.raises(ValueError, match="bloch_train_batch: 3 values of meq for 2 pulses"):
        call([p, p], df, dp, 4, meq=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="bloch_prop_batch: no pulses"):
        prop([], df, dp)
    with pytest.raises(ValueError, match=r"bloch_prop_batch: echo of pulse 0 must lie in \[0, ntime\]"):
        prop([p], df, dp, echo=5)
    with pytest.raises(ValueError, match="bloch_prop_batch: 2 values of echo for 1 pulses"):
        prop([p], df, dp, echo=[1, 2])
    with pytest.raises(TypeError):                                                 # the propagators know neither m0 nor meq
        prop([p], df, dp, meq=0.0)
