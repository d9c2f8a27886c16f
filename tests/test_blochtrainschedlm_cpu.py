"""tests/blochtrainschedlm_ref.py, the reference of the schedule's device Levenberg-Marquardt step, held to itself
without a GPU: the CG step meets the dense solve, the speculative refinement (the call that evaluates a trial solves the next step)
takes the iterates of the plain solve-then-evaluate loop, no case has an exactly zero gradient or operator (so the GPU tests need no
other right-hand side), and the Python-level argument errors of mbfir.bloch_train_lm_step_sched_batch and
mbfir.refine_bloch_train_sched_lm_batch, which are raised before the library is loaded."""
import importlib.util
import os

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("blochtrainschedlm_ref", os.path.join(ROOT, "tests", "blochtrainschedlm_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
SMALL = ("small", "repeat", "zerogain", "hard", "allgains")


def test_stride_is_the_shape_the_issue_names():
    c = ref.stride()
    assert len(c["pulses"]) == 1 and len(c["pulses"][0][0]) == 1 and len(c["dfs"][0]) == 1 and len(c["dps"][0]) == 1
    assert c["ntr"] == [257] and len(np.unique(c["gains"][0])) == 257
    assert c["w"][0] is not None and c["wf"][0] is not None and np.ndim(c["w"][0][0]) == 4


@pytest.mark.parametrize("vary", ref.VARIES)
@pytest.mark.parametrize("name", SMALL)
def test_the_cg_step_at_4n_is_the_dense_solve(name, vary):
    """(H + mu I) d = b with mu = 1e-2 trace(H) / n on the varied halves, cg = 4 n, rtol = 1e-16: the project's 1e-4 of max|d|"""
    c = ref.case_of(name)
    for q in range(len(c["pulses"])):
        ntr = c["ntr"][q]
        n = ntr * len(vary)
        H = ref.dense(c, q, vary)
        assert np.trace(H) > 0
        mu = 1e-2 * np.trace(H) / n
        _, g = ref.lsq(c, q, vary)
        on = np.r_[np.full(ntr, "gains" in vary), np.full(ntr, "phases" in vary)]
        want = np.zeros(2 * ntr)
        want[on] = np.linalg.solve((H + mu * np.eye(2 * ntr))[np.ix_(on, on)], ref.realform(-g)[on])
        d, info = ref.step(c, q, -g, mu, cg=4 * n, rtol=1e-16, vary=vary)
        err = np.abs(ref.realform(d) - want).max() / np.abs(want).max()
        print("%s pulse %d %s: against the dense solve %.3g after %d iterations (%s)" % (name, q, vary, err, info["ncg"], info["status"]))
        assert err <= 1e-4
        assert not ref.realform(d)[~on].any()


@pytest.mark.parametrize("vary", ref.VARIES)
def test_the_speculative_loop_takes_the_iterates_of_the_plain_loop(vary):
    """the same operator, the same mu sequence: equal bit for bit, with one fused call per accepted iterate after the first and two
    where a step was refused; a large first mu and a tiny one, so that both branches are taken"""
    c = ref.case_of("small")
    _, g = ref.lsq(c, 0, vary)
    quot = ref.dot(g, ref.gn(c, 0, g, vary)) / ref.dot(g, g)
    seen = set()
    for mu0 in (1e-3 * quot, 1e-9 * quot):
        n = c["ntr"][0] * len(vary)
        xs, Ls, refused = ref.refine_plain(c, 0, mu0, 3, 4 * n, vary=vary)
        xs2, Ls2, refused2, calls = ref.refine_speculative(c, 0, mu0, 3, 4 * n, vary=vary)
        print("%s mu0 %.3g: losses %s, refused %d, fused calls %d" % (vary, mu0, ["%.6g" % v for v in Ls], refused, calls))
        assert len(xs) == len(xs2) and all(np.array_equal(a, b) for a, b in zip(xs, xs2)) and Ls == Ls2 and refused == refused2
        assert all(b < a for a, b in zip(Ls, Ls[1:])) and len(Ls) >= 2
        steps = len(Ls) - 1 + refused
        assert calls <= 2 * steps and (refused > 0 or calls == steps + 1)
        seen.add(refused > 0)
    print("branches taken: refused %s" % sorted(seen))


@pytest.mark.parametrize("name", ref.names())
def test_no_case_has_an_exactly_zero_gradient_or_operator(name):
    c = ref.case_of(name)
    for q in range(len(c["pulses"])):
        for vary in ref.VARIES:
            _, g = ref.lsq(c, q, vary)
            assert ref.dot(g, g) > 0, (q, vary)
            assert ref.dot(g, ref.gn(c, q, -g, vary)) != 0 and ref.dot(-g, ref.gn(c, q, -g, vary)) > 0, (q, vary)


def test_python_level_argument_errors():
    p = (np.full(3, 1e-5 + 1e-5j), None, 1e-5, 1.0, 1.0, 1.0)
    df, dp, tri = np.zeros(2), np.zeros(3), (1.0, 1.0, 1.0)
    tg = tuple(np.zeros((1, 4, 2, 3)) for _ in range(3))
    f = mbfir.bloch_train_lm_step_sched_batch
    ok = dict(targets=[tg], gains=np.array([0.5, 1.0, 1.0, 0.5]), phases=0.0, echo=2)
    z = np.zeros(4)
    for kw, why in ((dict(vary=()), "vary must name"), (dict(vary=("gains", "gains")), "vary must name"), (dict(vary="b1"), "vary must name"),
                    (dict(targets=None), "neither targets nor a right-hand side"), (dict(cg=-1), "cg must be an integer"),
                    (dict(cg=1.5), "cg must be an integer"), (dict(rtol=-1.0), "rtol is negative"), (dict(rtol=float("nan")), "rtol is negative"),
                    (dict(targets_final=[tri]), "targets_final are given for a final term that has no weights"),
                    (dict(weights_final=[tri]), "every term that has weights needs its own"),
                    (dict(b=[(z, z), (z, z)]), "2 right-hand sides for 1 pulses"), (dict(b=[z]), "must be a pair"),
                    (dict(b=[(z, None)]), "None for the phases, which vary"), (dict(b=[(z, z)], vary=("gains",)), "a half for the phases"),
                    (dict(b=[(z[:3], z)]), "has shape (3,), not (4,)")):
        with pytest.raises(ValueError, match=why.replace("(", r"\(").replace(")", r"\)")):
            f([p], df, dp, 4, [tri], 1.0, **dict(ok, **kw))
    for mu in (-1.0, float("nan"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="mu"):
            f([p], df, dp, 4, [tri], mu, **ok)
    with pytest.raises(ValueError, match="neither an echo term nor a final term"):
        f([p], df, dp, 4, None, 1.0, b=[(z, z)], gains=ok["gains"])
    with pytest.raises(ValueError, match="targets are given for an echo term that has no weights"):
        f([p], df, dp, 4, None, 1.0, weights_final=[tri], **ok)
    r = mbfir.refine_bloch_train_sched_lm_batch
    for kw, why in ((dict(solver="gpu"), "solver must be 'host' or 'device'"), (dict(solver="device", cg=0), "cg at least 1"),
                    (dict(solver="device", iters=-1), "iters must be at least 0"), (dict(solver="device", vary=()), "vary must name"),
                    (dict(solver="device", ntr=[4, 5], pulses=[p, p], targets=[tg, tg], weights=[tri, tri]), "must share ntr")):
        a = dict(pulses=[p], ntr=4, targets=[tg], weights=[tri])
        a.update({k: kw[k] for k in a if k in kw})
        rest = {k: v for k, v in kw.items() if k not in a}
        with pytest.raises(ValueError, match=why):
            r(a["pulses"], df, dp, a["ntr"], a["targets"], a["weights"], **rest)
    with pytest.raises(ValueError, match="no pulses"):
        r([], df, dp, 4, [], [], solver="device")
