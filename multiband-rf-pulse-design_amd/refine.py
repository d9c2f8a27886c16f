"""Batched Levenberg-Marquardt refinement of RF pulses against a target profile: the loop of
examples/spiral2d_gauss_newton.py, run in lock step over many pulses on the fused device products.  Per pulse, with
L = 1/2 sum w |f - t|^2, g = J^H W (f - t) and H = J^H W J (abr_lsq_batch / abr_gn_batch and their 2D twins):
    each step solves (H + mu I) d = -g by conjugate gradients from d = 0 on the real form of rf, one gn call per CG iteration over
    the pulses whose CG is still running (one direction each), and tries rf + d with one lsq call, which also returns the gradient
    of the next step;  mu <- mu / 3 after a step that lowers L, mu <- 4 mu after one that does not (the step is then solved again);
    the first mu is 1e-3 times the Rayleigh quotient <g, H g> / <g, g>.
refine_bloch_batch runs the same loop (_lm_loop, _host_steps) on bloch_lsq_batch / bloch_gn_batch, the Bloch model with relaxation,
or with solver='device' each step as one bloch_lm_step_batch call, or with steady_state=True on bloch_ss_lsq_batch /
bloch_ss_gn_batch, the steady state of the period; refine_bloch_ss_batch is that loop with both solvers, the device one
taking each step as one bloch_ss_lm_step_batch call.
refine_bloch_train_batch runs the loop on bloch_train_lsq_batch / bloch_train_gn_batch, the echoes of a pulse train;
refine_bloch_train_lm_batch is that loop with both solvers, the device one taking each step as one bloch_train_lm_step_batch call
(DESIGN 8ac).
refine_bloch_train_sched_batch refines the train's schedule, the gain and the RF phase of every repetition, on
bloch_train_lsq_sched_batch / bloch_train_gn_sched_batch: a schedule has 2 ntr real unknowns, so each step forms the dense H
with one gn call and solves (H + mu I) d = -g by a Cholesky factorisation on the host instead of conjugate gradients.
refine_bloch_train_sched_lm_batch is that loop with both solvers, the device one on bloch_train_lm_step_sched_batch, which evaluates a
trial and solves the next step in the same call.
Every per-pulse scalar is host arithmetic on that pulse's own numbers, and the device calls return bits that do not depend on the
batch, so a pulse refined in a batch has the bits of the same pulse refined alone."""
import importlib

import numpy as np

MU_MAX = 1e12          # a pulse whose mu grows past this gives up


def _dot(u, v):
    """the inner product of the real forms"""
    return float((np.conj(u) * v).real.sum())


def refine_batch(pulses, x, *args, profile="ex", scales=(1.0,), hard_pulse=False, iters=5, cg=8, mu0=None, rtol=1e-6, solver="host",
                 ctx=None):
    """refine_batch(pulses, x, targets, weights, ...) for abr_batch's model, refine_batch(pulses, x, y, targets, weights, ...) for
    abr2_batch's.  pulses: rf or (rf, g) each; x (and y): one grid shared by every pulse or a list of one per pulse; targets,
    weights, profile, scales and hard_pulse as for abr_lsq_batch / abr2_lsq_batch.  iters: accepted steps per pulse at the most;
    cg: CG iterations per step at the most, stopped once |residual|^2 <= rtol |g|^2; mu0: None (the Rayleigh quotient), a number,
    or one number per pulse.  Returns (rfs, infos): the refined rf per pulse and a dict per pulse with 'losses' (L at the start and
    after every accepted step), 'mu' (the last one), 'status' ('iters', 'converged': a zero gradient, or 'gave_up': mu past 1e12),
    'refused' (steps that did not lower L) and 'calls' (the lsq and gn calls the pulse took part in).  solver: 'host' runs the CG
    recurrence here, one gn call per iteration; 'device' solves and tries each step in one abr_lm_step_batch / abr2_lm_step_batch
    call over the active pulses ('calls' then counts them under 'lm'), a CG breakdown counting as a refused step."""
    mb = importlib.import_module(__package__)
    if len(args) == 2:
        two, y = False, None
        targets, weights = args
    elif len(args) == 3:
        two = True
        y, targets, weights = args
    else:
        raise ValueError("refine_batch: takes (pulses, x, targets, weights) or (pulses, x, y, targets, weights)")
    pulses = list(pulses)
    P = len(pulses)
    if P == 0:
        raise ValueError("refine_batch: no pulses")
    targets, weights = list(targets), list(weights)
    if len(targets) != P or len(weights) != P:
        raise ValueError("refine_batch: %d targets and %d weight arrays for %d pulses" % (len(targets), len(weights), P))
    if iters < 0 or cg < 1:
        raise ValueError("refine_batch: iters must be at least 0 and cg at least 1")
    if solver not in ("host", "device"):
        raise ValueError("refine_batch: solver must be 'host' or 'device', not %r" % (solver,))
    gs = [p[1] if isinstance(p, tuple) else None for p in pulses]
    rfs = [np.array(p[0] if isinstance(p, tuple) else p, dtype=np.complex128).ravel() for p in pulses]
    kw = dict(profile=profile, scales=scales, hard_pulse=hard_pulse, ctx=ctx)

    def grid(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P and all(np.ndim(e) >= 1 for e in v) else v

    def pack(idx, rf_of):
        return [rf_of[q] if gs[q] is None else (rf_of[q], gs[q]) for q in idx]

    def lsq(idx, rf_of):
        pos = (grid(x, idx), grid(y, idx)) if two else (grid(x, idx),)
        fn = mb.abr2_lsq_batch if two else mb.abr_lsq_batch
        for q in idx:
            infos[q]["calls"]["lsq"] += 1
        return fn(pack(idx, rf_of), *pos, [targets[q] for q in idx], [weights[q] for q in idx], **kw)

    def gn(idx, v_of):
        pos = (grid(x, idx), grid(y, idx)) if two else (grid(x, idx),)
        fn = mb.abr2_gn_batch if two else mb.abr_gn_batch
        for q in idx:
            infos[q]["calls"]["gn"] += 1
        return fn(pack(idx, rfs), *pos, [v_of[q] for q in idx], [weights[q] for q in idx], **kw)

    def lm(idx, grad, mu):
        """the step of every active pulse, solved and tried on the device: (rf + d, L and g there, whether CG broke down)"""
        pos = (grid(x, idx), grid(y, idx)) if two else (grid(x, idx),)
        fn = mb.abr2_lm_step_batch if two else mb.abr_lm_step_batch
        for q in idx:
            infos[q]["calls"]["lm"] += 1
        res = fn(pack(idx, rfs), *pos, [-grad[q] for q in idx], [weights[q] for q in idx], [mu[q] for q in idx],
                 targets=[targets[q] for q in idx], cg=cg, rtol=rtol, **kw)
        return [(rfs[q] + d, i["loss"], i["grad"], i["status"] == "breakdown") for q, (d, i) in zip(idx, res)]

    calls = dict(lsq=0, gn=0, lm=0) if solver == "device" else dict(lsq=0, gn=0)
    infos = [dict(losses=[], mu=None, status="iters", refused=0, calls=dict(calls)) for _ in range(P)]
    if solver == "device":
        step = lm
    else:
        def step(idx, grad, mu):
            return _host_steps(idx, rfs, grad, mu, lsq, gn, cg, rtol)
    return _lm_loop(rfs, infos, lsq, gn, step, iters, mu0)


def _host_steps(idx, rfs, grad, mu, lsq, gn, cg, rtol):
    """The step of every pulse of idx on the host: CG on (H + mu I) d = -g from d = 0, one gn call per iteration over the pulses
    whose CG still runs, then one lsq call at rf + d -> [(rf + d, L and g there, False)]"""
    d = {q: np.zeros_like(rfs[q]) for q in idx}
    r = {q: -grad[q] for q in idx}
    p = {q: r[q].copy() for q in idx}
    rr = {q: _dot(r[q], r[q]) for q in idx}
    gg = dict(rr)
    ncg = {q: 0 for q in idx}
    while True:
        run = [q for q in idx if ncg[q] < cg and rr[q] > rtol * gg[q]]
        if not run:
            break
        for q, hp in zip(run, gn(run, p)):
            ap = hp + mu[q] * p[q]
            alpha = rr[q] / _dot(p[q], ap)
            d[q], r[q] = d[q] + alpha * p[q], r[q] - alpha * ap
            rr[q], old = _dot(r[q], r[q]), rr[q]
            p[q] = r[q] + (rr[q] / old) * p[q]
            ncg[q] += 1
    trial = {q: rfs[q] + d[q] for q in idx}
    return [(trial[q], L, g, False) for q, (L, g) in zip(idx, lsq(idx, trial))]


def _lm_loop(rfs, infos, lsq, gn, step, iters, mu0):
    """The lock-step Levenberg-Marquardt loop of refine_batch and refine_bloch_batch, from the first loss to the end.  rfs: the
    pulses' samples, replaced in place by the accepted trials; lsq(idx, rf_of) -> [(L, g)] and gn(idx, v_of) -> [H v] for the
    pulses idx (gn at the current rfs); step(idx, grad, mu) -> [(trial, L and g at the trial, whether the solve broke down)].
    Returns (rfs, infos)."""
    P = len(rfs)
    every = list(range(P))
    loss, grad, done = [0.0] * P, [None] * P, [0] * P
    for q, (L, g) in zip(every, lsq(every, rfs)):
        loss[q], grad[q] = L, g
        infos[q]["losses"].append(L)
    active = []
    for q in every:
        if iters == 0:
            continue
        if _dot(grad[q], grad[q]) == 0.0:
            infos[q]["status"] = "converged"
            continue
        active.append(q)
    mu = [None] * P
    if mu0 is not None:
        m = np.broadcast_to(np.asarray(mu0, dtype=np.float64), (P,))
        mu = [float(v) for v in m]
    need = [q for q in active if mu[q] is None]
    if need:
        for q, hg in zip(need, gn(need, grad)):
            mu[q] = 1e-3 * _dot(grad[q], hg) / _dot(grad[q], grad[q])       # a Rayleigh quotient of H sets the scale of mu
    while active:
        still = []
        for q, (trial, L, g, broke) in zip(active, step(active, grad, mu)):
            if L < loss[q] and not broke:
                rfs[q], loss[q], grad[q], mu[q] = trial, L, g, mu[q] / 3
                infos[q]["losses"].append(L)
                done[q] += 1
                if _dot(g, g) == 0.0:
                    infos[q]["status"] = "converged"
                elif done[q] < iters:
                    still.append(q)
            else:
                mu[q] *= 4
                infos[q]["refused"] += 1
                if mu[q] > MU_MAX:
                    infos[q]["status"] = "gave_up"
                else:
                    still.append(q)
        active = still
    for q in every:
        infos[q]["mu"] = mu[q]
    return rfs, infos


def refine_bloch_batch(pulses, df, dp, targets, weights, *, scales=(1.0,), m0=None, iters=5, cg=8, mu0=None, rtol=1e-6, solver="host",
                       steady_state=False, magnitude=False, ctx=None):
    """refine_batch for bloch_batch's model, relaxation included: the same lock-step Levenberg-Marquardt / CG loop
    on bloch_lsq_batch and bloch_gn_batch.  pulses: (b1, gr, tp, t1, t2, nucleus) each, of which only b1 changes; df, dp:
    one grid shared by every pulse or a list of one per pulse; targets, weights, scales and m0 (None, one (mx, my, mz), or a list
    of one per pulse) as for bloch_lsq_batch; iters, cg, mu0 and rtol as for refine_batch.  Returns (b1s, infos) as refine_batch
    does.  solver: 'host' runs the CG recurrence on the host, one bloch_gn_batch call per iteration; 'device' solves and tries each
    step in one bloch_lm_step_batch call over the active pulses ('calls' then counts them under 'lm'), a CG breakdown counting as a
    refused step.  steady_state: fit the steady state of the period (bloch_batch's mode 1) instead of the end point, on
    bloch_ss_lsq_batch and bloch_ss_gn_batch; each pulse is then one period, targets and weights lie as mode 1's outputs
    do, there is no m0, and the solver is 'host' (refine_bloch_ss_batch has both solvers).  magnitude: fit (|Mxy|, mz) instead of
    (mx, my, mz): targets and weights are pairs (xy, z) per pulse, every call of the loop is made with magnitude=True,
    and both solvers work.  A pulse refined in a batch has the bits of the same pulse refined alone."""
    return _refine_bloch("refine_bloch_batch", False, pulses, df, dp, targets, weights, scales, m0, iters, cg, mu0, rtol, solver,
                         steady_state, magnitude, ctx)


def refine_bloch_ss_batch(pulses, df, dp, targets, weights, *, scales=(1.0,), iters=5, cg=8, mu0=None, rtol=1e-6, solver="host",
                          magnitude=False, ctx=None):
    """refine_bloch_batch(steady_state=True) with both solvers: the lock-step Levenberg-Marquardt / CG loop on the
    steady state of the period, bloch_batch's mode 1.  pulses: (b1, gr, tp, t1, t2, nucleus) each, one period, of which only b1
    changes; df, dp, targets, weights and scales as for bloch_ss_lsq_batch; iters, cg, mu0 and rtol as for refine_batch; there is no
    m0.  Returns (b1s, infos) as refine_batch does.  solver: 'host' runs the CG recurrence on the host, one bloch_ss_gn_batch call
    per iteration, and returns the bits and the 'calls' of refine_bloch_batch(steady_state=True); 'device' solves and tries each
    step in one bloch_ss_lm_step_batch call over the active pulses ('calls' then counts them under 'lm'), a CG breakdown counting as
    a refused step.  magnitude: as for refine_bloch_batch.  A pulse refined in a batch has the bits of the same pulse refined
    alone."""
    return _refine_bloch("refine_bloch_ss_batch", True, pulses, df, dp, targets, weights, scales, None, iters, cg, mu0, rtol, solver,
                         True, magnitude, ctx)


def _refine_bloch(who, ss_device, pulses, df, dp, targets, weights, scales, m0, iters, cg, mu0, rtol, solver, steady_state, magnitude,
                  ctx):
    """The body of refine_bloch_batch and refine_bloch_ss_batch; who: the entry point, for the messages; ss_device: whether the
    steady state's device step may be taken."""
    mb = importlib.import_module(__package__)
    pulses = list(pulses)
    P = len(pulses)
    if P == 0:
        raise ValueError("%s: no pulses" % who)
    if steady_state and m0 is not None:
        raise ValueError("%s: the steady state does not depend on m0; with steady_state, m0 must be None" % who)
    if steady_state and solver == "device" and not ss_device:
        raise ValueError("%s: the steady-state device step is not built into this entry point; call refine_bloch_ss_batch(..., "
                         "solver='device')" % who)
    targets, weights = list(targets), list(weights)
    if len(targets) != P or len(weights) != P:
        raise ValueError("%s: %d target and %d weight %s for %d pulses"
                         % (who, len(targets), len(weights), "pairs" if magnitude else "triples", P))
    if iters < 0 or cg < 1:
        raise ValueError("%s: iters must be at least 0 and cg at least 1" % who)
    if solver not in ("host", "device"):
        raise ValueError("%s: solver must be 'host' or 'device', not %r" % (who, solver))
    rest = [tuple(p[1:]) for p in pulses]
    b1s = [np.array(p[0], dtype=np.complex128).ravel() for p in pulses]
    each = isinstance(m0, list) and len(m0) == P and all(isinstance(t, tuple) and len(t) == 3 for t in m0)

    def grid(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P and all(np.ndim(e) >= 1 for e in v) else v

    def args(idx, b1_of):
        return [(b1_of[q],) + rest[q] for q in idx], grid(df, idx), grid(dp, idx)

    def kw(idx):
        mag = dict(magnitude=True) if magnitude else {}                          # without it the calls are the ones they were
        if steady_state:
            return dict(scales=scales, ctx=ctx, **mag)
        return dict(scales=scales, m0=[m0[q] for q in idx] if each else m0, ctx=ctx, **mag)

    def lsq(idx, b1_of):
        for q in idx:
            infos[q]["calls"]["lsq"] += 1
        fn = mb.bloch_ss_lsq_batch if steady_state else mb.bloch_lsq_batch
        return fn(*args(idx, b1_of), [targets[q] for q in idx], [weights[q] for q in idx], **kw(idx))

    def gn(idx, v_of):
        for q in idx:
            infos[q]["calls"]["gn"] += 1
        fn = mb.bloch_ss_gn_batch if steady_state else mb.bloch_gn_batch
        return fn(*args(idx, b1s), [v_of[q] for q in idx], [weights[q] for q in idx], **kw(idx))

    def lm(idx, grad, mu):
        """the step of every active pulse, solved and tried on the device: (b1 + d, L and g there, whether CG broke down)"""
        for q in idx:
            infos[q]["calls"]["lm"] += 1
        fn = mb.bloch_ss_lm_step_batch if steady_state else mb.bloch_lm_step_batch
        res = fn(*args(idx, b1s), [-grad[q] for q in idx], [weights[q] for q in idx], [mu[q] for q in idx],
                 targets=[targets[q] for q in idx], cg=cg, rtol=rtol, **kw(idx))
        return [(b1s[q] + d, i["loss"], i["grad"], i["status"] == "breakdown") for q, (d, i) in zip(idx, res)]

    def step(idx, grad, mu):
        return _host_steps(idx, b1s, grad, mu, lsq, gn, cg, rtol)

    calls = dict(lsq=0, gn=0, lm=0) if solver == "device" else dict(lsq=0, gn=0)
    infos = [dict(losses=[], mu=None, status="iters", refused=0, calls=dict(calls)) for _ in range(P)]
    return _lm_loop(b1s, infos, lsq, gn, lm if solver == "device" else step, iters, mu0)


def refine_bloch_train_batch(pulses, df, dp, ntr, targets, weights, *, rep_weights=None, targets_final=None, weights_final=None,
                             phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, iters=5, cg=8, mu0=None,
                             rtol=1e-6, solver="host", magnitude=False, ctx=None):
    """refine_batch for bloch_train_batch's model: the same lock-step Levenberg-Marquardt / CG loop on
    bloch_train_lsq_batch and bloch_train_gn_batch.  pulses: (b1, gr, tp, t1, t2, nucleus) each, one period, of which only b1
    changes; df, dp: one grid shared by every pulse or a list of one per pulse; ntr, targets, weights, rep_weights, targets_final,
    weights_final, phases, gains, echo, scales, m0, meq and demod as for bloch_train_lsq_batch, what is given per pulse as a Python
    list of one entry per pulse; iters, cg, mu0 and rtol as for refine_batch.  Returns (b1s, infos) as refine_batch does.  solver:
    'host' runs the CG recurrence on the host, one bloch_train_gn_batch call per iteration; this entry point has no device step
    (refine_bloch_train_lm_batch has both solvers).  magnitude: fit (|Mxy|, mz) of every echo and of the final state
    instead of the vectors: targets, weights, targets_final and weights_final are pairs (xy, z) per pulse and every call
    of the loop is made with magnitude=True.  A pulse refined in a batch has the bits of the same pulse refined alone."""
    return _refine_bloch_train("refine_bloch_train_batch", False, pulses, df, dp, ntr, targets, weights, rep_weights, targets_final,
                               weights_final, phases, gains, echo, scales, m0, meq, demod, iters, cg, mu0, rtol, solver, magnitude,
                               ctx)


def refine_bloch_train_lm_batch(pulses, df, dp, ntr, targets, weights, *, rep_weights=None, targets_final=None, weights_final=None,
                                phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, iters=5, cg=8,
                                mu0=None, rtol=1e-6, solver="host", magnitude=False, ctx=None):
    """refine_bloch_train_batch with both solvers: the lock-step Levenberg-Marquardt / CG loop on the echoes of a
    pulse train; arguments and return value as for refine_bloch_train_batch.  solver: 'host' runs the CG recurrence on the host, one
    bloch_train_gn_batch call per iteration, and returns the bits and the 'calls' of refine_bloch_train_batch; 'device' solves and
    tries each step in one bloch_train_lm_step_batch call over the active pulses ('calls' then counts them under 'lm'), a CG
    breakdown counting as a refused step.  magnitude: as for refine_bloch_train_batch, with both solvers.  A pulse refined in a batch
    has the bits of the same pulse refined alone."""
    return _refine_bloch_train("refine_bloch_train_lm_batch", True, pulses, df, dp, ntr, targets, weights, rep_weights, targets_final,
                               weights_final, phases, gains, echo, scales, m0, meq, demod, iters, cg, mu0, rtol, solver, magnitude,
                               ctx)


def _refine_bloch_train(who, device_ok, pulses, df, dp, ntr, targets, weights, rep_weights, targets_final, weights_final, phases,
                        gains, echo, scales, m0, meq, demod, iters, cg, mu0, rtol, solver, magnitude, ctx):
    """The body of refine_bloch_train_batch and refine_bloch_train_lm_batch; who: the entry point, for the messages; device_ok:
    whether the device step may be taken."""
    mb = importlib.import_module(__package__)
    pulses = list(pulses)
    P = len(pulses)
    if P == 0:
        raise ValueError("%s: no pulses" % who)
    if not device_ok:
        if solver == "device":
            raise ValueError("%s: the train has no device step in this entry point; solver must be 'host' (call "
                             "refine_bloch_train_lm_batch(..., solver='device'))" % who)
        if solver != "host":
            raise ValueError("%s: solver must be 'host', not %r" % (who, solver))
    elif solver not in ("host", "device"):
        raise ValueError("%s: solver must be 'host' or 'device', not %r" % (who, solver))
    if iters < 0 or cg < 1:
        raise ValueError("%s: iters must be at least 0 and cg at least 1" % who)
    if targets is None and targets_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    for what, v in (("targets", targets), ("weights", weights), ("targets_final", targets_final), ("weights_final", weights_final)):
        if v is not None and len(list(v)) != P:
            raise ValueError("%s: %d %s %s for %d pulses" % (who, len(list(v)), what, "pairs" if magnitude else "triples", P))
    mag = dict(magnitude=True) if magnitude else {}                              # without it the calls are the ones they were
    rest = [tuple(p[1:]) for p in pulses]
    b1s = [np.array(p[0], dtype=np.complex128).ravel() for p in pulses]
    each_m0 = isinstance(m0, list) and len(m0) == P and all(isinstance(t, tuple) and len(t) == 3 for t in m0)

    def grid(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P and all(np.ndim(e) >= 1 for e in v) else v

    def pick(v, idx):
        """a keyword given per pulse (a Python list of P entries) -> the entries of idx; anything else serves every pulse"""
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P else v

    def sub(v, idx):
        return None if v is None else [v[q] for q in idx]

    def kw(idx):
        return dict(rep_weights=pick(rep_weights, idx), weights_final=sub(weights_final, idx), phases=pick(phases, idx),
                    gains=pick(gains, idx), echo=pick(echo, idx), scales=scales, m0=[m0[q] for q in idx] if each_m0 else m0,
                    meq=pick(meq, idx) if isinstance(meq, list) else meq, demod=demod, ctx=ctx, **mag)

    def args(idx, b1_of):
        return [(b1_of[q],) + rest[q] for q in idx], grid(df, idx), grid(dp, idx), pick(ntr, idx)

    def lsq(idx, b1_of):
        for q in idx:
            infos[q]["calls"]["lsq"] += 1
        return mb.bloch_train_lsq_batch(*args(idx, b1_of), sub(targets, idx), sub(weights, idx), targets_final=sub(targets_final, idx),
                                        **kw(idx))

    def gn(idx, v_of):
        for q in idx:
            infos[q]["calls"]["gn"] += 1
        return mb.bloch_train_gn_batch(*args(idx, b1s), [v_of[q] for q in idx], sub(weights, idx), **kw(idx))

    def lm(idx, grad, mu):
        """the step of every active pulse, solved and tried on the device: (b1 + d, L and g there, whether CG broke down)"""
        for q in idx:
            infos[q]["calls"]["lm"] += 1
        res = mb.bloch_train_lm_step_batch(*args(idx, b1s), [-grad[q] for q in idx], sub(weights, idx), [mu[q] for q in idx],
                                           targets=sub(targets, idx), targets_final=sub(targets_final, idx), cg=cg, rtol=rtol,
                                           **kw(idx))
        return [(b1s[q] + d, i["loss"], i["grad"], i["status"] == "breakdown") for q, (d, i) in zip(idx, res)]

    def step(idx, grad, mu):
        return _host_steps(idx, b1s, grad, mu, lsq, gn, cg, rtol)

    calls = dict(lsq=0, gn=0, lm=0) if solver == "device" else dict(lsq=0, gn=0)
    infos = [dict(losses=[], mu=None, status="iters", refused=0, calls=dict(calls)) for _ in range(P)]
    return _lm_loop(b1s, infos, lsq, gn, lm if solver == "device" else step, iters, mu0)


def refine_bloch_train_sched_batch(pulses, df, dp, ntr, targets, weights, *, vary=("gains", "phases"), iters=5, mu0=None,
                                   rep_weights=None, targets_final=None, weights_final=None, phases=np.pi, gains=1.0, echo=None,
                                   scales=(1.0,), m0=None, meq=1.0, demod=False, magnitude=False, ctx=None):
    """Lock-step Levenberg-Marquardt on the schedule of a pulse train, the gain and the RF phase of every repetition, with the pulses
    held fixed: _lm_loop on bloch_train_lsq_sched_batch / bloch_train_gn_sched_batch.  pulses, df, dp, targets, weights,
    rep_weights, targets_final, weights_final, echo, scales, m0, meq and demod as for refine_bloch_train_batch; ntr: an int, the pulses
    of a call share it; phases / gains: the starting schedule, as bloch_train_batch takes them.  vary: ("gains", "phases"),
    ("gains",) or ("phases",): the part that moves; the iterate is the real vector [gains; phases] restricted to it, of length n =
    ntr x len(vary).  Each step forms H once per accepted iterate (one gn call with the n unit directions, kept while steps are
    refused: H does not depend on mu), symmetrises it, solves (H + mu I) d = -g by a dense Cholesky factorisation on the host and
    evaluates one lsq call at the trial.  iters and mu0 as for refine_batch (mu0 None: 1e-3 times the Rayleigh quotient <g, H g> /
    <g, g>, one gn call).  Returns (schedules, infos): per pulse (gains, phases), float64 of shape (ntr,), and refine_batch's info
    dict ('calls' counts 'lsq' and 'gn').  Without "gains" in vary the period's tangent is never launched.  magnitude: fit
    (|Mxy|, mz) of every echo and of the final state instead of the vectors: targets and weights are pairs (xy, z) per
    pulse and every call of the loop is made with magnitude=True.  A pulse refined in a batch has the bits of the same pulse refined
    alone."""
    who = "refine_bloch_train_sched_batch"
    mb = importlib.import_module(__package__)
    pulses = list(pulses)
    P = len(pulses)
    if P == 0:
        raise ValueError("%s: no pulses" % who)
    vg, vp = mb._sched_vary(who, vary)
    if iters < 0:
        raise ValueError("%s: iters must be at least 0" % who)
    if targets is None and targets_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    for what, v in (("targets", targets), ("weights", weights), ("targets_final", targets_final), ("weights_final", weights_final)):
        if v is not None and len(list(v)) != P:
            raise ValueError("%s: %d %s %s for %d pulses" % (who, len(list(v)), what, "pairs" if magnitude else "triples", P))
    mag = dict(magnitude=True) if magnitude else {}                              # without it the calls are the ones they were
    n = mb._train_ints(who, "ntr", ntr, P)
    if any(e != n[0] for e in n):
        raise ValueError("%s: the pulses of a call must share ntr" % who)
    if n[0] < 1:
        raise ValueError("%s: ntr of pulse 0 must be at least 1" % who)
    N = n[0]
    g0 = [np.array(v, dtype=np.float64) for v in mb._train_tables(who, "gains", gains, n, False)]
    p0 = [np.array(v, dtype=np.float64) for v in mb._train_tables(who, "phases", phases, n, True)]
    each_m0 = isinstance(m0, list) and len(m0) == P and all(isinstance(t, tuple) and len(t) == 3 for t in m0)

    def grid(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P and all(np.ndim(e) >= 1 for e in v) else v

    def pick(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P else v

    def sub(v, idx):
        return None if v is None else [v[q] for q in idx]

    def sched(q, x):
        """the iterate of pulse q -> (gains, phases)"""
        return (x[:N] if vg else g0[q]), (x[N:] if vg and vp else x if vp else p0[q])

    def kw(idx, x_of):
        sc = [sched(q, x_of[q]) for q in idx]
        return dict(rep_weights=pick(rep_weights, idx), weights_final=sub(weights_final, idx), phases=[s[1] for s in sc],
                    gains=[s[0] for s in sc], echo=pick(echo, idx), scales=scales, m0=[m0[q] for q in idx] if each_m0 else m0,
                    meq=pick(meq, idx) if isinstance(meq, list) else meq, demod=demod, ctx=ctx, **mag)

    def args(idx):
        return [pulses[q] for q in idx], grid(df, idx), grid(dp, idx), N

    def halves(v):
        return (v[..., :N] if vg else None), (v[..., N:] if vg and vp else v if vp else None)

    def join(a, b):
        return np.concatenate([v for v in (a, b) if v is not None], -1)

    def lsq(idx, x_of):
        for q in idx:
            infos[q]["calls"]["lsq"] += 1
        res = mb.bloch_train_lsq_sched_batch(*args(idx), sub(targets, idx), sub(weights, idx), targets_final=sub(targets_final, idx),
                                             grad_gains=vg, grad_phases=vp, **kw(idx, x_of))
        return [(r[0], join(r[1], r[2])) for r in res]

    def gn_dirs(idx, dirs):
        """H along dirs[q] ((n,) or (K, n)) of every pulse of idx at the current iterate, the two halves joined"""
        for q in idx:
            infos[q]["calls"]["gn"] += 1
        hv = [halves(dirs[q]) for q in idx]
        res = mb.bloch_train_gn_sched_batch(*args(idx), sub(weights, idx), tangents_gains=[h[0] for h in hv] if vg else None,
                                            tangents_phases=[h[1] for h in hv] if vp else None, prod_gains=vg, prod_phases=vp,
                                            **kw(idx, xs))
        return [join(a, b) for a, b in res]

    def gn(idx, v_of):
        return gn_dirs(idx, v_of)

    eye = np.eye(N * (int(vg) + int(vp)))
    held = {}                                                                    # q -> (the iterate H was formed at, H)

    def step(idx, grad, mu):
        need = [q for q in idx if q not in held or held[q][0] is not xs[q]]
        if need:
            for q, H in zip(need, gn_dirs(need, {q: eye for q in need})):
                held[q] = (xs[q], (H + H.T) / 2)
        trial, broke = {}, {}
        for q in idx:
            try:
                c = np.linalg.cholesky(held[q][1] + mu[q] * eye)
                trial[q], broke[q] = xs[q] + np.linalg.solve(c.T, np.linalg.solve(c, -grad[q])), False
            except np.linalg.LinAlgError:                                        # not positive definite to rounding: a refused step
                trial[q], broke[q] = xs[q], True
        ok = [q for q in idx if not broke[q]]
        at = dict(zip(ok, lsq(ok, trial))) if ok else {}
        return [(trial[q],) + (at[q] if q in at else (np.inf, grad[q])) + (broke[q],) for q in idx]

    xs = [join(g0[q] if vg else None, p0[q] if vp else None) for q in range(P)]
    infos = [dict(losses=[], mu=None, status="iters", refused=0, calls=dict(lsq=0, gn=0)) for _ in range(P)]
    xs, infos = _lm_loop(xs, infos, lsq, gn, step, iters, mu0)
    return [tuple(np.array(v) for v in sched(q, xs[q])) for q in range(P)], infos


def refine_bloch_train_sched_lm_batch(pulses, df, dp, ntr, targets, weights, *, vary=("gains", "phases"), iters=5, mu0=None,
                                      rep_weights=None, targets_final=None, weights_final=None, phases=np.pi, gains=1.0, echo=None,
                                      scales=(1.0,), m0=None, meq=1.0, demod=False, solver="host", cg=8, rtol=1e-6, magnitude=False,
                                      ctx=None):
    """refine_bloch_train_sched_batch with both solvers; arguments and return value as for that function.  solver:
    'host' is refine_bloch_train_sched_batch, bit for bit, infos included (cg and rtol are not used).  'device' takes the steps with
    bloch_train_lm_step_sched_batch, which evaluates and solves at the same schedule, through the same _lm_loop: the call that
    evaluates a trial x + d also solves, speculatively, the next step at the trial with the damping the loop will use if the trial is
    accepted (mu / 3), so an accepted iterate costs one call and one set of propagator sweeps where the host solver runs two.  The
    speculative d is kept per pulse, keyed by the iterate and by mu; a pulse without a valid one (the first step, or after a refused
    step) takes part in one solve-only call with b = -grad first.  cg: CG iterations per step at the most (n = ntr x len(vary)
    reaches the exact step to rounding), stopped once |residual|^2 <= rtol |g|^2; a CG breakdown counts as a refused step.
    'calls' then counts the fused calls under 'lm'.  The speculative solve of a call is skipped (cg = 0) when every trial in it would
    end its pulse's refinement; in a batch whose pulses are at different steps (after refusals) a pulse on its last trial still
    pays the cg rounds its neighbours need, and their result is dropped.  The speculative d is never part of a result, so a pulse
    refined in a batch has the bits of the same pulse refined alone.  magnitude: as for refine_bloch_train_sched_batch, with both
    solvers."""
    who = "refine_bloch_train_sched_lm_batch"
    mb = importlib.import_module(__package__)
    if solver not in ("host", "device"):
        raise ValueError("%s: solver must be 'host' or 'device', not %r" % (who, solver))
    if solver == "host":
        return refine_bloch_train_sched_batch(pulses, df, dp, ntr, targets, weights, vary=vary, iters=iters, mu0=mu0,
                                              rep_weights=rep_weights, targets_final=targets_final, weights_final=weights_final,
                                              phases=phases, gains=gains, echo=echo, scales=scales, m0=m0, meq=meq, demod=demod,
                                              magnitude=magnitude, ctx=ctx)
    pulses = list(pulses)
    P = len(pulses)
    if P == 0:
        raise ValueError("%s: no pulses" % who)
    vg, vp = mb._sched_vary(who, vary)
    if iters < 0 or cg < 1:
        raise ValueError("%s: iters must be at least 0 and cg at least 1" % who)
    if targets is None and targets_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    for what, v in (("targets", targets), ("weights", weights), ("targets_final", targets_final), ("weights_final", weights_final)):
        if v is not None and len(list(v)) != P:
            raise ValueError("%s: %d %s %s for %d pulses" % (who, len(list(v)), what, "pairs" if magnitude else "triples", P))
    mag = dict(magnitude=True) if magnitude else {}                              # without it the calls are the ones they were
    n = mb._train_ints(who, "ntr", ntr, P)
    if any(e != n[0] for e in n):
        raise ValueError("%s: the pulses of a call must share ntr" % who)
    if n[0] < 1:
        raise ValueError("%s: ntr of pulse 0 must be at least 1" % who)
    N = n[0]
    g0 = [np.array(v, dtype=np.float64) for v in mb._train_tables(who, "gains", gains, n, False)]
    p0 = [np.array(v, dtype=np.float64) for v in mb._train_tables(who, "phases", phases, n, True)]
    each_m0 = isinstance(m0, list) and len(m0) == P and all(isinstance(t, tuple) and len(t) == 3 for t in m0)

    def grid(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P and all(np.ndim(e) >= 1 for e in v) else v

    def pick(v, idx):
        return [v[q] for q in idx] if isinstance(v, list) and len(v) == P else v

    def sub(v, idx):
        return None if v is None else [v[q] for q in idx]

    def sched(q, x):
        """the iterate of pulse q -> (gains, phases)"""
        return (x[:N] if vg else g0[q]), (x[N:] if vg and vp else x if vp else p0[q])

    def kw(idx, x_of):
        sc = [sched(q, x_of[q]) for q in idx]
        return dict(rep_weights=pick(rep_weights, idx), weights_final=sub(weights_final, idx), phases=[s[1] for s in sc],
                    gains=[s[0] for s in sc], echo=pick(echo, idx), scales=scales, m0=[m0[q] for q in idx] if each_m0 else m0,
                    meq=pick(meq, idx) if isinstance(meq, list) else meq, demod=demod, ctx=ctx, **mag)

    def args(idx):
        return [pulses[q] for q in idx], grid(df, idx), grid(dp, idx), N

    def halves(v):
        return (v[..., :N] if vg else None), (v[..., N:] if vg and vp else v if vp else None)

    def join(a, b):
        return np.concatenate([v for v in (a, b) if v is not None], -1)

    def lsq(idx, x_of):
        for q in idx:
            infos[q]["calls"]["lsq"] += 1
        res = mb.bloch_train_lsq_sched_batch(*args(idx), sub(targets, idx), sub(weights, idx), targets_final=sub(targets_final, idx),
                                             grad_gains=vg, grad_phases=vp, **kw(idx, x_of))
        return [(r[0], join(r[1], r[2])) for r in res]

    def gn(idx, v_of):
        for q in idx:
            infos[q]["calls"]["gn"] += 1
        hv = [halves(v_of[q]) for q in idx]
        res = mb.bloch_train_gn_sched_batch(*args(idx), sub(weights, idx), tangents_gains=[h[0] for h in hv] if vg else None,
                                            tangents_phases=[h[1] for h in hv] if vp else None, prod_gains=vg, prod_phases=vp,
                                            **kw(idx, xs))
        return [join(a, b) for a, b in res]

    def lm(idx, x_of, mus, b_of, evaluate, cg=cg):
        """one fused call over idx at the schedules x_of: [(d, info)], d the two varied halves joined"""
        for q in idx:
            infos[q]["calls"]["lm"] += 1
        res = mb.bloch_train_lm_step_sched_batch(*args(idx), sub(weights, idx), [mus[q] for q in idx], vary=vary,
                                                 b=None if b_of is None else [halves(b_of[q]) for q in idx],
                                                 targets=sub(targets, idx) if evaluate else None,
                                                 targets_final=sub(targets_final, idx) if evaluate else None, cg=cg, rtol=rtol,
                                                 **kw(idx, x_of))
        return [(join(dg, dp_), info) for dg, dp_, info in res]

    held = {}                                       # q -> (the iterate the step was solved at, its mu, d, whether CG broke down)

    def step(idx, grad, mu):
        need = [q for q in idx if q not in held or held[q][0] is not xs[q] or held[q][1] != mu[q]]
        if need:                                    # the first step, or after a refusal: solve only, b = -grad
            for q, (d, info) in zip(need, lm(need, xs, mu, {q: -grad[q] for q in need}, False)):
                held[q] = (xs[q], mu[q], d, info["status"] == "breakdown")
        broke = {q: held[q][3] for q in idx}
        trial = {q: xs[q] if broke[q] else xs[q] + held[q][2] for q in idx}
        ok = [q for q in idx if not broke[q]]
        at = {}
        if ok:                                      # evaluate the trials and solve the next step at each, at the next mu
            nxt = {q: mu[q] / 3 for q in ok}
            # a trial that ends its pulse's refinement if accepted needs no next step: when that holds for every pulse of the call,
            # the call evaluates only (cg is the call's, not a pulse's, so one pulse with steps left keeps the solve for all)
            ends = all(len(infos[q]["losses"]) >= iters for q in ok)
            for q, (d, info) in zip(ok, lm(ok, trial, nxt, None, True, 0 if ends else cg)):
                at[q] = (info["loss"], join(info["grad_gains"], info["grad_phases"]))
                held[q] = (trial[q], nxt[q], d, info["status"] == "breakdown")
        return [(trial[q],) + (at[q] if q in at else (np.inf, grad[q])) + (broke[q],) for q in idx]

    xs = [join(g0[q] if vg else None, p0[q] if vp else None) for q in range(P)]
    infos = [dict(losses=[], mu=None, status="iters", refused=0, calls=dict(lsq=0, gn=0, lm=0)) for _ in range(P)]
    xs, infos = _lm_loop(xs, infos, lsq, gn, step, iters, mu0)
    return [tuple(np.array(v) for v in sched(q, xs[q])) for q in range(P)], infos
