"""NumPy restatement of the Levenberg-Marquardt step that mbfir.abr_lm_step_batch / abr2_lm_step_batch solve on the device (helper
of tests/test_simlm_cpu.py and tests/test_simlm_gpu.py; not collected).  Conjugate gradients on (H + mu I) d = b from d = 0 in the
inner product of the real forms, with mbfir.refine's _dot and the order of operations of its host loop, so that on the same
operator it reproduces that loop's bits.  The operator is a callable p -> H p: simgn_ref.gn here (step), or whatever the caller
passes (cg_solve), the shipped device call for instance."""
import importlib.util
import os

import numpy as np

from mbfir.refine import _dot

_spec = importlib.util.spec_from_file_location("simgn_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "simgn_ref.py"))
gnref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gnref)

STATUS = ("rtol", "cg", "breakdown")


def cg_solve(op, b, mu, cg, rtol):
    """(d, info) with info = dict(ncg, rr, gg, status).  The pulse runs while ncg < cg and rr > rtol gg; an iteration whose
    <p, (H + mu) p> is not finite or not > 0 ends it with status 'breakdown' and d, r, ncg as they were; otherwise the status is
    'rtol' when rr > rtol gg no longer holds and 'cg' when it still does (the cap ended the loop)."""
    b = np.asarray(b, dtype=np.complex128)
    d = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr = _dot(r, r)
    gg = rr
    ncg, broke = 0, False
    while ncg < cg and rr > rtol * gg:
        hp = op(p)
        ap = hp + mu * p
        pap = _dot(p, ap)
        if not (np.isfinite(pap) and pap > 0):
            broke = True
            break
        alpha = rr / pap
        d, r = d + alpha * p, r - alpha * ap
        rr, old = _dot(r, r), rr
        p = r + (rr / old) * p
        ncg += 1
    status = "breakdown" if broke else ("cg" if rr > rtol * gg else "rtol")
    return d, dict(ncg=ncg, rr=rr, gg=gg, status=status)


def step(rf, g, x, b, w, mu, scales, kind="ex", y=None, hard_pulse=False, cg=8, rtol=1e-6, target=None):
    """One pulse of abr_lm_step_batch (y None) or abr2_lm_step_batch on simgn_ref: (d, info), info with 'loss' and 'grad' at rf + d
    when a target is given."""
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    d, info = cg_solve(lambda p: gnref.gn(rf, g, x, p, w, scales, kind, y, hard_pulse), b, mu, cg, rtol)
    if target is not None:
        info["loss"], info["grad"] = gnref.lsq(rf + d, g, x, target, w, scales, kind, y, hard_pulse)
    return d, info
