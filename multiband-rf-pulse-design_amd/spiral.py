"""Spiral 2D pulses: rf_tools/dz2d.m with csg.m, and the k-space helpers ktog.m, ktos.m and gt2cm.m.

    rf, g, ms = dz2d(nt, bw, tbp, ns, mxg, mxs)     # rf_tools/dz2d.m   jinc-weighted inward spiral
    designs = dz2d_batch(specs)                     # many designs, each its single call
    nk, ms = csg(k, mxg, mxs)                       # rf_tools/csg.m    time-warp a trajectory to the gradient limits
    g = ktog(k, dt), s = ktos(k, dt)                # rf_tools/ktog.m, ktos.m
    xs = gt2cm(x, g, t)                             # rf_tools/gt2cm.m

Host NumPy throughout (the Bessel function from SciPy): a design is a few cumulative sums and two interpolations over ns
samples.  What checks such a pulse is the 2D simulation, mbfir.abr2_batch: `abr2_batch([(rf * flip, g)], x, y)` with x, y in cm.
Two intended differences from the reference: csg returns the gradient duration and does not print it, and a query of its
interpolations that misses the knot range only by rounding takes the end knot's value (see csg).  csg2.m, which needs the MEX
spline csplinx, is not restated.
"""
import numpy as np

_GAMMA_CSG = 4.26          # kHz/G as csg.m:25, :36 writes it
_GAMMA = 4.257             # kHz/G as ktog.m, ktos.m and gt2cm.m write it
_KNOT_RTOL = 1e-12         # csg: a query this close (relative) to an end knot is that knot


def _interp1(xk, yk, xq):
    """interp1(xk, yk, xq), linear, for complex yk and ascending xk: NaN outside [xk[0], xk[-1]] as interp1 returns it, but a query
    within _KNOT_RTOL (relative) of an end knot takes that knot's value."""
    lo, hi = xk[0], xk[-1]
    out = np.interp(xq, xk, yk.real) + 1j * np.interp(xq, xk, yk.imag)       # clamps outside the knots
    out[(xq < lo - _KNOT_RTOL * abs(lo)) | (xq > hi + _KNOT_RTOL * abs(hi))] = np.nan
    return out


def csg(k, mxg, mxs):
    """`nk = csg(k, mxg, mxs)` (csg.m:19-44): warp the time axis of the k-space trajectory k (cycles/cm, complex kx + i ky, over a
    nominal 1 ms) so that it keeps to the slew rate mxs ((G/cm)/ms) and then to the gradient amplitude mxg (G/cm).  Returns
    (nk, duration in ms); the reference prints the duration.

    Stage 1 (:25-33) takes the time step of sample j as sqrt(|s_j| / mxs) of the nominal one, s the slew rate of k, and resamples
    k uniformly on the warped axis.  Stage 2 (:36-41) stretches every step whose gradient exceeds mxg.  Kept from the reference:
    gamma = 4.26 kHz/G, the repeated last slew sample, and `max(abs(g), mxg)` with the division by mxg outside the cumulative sum.

    interp1 returns NaN for a query outside the knots.  In stage 2 the first query is the first knot up to rounding whenever the
    amplitude limit is not active (both are nt(len) / len), and the last query is ((len t) / len) against the last knot t.  So a
    query within 1e-12 (relative) of an end knot takes the knot's value; one further outside is NaN, as in the reference (stage 1
    does that when the trajectory starts with more than its mean slew step)."""
    k = np.asarray(k, dtype=np.complex128).ravel()
    n = len(k)
    if n < 3:
        raise ValueError("csg: the trajectory needs at least 3 samples")
    if not (mxg > 0 and mxs > 0 and np.isfinite(mxg) and np.isfinite(mxs)):
        raise ValueError("csg: mxg and mxs must be positive and finite")
    if not np.all(np.isfinite(k)):
        raise ValueError("csg: the trajectory must be finite")
    td = 1.0
    j = np.arange(1, n + 1)
    g = np.concatenate([[0], np.diff(k)]) / (_GAMMA_CSG * (td / n))                    # :25
    s = np.diff(g) / (td / n)                                                          # :26
    s = np.concatenate([s, s[-1:]])                                                    # :27
    ndts = np.sqrt(np.abs(s / mxs))                                                    # :30
    t1 = np.cumsum(ndts) * td / n                                                      # :31
    if not np.all(np.diff(t1) > 0):
        raise ValueError("csg: the trajectory has a sample of zero slew rate (interp1 needs distinct knots)")
    nk = _interp1(t1, k, j * t1[-1] / n)                                               # :33
    g = np.concatenate([[0], np.diff(nk)]) / (_GAMMA_CSG * (t1[-1] / n))               # :36
    ndtg = np.maximum(np.abs(g), mxg)                                                  # :38
    t2 = np.cumsum(ndtg) * t1[-1] / (mxg * n)                                          # :39
    nk = _interp1(t2, nk, j * t2[-1] / n)                                              # :41
    return nk, float(t2[-1])


def dz2d(nt, bw, tbp, ns, mxg, mxs):
    """`[rf, g] = dz2d(nt, bw, tbp, ns, mxg, mxs)` (dz2d.m:26-55): a 2D pulse on an inward spiral of nt turns that reaches bw / 2
    cycles/cm, ns samples, with a jinc weighting of time-bandwidth tbp under a Gaussian envelope, limited to mxg G/cm and mxs
    (G/cm)/ms by csg.  Returns (rf, g, duration in ms): rf real with sum(rf) = 1; g = gx + i gy with cumsum(g[::-1]) / (2 pi) the
    trajectory in cycles/cm, so that `abrm(rf * flip, g, x, y)` takes x and y in cm."""
    if int(ns) != ns or ns < 3:
        raise ValueError("dz2d: ns must be an integer >= 3")
    ns = int(ns)
    if not (nt > 0 and bw > 0 and tbp > 0 and np.isfinite(nt) and np.isfinite(bw) and np.isfinite(tbp)):
        raise ValueError("dz2d: nt, bw and tbp must be positive and finite")
    from scipy.special import jv
    t = np.arange(1, ns + 1) / ns
    kl = t * np.exp(1j * 2 * np.pi * t * nt) * bw / 2                 # prototype linear spiral          (:29)
    k, dur = csg(kl, mxg, mxs)                                        # (:32)
    kr = np.abs(k) / (bw / 2)                                         # tau(t) from zero to one          (:35)
    arg = kr * np.pi * tbp / 2 + 0.0001
    rf = jv(1, arg) / arg                                             # jinc                             (:38)
    rf = rf * np.exp(-kr * kr * 2)                                    # Gaussian envelope                (:41)
    g = np.diff(np.concatenate([[0], k]))                             # (:44)
    omt = 2 * np.pi * nt
    w = (omt * kr) / np.sqrt(omt * omt * kr * kr + 1)                 # density compensation             (:47-48)
    rf = rf * w
    rf = rf * np.abs(g)                                               # (:50)
    rf = rf[::-1]
    rf = rf / np.sum(rf)                                              # (:53-54)
    return rf, g[::-1] * 2 * np.pi, dur


_SPEC_NAMES = ("nt", "bw", "tbp", "ns", "mxg", "mxs")


def dz2d_batch(specs):
    """Many dz2d designs: specs are tuples of dz2d's positional arguments or dicts of its argument names.  Returns the list of
    (rf, g, duration in ms), each its single call (host only: there is no device work to group)."""
    out = []
    for s in specs:
        if isinstance(s, dict):
            missing = [k for k in _SPEC_NAMES if k not in s]
            if missing or len(s) != len(_SPEC_NAMES):
                raise ValueError("dz2d: takes the arguments %s" % ", ".join(_SPEC_NAMES))
            s = tuple(s[k] for k in _SPEC_NAMES)
        s = tuple(s)
        if len(s) != len(_SPEC_NAMES):
            raise ValueError("dz2d: takes the arguments %s" % ", ".join(_SPEC_NAMES))
        out.append(dz2d(*s))
    return out


def ktog(k, dt):
    """`g = ktog(k, dt)` (ktog.m): gradient (G/cm) of the trajectory k (cycles/cm) sampled every dt ms."""
    return np.diff(np.asarray(k).ravel()) / (_GAMMA * dt)


def ktos(k, dt):
    """`s = ktos(k, dt)` (ktos.m): slew rate ((G/cm)/ms) of the trajectory k (cycles/cm) sampled every dt ms."""
    return np.diff(np.diff(np.asarray(k).ravel()) / (dt * _GAMMA)) / dt


def gt2cm(x, g, t):
    """`xs = gt2cm(x, g, t)` (gt2cm.m): abr's dimensionless x -> cm for a gradient of g G/cm and a pulse of t ms."""
    return np.asarray(x) / (_GAMMA * g * t)
