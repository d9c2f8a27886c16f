"""NumPy restatement of a pulse train of the Bloch simulator with relaxation (helper of tests/test_blochtrain_cpu.py and
tests/test_blochtrain_gpu.py; not collected), vectorised over the (frequency, position) points, in float64 or np.longdouble.  The
per-sample quantities (Setup), the rotation (_rot) and the cases' grids are those of tests/blochgrad_ref.py, loaded by path through
tests/blochss_ref.py.

A period is a pulse tuple (b1, gr, tp, t1, t2, nucleus); a train plays it ntr times, repetition k at gains[k] exp(i phases[k]) b1.
Two forms of the same thing:
    tiled: the sample-by-sample recursion m_t = D_t R_t m_{t-1} + meq c_t over the tiled waveform.  b1 e^{i phi} turns the axis of
           a sample about z: (rotx, roty) -> Z(-phi) (rotx, roty), since rotx = -Re b1 and roty = +Im b1.
    train: the propagator form.  (A, B) of the period and (A_e, B_e) of its first `echo` samples at RF phase 0 (prop), then
           u = Z(+phi_k) m_k,  echo_k = Z(-phi_k) (A_e u + meq B_e),  m_{k+1} = Z(-phi_k) (A u + meq B).
Inputs of both recursions, formed once in float64 whatever the dtype: E1 and E2 (as in blochgrad_ref), and the amplitude scale x gain
of a repetition (one float64 product, as the host forms it for the device).  cos phi_k and sin phi_k are taken in the dtype, so the
long-double runs see the phases themselves while the float64 runs and the device see the float64 table.

Bound.  With u = 2^-53 and mu = max(|m0|inf, |meq|, 1) over the point, an echo or final entry of a train of ntr repetitions of a
period of ntime samples is held to C u ntr (ntime + 4) mu, an entry of a period's propagators to C u (ntime + 4), C = 200, counted
for samples that turn by at most 2 pi (bound_* assert that of their case):
  one sample, in units of u |m|_2.  The axis: rotx and roty carry 3 roundings, rotz up to 5 (two on the host per gradient term, the
    product with the position, two sums), so the axis is off by 5 u phi <= 32 and the rotation by as much.  phi = sqrt(sum of three
    squares), 3; the half angle into sincos 3.5 phi / 2 <= 11, sincos 2, the quotient sin / phi 4, the products with the axis 1:
    each Cayley-Klein parameter is off by at most 18 and their 4-vector by 36, which moves the rotation (quadratic in them) by 72.
    Forming the nine entries (four products, three sums each) 6, the matrix-vector product 5, the decay 1, the recovery term 2:
    118 in all, times sqrt(3) from the 2-norm of m to the largest entry of the result: 204, of which the two axis terms overlap
    (both count the rounding of phi); C = 200 stands for it.
  one repetition: two rotations about z from a table that is off by 1 each (4 each with their products), two matrix-vector products
    with the fused recovery term (6 each), and, on the device's side only, the rounding of the amplitude (1 phi <= 7): 27, well
    within the four samples' worth that the factor (ntime + 4) grants.
Every step is a contraction in the 2-norm (a rotation, a decay and a shift), so the errors add up and |m_k|_2 <= sqrt(3) mu.
Measured shares of the bound: tests/test_blochtrain_cpu.py prints the float64 twin's, tests/test_blochtrain_gpu.py the device's;
DESIGN section 8y quotes both."""
import functools
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("blochss_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "blochss_ref.py"))
ss = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ss)
_grad, gamma_of, intervals, _grid = ss._grad, ss.gamma_of, ss.intervals, ss._grid

GAMMA_H1, GAMMA_C13 = _grad.GAMMA_H1, _grad.GAMMA_C13
U = 2.0 ** -53
C_BOUND = 200.0


def _setup(pulse, df, pos, amp, dtype):
    b1, gr, tp, t1, t2, nucleus = pulse
    return _grad.Setup(b1, gr, tp, t1, t2, df, pos, gamma_of(nucleus), amp, dtype)


def _rot_of(nx, ny, nz):
    """The rotation of a sample from its axis over the points, as blochgrad_ref.Setup.ck forms it"""
    phi = np.sqrt(nx * nx + ny * ny + nz * nz)
    sp, _ = _grad._half_sinc(phi)
    return _grad._rot(np.cos(phi / 2), -nz * sp, ny * sp, -nx * sp)


def _zp(c, s, v):
    """Z(+phi) v"""
    return [c * v[0] - s * v[1], s * v[0] + c * v[1], v[2]]


def _zm(c, s, v):
    """Z(-phi) v"""
    return [c * v[0] + s * v[1], c * v[1] - s * v[0], v[2]]


def _table(phases, dtype):
    ph = np.asarray(phases, dtype=np.float64).astype(dtype)
    return np.cos(ph), np.sin(ph)


def _amps(scale, gains):
    """The float64 amplitude of every repetition, one product each"""
    return np.float64(scale) * np.asarray(gains, dtype=np.float64)


def _start(m0, Q, dtype):
    return [np.array(v) for v in _grad._m0(m0, Q.nf, Q.npos, dtype)]


def tiled(pulse, df, pos, ntr, phases, gains, echo, scale=1.0, m0=None, meq=1.0, dtype=np.float64):
    """(E (ntr, 3, nf, npos), F (3, nf, npos)): the state after `echo` samples of every repetition and after the last sample, by
    the recursion over the tiled waveform"""
    cs, sn = _table(phases, dtype)
    amps = _amps(scale, gains)
    Qs = {a: _setup(pulse, df, pos, a, dtype) for a in set(amps.tolist())}
    Q0 = next(iter(Qs.values()))
    m, mq, E = _start(m0, Q0, dtype), dtype(meq), []
    for k in range(ntr):
        Q, c, s = Qs[float(amps[k])], cs[k], sn[k]
        if echo == 0:
            E.append(m)
        for t in range(Q.n):
            nz = Q.rotz[t]
            nx = np.full_like(nz, c * Q.rotx[t] + s * Q.roty[t])
            ny = np.full_like(nz, c * Q.roty[t] - s * Q.rotx[t])
            o = _grad._mat_vec(_rot_of(nx, ny, nz), m)
            m = [Q.e2[t] * o[0], Q.e2[t] * o[1], Q.e1[t] * o[2] + mq * (1 - Q.e1[t])]
            if t + 1 == echo:
                E.append(m)
    return np.stack([np.stack(e) for e in E]), np.stack(m)


def prop(pulse, df, pos, amp, echo, dtype=np.float64):
    """(A, B, Ae, Be) of the period at RF amplitude amp and phase 0: A[i][j] and B[i] over the points, in the kernel's order (A <- D R
    A column by column, B <- D R B + c with meq = 1); (Ae, Be) after `echo` samples"""
    Q = _setup(pulse, df, pos, amp, dtype)
    one, zero = np.ones((Q.nf, Q.npos), dtype=dtype), np.zeros((Q.nf, Q.npos), dtype=dtype)
    A = [[one if i == j else zero for j in range(3)] for i in range(3)]
    B = [zero, zero, zero]
    Ae, Be = A, B
    for t in range(Q.n):
        R = _rot_of(np.full_like(Q.rotz[t], Q.rotx[t]), np.full_like(Q.rotz[t], Q.roty[t]), Q.rotz[t])
        e1, e2 = Q.e1[t], Q.e2[t]
        cols = []
        for j in range(3):
            o = _grad._mat_vec(R, [A[0][j], A[1][j], A[2][j]])
            cols.append([e2 * o[0], e2 * o[1], e1 * o[2]])
        A = [[cols[j][i] for j in range(3)] for i in range(3)]
        o = _grad._mat_vec(R, B)
        B = [e2 * o[0], e2 * o[1], e1 * o[2] + (1 - e1)]
        if t + 1 == echo:
            Ae, Be = A, B
    return A, B, Ae, Be


def prop_arrays(pulse, df, pos, scales, echo, dtype=np.float64):
    """(A (S, nf, npos, 3, 3), B (S, nf, npos, 3), Ae, Be) as mbfir.bloch_prop_batch returns them"""
    res = [prop(pulse, df, pos, np.float64(s), echo, dtype) for s in scales]
    mat = lambda k: np.stack([np.stack([np.stack(r[k][i], -1) for i in range(3)], -2) for r in res])
    vec = lambda k: np.stack([np.stack(r[k], -1) for r in res])
    return mat(0), vec(1), mat(2), vec(3)


def train(pulse, df, pos, ntr, phases, gains, echo, scale=1.0, m0=None, meq=1.0, demod=False, dtype=np.float64):
    """(E (ntr, 3, nf, npos), F (3, nf, npos)) by the propagator form"""
    cs, sn = _table(phases, dtype)
    amps = _amps(scale, gains)
    Ps = {a: prop(pulse, df, pos, a, echo, dtype) for a in set(amps.tolist())}
    Q0 = _setup(pulse, df, pos, 1.0, dtype)
    m, mq, E = _start(m0, Q0, dtype), dtype(meq), []
    for k in range(ntr):
        A, B, Ae, Be = Ps[float(amps[k])]
        c, s = cs[k], sn[k]
        u = _zp(c, s, m)
        e = [a + mq * b for a, b in zip(_grad._mat_vec(Ae, u), Be)]
        n = [a + mq * b for a, b in zip(_grad._mat_vec(A, u), B)]
        E.append(e if demod else _zm(c, s, e))
        m = _zm(c, s, n)
    return np.stack([np.stack(e) for e in E]), np.stack(m)


def demodulate(E, phases, dtype):
    """Z(+phi_k) applied to the echoes E (ntr, 3, nf, npos) of the laboratory frame"""
    cs, sn = _table(phases, dtype)
    c, s = cs[:, None, None], sn[:, None, None]
    return np.stack([c * E[:, 0] - s * E[:, 1], s * E[:, 0] + c * E[:, 1], E[:, 2]], 1)


def max_angle(pulse, df, pos, amp):
    """The largest rotation angle of one sample over the points"""
    Q = _setup(pulse, df, pos, amp, np.float64)
    return float(np.sqrt((Q.rotx ** 2 + Q.roty ** 2)[:, None, None] + Q.rotz ** 2).max())


def mu_of(m0, meq, nf, npos):
    """max(|m0|inf, |meq|, 1) per point, (nf, npos)"""
    m = np.abs(np.stack([np.asarray(v, dtype=np.float64) for v in _grad._m0(m0, nf, npos, np.float64)])).max(0)
    return np.maximum(np.maximum(m, abs(float(meq))), 1.0)


def bound_train(ntr, ntime, mu):
    return C_BOUND * U * ntr * (ntime + 4) * mu


def bound_prop(ntime):
    return C_BOUND * U * (ntime + 4)


def tile_b1(b1, phases, gains):
    """The tiled waveform concat_k gains[k] e^{i phi_k} b1 in complex128, as a caller without the train has to form it"""
    b1 = np.asarray(b1, dtype=np.complex128)
    return np.concatenate([g * np.exp(1j * p) * b1 for p, g in zip(phases, gains)])


def tile_pulse(pulse, phases, gains):
    b1, gr, tp, t1, t2, nucleus = pulse
    n, N = len(b1), len(phases)
    gr = None if gr is None else np.tile(np.asarray(gr, dtype=np.float64).reshape(n, -1), (N, 1))
    tp = np.tile(intervals(pulse), N)
    return (tile_b1(b1, phases, gains), gr, tp, t1, t2, nucleus)


# ---- the cases that tests/test_blochtrain_cpu.py and tests/test_blochtrain_gpu.py share ---------------------------------------
def _period(rng, n, nucleus, t1, t2, flip, dead, grad):
    """n samples: n - 1 of 0.25 ms that carry b1 (|flip| radians in all, a complex envelope, one sample exactly zero for n >= 4)
    and a last dead-time sample of `dead` seconds without b1 or gradient.  n = 1: the one sample carries b1 and lasts `dead`."""
    gamma = gamma_of(nucleus)
    nrf = max(n - 1, 1)
    dt = 2.5e-4 if n <= 9 else 2e-3 / nrf
    tp = np.full(n, dt)
    tp[-1] = dead
    dur = tp[:nrf].sum()
    b1 = (rng.uniform(0.5, 1.5, n) + 0.3j * rng.standard_normal(n)) * (flip / (gamma * dur))
    gr = rng.uniform(0.5, 1.5, (n, 1)) * 0.02 * (GAMMA_H1 / gamma) if grad else None
    if n >= 4:
        b1[n // 3] = 0.0
    if n > 1:
        b1[-1] = 0.0
        if grad:
            gr[-1] = 0.0
    return (b1, gr, tp, t1, t2, nucleus)


def _m0(rng, nf, npos):
    v = rng.standard_normal((3, nf, npos))
    return tuple(v * (rng.uniform(0.2, 1.0, (nf, npos)) / np.sqrt((v * v).sum(0))))


C13 = ("C-13", 30.0, 2.0)
H1 = ("H-1", 1.0, 0.1)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(pulses, dfs, dps (one per pulse), shared (the grids are one object), ntr, phases, gains, echo, m0 (per pulse),
    scales).  Periods of 1, 9 and 257 samples (257: a second LDS tile), every one but the single sample ending in a dead time
    longer than its other samples, the 9-sample ones with a gradient; trains of 1, 2 and 257 repetitions (257: a second tile of
    the repetition table); echo 0, mid-period, ntime and, for 257 samples, 256; one distinct gain and three in a ramp; scales
    (1.0,) and (0.9, 1.0, 1.1); grids of 3 x 2 points, of 300 points (two chunks, the last partial), shared and per pulse; a batch
    of three pulses of different lengths; C-13 (T1 30 s, T2 2 s) and H-1 (T1 1 s, T2 0.1 s)."""
    rng = np.random.default_rng(23)
    f3, p2 = _grid(3, 60.0), np.array([[-1.0], [0.7]])
    ramp = lambda n: np.minimum(1.0, 0.5 + 0.25 * np.arange(n))           # 0.5, 0.75, 1, 1, ...: three distinct gains
    out = {}
    # alternating bSSFP with an alpha/2-like ramp: 9 samples with a gradient, 257 repetitions, echo mid-period, a scale sweep
    out["c13_ramp"] = dict(pulses=[_period(rng, 9, *C13, 0.6, 4e-3, True)], dfs=[f3], dps=[p2], ntr=[257], phases=[np.pi * np.arange(257)],
                           gains=[ramp(257)], echo=[4], m0=[_m0(rng, 3, 2)], scales=(0.9, 1.0, 1.1))
    # 257 samples on 300 points, two repetitions at arbitrary phases, echo in the second tile's first sample
    out["h1_long"] = dict(pulses=[_period(rng, 257, *H1, 1.2, 3e-3, False)], dfs=[_grid(2, 40.0)], dps=[_grid(150, 1.5)[:, None]],
                          ntr=[2], phases=[np.array([0.3, -2.1])], gains=[np.full(2, 0.8)], echo=[256], m0=[_m0(rng, 2, 150)],
                          scales=(1.0,))
    # one sample, one repetition, phase 0 and gain 1: the simulator's own end point
    out["one"] = dict(pulses=[_period(rng, 1, *H1, 0.4, 1e-3, False)], dfs=[f3], dps=[p2], ntr=[1], phases=[np.zeros(1)],
                      gains=[np.ones(1)], echo=[1], m0=[None], scales=(1.0,))
    # three periods of different lengths in one call, a grid per pulse, every echo edge, a quadratic phase schedule
    quad = lambda n: 0.5 * np.deg2rad(117.0) * np.arange(n) * (np.arange(n) + 1)
    out["batch"] = dict(pulses=[_period(rng, 9, *H1, 0.9, 2e-3, True), _period(rng, 257, *C13, 0.5, 4e-3, False),
                                _period(rng, 1, *C13, 0.3, 2e-3, False)],
                        dfs=[f3, _grid(2, 50.0), _grid(1, 0.0)], dps=[p2, _grid(3, 1.0)[:, None], _grid(5, 2.0)[:, None]],
                        ntr=[2, 1, 257], phases=[quad(2), quad(1), quad(257)], gains=[ramp(2), np.ones(1), ramp(257)],
                        echo=[0, 257, 0], m0=[_m0(rng, 3, 2), _m0(rng, 2, 3), _m0(rng, 1, 5)], scales=(0.9, 1.0, 1.1))
    # the same three periods on one shared grid, echo = ntime everywhere, one gain each
    out["shared"] = dict(pulses=out["batch"]["pulses"], dfs=[f3] * 3, dps=[p2] * 3, ntr=[2, 2, 2],
                         phases=[np.pi * np.arange(2)] * 3, gains=[np.ones(2)] * 3, echo=[9, 257, 1],
                         m0=[out["batch"]["m0"][0]] * 3, scales=(1.0,))
    return out


MEQS = (1.0, 1e-4, 0.0)


@functools.lru_cache(maxsize=None)
def reference(name, meq):
    """The long-double tiled recursion of a case: per pulse (E (S, ntr, 3, nf, npos), F (S, 3, nf, npos)), computed once"""
    c = cases()[name]
    res = []
    for q, p in enumerate(c["pulses"]):
        r = [tiled(p, c["dfs"][q], c["dps"][q], c["ntr"][q], c["phases"][q], c["gains"][q], c["echo"][q], s, c["m0"][q], meq,
                   np.longdouble) for s in c["scales"]]
        res.append((np.stack([e for e, _ in r]), np.stack([f for _, f in r])))
    return res


def case_bounds(name, meq):
    """Per pulse the bound (nf, npos) of an echo or final entry; asserts that no sample turns by more than 2 pi"""
    c = cases()[name]
    out = []
    for q, p in enumerate(c["pulses"]):
        amax = max(abs(s) for s in c["scales"]) * float(np.abs(c["gains"][q]).max())
        assert max_angle(p, c["dfs"][q], c["dps"][q], amax) <= 2 * np.pi
        nf, npos = len(c["dfs"][q]), len(c["dps"][q])
        out.append(bound_train(c["ntr"][q], len(p[0]), mu_of(c["m0"][q], meq, nf, npos)))
    return out
