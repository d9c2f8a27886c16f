"""A dense high-precision reference of a unit's operators G v, G'u, W^-2 G v and H = G'W^-2 G, the error bounds the device
results are held to, and a float64 model of the lattice recurrences the bounds are checked against on the CPU
(tests/test_latticeops_cpu.py; the device tests are tests/test_latticeops_gpu.py).

The reference is independent of the product's numerics and of the oracle: the program's structured rows come from the
accessors of include/mbfir.h (mbfir_program_dims / _trig / _rows), everything after that is numpy.longdouble (64-bit mantissa
here): w * tau, the trigonometry, the textbook Nesterov-Todd scaling of (s, z) and the products.

Bounds.  u = 2^-53.  Each bound is K u times an ENVELOPE of the sum the kernel forms; K is assembled from the constants of
solver.hip (SEGMAX, CHUNK_LEN, CGRP, the snap tolerance of analyse_lattice), never from a device result:
  trig(K_steps) = 9 X + 1 + 7 K_steps, the absolute error of one cos / sin value in units of u times its amplitude, with
      X = max(1, |w|max) * |t|max:  X + 1 for the seed (the argument w t rounded, then sincos), 4 X for the snap of the folded grid
      (tol = 2 eps wmax = 4 u wmax per frequency moves cos(w t) by |t| tol) and 4 X for a run's straight line through its end
      points (the same tol), and per recurrence step 4 roundings of the rotation plus 3 for the error of the step's own
      (cos, sin) pair, whose argument is rounded too;
  K_G  = trig(min(SEGMAX, D1)) + Nt + useg + Ne + 8: at most SEGMAX = 128 steps, then the length of the row's sum;
  K_GT = trig(CHUNK_LEN) + CHUNK_LEN * CGRP + nchunk + 2 rows_per_freq + rows_per_col + 24: CHUNK_LEN = 64 steps; a thread adds
      up to CGRP chunks of CHUNK_LEN frequencies, the folds add the nchunk / cgrp partials and the GTG = 16 column groups;
  K_H  = trig(CHUNK_LEN) at 2 X (the sum progression reaches t = 2 |t|max) + CHUNK_LEN * CGRP + nchunk + K_W + 16: the
      moments' sums, the NT weights (K_W = 32 roundings of the scaling formulas, + the length of the big cone's dot products),
      and the four moment terms of an entry;
  dense path (opts.dense_trig): every trig value is a sincos of its own, trig(0), and the sums run over Nt resp. Mf terms in
      an order the bound does not know: their whole length is charged.
Envelopes: the amplitude matrix Ghat (every trig entry replaced by |alpha_i| col_scale_j, resp. |beta_i| |psign_j| col_scale_pcol(j))
carries the absolute error of a trig value, which does not shrink where cos(w t) does: |G v - ref|_i <= K_G u (Ghat |v|)_i, the
analogue for G'u, and |H - H_ref|_jk <= K_H u E_jk with E = Ghat'|W^-2| Ghat (the moment form 1/2 [mom(ta - tb) +- mom(ta + tb)]
cancels, so |G|'|W^-2||G| is not the scale of its error).  For a vector without zeros (|G| |v|)_i is within a small factor of
(Ghat |v|)_i, and the tests also hold G v to K_G u (|G| |v|)_i there; for a unit vector e_j that form asks for a RELATIVE error
of the single entry G_ij, which no double-precision cos(w t) has near its zeros (the argument's rounding alone moves it by X u),
so the unit vectors are held to the amplitude form.

The bounds are measured against the float64 model below, not against the device: tests/test_latticeops_cpu.py asserts them
with a margin of 4 on the grids of the device tests, prints the ratios and records them in its docstring.
"""
import ctypes as C

import numpy as np

import mbfir

LD = np.longdouble
U = 2.0 ** -53
# constants of solver.hip the bounds and the model are built from
SEGMAX, CHUNK_LEN, CGRP, MPTS, GTG = 128, 64, 4, 256, 16
K_W = 32
WHICH = {"fir_ap_cvx": 0, "fir_qp_cvx": 1, "fir_linprog": 2, "fir_qprog_phs": 3}


def _params(fn, args):
    if fn == "fir_ap_cvx":
        return list(args[4:6])
    if fn == "fir_qp_cvx":
        obj = np.atleast_1d(args[5]).astype(float)
        return [args[4]] + list(obj) + [0.0] * (2 - len(obj)) + [len(obj)]
    return [0.0]


def program(fn, args, grid_m=0):
    """The structured program of design (fn, args) as the accessors of include/mbfir.h give it (host only)."""
    lib = mbfir.load_library()
    which = WHICH[fn]
    n, f = int(args[0]), mbfir._vec(args[1])
    if which == 3:
        ac, dc = np.asarray(args[2], dtype=np.complex128).ravel(), np.asarray(args[3], dtype=np.complex128).ravel()
        a, d = mbfir._vec(np.stack([ac.real, ac.imag], 1)), mbfir._vec(np.stack([dc.real, dc.imag], 1))
    else:
        a, d = mbfir._vec(args[2]), mbfir._vec(args[3])
    params = mbfir._vec(_params(fn, args) + [0.0] * 4)
    out, err = C.c_void_p(), C.create_string_buffer(256)
    dp, ip = mbfir._ptr, lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.mbfir_assemble(which, n, len(f) // 2, dp(f), dp(a), dp(d), dp(params), int(grid_m), C.byref(out), err, 256)
    assert rc == 0, err.value.decode()
    try:
        dims = np.zeros(10, dtype=np.int32)
        lib.mbfir_program_dims(out, ip(dims))
        Nt, Ne, R, l, nq3, big, Mf, quad = [int(x) for x in dims[:8]]
        w, tau, scale, psign, c = np.zeros(Mf), np.zeros(Nt), np.zeros(Nt), np.zeros(Nt), np.zeros(Nt + Ne)
        kind, pcol = np.zeros(Nt, dtype=np.int32), np.zeros(Nt, dtype=np.int32)
        lib.mbfir_program_trig(out, dp(w), ip(kind), dp(tau), dp(scale), ip(pcol), dp(psign), dp(c))
        freq, col = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
        al, be, ey, h = np.zeros(R), np.zeros(R), np.zeros((R, 3)), np.zeros(R)
        lib.mbfir_program_rows(out, ip(freq), ip(col), dp(al), dp(be), dp(ey), dp(h))
    finally:
        lib.mbfir_program_free(out)
    assert R == l + 3 * nq3 + big and not np.any((freq >= 0) & (col >= 0))
    return dict(fn=fn, args=args, grid_m=grid_m, Nt=Nt, Ne=Ne, N=Nt + Ne, R=R, l=l, nq3=nq3, big=big, Mf=Mf, quad=bool(quad), w=w, tau=tau,
                scale=scale, psign=psign, kind=kind, pcol=pcol, freq=freq, col=col, al=al, be=be, ey=ey, h=h, c=c)


def _rows_from_trig(P, A1, A2, dtype):
    """G from the per-frequency trig matrices A1, A2 (Mf x Nt) and the structured rows."""
    G = np.zeros((P["R"], P["N"]), dtype=dtype)
    tr = P["freq"] >= 0
    fr = P["freq"][tr]
    G[tr, :P["Nt"]] = P["al"][tr, None].astype(dtype) * A1[fr] + P["be"][tr, None].astype(dtype) * A2[fr]
    idr = np.nonzero(P["col"] >= 0)[0]
    G[idr, P["col"][idr]] += P["al"][idr].astype(dtype)
    G[:, P["Nt"]:] = P["ey"][:, :P["Ne"]].astype(dtype)
    return G


def G_ref(P, round_arg=False):
    """G in longdouble: w tau and the trigonometry formed in longdouble from the program's float64 w, tau, scale.
    round_arg (a self-check only): the product w tau rounded to float64 first, as any float64 assembly has it."""
    arg = np.outer(P["w"].astype(LD), P["tau"].astype(LD))
    if round_arg:
        arg = arg.astype(np.float64).astype(LD)
    A1 = P["scale"].astype(LD) * np.where(P["kind"] == 0, np.cos(arg), np.sin(arg))
    A2 = P["psign"].astype(LD) * A1[:, P["pcol"]] if P["quad"] else np.zeros_like(A1)
    return _rows_from_trig(P, A1, A2, LD)


def G_hat(P):
    """The amplitude envelope of G (float64): |alpha_i| col_scale_j for a trig entry, |.| for the others."""
    A1 = np.broadcast_to(np.abs(P["scale"]), (P["Mf"], P["Nt"]))
    A2 = np.broadcast_to(np.abs(P["psign"]) * np.abs(P["scale"])[P["pcol"]], (P["Mf"], P["Nt"])) if P["quad"] else np.zeros((P["Mf"], P["Nt"]))
    Q = dict(P, al=np.abs(P["al"]), be=np.abs(P["be"]), ey=np.abs(P["ey"]))
    return _rows_from_trig(Q, A1, A2, np.float64)


# ---- Nesterov-Todd scaling of (s, z), textbook form (Vandenberghe, "The CVXOPT linear and quadratic cone program solvers", 2010) ----
def _soc_nt(s, z):
    """s, z: (..., m) interior points of the second-order cone.  Returns eta (...,) and wbar (..., m)."""
    sres = s[..., 0] ** 2 - (s[..., 1:] ** 2).sum(-1)
    zres = z[..., 0] ** 2 - (z[..., 1:] ** 2).sum(-1)
    assert np.all(sres > 0) and np.all(zres > 0) and np.all(s[..., 0] > 0) and np.all(z[..., 0] > 0), "(s, z) not strictly interior"
    sb, zb = s / np.sqrt(sres)[..., None], z / np.sqrt(zres)[..., None]
    gamma = np.sqrt((1 + (sb * zb).sum(-1)) / 2)
    jz = zb.copy()
    jz[..., 1:] = -jz[..., 1:]
    return np.sqrt(np.sqrt(sres / zres)), (sb + jz) / (2 * gamma)[..., None]


def _soc_blocks(eta, wb):
    """W, W^-1, W^-2 of cones with scaling (eta, wbar): arrays (..., m, m)."""
    m = wb.shape[-1]
    J = np.diag(np.array([1] + [-1] * (m - 1), dtype=LD))
    w0, w1 = wb[..., 0], wb[..., 1:]
    core = np.zeros(wb.shape + (m,), dtype=LD)
    core[..., 1:, 1:] = np.eye(m - 1, dtype=LD) + w1[..., :, None] * w1[..., None, :] / (1 + w0)[..., None, None]
    W, Wi = core.copy(), core.copy()
    W[..., 0, 0] = Wi[..., 0, 0] = w0
    W[..., 0, 1:], W[..., 1:, 0] = w1, w1
    Wi[..., 0, 1:], Wi[..., 1:, 0] = -w1, -w1
    q = wb @ J
    Wi2 = (2 * q[..., :, None] * q[..., None, :] - J) / (eta ** 2)[..., None, None]
    return W * eta[..., None, None], Wi / eta[..., None, None], Wi2


class Scaling:
    """W^-2 of the cone K = R+^l x (Q^3)^nq3 x Q^big at (s, z) in longdouble, kept by blocks."""

    def __init__(self, P, s, z):
        self.l, self.nq3, self.big, self.R = P["l"], P["nq3"], P["big"], P["R"]
        s, z = np.asarray(s, dtype=np.float64).astype(LD), np.asarray(z, dtype=np.float64).astype(LD)
        l, o3 = self.l, self.l + 3 * self.nq3
        assert np.all(s[:l] > 0) and np.all(z[:l] > 0)
        self.d = z[:l] / s[:l]
        self.s, self.z = s, z
        self.W3 = self.Wi3 = self.B3 = np.zeros((0, 3, 3), dtype=LD)
        if self.nq3:
            self.W3, self.Wi3, self.B3 = _soc_blocks(*_soc_nt(s[l:o3].reshape(-1, 3), z[l:o3].reshape(-1, 3)))
        self.Wb = self.Wib = self.Bb = np.zeros((0, 0), dtype=LD)
        if self.big:
            self.Wb, self.Wib, self.Bb = _soc_blocks(*_soc_nt(s[o3:], z[o3:]))

    def _apply(self, X, d, B3, Bb):
        X = np.asarray(X)
        one = X.ndim == 1
        X = X.reshape(self.R, -1)
        out = np.zeros(X.shape, dtype=np.result_type(X.dtype, d.dtype))
        l, o3 = self.l, self.l + 3 * self.nq3
        out[:l] = d[:, None] * X[:l]
        if self.nq3:
            out[l:o3] = np.einsum("cab,cbk->cak", B3, X[l:o3].reshape(self.nq3, 3, -1)).reshape(3 * self.nq3, -1)
        if self.big:
            out[o3:] = Bb @ X[o3:]
        return out[:, 0] if one else out

    def winv2(self, X):
        return self._apply(np.asarray(X).astype(LD), self.d, self.B3, self.Bb)

    def abs_winv2(self, X):
        """|W^-2| X in float64 (the envelope's weight)."""
        return self._apply(np.asarray(X, dtype=np.float64), np.abs(self.d).astype(np.float64), np.abs(self.B3).astype(np.float64), np.abs(self.Bb).astype(np.float64))


def H_ref(G, S, rows=None):
    """Rows `rows` (default all) of G'W^-2 G in longdouble."""
    T = S.winv2(G)
    Gt = np.ascontiguousarray(G.T if rows is None else G[:, rows].T)
    return Gt @ T


def H_env(Gh, S, rows=None):
    return (Gh.T if rows is None else Gh[:, rows].T) @ S.abs_winv2(Gh)


def seg_of(D1):
    """plan_unit's segment length of the row response: min(SEGMAX, max(64, D1 / 16 rounded up to 8))."""
    return min(SEGMAX, max(64, -(-(-(-max(D1, 1) // 16)) // 8) * 8))


# ---- the constants of the bounds ------------------------------------------------------------------------------------
def grid_facts(P):
    """What the bounds take from the program: X, D1, the run count of the grid (unfolded, the larger one), rows per frequency / column."""
    T = float(np.abs(P["tau"]).max())
    lat = P["tau"] - P["tau"].min()
    D1 = int(round(lat.max())) + 1
    runs = max(mbfir.test_fold(P["w"], fold=fo)["runs"] for fo in (True, False))
    fr = P["freq"][P["freq"] >= 0]
    cl = P["col"][P["col"] >= 0]
    return dict(X=max(1.0, float(np.abs(P["w"]).max())) * T, D1=D1, nchunk=int(runs), useg=-(-D1 // seg_of(D1)),
                rows_per_freq=int(np.bincount(fr).max()) if len(fr) else 0, rows_per_col=int(np.bincount(cl).max()) if len(cl) else 0)


def _trig(X, steps):
    return 9.0 * X + 1.0 + 7.0 * steps


def K_G(P, dense=False):
    F = grid_facts(P)
    if dense:
        return _trig(F["X"], 0) + P["Nt"] + P["Ne"] + 8
    return _trig(F["X"], min(SEGMAX, F["D1"])) + P["Nt"] + F["useg"] + P["Ne"] + 8


def K_GT(P, dense=False):
    F = grid_facts(P)
    if dense:
        return _trig(F["X"], 0) + P["Mf"] * max(F["rows_per_freq"], 1) + F["rows_per_col"] + 24
    return _trig(F["X"], CHUNK_LEN) + CHUNK_LEN * CGRP + F["nchunk"] + 2 * F["rows_per_freq"] + F["rows_per_col"] + 24


def K_H(P, dense=False):
    F = grid_facts(P)
    if dense:
        return 2 * _trig(F["X"], 0) + P["Mf"] + K_W + P["big"] + 16
    return _trig(2 * F["X"], CHUNK_LEN) + CHUNK_LEN * CGRP + F["nchunk"] + K_W + P["big"] + 16


def K_WG(P, dense=False):
    """W^-2 G v - sub: the error of G v through |W^-2|, the weights' own roundings, the block's dot product."""
    return K_G(P, dense) + K_W + P["big"] + 4


# ---- float64 model of the lattice recurrences (what the bounds are measured against on the CPU) --------------------------
def analyse(P, fold=True):
    """analyse_lattice's folded list and runs for the grid P['w'] (float64, the same arithmetic)."""
    w = P["w"]
    Mf = len(w)
    tol = 2 * 2.2204460492503131e-16 * max(1.0, float(np.abs(w).max()))
    wf, pos, neg = [], [], []
    if fold:
        for i in np.argsort(np.abs(w), kind="stable"):
            ng, aw = w[i] < 0, abs(w[i])
            if wf and aw - wf[-1] <= tol and (neg[-1] < 0 if ng else pos[-1] < 0):
                if ng:
                    neg[-1] = i
                else:
                    pos[-1] = i
                wf[-1] = 0.5 * (wf[-1] + aw)
            else:
                wf.append(aw), pos.append(-1 if ng else i), neg.append(i if ng else -1)
    else:
        wf, pos, neg = list(w), list(range(Mf)), [-1] * Mf
    W = np.array(wf)
    Nf = len(W)
    ch = []
    i = 0
    while i < Nf:
        cnt = min(CHUNK_LEN, Nf - i)
        while True:
            dw = (W[i + cnt - 1] - W[i]) / (cnt - 1) if cnt > 1 else 0.0
            q = np.arange(1, cnt - 1)
            ok = bool(np.all(np.abs(W[i + q] - (W[i] + q * dw)) <= tol))
            if ok or cnt <= 2:
                break
            cnt = max(2, cnt // 2)
        if (cnt == 2 and i + 2 < Nf and abs(W[i + 2] - (W[i] + 2 * dw)) > tol and abs(dw) > 0 and
                (i + 3 >= Nf or abs((W[i + 2] - W[i + 1]) - (W[i + 3] - W[i + 2])) <= tol)):
            cnt = 1
        if cnt <= 1:
            cnt, dw = 1, 0.0
        ch.append((i, cnt, W[i], dw))
        i += cnt
    tmin = float(P["tau"].min())
    lat = np.rint(P["tau"] - tmin).astype(int)
    return dict(wf=W, pos=np.array(pos), neg=np.array(neg), chunks=ch, tmin=tmin, lat=lat, D1=int(lat.max()) + 1)


def _rot(c, s, cd, sd):
    return c * cd - s * sd, s * cd + c * sd


def model_eval_trig(P, L):
    """(cos, sin)(w_i tau_j) as k_trig_eval forms them: one sincos per (folded frequency, segment), unit steps in between."""
    D1 = L["D1"]
    seg = seg_of(D1)
    Cf, Sf = np.zeros((len(L["wf"]), D1)), np.zeros((len(L["wf"]), D1))
    cw, sw = np.cos(L["wf"]), np.sin(L["wf"])
    for m0 in range(0, D1, seg):
        a = L["wf"] * (L["tmin"] + m0)
        c, s = np.cos(a), np.sin(a)
        for m in range(m0, min(m0 + seg, D1)):
            Cf[:, m], Sf[:, m] = c, s
            c, s = _rot(c, s, cw, sw)
    return _unfold(P, L, Cf, Sf)


def _unfold(P, L, Cf, Sf):
    Cm, Sm = np.zeros((P["Mf"], L["D1"])), np.zeros((P["Mf"], L["D1"]))
    p, n = L["pos"] >= 0, L["neg"] >= 0
    Cm[L["pos"][p]], Sm[L["pos"][p]] = Cf[p], Sf[p]
    Cm[L["neg"][n]], Sm[L["neg"][n]] = Cf[n], -Sf[n]
    return Cm, Sm


def chunk_trig(L, t):
    """(cos, sin)(wf_k t) for the points t as the moment kernels form them: per run one sincos seed pair, steps of dw."""
    t = np.asarray(t, dtype=np.float64)
    Cf, Sf = np.zeros((len(L["wf"]), len(t))), np.zeros((len(L["wf"]), len(t)))
    for (i0, cnt, w0, dw) in L["chunks"]:
        c, s, cd, sd = np.cos(w0 * t), np.sin(w0 * t), np.cos(dw * t), np.sin(dw * t)
        for q in range(cnt):
            Cf[i0 + q], Sf[i0 + q] = c, s
            c, s = _rot(c, s, cd, sd)
    return Cf, Sf


def model_G(P, Cm, Sm, L):
    """G in float64 from modelled per-frequency (cos, sin) tables on the lattice."""
    A1 = P["scale"] * np.where(P["kind"] == 0, Cm[:, L["lat"]], Sm[:, L["lat"]])
    A2 = P["psign"] * A1[:, P["pcol"]] if P["quad"] else np.zeros_like(A1)
    return _rows_from_trig(P, A1, A2, np.float64)


def freq_blocks(P, S):
    """The 2 x 2 forms [[d11, d12], [d12, d22]] of W^-2 on the rows of each frequency (longdouble, Mf each): H's trig block is
    A1'D11 A1 + A1'D12 A2 + A2'D12 A1 + A2'D22 A2.  Asserts that W^-2 couples no two frequencies."""
    Mf, l = P["Mf"], P["l"]
    D = np.zeros((3, Mf), dtype=LD)
    fr, al, be = P["freq"], P["al"].astype(LD), P["be"].astype(LD)

    def add(f, x1, y1, x2, y2, wgt):
        np.add.at(D[0], f, x1 * wgt * x2), np.add.at(D[1], f, x1 * wgt * y2), np.add.at(D[2], f, y1 * wgt * y2)
    r = np.nonzero(fr[:l] >= 0)[0]
    add(fr[r], al[r], be[r], al[r], be[r], S.d[r])
    assert not np.any(fr[l + 3 * P["nq3"]:] >= 0)
    for a in range(3):
        for b in range(3):
            ra, rb = l + 3 * np.arange(P["nq3"]) + a, l + 3 * np.arange(P["nq3"]) + b
            both = (fr[ra] >= 0) & (fr[rb] >= 0)
            assert np.all(fr[ra][both] == fr[rb][both]), "W^-2 couples two frequencies"
            ra, rb, wgt = ra[both], rb[both], S.B3[both, a, b]
            np.add.at(D[0], fr[ra], al[ra] * wgt * al[rb]), np.add.at(D[1], fr[ra], al[ra] * wgt * be[rb]), np.add.at(D[2], fr[ra], be[ra] * wgt * be[rb])
    return D


def model_H_trig(P, L, D):
    """The trig block of H as the lattice path assembles it, in float64: folded operands, the moments g, s on the difference and
    the sum progression by the runs' recurrences, then lat_T's 1/2 [mom(ta - tb) +- mom(ta + tb)]."""
    D1, lat, kind, sc = L["D1"], L["lat"], P["kind"], P["scale"]
    t = np.concatenate([np.arange(D1, dtype=float), 2 * L["tmin"] + np.arange(2 * D1 - 1, dtype=float)])
    Cf, Sf = chunk_trig(L, t)
    D = np.asarray(D, dtype=np.float64)
    Dz = np.concatenate([D, np.zeros((3, 1))], axis=1)          # (index -1: the empty side)
    pe, po = Dz[:, L["pos"]] + Dz[:, L["neg"]], Dz[:, L["pos"]] - Dz[:, L["neg"]]
    Gm, Sm = pe @ Cf, po @ Sf                                   # (3, 3 D1 - 1)

    def lat_T(wi, j, k):
        mj, mk = lat[j][:, None], lat[k][None, :]
        kj, kk = kind[j][:, None], kind[k][None, :]
        d, si = mj - mk, D1 + mj + mk
        g, s = Gm[wi], Sm[wi]
        sdv = np.where(d < 0, -s[np.abs(d)], s[np.abs(d)])
        v = np.where((kj == 0) & (kk == 0), g[np.abs(d)] + g[si], np.where((kj == 1) & (kk == 1), g[np.abs(d)] - g[si],
                     np.where(kj == 0, s[si] - sdv, s[si] + sdv)))
        return 0.5 * v * sc[j][:, None] * sc[k][None, :]
    j = np.arange(P["Nt"])
    H = lat_T(0, j, j)
    if P["quad"]:
        p, sg = P["pcol"], P["psign"]
        H = H + sg[:, None] * sg[None, :] * lat_T(2, p, p) + sg[None, :] * lat_T(1, j, p) + sg[:, None] * lat_T(1, p, j)
    return H


def H_trig_ref(P, D, amplitude=False):
    """The same block from the longdouble trig matrix (or, amplitude=True, its float64 envelope with |D|)."""
    if amplitude:
        A1 = np.broadcast_to(np.abs(P["scale"]), (P["Mf"], P["Nt"])).astype(np.float64)
        A2 = np.abs(P["psign"]) * A1[:, P["pcol"]]
        D = np.abs(np.asarray(D, dtype=np.float64))     # (|sum| <= sum |.|: never above E's weights, so the model is held to the smaller envelope)
    else:
        arg = np.outer(P["w"].astype(LD), P["tau"].astype(LD))
        A1 = P["scale"].astype(LD) * np.where(P["kind"] == 0, np.cos(arg), np.sin(arg))
        A2 = P["psign"].astype(LD) * A1[:, P["pcol"]]
    H = A1.T @ (D[0][:, None] * A1)
    if P["quad"]:
        X = A1.T @ (D[1][:, None] * A2)
        H = H + X + X.T + A2.T @ (D[2][:, None] * A2)
    return H


# ---- test inputs ----------------------------------------------------------------------------------------------------
def draw_sz(P, rng, wide):
    """A strictly interior pair (s, z): well centred, or (wide) with the orthant weights z / s spread over 1e8."""
    R, l, nq3, big = P["R"], P["l"], P["nq3"], P["big"]
    s, z = np.ones(R), np.ones(R)
    if wide:
        r = 10.0 ** rng.uniform(-4, 4, l)
        if l >= 2:
            r[l // 3], r[(2 * l) // 3] = 0.9e-4, 1.1e4          # (the span itself, whatever the draw)
        c = rng.uniform(0.5, 2, l)
        s[:l], z[:l] = c / np.sqrt(r), c * np.sqrt(r)
    else:
        s[:l], z[:l] = rng.uniform(0.5, 2, l), rng.uniform(0.5, 2, l)

    def cone(m, k):
        x = rng.standard_normal((k, m))
        x[:, 0] = np.sqrt((x[:, 1:] ** 2).sum(1)) + rng.uniform(0.5, 1.5, k)
        return x * rng.uniform(0.5, 2, k)[:, None]
    o3 = l + 3 * nq3
    if nq3:
        s[l:o3], z[l:o3] = cone(3, nq3).ravel(), cone(3, nq3).ravel()
    if big:
        s[o3:], z[o3:] = cone(big, 1).ravel(), cone(big, 1).ravel()
    return s, z


def unit_columns(P):
    """One column per column kind (a cosine column, a sine column, a slack column): where the unit-vector inputs have their 1."""
    js = [int(np.nonzero(P["kind"] == 0)[0][len(np.nonzero(P["kind"] == 0)[0]) // 2])]
    if np.any(P["kind"] == 1):
        js.append(int(np.nonzero(P["kind"] == 1)[0][-1]))
    if P["Ne"]:
        js.append(P["N"] - 1)
    return js


# ---- the designs of the device tests (the CPU tests check what the device tests rely on) ---------------------------------
def _c13(n):
    from conftest import c13
    return ("fir_ap_cvx", (n,) + tuple(c13(n)) + (0.1, 1e-3))


def unit_cases():
    """name -> dict(job=(designer, args), grid_m, ddkkt, expect): expect holds the facts of the path the case is there for; the
    CPU tests derive them from the program and mbfir_test_fold, the device tests read them from the hook's report."""
    from conftest import CASES
    qphs = CASES["qphs21"][1]
    return {
        # bSSFP spec: one partly filled workgroup everywhere, origin 0, the one-pass build (NOT a quad program: no designer of
        # fir_ap_cvx's form is; the quad forms are cases 4 - 6)
        "c1_ap24": dict(job=_c13(24), grid_m=512, expect=dict(useg=1, tmin=0.0, one_pass=1, quad=False, mom_blocks=1, multi_group=True)),
        # D1 = 150: the segment length is 64 up to D1 = 1024 (plan_unit), so THREE segments; 449 moment points: two workgroups
        "c2_ap150": dict(job=_c13(150), grid_m=2048, expect=dict(useg=3, tmin=0.0, one_pass=1, quad=False, mom_blocks=2, multi_group=True, nfold_above=256)),
        "c3_lin64": dict(job=CASES["lin_real64"], grid_m=0, expect=dict(useg=1, tmin=0.5, one_pass=0, quad=False, mom_blocks=1, multi_group=True, no_pairs=True)),
        "c4_qphs21": dict(job=CASES["qphs21"], grid_m=0, expect=dict(useg=1, tmin=-10.0, one_pass=0, quad=True, mom_blocks=1, multi_group=True, rows_per_freq_above=2)),
        # the golden qphs22 spec is symmetric about 0 and folds without an empty side: band edges moved off the mirror image
        "c5_qphs22": dict(job=("fir_qprog_phs", (22, [-0.6, -0.3, -0.1, 0.15, 0.35, 0.7]) + tuple(qphs[2:])), grid_m=0,
                          expect=dict(useg=1, tmin=-10.5, one_pass=0, quad=True, mom_blocks=1, multi_group=True, rows_per_freq_above=2, empty_side_above=0)),
        "c6_qp25": dict(job=CASES["qp_modelB25"], grid_m=0, ddkkt=-1, expect=dict(useg=1, tmin=0.0, one_pass=0, quad=True, mom_blocks=1, multi_group=False, big=True)),
        "c7_ap58": dict(job=CASES["ap_c13_58"], grid_m=0, expect=dict(useg=1, tmin=0.0, one_pass=1, quad=False, mom_blocks=1, multi_group=True, nq3_above=0)),
        "c8_dup12": dict(job=("fir_ap_cvx", (12, [-1.0, -0.5, 0.25, 0.25, 0.6, 1.0], [0, 0, 0.8, 0.3, 0, 0], [0.05, 0.1, 0.05], 0.5, 1e-1)), grid_m=0,
                         expect=dict(useg=1, tmin=0.0, one_pass=1, quad=False, mom_blocks=1, multi_group=True, duplicates=True, lone_runs=True)),
    }


def hetero_jobs():
    """Two orders in one unit (the probes of a min-order search): per-lane dimensions, nothing pairs."""
    return [_c13(20), _c13(24)], 512
