"""The reference of the plain KKT solve [0 G'; G -W^2][dx; dz] = [bx; bz] (Impl::kkt_solve: the Cholesky solve, the sweeps of
preconditioned CG on G'W^-2 G, the residual norms the sweep controller reads) and of the residual kernels in front of it, for
mbfir.test_unit_kkt: tests/test_kkt_gpu.py holds the device to it group of launches by group of launches, tests/test_kkt_cpu.py
checks the bounds against a float64 twin without a GPU.

Everything is numpy.longdouble on top of lattice_ref (program, G_ref, G_hat, Scaling, K_G, K_GT) and cone_ref (designs, iterate,
rcond, kd).  Every stage takes the device's earlier outputs as exact, so one wrong kernel fails alone; the factor is the device's
own inverse factor M (H^-1 = M'M): the factorisation has its tests.  u = 2^-53.  The bound of a stage is K u times an envelope of
the sum the kernels form, K assembled from constants of the code and from the iterate, never from a device result:

  stage 0 (W^-2 bz), the W^-2 of 3 and 6:  orthant rows 8 u |d v| (the quotient z / s and the product: two roundings, times the margin of 4); a second-order cone of m rows
      [2 (bq |q|' + |q| bq') + (2 r_eta + (kd(m) + 8) u) (2 |q||q|' + I)] |v| / eta^2: the kernels apply W^-2 = (2 q q' - J) / eta^2 as
      2 q (q'v) - J v, whose dot product is accurate relative to |q|'|v|; bq and r_eta are cone_ref's bounds of the float64 NT scaling
      (w component by component -- the difference sb - J zb cancels -- and eta), which lose 1 / gap of the pair (cone_ref.rcond;
      tests/test_cone_cpu.py shows that no constant could stand in for it);
  stages 1, 4, 7 (G'u):  lattice_ref.K_GT u Ghat'|u|;   stages 3, 6 (G v):  lattice_ref.K_G u Ghat |v|, carried through |W^-2| into
      W^-2 G v - sub, plus the rounding of the subtraction (4 u |result|: one rounding, times the margin of 4);
  stage 2, and z in 5 / 9 (M'(M rhs)):  (2 np + HS_PARTS + 8) u |M|'(|M| |rhs|): a row's dot product and the sum over the rows are np
      terms each, the fold adds HS_PARTS partial vectors, rhs = bx + t is one rounding;
  stage 4:  r = fl(bx - t) of the device's own t, bit for bit; n_0 = max_v ||r_v|| within K_N u n_0, K_N = ceil(N / SCAL_T) + 13 (a
      thread's strided terms, the wave's six levels, four waves, the square, the root);
  stages 5 / 9:  rz = r'z within K_N u |r|'|z| (where the fused form keeps z in LDS: within |r|'bound(z) more); beta = rz_new /
      rz_old in float64 exactly as the kernel forms it from the two scalars it reads and writes, 0 at the first start and for
      rz_old <= 0; p within two roundings of z + beta p (an fma is one of them);
  stage 8:  p'Hp within K_N u |p|'|Hp|; alpha = rz / p'Hp within that and two roundings, exactly 0 where p'Hp <= 0 (the decision is
      held where the reference's sign is not in doubt); dx, r, gdx, dz within two roundings each of the device's own alpha and
      operands; n_{q+1} as n_0; every vector has its own alpha;
  the end, with no hand-over:  ||bx - G'dz|| in longdouble against the last norm, gdx against G dx, dz against W^-2 gdx - W^-2 bz,
      each within the sum of the bounds of the stages that built them;
  the residual kernels:  rz = G x + s - h tau (K_G, and 8 u (|G x| + |s| + |h tau|): its three roundings come to 2 u of that, times the margin of 4), bz2 = (h, fl(s - rz)) exactly, G'z (K_GT), rx = G'z + c tau
      (two roundings), bx2 = (-c, -rx) exactly; the row sums within K_R u sum |terms| (K_R = ceil(blocks / SCAL_T) + 22), the column
      sums within K_N; each scalar by its definition in k_scal_resid from the device's own sums where it reads them back from Sc; the
      decisions den > 0, hz < 0, cx < 0 (else 1e300) are the reference's exactly.

That the sweeps refine at all is measured against the twin, not against the device: twin() restates oracle/conic_ipm.py's kkt_solve
in float64 with an explicit M.  Its norms n_q under two summation orders (the folding kernels' own -- a thread's strided terms, then a tree --, and a strict left-to-right loop) and
the two forms of the preconditioner (M'(M r); the two triangular solves with the Cholesky factor) are compared as max(n_q, floor),
the floor being stage 4's bound of r as a norm.  Measured: the spread is 1.000 on all 16 runs -- the twin's M is the exact inverse
factor of its own operator, so its n_0 (1e-15 .. 4e-4) already lies a factor 7 .. 400 below the floor and every later n_q a factor
1e-14 below the one before.  Hence SPREAD_MEASURED = 1 and FACTOR = 4 x 1 (the project's usual margin): the device's n_q may not
exceed 4 max(twin n_q, floor).  tests/test_kkt_cpu.py measures the spread and asserts that FACTOR covers it.
"""
import numpy as np

import cone_ref as CR
import lattice_ref as L

LD = np.longdouble
U = 2.0 ** -53
SCAL_T, HS_PARTS, MAX_SWEEPS = 256, 32, 8
SPREAD_MEASURED = 1.0        # (test_kkt_cpu.test_twin_spread_sets_the_factor prints the measured value)
FACTOR = 4.0
# the bounds that COUNT the roundings of one short expression (two roundings of a + alpha b, the quotients and sums of k_scal_resid's
# thread 0): float64 arithmetic attains them, so the twin is held to the bound itself there, and to a quarter of every other bound
COUNTED = {("8", "dx"), ("8", "r"), ("8", "gdx"), ("8", "dz"), ("9", "p"), ("res", "rx"), ("res", "rt"), ("res", "mu"), ("res", "pcost"),
           ("res", "dcost"), ("res", "gap"), ("res", "relgap")}


def ld(a):
    a = np.asarray(a)
    return a if a.dtype == LD else a.astype(np.float64).astype(LD)


def f64(a):
    return np.asarray(a).astype(np.float64)


def k_n(N):
    return -(-N // SCAL_T) + 13


def k_r(P):
    return -(-(-(-P["R"] // 256)) // SCAL_T) + 22


def k_m(npd):
    return 2 * npd + HS_PARTS + 8


# ---- the operators of one design at one iterate -------------------------------------------------------------------------------------
class Ops:
    """G, its envelope, W^-2 at (s, z) and the constants of the bounds.  unit: W = I (the initial point)."""

    def __init__(self, P, s, z, dense=False, unit=False):
        self.P = P
        self.G, self.Gh = L.G_ref(P), L.G_hat(P)
        self.kg, self.kgt = L.K_G(P, dense), L.K_GT(P, dense)
        self.rescale(s, z, unit)

    def rescale(self, s, z, unit=False):
        P = self.P
        if unit:
            s = z = CR_e(P)
        self.S = L.Scaling(P, s, z)
        self.blocks = []
        for (r0, m, kind, c) in CR.socs(P):
            sf, zf = np.asarray(s, dtype=np.float64)[r0:r0 + m], np.asarray(z, dtype=np.float64)[r0:r0 + m]
            rs, rz, kd = CR.rcond(sf, m), CR.rcond(zf, m), CR.kd(m)
            sl, zl = ld(sf), ld(zf)
            sb = sl / np.sqrt(sl[0] ** 2 - (sl[1:] ** 2).sum())
            zb = zl / np.sqrt(zl[0] ** 2 - (zl[1:] ** 2).sum())
            gam = np.sqrt((1 + (sb * zb).sum()) / 2)
            eta, wb = L._soc_nt(sl[None], zl[None])
            q, sa, za = np.abs(f64(wb[0])), np.abs(f64(sb)), np.abs(f64(zb))
            # the error of the float64 w, component by component (cone_ref.check_scaling): the difference sb - J zb cancels
            E = float(sa @ za) / float(1 + (sb * zb).sum())
            bq = U * ((sa * rs + za * rz) / (2 * float(gam)) + q * (E * (rs + rz + kd) / 2 + 4))
            reta = U * ((rs + rz) / 2 + 3)
            env = (2 * np.outer(q, q) + np.eye(m)) / float(eta[0]) ** 2
            err = 2 * (np.outer(bq, q) + np.outer(q, bq)) / float(eta[0]) ** 2 + (2 * reta + (kd + 8) * U) * env
            self.blocks.append((r0, m, env, err))
        return self

    def _rows(self, X, which, korth):
        out = np.empty_like(X)
        l = self.P["l"]
        out[:l] = korth * f64(self.S.d)[:, None] * X[:l]
        for blk in self.blocks:
            out[blk[0]:blk[0] + blk[1]] = blk[which] @ X[blk[0]:blk[0] + blk[1]]
        return out

    def env_winv2(self, X):
        """(2 |q||q|' + I) / eta^2 |X| on the cones, |d| |X| on the orthant; X: (R, k) float64, non-negative."""
        return self._rows(X, 2, 1.0)

    def err_winv2(self, X):
        """the bound of the kernels' W^-2 X for an exact X >= 0 (see the module docstring)."""
        return self._rows(X, 3, 8 * U)

    # vectors are (nv, n) arrays; every product returns (reference in longdouble, bound in float64)
    def gv(self, v):
        return (self.G @ ld(v).T).T, self.kg * U * (self.Gh @ np.abs(f64(v)).T).T

    def gtv(self, u):
        return (self.G.T @ ld(u).T).T, self.kgt * U * (self.Gh.T @ np.abs(f64(u)).T).T

    def winv2(self, g, gb=None, sub=None):
        """W^-2 g - sub for g known within gb."""
        ref = self.S.winv2(ld(g).T).T
        b = self.err_winv2(np.abs(f64(g)).T).T
        if gb is not None:
            b = b + self.env_winv2(gb.T).T
        if sub is not None:
            ref = ref - ld(sub)
            b = b + U * (4 * np.abs(f64(ref)) + np.abs(f64(sub)))
        return ref, b


def CR_e(P):
    e = np.zeros(P["R"])
    e[:P["l"]] = 1.0
    for (r0, m, kind, c) in CR.socs(P):
        e[r0] = 1.0
    return e


def msolve(M, rhs, N):
    """M'(M rhs) of the np x np inverse factor for rhs (nv, N), and its bound."""
    npd = M.shape[0]
    r = np.zeros((rhs.shape[0], npd), dtype=LD)
    r[:, :N] = ld(rhs)
    Ml, Ma = ld(M), np.abs(M)
    ref = (Ml.T @ (Ml @ r.T)).T[:, :N]
    b = k_m(npd) * U * (Ma.T @ (Ma @ np.abs(f64(r)).T)).T[:, :N]
    return ref, b


def vnorm(r):
    return np.sqrt((ld(r) ** 2).sum(1)).max()


def rows_dot(a, b):
    return (ld(a) * ld(b)).sum(1), (np.abs(f64(a)) * np.abs(f64(b))).sum(1)


# ---- the hook's result -----------------------------------------------------------------------------------------------------------
def unpack(o, b, P, nv):
    """lane b of mbfir.test_unit_kkt's result as a dict of named blocks (nv, N) / (nv, R), cut to the lane's own rows."""
    import mbfir
    R, N = P["R"], P["N"]
    D = {k: o["out_x"][b, i, :nv, :N].copy() for i, k in enumerate(mbfir.UNIT_KKT_OUT_X)}
    D.update({k: o["out_r"][b, i, :nv, :R].copy() for i, k in enumerate(mbfir.UNIT_KKT_OUT_R)})
    D["sc"] = {sn: dict(zip(mbfir.UNIT_KKT_SC, o["sc"][b, i])) for i, sn in enumerate(mbfir.UNIT_KKT_SNAPS)}
    D["res"] = {k: o["res_r"][b, i, :R].copy() for i, k in enumerate(mbfir.UNIT_KKT_RES_R)}
    D["res"].update({k: o["res_x"][b, i, :N].copy() for i, k in enumerate(mbfir.UNIT_KKT_RES_X)})
    D["res"]["sc"] = dict(zip(mbfir.UNIT_KKT_RES_SC, o["res_sc"][b]))
    npd = -(-N // 64) * 64
    D["M"] = o["M"][b, :npd, :npd].copy()
    D["flag"] = int(o["flag"][b])
    D["init"] = {k: o["init_r"][b, i, :R].copy() for i, k in enumerate(mbfir.UNIT_KKT_INIT_R)}
    D["init"].update({"x_" + k if k == "x" else "i" + k: o["init_x"][b, i, :N].copy() for i, k in enumerate(mbfir.UNIT_KKT_INIT_X)})
    D["init"]["w3"] = o["w3"][b].copy()
    D["raw_x"], D["raw_r"], D["raw_sc"] = o["out_x"][b].copy(), o["out_r"][b].copy(), o["sc"][b].copy()
    return D


def two_roundings(rec, st, name, dev, a, t, extra=0.0):
    """dev within two roundings of a + t (the product t rounded, the sum rounded; an fma rounds once)."""
    ref = ld(a) + t
    rec.add(st, name, np.abs(ld(dev) - ref), extra + 1.001 * U * (np.abs(f64(t)) + np.abs(f64(ref))))


# ---- the solve, stage by stage ---------------------------------------------------------------------------------------------------
def check_solve(P, O, D, bx, bz, ns, nv, z_written, rec=None, sentinel=np.nan):
    """Holds lane data D (unpack) of a solve of (bx, bz) (nv, N) / (nv, R) with ns sweeps to the reference.  Returns (rec, facts)."""
    rec = rec or CR.Rec()
    N, R = P["N"], P["R"]
    M = D["M"]

    def kept(v):
        return bool(np.isnan(v) if np.isnan(sentinel) else v == sentinel)
    kn = k_n(N)
    sc = D["sc"]
    facts = dict(pHp_pos=[], beta_zero=[], undecided=[], norms=[])
    bx, bz = np.asarray(bx, dtype=np.float64), np.asarray(bz, dtype=np.float64)
    ref, b0 = O.winv2(bz)
    rec.add("0", "wbz", np.abs(ld(D["wbz"]) - ref), b0)
    ref, b1 = O.gtv(D["wbz"])
    rec.add("1", "G'wbz", np.abs(ld(D["gtwbz"]) - ref), b1)
    ref, b2 = msolve(M, ld(bx) + ld(D["gtwbz"]), N)
    rec.add("2", "dx", np.abs(ld(D["dxc"]) - ref), b2)
    g, gb = O.gv(D["dxc"])
    rec.add("3", "gdx", np.abs(ld(D["gdxc"]) - g), gb)
    ref, b3 = O.winv2(g, gb, D["wbz"])
    rec.add("3", "dz", np.abs(ld(D["dzc"]) - ref), b3)
    ref, b4 = O.gtv(D["dzc"])
    rec.add("4", "G'dz", np.abs(ld(D["gtdz"]) - ref), b4)
    rec.exact("4", "r = fl(bx - t)", np.array_equal(D["rc"], bx - D["gtdz"]))

    def norm_check(st, r, q, snap, prev):
        n = vnorm(r)
        rec.add(st, "n%d" % q, abs(LD(sc[snap]["n%d" % q]) - n), kn * U * float(n))
        for k in range(MAX_SWEEPS + 1):
            v = sc[snap]["n%d" % k]
            if k > q:
                rec.exact(st, "n%d untouched after %s" % (k, snap), kept(v))
            elif k < q:
                rec.exact(st, "n%d kept after %s" % (k, snap), v == sc[prev]["n%d" % k])
        facts["norms"].append(float(sc[snap]["n%d" % q]))
    norm_check("4", D["rc"], 0, "resid", None)
    floor = float(np.sqrt((b4 ** 2).sum(1)).max()) + 2 * U * float(np.sqrt(((np.abs(bx) + np.abs(D["gtdz"])) ** 2).sum(1)).max())
    facts["floor"] = floor

    def start(q, r, p_old):
        """the start of sweep q (q = 0: first): z = M'M r, rz, beta, p."""
        st = "5" if q == 0 else "9"
        zr, zb = msolve(M, r, N)
        p = D["p%d" % q]
        extra = np.zeros((nv, N))
        if z_written:
            rec.add(st, "z", np.abs(ld(D["z%d" % q]) - zr), zb)
            z = D["z%d" % q]
        elif q == 0:
            rec.add(st, "p = z", np.abs(ld(p) - zr), zb)
            z = p
        else:
            z, extra = zr, zb
        dot, env = rows_dot(r, z)
        more = (np.abs(f64(r)) * extra).sum(1)
        for v in range(nv):
            rec.add(st, "rz", abs(LD(sc["start%d" % q]["rz%d" % v]) - dot[v]), more[v] + kn * U * env[v])
        if q == 0:
            if z_written:
                rec.exact(st, "p = z at the first start", np.array_equal(p, z))
            return
        for v in range(nv):
            new, old = sc["start%d" % q]["rz%d" % v], sc["start%d" % (q - 1)]["rz%d" % v]
            beta = new / old if old > 0 else 0.0
            facts["beta_zero"].append(not old > 0)
            two_roundings(rec, st, "p", p[v], z[v], LD(beta) * ld(p_old[v]), extra[v])

    acc = dict(gt=np.abs(D["dzc"]).copy(), g=np.abs(D["dxc"]).copy(), r_round=np.zeros((nv, N)), dz_round=np.zeros((nv, R)),
               gdx_round=np.zeros((nv, R)), dx_round=np.zeros((nv, N)), w=b3.copy())
    last = dict(dx=D["dxc"], r=D["rc"], gdx=D["gdxc"], dz=D["dzc"])
    if ns > 0:
        start(0, D["rc"], None)
    for q in range(ns):
        p = D["p%d" % q]
        g, gb = O.gv(p)
        rec.add("6", "Gp", np.abs(ld(D["gp%d" % q]) - g), gb)
        ref, b6 = O.winv2(g, gb)
        rec.add("6", "W^-2 Gp", np.abs(ld(D["wp%d" % q]) - ref), b6)
        ref, b7 = O.gtv(D["wp%d" % q])
        hp = D["hp%d" % q]
        rec.add("7", "Hp", np.abs(ld(hp) - ref), b7)
        dot, env = rows_dot(p, hp)
        al = np.zeros(nv)
        for v in range(nv):
            a_dev = sc["step%d" % q]["alpha%d" % v]
            al[v] = a_dev
            pb = kn * U * env[v]
            rzv = sc["start%d" % q]["rz%d" % v]
            if dot[v] > pb:
                a_ref = LD(rzv) / dot[v]
                rec.add("8", "alpha", abs(LD(a_dev) - a_ref), (pb / float(dot[v] - pb) + 2 * U) * abs(float(a_ref)))
                facts["pHp_pos"].append(True)
            elif dot[v] < -pb or (dot[v] == 0 and pb == 0):
                rec.exact("8", "alpha = 0 where p'Hp <= 0", a_dev == 0.0)
                facts["pHp_pos"].append(False)
            else:
                facts["undecided"].append((q, v))
        A = ld(al)[:, None]
        for name, old, t in (("dx", last["dx"], A * ld(p)), ("r", last["r"], -A * ld(hp)), ("gdx", last["gdx"], A * ld(D["gp%d" % q])),
                             ("dz", last["dz"], A * ld(D["wp%d" % q]))):
            two_roundings(rec, "8", name, D["%s%d" % (name, q)], old, t)
        norm_check("8", D["r%d" % q], q + 1, "step%d" % q, "start%d" % q)
        aa = np.abs(al)[:, None]
        acc["gt"] += aa * np.abs(D["wp%d" % q])
        acc["g"] += aa * np.abs(p)
        acc["w"] += aa * b6
        acc["r_round"] += 2 * U * (np.abs(last["r"]) + aa * np.abs(hp))
        acc["dx_round"] += 2 * U * (np.abs(last["dx"]) + aa * np.abs(p))
        acc["gdx_round"] += 2 * U * (np.abs(last["gdx"]) + aa * np.abs(D["gp%d" % q]))
        acc["dz_round"] += 2 * U * (np.abs(last["dz"]) + aa * np.abs(D["wp%d" % q]))
        last = {k: D["%s%d" % (k, q)] for k in ("dx", "r", "gdx", "dz")}
        if q + 1 < ns:
            start(q + 1, D["r%d" % q], p)
    # ---- the end: what the solve leaves, and the three identities with no hand-over -----------------------------------------------
    for k in ("dx", "r", "gdx", "dz"):
        rec.exact("end", k + " as the last sweep left it", np.array_equal(D[k + "_end"], last[k]))
    for k in range(MAX_SWEEPS + 1):
        v = sc["end"]["n%d" % k]
        rec.exact("end", "n%d" % k, kept(v) if k > ns else v == facts["norms"][k])
    for v in range(nv):                                     # the sweep's scalars: as the lane's own last start and step left them
        for k, snap in (("rz%d" % v, "start%d" % (ns - 1)), ("alpha%d" % v, "step%d" % (ns - 1))):
            rec.exact("end", k + " as the lane's last sweep left it", kept(sc["end"][k]) if ns == 0 else sc["end"][k] == sc[snap][k])
    Gabs = np.abs(f64(O.G))
    true_r = ld(bx) - (O.G.T @ ld(D["dz_end"]).T).T
    br = O.kgt * U * (O.Gh.T @ acc["gt"].T).T + acc["r_round"] + (Gabs.T @ acc["dz_round"].T).T + 2 * U * (np.abs(bx) + np.abs(D["gtdz"]))
    n_true = np.sqrt((true_r ** 2).sum(1)).max()
    rec.add("end", "||bx - G'dz|| = n_last", abs(LD(facts["norms"][ns]) - n_true), float(np.sqrt((br ** 2).sum(1)).max()) + kn * U * float(n_true))
    bg = O.kg * U * (O.Gh @ acc["g"].T).T + acc["gdx_round"] + (Gabs @ acc["dx_round"].T).T
    rec.add("end", "gdx = G dx", np.abs(ld(D["gdx_end"]) - (O.G @ ld(D["dx_end"]).T).T), bg)
    ref, bw = O.winv2(D["gdx_end"], None, D["wbz"])
    bw = bw + acc["w"] + acc["dz_round"] + O.env_winv2((acc["gdx_round"] + bg).T).T
    rec.add("end", "dz = W^-2 gdx - W^-2 bz", np.abs(ld(D["dz_end"]) - ref), bw)
    return rec, facts


def untouched(P, D, ns, nv, z_written, sentinel=np.nan):
    """names of the blocks and snapshots that do not hold the sentinel where no launch of this lane writes: the sweeps past the
    lane's count, the second vector where nv = 1, z where the fused form keeps it in LDS, and (P given) the entries past the lane's
    own N / R -- but for dx and z, which M'(M b) writes over all np entries."""
    import re

    import mbfir

    def kept(a):
        return bool(np.all(np.isnan(a) if np.isnan(sentinel) else a == sentinel))
    bad = []
    for names, raw, n in ((mbfir.UNIT_KKT_OUT_X, D["raw_x"], P["N"] if P else None), (mbfir.UNIT_KKT_OUT_R, D["raw_r"], P["R"] if P else None)):
        for i, k in enumerate(names):
            if nv == 1 and not kept(raw[i, 1]):
                bad.append(k + " vector 1")
            m = re.match(r"^([a-z]+)(\d)$", k)
            dead = bool(m) and (int(m.group(2)) >= ns or (m.group(1) == "z" and not z_written))
            if dead and not kept(raw[i]):
                bad.append(k)
            if n is not None and not k.startswith(("dx", "z")) and not kept(raw[i, :, n:]):
                bad.append(k + " past the lane's rows")
    for i, sn in enumerate(mbfir.UNIT_KKT_SNAPS):
        m = re.match(r"^([a-z]+)(\d)$", sn)
        if m and int(m.group(2)) >= ns and not kept(D["raw_sc"][i]):
            bad.append("snapshot " + sn)
    return bad


# ---- the residual kernels --------------------------------------------------------------------------------------------------------
def check_residuals(P, O, D, I, form, rec=None, sentinel=np.nan):
    """I: dict(s, z, x, tau, kappa).  Returns (rec, facts): facts holds the signs of hz and cx and their margins."""
    rec = rec or CR.Rec()
    N, R = P["N"], P["R"]
    res, sc = D["res"], D["res"]["sc"]
    s, z, x, tau, kap = I["s"], I["z"], I["x"], I["tau"], I["kappa"]
    h, c = P["h"], P["c"]
    st = "res"
    rec.exact(st, "tau, kappa", sc["tau"] == tau and sc["kappa"] == kap)
    g, gb = O.gv(x[None])
    g, gb = g[0], gb[0]
    ref = g + ld(s) - ld(h) * LD(tau)
    rec.add(st, "rz", np.abs(ld(res["rz"]) - ref), gb + 8 * U * (np.abs(f64(g)) + np.abs(s) + np.abs(h * tau)))
    rec.exact(st, "bz2[0] = h", np.array_equal(res["bz2a"], h))
    rec.exact(st, "bz2[1] = fl(s - rz)", np.array_equal(res["bz2b"], s - res["rz"]))
    gt, gtb = O.gtv(z[None])
    rec.add(st, "G'z", np.abs(ld(res["gtz"]) - gt[0]), gtb[0])
    two_roundings(rec, st, "rx", res["rx"], res["gtz"], ld(c) * LD(tau))
    rec.exact(st, "bx2[0] = -c", np.array_equal(res["bx2a"], -c))
    rec.exact(st, "bx2[1] = -rx", np.array_equal(res["bx2b"], -res["rx"]))
    kr, kn = k_r(P), k_n(N)

    def rsum(a, b):
        return (ld(a) * ld(b)).sum(), float((np.abs(f64(a)) * np.abs(f64(b))).sum())
    hz, hze = rsum(h, z)
    sz, sze = rsum(s, z)
    cx, cxe = rsum(c, x)
    rz2, _ = rsum(res["rz"], res["rz"])
    rx2, _ = rsum(res["rx"], res["rx"])
    gtz2, _ = rsum(res["gtz"], res["gtz"])
    gxs = g + ld(s)
    gxs2 = (gxs ** 2).sum()
    gxs2_b = float((2 * np.abs(f64(gxs)) * (gb + U * np.abs(f64(gxs)))).sum()) + (kr + 2) * U * float(gxs2)
    rec.add(st, "hz", abs(LD(sc["hz"]) - hz), kr * U * hze)
    rec.add(st, "sz", abs(LD(sc["sz"]) - sz), kr * U * sze)
    rec.add(st, "cx", abs(LD(sc["cx"]) - cx), kn * U * cxe)
    # from here every scalar by its definition, from the sums the kernel itself wrote to Sc (cx, hz, sz) and the reference's others
    dcx, dhz, dsz = LD(sc["cx"]), LD(sc["hz"]), LD(sc["sz"])
    T, K = LD(tau), LD(kap)

    def rel(name, ref, k):
        rec.add(st, name, abs(LD(sc[name]) - ref), k * U * abs(float(ref)))
    ref = K + dcx + dhz
    rec.add(st, "rt", abs(LD(sc["rt"]) - ref), 2 * U * (abs(float(K + dcx)) + abs(float(ref))))
    rel("mu", (dsz + K * T) / (LD(sc["deg"]) + 1), 4)
    rel("pcost", dcx / T, 1)
    rel("dcost", -dhz / T, 1)
    rel("gap", dsz / (T * T), 2)
    rel("nrmh", max(LD(1), np.sqrt((ld(h) ** 2).sum())), R + 2)          # (the host's sequential sums)
    rel("nrmc", max(LD(1), np.sqrt((ld(c) ** 2).sum())), N + 2)
    rec.exact(st, "degree", sc["deg"] == P["l"] + P["nq3"] + (1 if P["big"] else 0))
    rel("pres", np.sqrt(rz2) / T / LD(sc["nrmh"]), kr / 2 + 5)
    rel("dres", np.sqrt(rx2) / T / LD(sc["nrmc"]), kn / 2 + 5)
    den = max(abs(sc["pcost"]), abs(sc["dcost"]))
    rec.exact(st, "den > 0", den > 0)
    if den > 0:
        rel("relgap", LD(sc["gap"]) / LD(den), 1)
    facts = dict(hz_neg=bool(hz < 0), cx_neg=bool(cx < 0), hz_margin=abs(float(hz)) / max(hze, 1e-300), cx_margin=abs(float(cx)) / max(cxe, 1e-300))
    if hz < 0:
        rel("pinf", np.sqrt(gtz2) / (-dhz), kn / 2 + 4)
    else:
        rec.exact(st, "pinf = 1e300", sc["pinf"] == 1e300)
    if cx < 0:
        ref = np.sqrt(gxs2) / (-dcx)
        rec.add(st, "dinf", abs(LD(sc["dinf"]) - ref), (gxs2_b / float(gxs2) / 2 + 4 * U) * float(ref))
    else:
        rec.exact(st, "dinf = 1e300", sc["dinf"] == 1e300)
    rec.exact(st, "cholfix", sc["cholfix"] == 0.0)
    # the mailbox: the four row sums (and the pivot count) where the two-phase form folds them, untouched otherwise
    rb = [sc["rb%d" % k] for k in range(5)]
    if form:
        rec.add(st, "mailbox rz2", abs(LD(rb[0]) - rz2), (kr + 2) * U * float(rz2))
        rec.exact(st, "mailbox sz, hz", rb[1] == sc["sz"] and rb[2] == sc["hz"])
        rec.add(st, "mailbox gxs2", abs(LD(rb[3]) - gxs2), gxs2_b)
        rec.exact(st, "mailbox pivots", rb[4] == 0.0)
    else:
        rec.exact(st, "mailbox untouched", all(np.isnan(v) if np.isnan(sentinel) else v == sentinel for v in rb))
    return rec, facts


# ---- the float64 twin (oracle/conic_ipm.py kkt_solve with an explicit M) ---------------------------------------------------------------
def seq_sum(a):
    out = np.zeros(a.shape[1:])
    for row in a:
        out = out + row
    return out


def tree_sum(a):
    """the sum over axis 0 by halving (a power-of-two count): the depth of a wave's butterfly and the fold of the waves."""
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def dev_sum(a, threads=SCAL_T):
    """the sum over axis 0 as a one-workgroup folding kernel forms it: thread t adds its entries t, t + threads, ... in order, the
    threads' partial sums are added by a tree."""
    n = a.shape[0]
    pad = np.zeros((-(-n // threads) * threads,) + a.shape[1:])
    pad[:n] = a
    return tree_sum(seq_sum(pad.reshape((-1, threads) + a.shape[1:])))


def dev_row_sum(a):
    """a sum over the rows as k_resid_rows and k_scal_resid form it: a tree per block of 256 rows, then dev_sum over the blocks."""
    n = a.shape[0]
    pad = np.zeros((-(-n // 256) * 256,) + a.shape[1:])
    pad[:n] = a
    return dev_sum(np.stack([tree_sum(b) for b in pad.reshape((-1, 256) + a.shape[1:])]))


def factor64(P, Gm, Wm):
    """M = L^-1 of the np x np padded H = G'W^-2 G (float64), and L."""
    from scipy.linalg import cholesky, solve_triangular
    N = P["N"]
    npd = -(-N // 64) * 64
    H = np.eye(npd)
    H[:N, :N] = Gm.T @ (Wm.inv2(Gm) if Wm is not None else Gm)
    Lc = cholesky(H, lower=True)
    return solve_triangular(Lc, np.eye(npd), lower=True), Lc


def twin(P, Gm, Wm, M, bx, bz, ns, order="device", precond="M", Lc=None):
    """kkt_solve in float64 on the model G; returns the blocks of unpack() that check_solve reads.  order: 'device' (dev_sum) | 'seq'
    (left to right), the sums of the dot products and norms; precond: 'M' (M'(M r)) | 'chol' (two triangular solves with Lc)."""
    from scipy.linalg import solve_triangular
    N, R = P["N"], P["R"]
    nv = bx.shape[0]
    npd = M.shape[0]
    add = dev_sum if order == "device" else seq_sum
    inv2 = (lambda v: Wm.inv2(v)) if Wm is not None else (lambda v: v.copy())

    def hs(r):                                              # columns
        rp = np.zeros((npd, nv))
        rp[:N] = r
        if precond == "M":
            return (M.T @ (M @ rp))[:N]
        return solve_triangular(Lc, solve_triangular(Lc, rp, lower=True), lower=True, trans="T")[:N]

    def norm(r):
        return float(np.sqrt(add(r * r)).max())
    D, sc = {}, {}
    nan9 = {"n%d" % k: np.nan for k in range(MAX_SWEEPS + 1)}
    BX, BZ = bx.T.copy(), bz.T.copy()
    wbz = inv2(BZ)
    t1 = Gm.T @ wbz
    dx = hs(BX + t1)
    gdx = Gm @ dx
    dz = inv2(gdx) - wbz
    t4 = Gm.T @ dz
    r = BX - t4
    norms = dict(nan9, n0=norm(r))
    for k, v in (("wbz", wbz), ("gtwbz", t1), ("dxc", dx), ("gdxc", gdx), ("dzc", dz), ("gtdz", t4), ("rc", r)):
        D[k] = v.T.copy()
    sc["resid"] = dict(norms)
    rz = np.zeros(nv)
    p = None
    for q in range(ns):
        z = hs(r)
        rz_new = add(r * z)
        if q == 0:
            p = z.copy()
        else:
            beta = np.where(rz > 0, rz_new / np.where(rz > 0, rz, 1.0), 0.0)
            p = z + beta * p
        rz = rz_new
        D["z%d" % q], D["p%d" % q] = z.T.copy(), p.T.copy()
        sc["start%d" % q] = dict(norms, rz0=rz[0], rz1=rz[-1])
        gp = Gm @ p
        wp = inv2(gp)
        hp = Gm.T @ wp
        pHp = add(p * hp)
        al = np.where(pHp > 0, rz / np.where(pHp > 0, pHp, 1.0), 0.0)
        dx, r, gdx, dz = dx + al * p, r - al * hp, gdx + al * gp, dz + al * wp
        norms["n%d" % (q + 1)] = norm(r)
        for k, v in (("gp", gp), ("wp", wp), ("hp", hp), ("dx", dx), ("r", r), ("gdx", gdx), ("dz", dz)):
            D["%s%d" % (k, q)] = v.T.copy()
        sc["step%d" % q] = dict(norms, rz0=rz[0], rz1=rz[-1], alpha0=al[0], alpha1=al[-1])
    for k, v in (("dx", dx), ("r", r), ("gdx", gdx), ("dz", dz)):
        D[k + "_end"] = v.T.copy()
    sc["end"] = dict(sc["step%d" % (ns - 1)], **norms) if ns else dict(norms, rz0=np.nan, rz1=np.nan, alpha0=np.nan, alpha1=np.nan)
    D["sc"], D["M"] = sc, M
    return D


def refines(facts, twin_sc, ns):
    """the device's norms (facts of check_solve) against the twin's: the q that exceed FACTOR max(twin n_q, floor)."""
    return [(q, facts["norms"][q], twin_sc["end"]["n%d" % q]) for q in range(ns + 1)
            if not facts["norms"][q] <= FACTOR * max(twin_sc["end"]["n%d" % q], facts["floor"])]


def check_shift(P, v, out, rec, name):
    """cone_ref's shift rule (k_cone_shift) applied to v: with t = the largest cone distance of v, every cone's head entry becomes
    v + (1 + t) where t >= -1e-8 max(1, ||v||); everything else is v bit for bit.  Returns whether it shifted (None: not decidable)."""
    l = P["l"]
    dist, bd, heads = [-np.inf], [0.0], list(range(l))
    if l:
        dist.append(float(np.max(-v[:l])))
    for (r0, m, kind, c) in CR.socs(P):
        vm = CR.mpv(v[r0:r0 + m])
        dist.append(float(CR.mnorm(vm[1:]) - vm[0]))
        bd.append(U * (CR.kd(m) / 2 + 2) * (float(np.linalg.norm(v[r0 + 1:r0 + m])) + abs(v[r0])))
        heads.append(r0)
    t, n2 = max(dist), float((ld(v) ** 2).sum())
    thr = -1e-8 * max(1.0, np.sqrt(n2))
    other = np.ones(len(v), dtype=bool)
    other[heads] = False
    rec.exact("init", name + ": entries that are no cone's head", np.array_equal(out[other], v[other]))
    if abs(t - thr) <= 1e-6 * max(abs(t), abs(thr)):
        return None
    if t >= thr:
        want = ld(v[heads]) + (LD(1) + LD(t))
        rec.add("init", name + " shifted", np.abs(ld(out[heads]) - want), 3 * U * (np.abs(v[heads]) + 1 + abs(t)) + max(bd))
    else:
        rec.exact("init", name + " not shifted", np.array_equal(out[heads], v[heads]))
    return t >= thr


def twin_residuals(P, Gm, I, form):
    """k_resid_rows / k_scal_resid in float64 on the model G: the blocks of unpack()['res']."""
    s, z, x, tau, kap = I["s"], I["z"], I["x"], I["tau"], I["kappa"]
    h, c = P["h"], P["c"]
    gx = Gm @ x
    rz = gx + s - h * tau
    gtz = Gm.T @ z
    rx = gtz + c * tau
    cx, hz, sz = float(dev_sum(c * x)), float(dev_row_sum(h * z)), float(dev_row_sum(s * z))
    deg = P["l"] + P["nq3"] + (1 if P["big"] else 0)
    nrmh, nrmc = max(1.0, float(np.linalg.norm(h))), max(1.0, float(np.linalg.norm(c)))
    pcost, dcost, gap = cx / tau, -hz / tau, sz / (tau * tau)
    den = max(abs(pcost), abs(dcost))
    sc = dict(rt=kap + cx + hz, mu=(sz + kap * tau) / (deg + 1.0), pcost=pcost, dcost=dcost, gap=gap, relgap=gap / den if den > 0 else 1e300,
              pres=np.sqrt(dev_row_sum(rz * rz)) / tau / nrmh, dres=np.sqrt(dev_sum(rx * rx)) / tau / nrmc,
              pinf=np.sqrt(dev_sum(gtz * gtz)) / (-hz) if hz < 0 else 1e300, dinf=np.sqrt(dev_row_sum((gx + s) * (gx + s))) / (-cx) if cx < 0 else 1e300, cx=cx, hz=hz, sz=sz, cholfix=0.0, tau=tau, kappa=kap,
              nrmh=nrmh, nrmc=nrmc, deg=float(deg))
    rb = [rz @ rz, sz, hz, (gx + s) @ (gx + s), 0.0] if form else [np.nan] * 5
    sc.update({"rb%d" % k: v for k, v in enumerate(rb)})
    return dict(rz=rz, bz2a=h.copy(), bz2b=s - rz, gtz=gtz, rx=rx, bx2a=-c, bx2b=-rx, sc=sc)


def rhs_of(run, I, res):
    """the right-hand sides (bx, bz) of a run: its own draw, or what the residual kernels left (res: unpack()['res'])."""
    if run[2] != "own":
        return I["bx"], I["bz"]
    return np.stack([res["bx2a"], res["bx2b"]]), np.stack([res["bz2a"], res["bz2b"]])


def model_G(P, dense=False):
    """G in float64 as the kernels form it: lattice_ref's model of the recurrences, or (dense) one sincos per entry."""
    if dense:
        return L.G_ref(P, round_arg=True).astype(np.float64)
    La = L.analyse(P)
    return L.model_G(P, *L.model_eval_trig(P, La), La)


def oracle_scaling(P, s, z):
    from oracle import conic_ipm as O
    return O._Scaling(O._Cone(P["l"], P["nq3"], P["big"]), np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64))


# ---- the designs and runs of the device tests ------------------------------------------------------------------------------------
def designs():
    """cone_ref's small designs and four more: three evaluation segments and N > SCAL_T (c2_ap150), the dense operators (c1_ap24
    with opts.dense_trig), and the two orders either side of np = 1024."""
    out = {k: dict(v) for k, v in CR.designs().items() if k != "n600"}
    U_ = L.unit_cases()
    out["c2_ap150"] = dict(job=U_["c2_ap150"]["job"], grid_m=U_["c2_ap150"]["grid_m"], ddkkt=0)
    out["c1_ap24d"] = dict(job=U_["c1_ap24"]["job"], grid_m=U_["c1_ap24"]["grid_m"], ddkkt=0, dense=True)
    # np = 1024, the benchmark unit's size: the largest the one-pass M'(M b) and the 1024-thread k_fold_cg_start take; and the smallest
    # order of fir_qprog_phs past it (np = 1088): the two triangular products by size, k_cg_start.  The grids are the smallest the
    # designers accept for these orders.
    from conftest import CASES, c13
    out["n512_ap"] = dict(job=("fir_ap_cvx", (512,) + tuple(c13(512)) + (0.1, 1e-3)), grid_m=1100, ddkkt=0)
    out["n512_qphs"] = dict(job=("fir_qprog_phs", (512,) + tuple(CASES["qphs21"][1][1:])), grid_m=600, ddkkt=0)
    return out


# (design, iterate, right-hand sides, nv, wbz_ready, h'z < 0): 'own' = the two the residual kernels leave, 'random', 'zero' = random
# with an all-zero second column; h'z < 0: z on the orthant rows with h < 0 is raised (and s lowered: s z stays) until h'z < 0 with a margin
RUNS = (
    ("c8_dup12", "centred", "own", 2, True, False),
    ("c8_dup12", "late", "own", 2, True, False),
    ("c8_dup12", "wide", "random", 1, False, False),
    ("c8_dup12", "centred", "zero", 2, False, False),
    ("c2_ap150", "centred", "own", 2, True, False),
    ("c2_ap150", "late", "random", 1, False, False),
    ("c3_lin64", "wide", "own", 2, True, True),
    ("c3_lin64", "late", "random", 2, False, False),
    ("c4_qphs21", "centred", "own", 2, True, False),
    ("c4_qphs21", "late", "random", 1, False, False),
    ("c6_qp25", "centred", "own", 2, True, False),
    ("c6_qp25", "late", "zero", 2, True, False),
    ("c1_ap24d", "wide", "own", 2, True, False),
    ("c1_ap24d", "centred", "random", 1, False, False),
    ("n512_ap", "centred", "own", 2, True, False),
    ("n512_qphs", "late", "own", 2, True, False),
)
SWEEPS = (0, 1, 3, 8)
_PROGRAMS, _OPS = {}, {}


def run_id(run):
    return "%s-%s-%s-nv%d%s" % (run[0], run[1], run[2], run[3], "-wbz" if run[4] else "")


def program_of(name):
    if name not in _PROGRAMS:
        d = designs()[name]
        _PROGRAMS[name] = L.program(*d["job"], grid_m=d["grid_m"])
    return _PROGRAMS[name]


def make_opts_of(name, **kw):
    import mbfir
    d = designs()[name]
    if d.get("dense"):
        kw["dense_trig"] = 1
    if d["ddkkt"]:
        kw["ddkkt"] = d["ddkkt"]
    return mbfir.make_opts(grid_m=d["grid_m"], **kw)


def run_inputs(run, seed=0):
    """(P, I): the iterate (s, z), x, tau, kappa and the right-hand sides of one run (deterministic).  The signs of h'z and c'x are
    the run's: x and z are drawn so that both come out on either side of zero among the runs, with a margin."""
    import zlib
    P = program_of(run[0])
    rng = np.random.default_rng(zlib.crc32(run_id(run).encode()) + seed)
    s, z = CR.iterate(P, run[1], rng)
    N, R, nv = P["N"], P["R"], run[3]
    x = rng.standard_normal(N)
    # c'x on the side the run asks for (centred / wide: negative, late: positive), well away from zero
    cx_sign = 1.0 if run[1] == "late" else -1.0
    c = P["c"]
    if np.any(c != 0):
        x = x + (cx_sign * (0.5 * np.abs(c) @ np.abs(x)) - c @ x) * c / (c @ c)
    if run[5]:
        h, l = P["h"], P["l"]
        neg = np.nonzero(h[:l] < 0)[0]
        pos, ng = float(h @ z - h[neg] @ z[neg]), float(h[neg] @ z[neg])
        f = 3.0 * pos / -ng
        z[neg], s[neg] = z[neg] * f, s[neg] / f
    I = dict(s=s, z=z, x=x, tau=float(rng.uniform(0.5, 2)), kappa=float(rng.uniform(0.1, 1)))
    if run[2] != "own":
        scale = 10.0 ** rng.uniform(-2, 2, (nv, 1))
        I["bx"] = rng.standard_normal((nv, N)) * scale
        I["bz"] = rng.standard_normal((nv, R)) * scale
        if run[2] == "zero":
            I["bx"][1], I["bz"][1] = 0.0, 0.0
    return P, I


def ops_of(run, I):
    """the operators of a run's design at its iterate (G once per design)."""
    name = run[0]
    P = program_of(name)
    if name not in _OPS:
        _OPS[name] = Ops(P, I["s"], I["z"], dense=bool(designs()[name].get("dense")))
    return _OPS[name].rescale(I["s"], I["z"])
