// What the batched Cayley-Klein simulators (slr.hip: k_abr_batch, k_abr2_batch), their adjoints (simgrad.hip, simgradg.hip), their
// tangents (simjvp.hip) and their least-squares products (simgn.hip) share: the step of the forward model, the helpers and the steps of its
// derivatives, the adjoint's reduction constants and fold, the per-pulse descriptors, and the host staging of one call.  Moved
// here from slr.hip, simgrad.hip and simjvp.hip token for token.  Further down: what the Bloch simulator with relaxation
// (k_bloch_batch) shares with its adjoint (blochgrad.hip).
#pragma once
#include "dev_common.h"
#include "pulse.h"
#include <algorithm>
#include <cstring>
#include <optional>

namespace mbfir {

// Forward simulation of an RF pulse over off-resonance: Cayley-Klein parameters per position.
//   mode 0: rf_tools/abrm.m:40-57 -- one rotation about (Re rf, Im rf, x g_m) per sample
//   mode 1: the hard-pulse model the inverse SLR transform inverts exactly -- free precession by x g_m on beta, then
//           the hard pulse of the sample
// abr_step is one sample of either model for one position (r: the rf sample, om: the precession angle of the sample; mode is
// uniform over the workgroup).  k_abr_batch (om = x g) and k_abr2_batch (om = x gx + y gy) step through it.  The state goes in and
// comes back by value: through references the kernels compile to other fused products (the compiler then promotes a and b to
// registers only after inlining, in another order), and the results differ from before in the last bits.
struct CayleyKlein {
    double2 a, b;
};
// What a step computes from r and om alone: cs = cos(ph / 2) with ph = phi (mode 0) or |r| (mode 1), inv = sin(ph / 2) / ph (0 at
// ph = 0), and sz, cz = sincos(-om) in mode 1.  The tangent kernels (simjvp.hip) take it from the step (KEEP) so that a sample's
// trigonometry is computed once; abr_step drops it, and compiles to what it compiled to before the body moved here.
struct AbrTrig {
    double cs, ph, inv, sz, cz;
};
template <bool KEEP>
__device__ __forceinline__ CayleyKlein abr_step_trig(int mode, double2 r, double om, double2 a, double2 b, AbrTrig& t) {
    double2 av, bv;                              // step: a' = av a - conj(bv) b ; b' = bv a + conj(av) b
    if (mode == 0) {
        const double phi = sqrt(r.x * r.x + r.y * r.y + om * om);
        double sn, cs;
        sincos(0.5 * phi, &sn, &cs);
        const double inv = phi > 0 ? sn / phi : 0.0;
        av = make_double2(cs, -om * inv);
        bv = make_double2(r.y * inv, -r.x * inv);                  // -i (n1 + i n2) sin
        const double2 an = make_double2(av.x * a.x - av.y * a.y - (bv.x * b.x + bv.y * b.y),
                                        av.x * a.y + av.y * a.x - (bv.x * b.y - bv.y * b.x));
        const double2 bn = make_double2(bv.x * a.x - bv.y * a.y + (av.x * b.x + av.y * b.y),
                                        bv.x * a.y + bv.y * a.x + (av.x * b.y - av.y * b.x));
        a = an; b = bn;
        if (KEEP) t = AbrTrig{cs, phi, inv, 0.0, 1.0};
    } else {
        const double th = hypot(r.x, r.y);
        double sn, cs, sz, cz;
        sincos(0.5 * th, &sn, &cs);
        sincos(-om, &sz, &cz);                                   // z^-1
        const double2 zb = make_double2(cz * b.x - sz * b.y, cz * b.y + sz * b.x);
        const double inv = th > 0 ? sn / th : 0.0;
        const double2 S = make_double2(-r.y * inv, r.x * inv);    // i e^{i arg rf} sin(th/2)
        const double2 an = make_double2(cs * a.x - (S.x * zb.x + S.y * zb.y), cs * a.y - (S.x * zb.y - S.y * zb.x));
        const double2 bn = make_double2(S.x * a.x - S.y * a.y + cs * zb.x, S.x * a.y + S.y * a.x + cs * zb.y);
        a = an; b = bn;
        if (KEEP) t = AbrTrig{cs, th, inv, sz, cz};
    }
    return CayleyKlein{a, b};
}
__device__ __forceinline__ CayleyKlein abr_step(int mode, double2 r, double om, double2 a, double2 b) {
    AbrTrig t;
    return abr_step_trig<false>(mode, r, om, a, b, t);
}

// Complex helpers of the derivative kernels (simgrad.hip, simjvp.hip).
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {        // a b
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cjmul(double2 a, double2 b) {       // conj(a) b
    return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ double redot(double2 a, double2 b) {        // Re(conj(a) b)
    return a.x * b.x + a.y * b.y;
}

// inv = sin(phi / 2) / phi and D = (d inv / d phi) / phi = (cos(phi / 2) / 2 - inv) / phi^2 from sn, cs = sincos(phi / 2).  Below
// 1e-4 the difference cancels and D is its series -1/24 + phi^2 / 960; phi = 0 (a zero rf sample at om = 0) gives the limits 1/2
// and -1/24.  d inv / dp = D p for p = Re r, Im r.  half_sinc_d: D from an inv that is already there.
__device__ __forceinline__ double half_sinc_d(double phi, double cs, double inv) {
    return phi < 1e-4 ? -1.0 / 24.0 + phi * phi * (1.0 / 960.0) : (0.5 * cs - inv) / (phi * phi);
}
__device__ __forceinline__ void half_sinc(double phi, double sn, double cs, double& inv, double& D) {
    inv = phi > 0 ? sn / phi : 0.5;
    D = half_sinc_d(phi, cs, inv);
}

// One sample backwards (cmul, cjmul, redot and half_sinc: sim_dev.h) for one point: (a, b) = psi_m -> psi_{m-1}, (la, lb) = lambda_m -> lambda_{m-1}; returns the sample's
// contribution (dL / d Re r, dL / d Im r).  With u, v the state before the sample and X = conj(la) v, Y = conj(lb) u:
//   mode 0: alpha = cs - i om inv, beta = -i r inv;  d alpha / dp = p kappa, kappa = -inv / 2 - i om D;
//           d beta / dp = D p (-i r) + inv e_p, e = (-i, 1)   ->   g = r C + inv (Im(X + Y), Re(Y - X))
//   mode 1: w = z^-1 v, S = i r inv;  d cs / dp = -p inv / 2;  dS / dp = D p (i r) + inv f_p, f = (i, -1)
//                                                          ->   g = r C + inv (-Im(X + Y), Re(X - Y)), X = conj(la) w
// where C = Re <lambda, (the part of dQ proportional to p) psi_{m-1}>.  i r inv is smooth at r = 0, where arg r is not.
__device__ __forceinline__ double2 abr_vjp_step(int mode, double2 r, double om, double2& a, double2& b, double2& la, double2& lb) {
    double sn, cs, inv, D;
    if (mode == 0) {
        const double phi = sqrt(r.x * r.x + r.y * r.y + om * om);
        sincos(0.5 * phi, &sn, &cs);
        half_sinc(phi, sn, cs, inv, D);
        const double2 al = make_double2(cs, -om * inv), be = make_double2(r.y * inv, -r.x * inv);
        const double2 bh = make_double2(r.y, -r.x), ka = make_double2(-0.5 * inv, -om * D);
        const double2 ta = cjmul(al, a), tb = cjmul(be, b), tc = cmul(al, b), td = cmul(be, a);
        const double2 u = make_double2(ta.x + tb.x, ta.y + tb.y), v = make_double2(tc.x - td.x, tc.y - td.y);
        const double2 p1 = cmul(ka, u), p2 = cjmul(bh, v), p3 = cmul(bh, u), p4 = cjmul(ka, v);
        const double2 t1 = make_double2(p1.x - D * p2.x, p1.y - D * p2.y), t2 = make_double2(D * p3.x + p4.x, D * p3.y + p4.y);
        const double C = redot(la, t1) + redot(lb, t2);
        const double2 X = cjmul(la, v), Y = cjmul(lb, u);
        const double2 g = make_double2(r.x * C + inv * (X.y + Y.y), r.y * C + inv * (Y.x - X.x));
        const double2 la1 = cjmul(al, la), la2 = cjmul(be, lb), lb1 = cmul(al, lb), lb2 = cmul(be, la);
        la = make_double2(la1.x + la2.x, la1.y + la2.y);
        lb = make_double2(lb1.x - lb2.x, lb1.y - lb2.y);
        a = u; b = v;
        return g;
    }
    const double th = hypot(r.x, r.y);
    double sz, cz;
    sincos(0.5 * th, &sn, &cs);
    sincos(-om, &sz, &cz);                                         // z^-1 = cz + i sz
    half_sinc(th, sn, cs, inv, D);
    const double2 S = make_double2(-r.y * inv, r.x * inv), sh = make_double2(-r.y, r.x), zi = make_double2(cz, sz);
    const double2 ta = cjmul(S, b), tb = cmul(S, a);
    const double2 u = make_double2(cs * a.x + ta.x, cs * a.y + ta.y), w = make_double2(cs * b.x - tb.x, cs * b.y - tb.y);
    const double2 p2 = cjmul(sh, w), p3 = cmul(sh, u);
    const double2 t1 = make_double2(-0.5 * inv * u.x - D * p2.x, -0.5 * inv * u.y - D * p2.y);
    const double2 t2 = make_double2(D * p3.x - 0.5 * inv * w.x, D * p3.y - 0.5 * inv * w.y);
    const double C = redot(la, t1) + redot(lb, t2);
    const double2 X = cjmul(la, w), Y = cjmul(lb, u);
    const double2 g = make_double2(r.x * C - inv * (X.y + Y.y), r.y * C + inv * (X.x - Y.x));
    const double2 l1 = cjmul(S, lb), l2 = cmul(S, la);
    const double2 lw = make_double2(cs * lb.x - l2.x, cs * lb.y - l2.y);
    la = make_double2(cs * la.x + l1.x, cs * la.y + l1.y);
    lb = cjmul(zi, lw);                                            // conj(z^-1) = z
    a = u; b = cjmul(zi, w);
    return g;
}

// Reduction tile: VJP_T samples x (Re, Im) rows of 256 contributions.  A row is padded to 272 doubles, so that two consecutive
// rows start 32 banks apart: the 32 lanes of an 8-byte read group (two rows x 16 lanes, below) then touch 64 distinct banks.
constexpr int VJP_T = 8;
constexpr int VJP_ROW = 256 + 16;

// Per-pulse descriptor of the partials: part holds nscale x nch rows of n double2 from p_off, row (scale, chunk) at
// (scale nch + chunk) n; the gradient of the pulse goes to r_off.
struct VjpPulseDev {
    long r_off, p_off;
    int n, nch;
};

// sum_s scales[s] (sum_c part(s, c, m)) of sample m of one pulse, chunks then scales in index order: the body of k_abr_vjp_fold
// (simgrad.hip), shared with the fold of the least-squares products (simgn.hip).
__device__ __forceinline__ double2 abr_vjp_fold_sum(const double2* __restrict__ part, const VjpPulseDev& V,
                                                    const double* __restrict__ scales, int nscale, int m) {
    double2 g = make_double2(0, 0);
    for (int s = 0; s < nscale; ++s) {
        double2 t = make_double2(0, 0);
        const double2* row = part + V.p_off + (long)s * V.nch * V.n + m;
        for (int c = 0; c < V.nch; ++c) {
            const double2 v = row[(long)c * V.n];
            t.x += v.x; t.y += v.y;
        }
        const double sc = scales[s];
        g.x += sc * t.x; g.y += sc * t.y;
    }
    return g;
}

// abr_vjp_step plus the sample's contribution dom = dL / d om to the gradient waveform's adjoint (simgradg.hip).  Q_m
// depends on om through
//   mode 0: d alpha / d om = dal = -om inv / 2 - i (inv + om^2 D),  d beta / d om = dbe = D om (-i r)
//           dom = Re( conj(la) (dal u - conj(dbe) v) + conj(lb) (dbe u + conj(dal) v) );  phi = 0 gives dal = -i / 2
//   mode 1: only z^-1 = exp(-i om): dw / d om = -i w   ->   dom = Re( conj(la) (i conj(S) w) + conj(lb) (-i cs w) )
// with u, v (w) the state before the sample and la, lb the multipliers after it, all of which the rf step already forms; no
// further sincos.  The rf pair is abr_vjp_step's arithmetic restated.
__device__ __forceinline__ double2 abr_vjp_step_g(int mode, double2 r, double om, double2& a, double2& b, double2& la, double2& lb,
                                                  double& dom) {
    double sn, cs, inv, D;
    if (mode == 0) {
        const double phi = sqrt(r.x * r.x + r.y * r.y + om * om);
        sincos(0.5 * phi, &sn, &cs);
        half_sinc(phi, sn, cs, inv, D);
        const double2 al = make_double2(cs, -om * inv), be = make_double2(r.y * inv, -r.x * inv);
        const double2 bh = make_double2(r.y, -r.x), ka = make_double2(-0.5 * inv, -om * D);
        const double2 ta = cjmul(al, a), tb = cjmul(be, b), tc = cmul(al, b), td = cmul(be, a);
        const double2 u = make_double2(ta.x + tb.x, ta.y + tb.y), v = make_double2(tc.x - td.x, tc.y - td.y);
        const double2 p1 = cmul(ka, u), p2 = cjmul(bh, v), p3 = cmul(bh, u), p4 = cjmul(ka, v);
        const double2 t1 = make_double2(p1.x - D * p2.x, p1.y - D * p2.y), t2 = make_double2(D * p3.x + p4.x, D * p3.y + p4.y);
        const double C = redot(la, t1) + redot(lb, t2);
        const double2 X = cjmul(la, v), Y = cjmul(lb, u);
        const double2 g = make_double2(r.x * C + inv * (X.y + Y.y), r.y * C + inv * (Y.x - X.x));
        const double Do = D * om;                                  // dbe = Do bh: p2 and p3 serve again
        const double2 dal = make_double2(-0.5 * om * inv, -(inv + om * Do));
        const double2 q1 = cmul(dal, u), q4 = cjmul(dal, v);
        const double2 s1 = make_double2(q1.x - Do * p2.x, q1.y - Do * p2.y), s2 = make_double2(Do * p3.x + q4.x, Do * p3.y + q4.y);
        dom = redot(la, s1) + redot(lb, s2);
        const double2 la1 = cjmul(al, la), la2 = cjmul(be, lb), lb1 = cmul(al, lb), lb2 = cmul(be, la);
        la = make_double2(la1.x + la2.x, la1.y + la2.y);
        lb = make_double2(lb1.x - lb2.x, lb1.y - lb2.y);
        a = u; b = v;
        return g;
    }
    const double th = hypot(r.x, r.y);
    double sz, cz;
    sincos(0.5 * th, &sn, &cs);
    sincos(-om, &sz, &cz);                                         // z^-1 = cz + i sz
    half_sinc(th, sn, cs, inv, D);
    const double2 S = make_double2(-r.y * inv, r.x * inv), sh = make_double2(-r.y, r.x), zi = make_double2(cz, sz);
    const double2 ta = cjmul(S, b), tb = cmul(S, a);
    const double2 u = make_double2(cs * a.x + ta.x, cs * a.y + ta.y), w = make_double2(cs * b.x - tb.x, cs * b.y - tb.y);
    const double2 p2 = cjmul(sh, w), p3 = cmul(sh, u);
    const double2 t1 = make_double2(-0.5 * inv * u.x - D * p2.x, -0.5 * inv * u.y - D * p2.y);
    const double2 t2 = make_double2(D * p3.x - 0.5 * inv * w.x, D * p3.y - 0.5 * inv * w.y);
    const double C = redot(la, t1) + redot(lb, t2);
    const double2 X = cjmul(la, w), Y = cjmul(lb, u);
    const double2 g = make_double2(r.x * C - inv * (X.y + Y.y), r.y * C + inv * (X.x - Y.x));
    const double2 sw = cjmul(S, w);                                // i conj(S) w = (-sw.y, sw.x);  -i cs w = cs (w.y, -w.x)
    dom = la.y * sw.x - la.x * sw.y + cs * (lb.x * w.y - lb.y * w.x);
    const double2 l1 = cjmul(S, lb), l2 = cmul(S, la);
    const double2 lw = make_double2(cs * lb.x - l2.x, cs * lb.y - l2.y);
    la = make_double2(cs * la.x + l1.x, cs * la.y + l1.y);
    lb = cjmul(zi, lw);                                            // conj(z^-1) = z
    a = u; b = cjmul(zi, w);
    return g;
}

// The reduction tile of the rf and g adjoint (simgradg.hip): VJG_T samples x four rows (Re, Im of the rf pair, x dom, y dom) of
// VJP_ROW doubles: 16 rows like the rf adjoint's tile, so the same LDS and the same 16-lanes-per-row pass.
constexpr int VJG_T = 4;

// Directions per workgroup: the largest of 1, 2, 4, 8 without scratch at no less than the forward kernels' occupancy minus one wave
// per SIMD (DESIGN 8l has the table).
#ifndef JVP_K
#define JVP_K 1
#endif

// One sample for the kcnt <= JVP_K tangents of one point: t = what abr_step_trig kept of the sample, (a, b) = psi_{m-1},
// dr[k * 256] = s v_m of direction k (the LDS tile), (da[k], db[k]) = dpsi_{m-1} -> dpsi_m.  dQ[dr] is real-linear in dr and splits, as in the adjoint (simgrad.hip), into a part
// proportional to rd = Re r Re dr + Im r Im dr, whose action on psi_{m-1} (T1, T2) every direction shares, and a part proportional
// to inv:
//   mode 0: d alpha = rd kappa, kappa = -inv / 2 - i om D;  d beta = D rd (-i r) + inv (-i dr)
//           da' = alpha da - conj(beta) db + rd T1 - conj(e) b,  db' = beta da + conj(alpha) db + rd T2 + e a,  e = inv (-i dr)
//   mode 1: z^-1 = cz + i sz, w = z^-1 b, dw = z^-1 db;  d cs = -rd inv / 2;  dS = D rd (i r) + inv (i dr)
//           da' = cs da - conj(S) dw + rd T1 - conj(f) w,  db' = S da + cs dw + rd T2 + f a,  f = inv (i dr)
__device__ __forceinline__ void abr_jvp_step(int mode, double2 r, double om, const AbrTrig& t, double2 a, double2 b,
                                             const double2* dr, int kcnt, double2 (&da)[JVP_K], double2 (&db)[JVP_K]) {
    const double cs = t.cs, inv = t.ph > 0 ? t.inv : 0.5, D = half_sinc_d(t.ph, cs, inv);      // half_sinc on the step's own quotient
    if (mode == 0) {
        const double2 al = make_double2(cs, -om * inv), be = make_double2(r.y * inv, -r.x * inv);
        const double2 bh = make_double2(r.y, -r.x), ka = make_double2(-0.5 * inv, -om * D);
        const double2 p1 = cmul(ka, a), p2 = cjmul(bh, b), p3 = cmul(bh, a), p4 = cjmul(ka, b);
        const double2 T1 = make_double2(p1.x - D * p2.x, p1.y - D * p2.y), T2 = make_double2(D * p3.x + p4.x, D * p3.y + p4.y);
#pragma unroll
        for (int k = 0; k < JVP_K; ++k) {
            if (k < kcnt) {
                const double2 d = dr[k * 256];
                const double rd = r.x * d.x + r.y * d.y;
                const double2 e = make_double2(inv * d.y, -(inv * d.x));
                const double2 q1 = cmul(al, da[k]), q2 = cjmul(be, db[k]), q3 = cmul(be, da[k]), q4 = cjmul(al, db[k]);
                const double2 q5 = cjmul(e, b), q6 = cmul(e, a);
                da[k] = make_double2(q1.x - q2.x + (rd * T1.x - q5.x), q1.y - q2.y + (rd * T1.y - q5.y));
                db[k] = make_double2(q3.x + q4.x + (rd * T2.x + q6.x), q3.y + q4.y + (rd * T2.y + q6.y));
            }
        }
        return;
    }
    const double2 S = make_double2(-r.y * inv, r.x * inv), sh = make_double2(-r.y, r.x), zi = make_double2(t.cz, t.sz);
    const double2 w = cmul(zi, b);
    const double2 p2 = cjmul(sh, w), p3 = cmul(sh, a);
    const double2 T1 = make_double2(-0.5 * inv * a.x - D * p2.x, -0.5 * inv * a.y - D * p2.y);
    const double2 T2 = make_double2(D * p3.x - 0.5 * inv * w.x, D * p3.y - 0.5 * inv * w.y);
#pragma unroll
    for (int k = 0; k < JVP_K; ++k) {
        if (k < kcnt) {
            const double2 d = dr[k * 256];
            const double rd = r.x * d.x + r.y * d.y;
            const double2 f = make_double2(-(inv * d.y), inv * d.x);
            const double2 dw = cmul(zi, db[k]);
            const double2 q2 = cjmul(S, dw), q3 = cmul(S, da[k]), q5 = cjmul(f, w), q6 = cmul(f, a);
            const double2 dak = make_double2(cs * da[k].x - q2.x + (rd * T1.x - q5.x), cs * da[k].y - q2.y + (rd * T1.y - q5.y));
            db[k] = make_double2(q3.x + cs * dw.x + (rd * T2.x + q6.x), q3.y + cs * dw.y + (rd * T2.y + q6.y));
            da[k] = dak;
        }
    }
}

// Per-pulse descriptors of the 1D and the 2D simulators (and of their adjoints, whose cotangents lie where the outputs do).
struct AbrPulseDev {
    long r_off, x_off, o_off;     // first rf / g sample, first position, first output entry
    int n, nx;
};
struct Abr2PulseDev {
    long r_off, x_off, y_off, o_off;     // first rf / gx / gy sample, first x, first y, first output entry
    int n, nx, ny, pad;
};

// One call of a batched simulator.  The caller adds its own sections, then add_tables; fills its sections (at<T>: add moves
// the buffer, so take pointers after the last add); uploads; launches nblk workgroups on the dev<T> addresses; downloads.
struct Staging {
    std::vector<char> h;                                  // host sections, each 256-byte aligned, uploaded with one copy
    std::optional<DevBuf> buf;                            // the sections, then the output region
    size_t o_sc = 0, o_pd = 0, o_bk = 0, o_out = 0;       // scales, per-pulse descriptors, block table; output region
    long nblk = 0;
    size_t add(size_t bytes) {
        const size_t o = (h.size() + 255) & ~size_t(255);
        h.resize(o + bytes);
        return o;
    }
    template <class T> T* at(size_t o) { return reinterpret_cast<T*>(h.data() + o); }
    template <class T> T* dev(size_t o) { return reinterpret_cast<T*>(buf->as<char>() + o); }
    // The sections every simulator has, filled: pd = npulse descriptors of pd_size bytes; ntime / npoint as sim_block_table.
    void add_tables(int npulse, const void* pd, size_t pd_size, const int* ntime, const long* npoint, int nscale,
                    const double* scales) {
        nblk = sim_block_table(npulse, ntime, npoint, nscale, nullptr);
        o_sc = add((size_t)nscale * 8);
        o_pd = add(npulse * pd_size);
        o_bk = add(nblk * sizeof(SimBlock));
        std::copy(scales, scales + nscale, at<double>(o_sc));
        std::memcpy(at<char>(o_pd), pd, npulse * pd_size);
        sim_block_table(npulse, ntime, npoint, nscale, at<SimBlock>(o_bk));
    }
    void upload(size_t out_bytes, hipStream_t st) {
        const size_t up = h.size();
        o_out = (up + 255) & ~size_t(255);
        buf.emplace(o_out + out_bytes);
        MBFIR_HIP(hipMemcpyAsync(buf->p, h.data(), up, hipMemcpyHostToDevice, st));
    }
    void download(void* out, size_t out_bytes, hipStream_t st) {     // after the launch
        MBFIR_HIP(hipGetLastError());
        MBFIR_HIP(hipMemcpyAsync(out, dev<char>(o_out), out_bytes, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipStreamSynchronize(st));
        MBFIR_HIP(hipGetLastError());
    }
};

// The block table of the tangent calls (simjvp.hip, blochjvp.hip) as a new section of S, after add_tables: the forward table with
// every entry repeated once per direction group, the group number in SimBlock::pad.  Returns the section's offset.
inline size_t sim_group_table(Staging& S, int ngrp) {
    const size_t o_jb = S.add(S.nblk * ngrp * sizeof(SimBlock));
    const SimBlock* fb = S.at<SimBlock>(S.o_bk);
    SimBlock* jb = S.at<SimBlock>(o_jb);
    for (long w = 0; w < S.nblk; ++w)
        for (int q = 0; q < ngrp; ++q) *jb++ = SimBlock{fb[w].pulse, fb[w].scale, fb[w].chunk, q};
    return o_jb;
}

// The inputs of one mbfir_abr_batch / mbfir_abr2_batch call, staged and filled (slr.hip): rf interleaved, the gradient weights with
// their defaults written out (a null g or gx is 2 pi / n per sample, a null gy is 0), the grids, and Staging's tables.  The forward
// calls upload this as it is; the adjoints add their own sections first.  ntime / npoint: per pulse, as sim_block_table takes them;
// O: output entries of a (and of b), scale-major per pulse.
struct AbrStaged {
    Staging S;
    size_t o_rf = 0, o_g = 0, o_x = 0;
    std::vector<int> ntime;
    std::vector<long> npoint;
    long O = 0;
};
void abr_stage(AbrStaged& A, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g, int nxgrid,
               const long* xoff, const double* x, int nscale, const double* scales);
struct Abr2Staged {
    Staging S;
    size_t o_rf = 0, o_gx = 0, o_gy = 0, o_x = 0, o_y = 0;
    std::vector<int> ntime;
    std::vector<long> npoint;
    long O = 0;
};
void abr2_stage(Abr2Staged& A, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff, const double* y,
                int nscale, const double* scales);

// What the Bloch simulator with relaxation (slr.hip k_bloch_batch), its adjoint (blochgrad.hip) and its tangent (blochjvp.hip)
// share, moved here from slr.hip token for token: the rotation of one sample (bloch_simulation/blochC.c calcrotmat :171-236), the staged row, the per-pulse
// descriptor, and the host staging of one call.
struct Rot3 {
    double m[9];           // column-major like the reference: m[i + 3 j]
};
// What a rotation computes from its angle alone: phi, sn, cp = sincos(phi / 2).  The tangent kernel (blochjvp.hip) takes it from
// the rotation (KEEP) so that a sample's trigonometry is computed once; bloch_rotmat drops it, and compiles to what it compiled to
// before the body became a template.
struct BlochTrig {
    double phi, sn, cp;
};
template <bool KEEP>
__device__ __forceinline__ void bloch_rotmat_trig(double nx, double ny, double nz, Rot3& R, BlochTrig& t) {
    const double phi = sqrt(nx * nx + ny * ny + nz * nz);
    if (phi == 0.0) {
        R.m[0] = 1; R.m[1] = 0; R.m[2] = 0; R.m[3] = 0; R.m[4] = 1; R.m[5] = 0; R.m[6] = 0; R.m[7] = 0; R.m[8] = 1;
        if (KEEP) t = BlochTrig{0.0, 0.0, 1.0};
        return;
    }
    double sn, cp;
    sincos(0.5 * phi, &sn, &cp);
    if (KEEP) t = BlochTrig{phi, sn, cp};
    const double sp = sn / phi;
    const double ar = cp, ai = -nz * sp, br = ny * sp, bi = -nx * sp;
    R.m[0] = ar * ar - ai * ai - br * br + bi * bi;
    R.m[1] = -2 * ar * ai - 2 * br * bi;
    R.m[2] = -2 * ar * br + 2 * ai * bi;
    R.m[3] = 2 * ar * ai - 2 * br * bi;
    R.m[4] = ar * ar - ai * ai + br * br - bi * bi;
    R.m[5] = -2 * ai * br - 2 * ar * bi;
    R.m[6] = 2 * ar * br + 2 * ai * bi;
    R.m[7] = 2 * ar * bi - 2 * ai * br;
    R.m[8] = ar * ar + ai * ai - br * br - bi * bi;
}
__device__ __forceinline__ void bloch_rotmat(double nx, double ny, double nz, Rot3& R) {
    BlochTrig t;
    bloch_rotmat_trig<false>(nx, ny, nz, R, t);
}
__device__ __forceinline__ void rot_vec(const Rot3& R, const double v[3], double o[3]) {
    o[0] = R.m[0] * v[0] + R.m[3] * v[1] + R.m[6] * v[2];
    o[1] = R.m[1] * v[0] + R.m[4] * v[1] + R.m[7] * v[2];
    o[2] = R.m[2] * v[0] + R.m[5] * v[1] + R.m[8] * v[2];
}
constexpr int BLOCH_CH = 256;
// in[t] = (b1 re, b1 im, gx, gy, gz (each * gamma * dt), dt * TWOPI, e1, e2, dt) per sample of every pulse (k_bloch_batch says how
// a workgroup turns it into its LDS rows).
constexpr int BLOCH_IN = 9;
struct BlochPulseDev {
    long t_off, f_off, p_off;     // first sample, first frequency, first position (3 doubles each)
    long m_off, o_off;            // first m0 block, first output entry
    int ntime, nf, npos, pad;
    double gamma;
};

// What the adjoint (blochgrad.hip), the tangent (blochjvp.hip) and the least-squares products (blochgn.hip) share, moved here from
// blochgrad.hip and blochjvp.hip token for token.
// One forward sample for one point, k_bloch_batch's arithmetic: s = the sample's LDS row, (px, py, pz, dfv) = the point.
__device__ __forceinline__ double bloch_rotz(const double* s, double px, double py, double pz, double dfv) {
    return -((s[2] * px + s[3] * py + s[4] * pz) + dfv * s[5]);
}
__device__ __forceinline__ void bloch_fwd_step(const double* s, double rotz, double m[3]) {
    Rot3 R;
    bloch_rotmat(s[0], s[1], rotz, R);
    const double e1 = s[6], e2 = s[7];
    double o[3];
    rot_vec(R, m, o);
    m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = e1 * o[2] + (1 - e1);
}

// One sample backwards for one point: mp = m_{t-1}, l = lambda_t -> lambda_{t-1}; returns (dL / d rotx, dL / d roty) of the sample.
// R is quadratic in the Cayley-Klein parameters (ar, ai, br, bi) = (cos(phi/2), -nz sp, ny sp, -nx sp), sp = sin(phi/2) / phi.
// With T = (D l) mp' and G_k = sum_ij T_ij dR_ij / dk for k = ar, ai, br, bi, and d ar / dp = -(sp / 2) p, d sp / dp = D p
// (half_sinc, sim_dev.h: the series below phi = 1e-4, the limits 1/2 and -1/24 at phi = 0):
//     dL / d nx = nx C - sp G_bi,  dL / d ny = ny C + sp G_br,  C = -(sp / 2) G_ar + D (-nz G_ai + ny G_br - nx G_bi)
// At phi = 0 this is the generator: (ar, ai, br, bi) = (1, 0, 0, 0), and the rotation below is the identity, as the forward step's.
__device__ __forceinline__ double2 bloch_vjp_step(const double* s, double nz, const double mp[3], double l[3]) {
    const double nx = s[0], ny = s[1], e1 = s[6], e2 = s[7];
    const double phi = sqrt(nx * nx + ny * ny + nz * nz);
    double sn, cp, sp, D;
    sincos(0.5 * phi, &sn, &cp);
    half_sinc(phi, sn, cp, sp, D);
    const double ar = cp, ai = -nz * sp, br = ny * sp, bi = -nx * sp;
    const double d0 = e2 * l[0], d1 = e2 * l[1], d2 = e1 * l[2];
    const double T00 = d0 * mp[0], T01 = d0 * mp[1], T02 = d0 * mp[2];
    const double T10 = d1 * mp[0], T11 = d1 * mp[1], T12 = d1 * mp[2];
    const double T20 = d2 * mp[0], T21 = d2 * mp[1], T22 = d2 * mp[2];
    const double a01 = T01 - T10, a02 = T02 - T20, a12 = T12 - T21;          // antisymmetric and symmetric parts
    const double s01 = T01 + T10, s02 = T02 + T20, s12 = T12 + T21;
    const double Gar = 2 * (ar * (T00 + T11 + T22) + ai * a01 + br * a02 + bi * a12);
    const double Gai = 2 * (ai * (T22 - T00 - T11) + ar * a01 + bi * s02 - br * s12);
    const double Gbr = 2 * (br * (T11 - T00 - T22) - bi * s01 + ar * a02 - ai * s12);
    const double Gbi = 2 * (bi * (T00 - T11 - T22) - br * s01 + ai * s02 + ar * a12);
    const double C = -0.5 * sp * Gar + D * (ny * Gbr - nz * Gai - nx * Gbi);
    const double2 g = make_double2(nx * C - sp * Gbi, ny * C + sp * Gbr);
    // lambda_{t-1} = R' (D l): R' is R's transpose, entry (i, j) of R at m[i + 3 j] in bloch_rotmat
    const double r00 = ar * ar - ai * ai - br * br + bi * bi, r10 = -2 * ar * ai - 2 * br * bi, r20 = -2 * ar * br + 2 * ai * bi;
    const double r01 = 2 * ar * ai - 2 * br * bi, r11 = ar * ar - ai * ai + br * br - bi * bi, r21 = -2 * ai * br - 2 * ar * bi;
    const double r02 = 2 * ar * br + 2 * ai * bi, r12 = 2 * ar * bi - 2 * ai * br, r22 = ar * ar + ai * ai - br * br - bi * bi;
    l[0] = r00 * d0 + r10 * d1 + r20 * d2;
    l[1] = r01 * d0 + r11 * d1 + r21 * d2;
    l[2] = r02 * d0 + r12 * d1 + r22 * d2;
    return g;
}

// bloch_vjp_step plus the sample's dL / d rotz, the third member of the pair above (blochgradg.hip): ai = -nz sp, so
//     dL / d nz = nz C - sp G_ai
// with C, sp and G_ai as the rf pair forms them; no further sincos.  At phi = 0 it is the generator T_10 - T_01.  The rf pair and
// the multiplier are bloch_vjp_step's arithmetic restated.  Returns (dL / d rotx, dL / d roty, dL / d rotz).
__device__ __forceinline__ double3 bloch_vjp_step_z(const double* s, double nz, const double mp[3], double l[3]) {
    const double nx = s[0], ny = s[1], e1 = s[6], e2 = s[7];
    const double phi = sqrt(nx * nx + ny * ny + nz * nz);
    double sn, cp, sp, D;
    sincos(0.5 * phi, &sn, &cp);
    half_sinc(phi, sn, cp, sp, D);
    const double ar = cp, ai = -nz * sp, br = ny * sp, bi = -nx * sp;
    const double d0 = e2 * l[0], d1 = e2 * l[1], d2 = e1 * l[2];
    const double T00 = d0 * mp[0], T01 = d0 * mp[1], T02 = d0 * mp[2];
    const double T10 = d1 * mp[0], T11 = d1 * mp[1], T12 = d1 * mp[2];
    const double T20 = d2 * mp[0], T21 = d2 * mp[1], T22 = d2 * mp[2];
    const double a01 = T01 - T10, a02 = T02 - T20, a12 = T12 - T21;          // antisymmetric and symmetric parts
    const double s01 = T01 + T10, s02 = T02 + T20, s12 = T12 + T21;
    const double Gar = 2 * (ar * (T00 + T11 + T22) + ai * a01 + br * a02 + bi * a12);
    const double Gai = 2 * (ai * (T22 - T00 - T11) + ar * a01 + bi * s02 - br * s12);
    const double Gbr = 2 * (br * (T11 - T00 - T22) - bi * s01 + ar * a02 - ai * s12);
    const double Gbi = 2 * (bi * (T00 - T11 - T22) - br * s01 + ai * s02 + ar * a12);
    const double C = -0.5 * sp * Gar + D * (ny * Gbr - nz * Gai - nx * Gbi);
    const double3 g = make_double3(nx * C - sp * Gbi, ny * C + sp * Gbr, nz * C - sp * Gai);
    const double r00 = ar * ar - ai * ai - br * br + bi * bi, r10 = -2 * ar * ai - 2 * br * bi, r20 = -2 * ar * br + 2 * ai * bi;
    const double r01 = 2 * ar * ai - 2 * br * bi, r11 = ar * ar - ai * ai + br * br - bi * bi, r21 = -2 * ai * br - 2 * ar * bi;
    const double r02 = 2 * ar * br + 2 * ai * bi, r12 = 2 * ar * bi - 2 * ai * br, r22 = ar * ar + ai * ai - br * br - bi * bi;
    l[0] = r00 * d0 + r10 * d1 + r20 * d2;
    l[1] = r01 * d0 + r11 * d1 + r21 * d2;
    l[2] = r02 * d0 + r12 * d1 + r22 * d2;
    return g;
}

// The reduction tile of the b1 and gradient-waveform adjoint (blochgradg.hip): a group of VJP_T samples is walked in sub-groups of
// BGR_T samples x five rows (the rf pair, px dz, py dz, pz dz) of VJP_ROW doubles: 15 of the 16 rows of the rf adjoint's tile, so
// the same LDS and the same 16-lanes-per-row pass; the sixteenth row is summed and never stored.
constexpr int BGR_T = 3;
constexpr int BGR_ROWS = 5;

// Per-pulse descriptor of the checkpoints: workgroup (scale, chunk) of the pulse owns ng = ceil(n / VJP_T) groups of 3 x 256
// doubles from c_off + (scale nch + chunk) ng 768, component c of group k of thread tid at (3 k + c) 256 + tid.
struct BlochCkDev {
    long c_off;
    int ng, pad;
};
constexpr int BLOCH_CK = 3 * 256;

// Launches k_bloch_vjp_fold (blochgrad.hip) on nfold workgroups: the fold of the steady state's adjoint (blochss.hip) is the
// transient adjoint's.
void bloch_vjp_fold_launch(hipStream_t st, long nfold, const double2* part, const VjpPulseDev* vp, const SimBlock* blocks,
                           const double* scales, int nscale, const double* in, const BlochPulseDev* pulses, double2* grad);
// Launches k_bloch_vjp_gr_fold (blochgradg.hip) on nfold workgroups: the fold of the steady state's adjoint in b1 and gr
// (blochssg.hip) is the transient adjoint's.
void bloch_vjp_gr_fold_launch(hipStream_t st, long nfold, const double2* part, const double* gpart, long npart, const VjpPulseDev* vp,
                              const SimBlock* blocks, const double* scales, int nscale, const double* in,
                              const BlochPulseDev* pulses, double2* grad, double* gg, long T);

// What the directions of one point share at one sample.  R is quadratic in the Cayley-Klein parameters (ar, ai, br, bi) =
// (cos(phi/2), -nz sp, ny sp, -nx sp), sp = sin(phi/2) / phi, and along dn = (dnx, dny, 0), with d sp = D (n.dn) (half_sinc),
//     d ar = -(sp/2)(n.dn),  d ai = -nz D (n.dn),  d br = ny D (n.dn) + sp dny,  d bi = -nx D (n.dn) - sp dnx
// so that dR[dn] m = (n.dn) U + dnx Vx + dny Vy: U is the derivative of the quadratic form along (-(sp/2), -nz D, ny D, -nx D)
// applied to m, Vx the one along d bi = -sp, Vy the one along d br = sp.  At phi = 0 (ar, ai, br, bi) = (1, 0, 0, 0), sp = 1/2:
// Vx = (0, -mz, my), Vy = (mz, 0, -mx), the generators, and n.dn = 0.
struct BlochJvpShared {
    double U[3], Vx[3], Vy[3];
};
__device__ __forceinline__ void bloch_jvp_shared(double nx, double ny, double nz, const BlochTrig& t, const double m[3],
                                                 BlochJvpShared& W) {
    double sp, D;
    half_sinc(t.phi, t.sn, t.cp, sp, D);
    const double ar = t.cp, ai = -nz * sp, br = ny * sp, bi = -nx * sp;
    const double dar = -0.5 * sp, dai = -nz * D, dbr = ny * D, dbi = -nx * D;
    const double p0 = ar * dar, p1 = ai * dai, p2 = br * dbr, p3 = bi * dbi;
    const double aai = dar * ai + ar * dai, bb = dbr * bi + br * dbi, abr = dar * br + ar * dbr, abi = dar * bi + ar * dbi;
    const double ib = dai * bi + ai * dbi, ir = dai * br + ai * dbr;
    W.U[0] = 2 * ((p0 - p1 - p2 + p3) * m[0] + (aai - bb) * m[1] + (abr + ib) * m[2]);
    W.U[1] = 2 * ((-aai - bb) * m[0] + (p0 - p1 + p2 - p3) * m[1] + (abi - ir) * m[2]);
    W.U[2] = 2 * ((ib - abr) * m[0] + (-ir - abi) * m[1] + (p0 + p1 - p2 - p3) * m[2]);
    const double f = 2 * sp;
    W.Vx[0] = -f * (bi * m[0] - br * m[1] + ai * m[2]);
    W.Vx[1] = -f * (ar * m[2] - br * m[0] - bi * m[1]);
    W.Vx[2] = -f * (ai * m[0] - ar * m[1] - bi * m[2]);
    W.Vy[0] = f * (ar * m[2] - br * m[0] - bi * m[1]);
    W.Vy[1] = f * (br * m[1] - bi * m[0] - ai * m[2]);
    W.Vy[2] = -f * (ar * m[0] + ai * m[1] + br * m[2]);
}

// Pass 0 of the steady state (blochss.hip DESIGN 8t, blochssgn.hip DESIGN 8u), moved here from blochss.hip token for token.
constexpr int BLOCH_SSINV = 9 * 256;                 // doubles of (I - A)^-1 per workgroup of the tangent

// Stages the rows t0 .. of the pulse b1 s into sst, as k_bloch_batch stages them.
__device__ __forceinline__ void bloch_ss_stage(double (*sst)[8], const double* __restrict__ in, long t_off, int ntime, int t0, double sc,
                                               double gamma) {
    __syncthreads();
    const int cnt = min(BLOCH_CH, ntime - t0), tid = threadIdx.x;
    if (tid < cnt) {
        const double* s = in + BLOCH_IN * (t_off + t0 + tid);
        const double dt = s[8];
        sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                      // rotx of the pulse b1 s, as k_bloch_batch forms it
        sst[tid][1] = ((s[1] * sc) * gamma) * dt;                         // roty
        for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
    }
    __syncthreads();
}

// R c for a column c of A with the fused products that k_bloch_batch's pass 0 compiles to: there the compiler rounds the middle
// product of a row, R_i1 c_1, and fuses the outer two onto it, whereas rot_vec on its own (and pass 0's own B update) rounds the
// first.  Written out so that M has mode 1's bits (tests/test_blochss_gpu.py holds the two equal).
__device__ __forceinline__ void bloch_ss_rot_col(const Rot3& R, const double c[3], double o[3]) {
    for (int i = 0; i < 3; ++i) o[i] = fma(R.m[6 + i], c[2], fma(R.m[i], c[0], R.m[3 + i] * c[1]));
}

// Pass 0 of k_bloch_batch for one point, statement by statement: (A, B) over the samples, inv = (I - A)^-1 by the adjugate
// (column-major), m = inv B.  Leaves the pulse's last tile staged.
__device__ __forceinline__ void bloch_ss_pass0(double (*sst)[8], const double* __restrict__ in, long t_off, int ntime, double sc,
                                               double gamma, double px, double py, double pz, double dfv, double (&inv)[9],
                                               double (&m)[3]) {
    double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, B[3] = {0, 0, 0};
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        bloch_ss_stage(sst, in, t_off, ntime, t0, sc, gamma);
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int q = 0; q < cnt; ++q) {
            const double* s = sst[q];
            const double rotz = -((s[2] * px + s[3] * py + s[4] * pz) + dfv * s[5]);
            Rot3 R;
            bloch_rotmat(s[0], s[1], rotz, R);
            const double e1 = s[6], e2 = s[7];
            double c[3], o[3];
            for (int j = 0; j < 3; ++j) {                                 // A <- D R A, column by column
                c[0] = A[3 * j]; c[1] = A[3 * j + 1]; c[2] = A[3 * j + 2];
                bloch_ss_rot_col(R, c, o);
                A[3 * j] = e2 * o[0]; A[3 * j + 1] = e2 * o[1]; A[3 * j + 2] = e1 * o[2];
            }
            rot_vec(R, B, o);
            B[0] = e2 * o[0]; B[1] = e2 * o[1]; B[2] = e1 * o[2] + (1 - e1);
        }
    }
    double K[9];
    for (int e = 0; e < 9; ++e) K[e] = ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0) - A[e];
    const double c00 = K[4] * K[8] - K[7] * K[5], c01 = K[7] * K[2] - K[1] * K[8], c02 = K[1] * K[5] - K[4] * K[2];
    const double det = K[0] * c00 + K[3] * c01 + K[6] * c02;
    const double iv[9] = {c00 / det, c01 / det, c02 / det,
                          (K[6] * K[5] - K[3] * K[8]) / det, (K[0] * K[8] - K[6] * K[2]) / det, (K[3] * K[2] - K[0] * K[5]) / det,
                          (K[3] * K[7] - K[6] * K[4]) / det, (K[6] * K[1] - K[0] * K[7]) / det, (K[0] * K[4] - K[3] * K[1]) / det};
    for (int i = 0; i < 3; ++i) m[i] = iv[i] * B[0] + iv[3 + i] * B[1] + iv[6 + i] * B[2];
    for (int e = 0; e < 9; ++e) inv[e] = iv[e];
}

// The inputs of one mbfir_bloch_batch call, staged and filled (slr.hip): the sample rows, the grids, the initial magnetisation
// and Staging's tables.  The forward call uploads this as it is; the adjoint adds its own sections first.  m0x / m0y / m0z: the
// initial magnetisation at the first entry of every (scale, frequency, position) block of the outputs' layout under `mode` (all
// three null: [0 0 1]).  ntime / npair: per pulse, as sim_block_table takes them; M: m0 blocks; O: output entries of one plane.
struct BlochStaged {
    Staging S;
    size_t o_in = 0, o_df = 0, o_pos = 0, o_m0 = 0;
    std::vector<BlochPulseDev> pd;
    std::vector<int> ntime;
    std::vector<long> npair;
    long M = 0, O = 0;
};
void bloch_stage(BlochStaged& B, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                 const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                 const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                 const double* dy, const double* dz, int nscale, const double* scales, int mode, const double* m0x,
                 const double* m0y, const double* m0z);

// What the pulse train (blochtrain.hip) shares with its adjoint (blochtrainvjp.hip), moved here from
// blochtrain.hip token for token: the planes' count, the per-pulse descriptor, the helpers of one repetition and the host staging.
constexpr int TRAIN_ENT = 24;                  // A (9), B (3), A_e (9), B_e (3), column-major like Rot3

// Per-pulse descriptor of a train.  Combination c = scale ngain + gain of the pulse has its amplitude at amp[a_off + c] and its
// planes from w_off + c 24 npair; repetition k has (cos, sin, gain index) at r_off + k; the echoes go to e_off + (scale ntr + k) npair
// + point.
struct TrainPulseDev {
    long w_off, a_off, r_off, e_off;
    int ntr, ngain, echo, pad;
    double meq;
};

// M v + meq b for a column-major M, every product and sum where it is written (explicit fma, contraction off), so that a
// repetition has the same bits whether its planes were hoisted out of the loop or loaded inside it.
__device__ __forceinline__ void train_affine(const double* M, const double* b, double meq, const double v[3], double o[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = fma(meq, b[i], fma(M[6 + i], v[2], fma(M[3 + i], v[1], M[i] * v[0])));
}
// Z(+phi) v and Z(-phi) v about z from (c, s) = (cos phi, sin phi), in place.
__device__ __forceinline__ void train_zp(double c, double s, double v[3]) {
#pragma clang fp contract(off)
    const double x = fma(c, v[0], -(s * v[1])), y = fma(s, v[0], c * v[1]);
    v[0] = x; v[1] = y;
}
__device__ __forceinline__ void train_zm(double c, double s, double v[3]) {
#pragma clang fp contract(off)
    const double x = fma(c, v[0], s * v[1]), y = fma(c, v[1], -(s * v[0]));
    v[0] = x; v[1] = y;
}
// The tangent of train_affine (blochtrainjvp.hip): M du + dM u + meq db for column-major M and dM, one chain of fma
// from the first product M[i] du[0] (contraction off), so that a tangent's bits depend neither on where its planes were loaded nor
// on its place in a direction group.
__device__ __forceinline__ void train_affine_jvp(const double* M, const double* dM, const double* db, double meq, const double u[3],
                                                 const double du[3], double o[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double lin = fma(M[6 + i], du[2], fma(M[3 + i], du[1], M[i] * du[0]));
        o[i] = fma(meq, db[i], fma(dM[6 + i], u[2], fma(dM[3 + i], u[1], fma(dM[i], u[0], lin))));
    }
}

struct TrainStaged {
    BlochStaged B;
    size_t o_amp = 0, o_tr = 0, o_rep = 0, o_gi = 0, o_pb = 0;
    long E = 0, W = 0, nprop = 0;                              // echo entries per plane, workspace doubles, workgroups of kernel 1
    std::vector<TrainPulseDev> tr;
};
// blochtrain.hip: the train's sections of one call after bloch_stage (arguments as bloch_train_batch_run's), and the launch of
// k_bloch_train_prop on them, which leaves the propagators' planes in ws.
void train_stage(TrainStaged& Ts, int npulse, int nscale, const double* scales, const int* ntr, const long* roff,
                 const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                 const double* meq);
void train_launch_prop(TrainStaged& Ts, hipStream_t st, double* ws, const double* in = nullptr);

// What the train's adjoint (blochtrainvjp.hip) shares with the fused products (blochtraingn.hip), moved here
// from blochtrainvjp.hip token for token.
constexpr int TRV_T = 8;                       // repetitions per checkpoint group of the run adjoint
static_assert(256 % TRV_T == 0, "a group of repetitions lies within one staged tile of the repetition table");

// The host side of the adjoint's tables (blochtrainvjp.hip train_vjp_stage): the partial and checkpoint descriptors, the table of the
// period adjoint (k_bloch_train_prop's order with chunks of 64 points) and the table of the fold, as sections of the staging, and
// the sizes of what stays on the device.
struct TrainVjpSections {
    size_t o_vp = 0, o_ckr = 0, o_ckp = 0, o_vb = 0, o_fb = 0;
    long npart = 0, nckr = 0, nckp = 0, nfold = 0, nwg = 0;     // double2 partials, checkpoint doubles of the two kernels, workgroups
};
TrainVjpSections train_vjp_stage(TrainStaged& Ts, int npulse, const long* toff, int nscale, const int* ntr);
// Launches k_bloch_train_prop_vjp (blochtrainvjp.hip) on the staged table: cw the planes' cotangents, part and ck its partials and
// checkpoints.  Launches on one stream are ordered, so one checkpoint region serves any number of them.  in (here and in
// train_launch_prop): the input rows on the device, null for the staged ones; the device step's trial passes the rows at b1 + d.
void train_launch_prop_vjp(TrainStaged& Ts, const TrainVjpSections& V, hipStream_t st, const double* cw, double2* part, double* ck,
                           const double* in = nullptr);
// Launches k_bloch_train_run_vjp (blochtrainvjp.hip) on the forward table, for the adjoint in gr and df too (blochtrainvjpg.hip, DESIGN
// 8aj): ws the propagators' planes, ce / cf the three echo / final cotangent planes one after the other on the device (null: none),
// ck its checkpoints, cw the planes' cotangents (zero on entry), gm the three planes of dL / d m0 (null: not wanted).
void train_launch_run_vjp(TrainStaged& Ts, const TrainVjpSections& V, hipStream_t st, const double* ws, int demod, const double* ce,
                          const double* cf, double* ck, double* cw, double* gm);
// The table of the period's tangent (blochtrainjvp.hip): k_bloch_train_prop_vjp's order, once per direction group; nwg receives its
// workgroups.  train_launch_prop_jvp launches k_bloch_train_prop_jvp on it: v the packed directions' section, dws the tangent planes.
size_t train_jvp_table(TrainStaged& Ts, int nscale, int ndir, long& nwg);
void train_launch_prop_jvp(TrainStaged& Ts, hipStream_t st, size_t o_qb, long nwg, size_t o_v, int ndir, double* dws);
// Launches k_bloch_train_prop_dgain (blochtrainsched.hip) on train_jvp_table's table of one direction: dws receives the planes'
// tangents in the gain, laid out as the primal planes.  Shared by the schedule's adjoint and its tangent (blochtrainschedjvp.hip).
void train_launch_prop_dgain(TrainStaged& Ts, hipStream_t st, size_t o_qb, long nwg, double* dws);

// What the schedule's adjoint (blochtrainsched.hip) and tangent (blochtrainschedjvp.hip) share with the fused
// products of the schedule (blochtrainschedgn.hip), moved here from the two files token for token.
// a . (M (J u) - J n) for a column-major M and n = M u + meq b: a repetition's share of dL / dphi through one of its two maps.
// Every product and sum where it is written (contraction off), so that the share has the same bits whatever else the call wants.
__device__ __forceinline__ double train_sched_dphi(const double* M, const double a[3], const double u[3], const double n[3]) {
#pragma clang fp contract(off)
    double p = fma(a[1], n[0], -(a[0] * n[1]));                           // -a . J n
    p = -p;
#pragma unroll
    for (int i = 0; i < 3; ++i) p = fma(a[i], fma(M[3 + i], u[0], -(M[i] * u[1])), p);
    return p;
}
// a . (M (J u)) alone: the demodulated echo is not turned back, so it has no J n term.
__device__ __forceinline__ double train_sched_dphi_demod(const double* M, const double a[3], const double u[3]) {
#pragma clang fp contract(off)
    double p = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) p = fma(a[i], fma(M[3 + i], u[0], -(M[i] * u[1])), p);
    return p;
}
__device__ __forceinline__ double train_sched_dot(const double a[3], const double v[3]) {
#pragma clang fp contract(off)
    return fma(a[2], v[2], fma(a[1], v[1], a[0] * v[0]));
}

// du = Z(+phi) dm + dp J u, in place.  Every product and sum where it is written (contraction off), here and below, so that a
// direction's bits depend neither on its slot in a group nor on what else the call was given.
__device__ __forceinline__ void train_sj_in(double c, double s, double dp, const double u[3], double d[3]) {
#pragma clang fp contract(off)
    train_zp(c, s, d);
    d[0] = fma(-dp, u[1], d[0]);
    d[1] = fma(dp, u[0], d[1]);
}
// o = M du + dg gv - (turn ? dp J n : 0) for a column-major M: one chain of fma from the first product M[i] du[0].
__device__ __forceinline__ void train_sj_map(const double* M, const double gv[3], const double n[3], double dg, double dp, bool turn,
                                             const double du[3], double o[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = fma(dg, gv[i], fma(M[6 + i], du[2], fma(M[3 + i], du[1], M[i] * du[0])));
    if (turn) {
        o[0] = fma(dp, n[1], o[0]);
        o[1] = fma(-dp, n[0], o[1]);
    }
}

// A section of weights or targets of the train's fused calls (train_gn_stage, sched_gn_stage): np planes of n entries each, three
// (x, y, z) or, with magnitude targets, two (xy, z); nothing where v[0] is null.
inline size_t add_planes(Staging& S, const double* const v[3], long n, int np) {
    const size_t o = S.add(v[0] ? (size_t)n * np * 8 : 0);
    if (v[0]) {
        double* d = S.at<double>(o);
        for (int c = 0; c < np; ++c) std::copy(v[c], v[c] + n, d + (size_t)c * n);
    }
    return o;
}
// The sections the train's fused calls add after train_stage and train_vjp_stage (blochtraingn.hip train_gn_stage, t* null for gn):
// the weights and targets, the repetitions' factors, the loss partials' offsets and the fold's table; nlp loss partials, ngf
// workgroups of the fold.  train_launch_run_lsq and train_launch_lsq_fold launch k_bloch_train_run_lsq and k_bloch_train_gn_fold (one
// direction, with the loss sum) on them; echo / rep / fin: whether the echo term, rw and the final term were staged.
struct TrainGnCall {
    TrainStaged Ts;
    TrainVjpSections V;
    size_t o_we = 0, o_te = 0, o_rw = 0, o_wf = 0, o_tf = 0, o_lp = 0, o_gf = 0;
    long PE = 0, nlp = 0, ngf = 0;
    bool mag = false;                   // the magnitude fits: the weight and target sections are two planes, (xy, z)
};
void train_gn_stage(TrainGnCall& Cl, int npulse, const long* toff, int nscale, const int* ntr, const long* roff, int ebcast, int ndir,
                    const double* const w[3], const double* const t[3], const double* rw, const double* const wf[3],
                    const double* const tf[3], bool mag = false);
void train_launch_run_lsq(TrainGnCall& Cl, hipStream_t st, int demod, int ebcast, bool echo, bool rep, bool fin, const double* ws,
                          double* ck, double* cw, double* gm, double* lpart);
void train_launch_lsq_fold(TrainGnCall& Cl, hipStream_t st, int nscale, const double2* part, const double* in, double2* grad,
                           const double* lpart, double* loss);

// What the train's device Levenberg-Marquardt step (blochtrainlm.hip) shares with the kernels it is made of: the bodies
// of k_bloch_train_prop_jvp (blochtrainjvp.hip), k_bloch_train_run_gn (blochtraingn.hip) and the two halves of k_bloch_train_prop_vjp
// (blochtrainvjp.hip), moved here token for token with the workgroup's table entry as an argument.  The shipped kernels call them;
// the step's kernels call them behind the run flag, so H p has the shipped product's bits.
// Directions per workgroup of the period's tangent (blochtrainjvp.hip says how it was chosen; DESIGN 8aa has the table).
#ifndef TJVP_K
#define TJVP_K 4
#endif
// Whether k_bloch_train_run_gn keeps the planes and their cotangents in registers over the whole walk when the pulse has one
// distinct gain, as k_bloch_train_run_vjp does.  DESIGN 8ab has the table of candidates.
#ifndef TGN_HOIST
#define TGN_HOIST 0
#endif

// bloch_fwd_step without the recovery term: a column of A.
__device__ __forceinline__ void bloch_hom_step(const double* s, double rotz, double m[3]) {
    Rot3 R;
    bloch_rotmat(s[0], s[1], rotz, R);
    const double e1 = s[6], e2 = s[7];
    double o[3];
    rot_vec(R, m, o);
    m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = e1 * o[2];
}

// k_bloch_train_prop_jvp for the workgroup bk = (pulse, combination, chunk of 64 points, direction group).
__device__ __forceinline__ void bloch_train_prop_jvp_body(const SimBlock bk, const double* __restrict__ in,
                                                          const double* __restrict__ df, const double* __restrict__ pos3,
                                                          const double* __restrict__ amp, const BlochPulseDev* __restrict__ pulses,
                                                          const TrainPulseDev* __restrict__ trains, const double2* __restrict__ v,
                                                          int ndir, double* __restrict__ dws) {
    __shared__ double sst[BLOCH_CH][8];
    __shared__ double2 sdn[TJVP_K][BLOCH_CH];
    const int tid = threadIdx.x, col = tid >> 6, lane = tid & 63;
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const double sc = amp[Tr.a_off + bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos, echo = Tr.echo;
    const int k0 = bk.pad * TJVP_K, kcnt = min(TJVP_K, ndir - k0);
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 64 + lane;
    const bool live = pair < npair;
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const bool rec = col == 3;                                            // uniform over the wavefront
    const int ent = rec ? 9 : 3 * col;                                    // the column's first entry among A (9), B (3)
    const double2* vg = v + (long)ndir * P.t_off + (long)k0 * ntime;      // the group's first direction
    // the column of direction k0 of the combination; a direction is TRAIN_ENT npair doubles
    double* w = dws + (long)ndir * Tr.w_off + ((long)bk.scale * ndir + k0) * TRAIN_ENT * npair + (long)ent * npair + (live ? pair : 0);
    const long dstr = (long)TRAIN_ENT * npair;
    double m[3] = {col == 0 ? 1.0 : 0.0, col == 1 ? 1.0 : 0.0, col == 2 ? 1.0 : 0.0}, dm[TJVP_K][3];
#pragma unroll
    for (int k = 0; k < TJVP_K; ++k) dm[k][0] = dm[k][1] = dm[k][2] = 0;
    if (echo == 0 && live) {                                              // (A_e, B_e) = (I, 0) has no tangent
#pragma unroll
        for (int k = 0; k < TJVP_K; ++k)
            if (k < kcnt) {
                double* o = w + k * dstr + 12 * npair;
                o[0] = 0; o[npair] = 0; o[2 * npair] = 0;
            }
    }
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        __syncthreads();
        const int cnt = min(BLOCH_CH, ntime - t0);
        if (tid < cnt) {
            const double* s = in + BLOCH_IN * (P.t_off + t0 + tid);
            const double dt = s[8];
            sst[tid][0] = ((-(s[0] * sc)) * gamma) * dt;                  // rotx of the pulse b1 amp, as k_bloch_train_prop forms it
            sst[tid][1] = ((s[1] * sc) * gamma) * dt;                     // roty
            for (int e = 2; e < 8; ++e) sst[tid][e] = s[e];
#pragma unroll
            for (int k = 0; k < TJVP_K; ++k)
                if (k < kcnt) {
                    const double2 d = vg[(long)k * ntime + t0 + tid];
                    sdn[k][tid] = make_double2(((-(d.x * sc)) * gamma) * dt, ((d.y * sc) * gamma) * dt);      // (dnx, dny)
                }
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const double* s = sst[q];
            const double rotz = bloch_rotz(s, px, py, pz, dfv);
            Rot3 R;
            BlochTrig tr;
            bloch_rotmat_trig<true>(s[0], s[1], rotz, R, tr);
            const double e1 = s[6], e2 = s[7];
            BlochJvpShared W;
            bloch_jvp_shared(s[0], s[1], rotz, tr, m, W);
#pragma unroll
            for (int k = 0; k < TJVP_K; ++k)
                if (k < kcnt) {
                    const double2 dn = sdn[k][q];
                    const double nd = s[0] * dn.x + s[1] * dn.y;
                    double o[3];
                    rot_vec(R, dm[k], o);
                    dm[k][0] = e2 * (o[0] + (nd * W.U[0] + dn.x * W.Vx[0] + dn.y * W.Vy[0]));
                    dm[k][1] = e2 * (o[1] + (nd * W.U[1] + dn.x * W.Vx[1] + dn.y * W.Vy[1]));
                    dm[k][2] = e1 * (o[2] + (nd * W.U[2] + dn.x * W.Vx[2] + dn.y * W.Vy[2]));
                }
            double o[3];
            rot_vec(R, m, o);
            m[0] = e2 * o[0]; m[1] = e2 * o[1];
            if (rec) m[2] = e1 * o[2] + (1 - e1); else m[2] = e1 * o[2];
            if (t0 + q + 1 == echo) {                                     // uniform over the workgroup: (dA_e, dB_e)
#pragma unroll
                for (int k = 0; k < TJVP_K; ++k)
                    if (k < kcnt) {
                        double* oe = w + k * dstr + 12 * npair;
                        oe[0] = dm[k][0]; oe[npair] = dm[k][1]; oe[2 * npair] = dm[k][2];
                    }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < TJVP_K; ++k)
        if (k < kcnt) {
            double* o = w + k * dstr;
            o[0] = dm[k][0]; o[npair] = dm[k][1]; o[2 * npair] = dm[k][2];
        }
}

// k_bloch_train_run_gn's body, bloch_train_run_gn_body, is in blochtrain_gn_bodies.inc, included below bloch_mag_seed.

// What the schedule's device Levenberg-Marquardt step (blochtrainschedlm.hip) shares with the fused products of the
// schedule (blochtrainschedgn.hip): the body of k_bloch_train_run_sched_gn, moved here token for token with the
// workgroup's table entry as an argument, its switch TSGN_HOIST and train_sg_back.  The shipped kernel calls the body; the step's
// kernel calls it behind the run flag, so H p has the shipped product's bits.
// Whether k_bloch_train_run_sched_gn keeps the 24 planes and their 24 tangents in registers over the whole walk when the pulse has
// one distinct gain.  0: twelve of each are loaded where a repetition needs them, as TGN_HOIST = 0 and k_bloch_train_run_sched_jvp
// do.  DESIGN 8af has the resource table of both.
#ifndef TSGN_HOIST
#define TSGN_HOIST 0
#endif

// o = M' a for a column-major M: a multiplier's step back through one of a repetition's two maps.  Every product and sum where it
// is written (contraction off), so that a product's bits do not depend on what surrounds the statement.
__device__ __forceinline__ void train_sg_back(const double* M, const double a[3], double o[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = fma(M[3 * i + 2], a[2], fma(M[3 * i + 1], a[1], M[3 * i] * a[0]));
}

// k_bloch_train_run_sched_gn's body, bloch_train_run_sched_gn_body, is in blochtrain_gn_bodies.inc, included below bloch_mag_seed.

// The thread of k_bloch_train_prop_vjp: wave = column of [A | B], lane = point, for the workgroup bk = (pulse, combination, chunk of
// 64 points) of the period adjoint's table.
struct TrainPropVjpThread {
    BlochPulseDev P;
    TrainPulseDev Tr;
    double sc, gamma, dfv, px, py, pz;
    int ntime, echo, col;
    long npair, pair;
    bool live, rec;
    double2* wpart;
    double* wck;
};
__device__ __forceinline__ TrainPropVjpThread bloch_train_prop_vjp_thread(
    const SimBlock bk, const double* __restrict__ df, const double* __restrict__ pos3, const double* __restrict__ amp,
    const BlochPulseDev* __restrict__ pulses, const TrainPulseDev* __restrict__ trains, const VjpPulseDev* __restrict__ vp,
    const BlochCkDev* __restrict__ cks, double2* __restrict__ part, double* ck) {
    TrainPropVjpThread C;
    const int tid = threadIdx.x, col = tid >> 6, lane = tid & 63;
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const VjpPulseDev V = vp[bk.pulse];
    const BlochCkDev K = cks[bk.pulse];
    const double sc = amp[Tr.a_off + bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos, echo = Tr.echo;
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 64 + lane;
    const bool live = pair < npair;                                       // a thread past the end of the grid sweeps the first point
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const long wg = (long)bk.scale * V.nch + bk.chunk;                    // the workgroup among its pulse's
    double2* wpart = part + V.p_off + wg * V.n;
    double* wck = ck + K.c_off + wg * K.ng * BLOCH_CK + tid;
    const bool rec = col == 3;                                            // uniform over the wavefront
    C.P = P; C.Tr = Tr; C.sc = sc; C.gamma = gamma; C.dfv = dfv; C.px = px; C.py = py; C.pz = pz;
    C.ntime = ntime; C.echo = echo; C.col = col; C.npair = npair; C.pair = pair; C.live = live; C.rec = rec;
    C.wpart = wpart; C.wck = wck;
    return C;
}
// The column's cotangents from the run adjoint's planes: l at the end of the period, le at the state after `echo` samples.
__device__ __forceinline__ void bloch_train_prop_vjp_seed(const TrainPropVjpThread& C, const SimBlock bk, const double* __restrict__ cw,
                                                          double l[3], double le[3]) {
    const int col = C.col;
    const long npair = C.npair, pair = C.pair;
    const TrainPulseDev& Tr = C.Tr;
    if (C.live) {
        const double* c = cw + Tr.w_off + (long)bk.scale * TRAIN_ENT * npair + pair;
#pragma unroll
        for (int i = 0; i < 3; ++i) { l[i] = c[(3 * col + i) * npair]; le[i] = c[(12 + 3 * col + i) * npair]; }
    }
}
// The forward half: the checkpoints of the primal column, which depend on b1 alone.  Leaves the pulse's last tile staged.
__device__ __forceinline__ void bloch_train_prop_vjp_forward(const TrainPropVjpThread& C, double (*sst)[8],
                                                             const double* __restrict__ in) {
    const BlochPulseDev& P = C.P;
    const double sc = C.sc, gamma = C.gamma, px = C.px, py = C.py, pz = C.pz, dfv = C.dfv;
    const int ntime = C.ntime, col = C.col;
    const bool rec = C.rec;
    double* wck = C.wck;
    double m[3] = {col == 0 ? 1.0 : 0.0, col == 1 ? 1.0 : 0.0, col == 2 ? 1.0 : 0.0};
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int q = 0; q < cnt; ++q) {
            if ((q & (VJP_T - 1)) == 0) {                                 // the column before sample t0 + q: the group's checkpoint
                double* w = wck + (long)((t0 + q) / VJP_T) * BLOCH_CK;
                w[0] = m[0]; w[256] = m[1]; w[512] = m[2];
            }
            const double* s = sst[q];
            const double rz = bloch_rotz(s, px, py, pz, dfv);
            if (rec) bloch_fwd_step(s, rz, m); else bloch_hom_step(s, rz, m);
        }
    }
}
// The backward half, the pulse's last tile being staged in sst and the checkpoints written: the partials of (l, le) into wpart.
__device__ __forceinline__ void bloch_train_prop_vjp_backward(const TrainPropVjpThread& C, double (*sst)[8], double* red,
                                                              const double* __restrict__ in, double l[3], const double le[3]) {
    const BlochPulseDev& P = C.P;
    const double sc = C.sc, gamma = C.gamma, px = C.px, py = C.py, pz = C.pz, dfv = C.dfv;
    const int ntime = C.ntime, echo = C.echo, tid = threadIdx.x;
    const bool rec = C.rec, live = C.live;
    double2* wpart = C.wpart;
    const double* wck = C.wck;
    const int tlast = (ntime - 1) / BLOCH_CH * BLOCH_CH;
    const int row = tid >> 4, ln = tid & 15;                              // reduction: 16 lanes per row of the tile
    for (int t0 = tlast; t0 >= 0; t0 -= BLOCH_CH) {
        if (t0 != tlast) bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);      // the forward sweep left the last tile staged
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int g0 = (cnt - 1) / VJP_T * VJP_T; g0 >= 0; g0 -= VJP_T) {
            const int ge = min(g0 + VJP_T, cnt);
            double ms[VJP_T][3];                                          // ms[j] = the column before sample t0 + g0 + j
            const double* w = wck + (long)((t0 + g0) / VJP_T) * BLOCH_CK;
            ms[0][0] = w[0]; ms[0][1] = w[256]; ms[0][2] = w[512];
#pragma unroll
            for (int j = 1; j < VJP_T; ++j) {
                ms[j][0] = ms[j - 1][0]; ms[j][1] = ms[j - 1][1]; ms[j][2] = ms[j - 1][2];
                if (g0 + j < ge) {
                    const double* s = sst[g0 + j - 1];
                    const double rz = bloch_rotz(s, px, py, pz, dfv);
                    if (rec) bloch_fwd_step(s, rz, ms[j]); else bloch_hom_step(s, rz, ms[j]);
                }
            }
#pragma unroll
            for (int j = VJP_T - 1; j >= 0; --j) {
                if (g0 + j < ge) {
                    if (t0 + g0 + j + 1 == echo) { l[0] += le[0]; l[1] += le[1]; l[2] += le[2]; }      // the state after `echo` samples
                    const double* s = sst[g0 + j];
                    const double2 c = bloch_vjp_step(s, bloch_rotz(s, px, py, pz, dfv), ms[j], l);
                    red[(2 * j) * VJP_ROW + tid] = live ? c.x : 0.0;
                    red[(2 * j + 1) * VJP_ROW + tid] = live ? c.y : 0.0;
                }
            }
            __syncthreads();
            double sum = 0;                                               // row = 2 (sample - g0) + (0: rotx, 1: roty); rows past ge are not stored
            for (int k = 0; k < 16; ++k) sum += red[row * VJP_ROW + ln + 16 * k];
            for (int off = 8; off > 0; off >>= 1) sum += __shfl_down(sum, off, 16);
            if (ln == 0 && row < 2 * (ge - g0)) reinterpret_cast<double*>(wpart + t0 + g0)[row] = sum;
            __syncthreads();
        }
    }
}

// The sections the Bloch least-squares calls add to the forward staging (blochgn.hip bloch_gn_stage, moved here token for token so
// that blochssgn.hip stages through it too), and the sizes of what stays on the device.
struct BlochGnSections {
    size_t o_w = 0, o_t = 0, o_v = 0, o_vp = 0, o_ck = 0, o_lp = 0, o_fb = 0, o_jb = 0;
    long npart = 0, nck = 0, nlp = 0, nfold = 0;        // double2 partials, checkpoint doubles, loss partials, workgroups of the fold
};
// mag: w and tg hold two planes each, (xy, z), and the sections are two planes long.
BlochGnSections bloch_gn_stage(BlochStaged& B, int npulse, const long* toff, int nscale, const double* const w[3],
                               const double* const tg[3], int ndir, const double* v_re, const double* v_im, bool mag = false);

// The transverse magnitude of the magnitude fits and its direction: rho = sqrt(mx mx + my my), every operation rounded
// once and none contracted, so that np.sqrt(mx * mx + my * my) on the forward call's output has its bits; u = (mx, my) / rho, and
// (0, 0) where rho is 0.
struct BlochMagDir {
    double rho, ux, uy;
};
__device__ __forceinline__ BlochMagDir bloch_mag_dir(double mx, double my) {
#pragma clang fp contract(off)                                            // the products are rounded before the sum: no fma
    BlochMagDir D;
    const double xx = mx * mx, yy = my * my;
    D.rho = __dsqrt_rn(xx + yy);
    const bool pos = D.rho > 0;
    D.ux = pos ? mx / D.rho : 0.0;
    D.uy = pos ? my / D.rho : 0.0;
    return D;
}
// bloch_fwd_step with the rounding k_bloch_batch's own sweep has, for the magnitude lsq kernel of the end point, whose rho has to have
// the bits of np.sqrt(mx * mx + my * my) of the forward call's output.  The two sweeps are the same expressions, but the compiler
// contracts R v differently in them: k_bloch_batch rounds the product with v[1] and fuses the other two, o_i = fma(R_i2, v2,
// fma(R_i0, v0, R_i1 v1)), bloch_fwd_step's callers round the one with v[0]; m ends an ulp or two apart at some points.  Everything
// else of a step (rotz, the rotation matrix, the decay and the recovery fma(e1, o_2, 1 - e1)) comes out alike in both, so stating
// R v with explicit fma is enough; tests/test_blochmag_gpu.py holds the end points equal bit for bit on every case.
__device__ __forceinline__ void bloch_fwd_step_batch(const double* s, double rotz, double m[3]) {
    Rot3 R;
    bloch_rotmat(s[0], s[1], rotz, R);
    const double e1 = s[6], e2 = s[7];
    double o[3];
    for (int i = 0; i < 3; ++i) o[i] = fma(R.m[6 + i], m[2], fma(R.m[i], m[0], R.m[3 + i] * m[1]));
    m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = fma(e1, o[2], 1 - e1);
}
// The cotangent of the magnitude fits from the pair of weights w = (w_xy, w_z): lsq with a = rho - t_xy and b = mz - t_z, gn with
// a = u . dm_xy and b = dm_z.  c = (w_xy a u_x, w_xy a u_y, w_z b); a dead thread's is zero.  Only w[0] and w[1] are read: the
// train's twins pass an array of two.
__device__ __forceinline__ void bloch_mag_seed(const BlochMagDir& D, const double w[3], double a, double b, bool live, double c[3]) {
    const double wa = w[0] * a;
    c[0] = live ? wa * D.ux : 0.0;
    c[1] = live ? wa * D.uy : 0.0;
    c[2] = live ? w[1] * b : 0.0;
}
// The bodies of the two Gauss-Newton walks of the pulse train, bloch_train_run_gn_body and
// bloch_train_run_sched_gn_body, twice: as they are, the component fits, and as ..._mag, the magnitude fits of
// (|Mxy|, mz) per echo and at the final state.  Plain text on both sides, as blochssgn_kernels.inc is.
#define TRAIN_GN_BODY(name) name
#define TRAIN_MAG false
#include "blochtrain_gn_bodies.inc"
#undef TRAIN_GN_BODY
#undef TRAIN_MAG
#define TRAIN_GN_BODY(name) name##_mag
#define TRAIN_MAG true
#include "blochtrain_gn_bodies.inc"
#undef TRAIN_GN_BODY
#undef TRAIN_MAG
// Launches k_bloch_gn_fold (blochgn.hip) on nfold workgroups; lpart, lp, loss as the kernel takes them (loss null: no loss sum).
void bloch_gn_fold_launch(hipStream_t st, long nfold, const double2* part, const VjpPulseDev* vp, const SimBlock* blocks,
                          const double* scales, int nscale, const double* in, const BlochPulseDev* pulses, double2* out,
                          const double* lpart, const long* lp, double* loss);

// What the Levenberg-Marquardt steps on the device share (simgn.hip DESIGN 8n, blochgn.hip DESIGN 8s), moved here from simgn.hip
// token for token.  A pulse whose CG has stopped has run = 0: its workgroups of every later launch return at once, so its bits do
// not depend on how long its neighbours go on.
struct LmState {
    double rr, gg, mu;
    int ncg, run, status, pad;         // status: 0 tolerance reached, 1 the cap cg reached, 2 breakdown
};

// The sum of one double per thread of the 256 by a fixed tree in LDS (sw: 256 doubles); every thread gets it.  No shuffles: a
// second width of __shfl_down in simgn.hip changed how the compiler lowers the width-16 ones of abr_gn_sweeps in the shipped kernels
// (DESIGN 8n), and bloch_gn_sweeps of blochgn.hip has the same width-16 pass.
__device__ __forceinline__ double lm_block_sum(double s, double* sw) {
    __syncthreads();                                              // sw is free again
    sw[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sw[threadIdx.x] += sw[threadIdx.x + o];
        __syncthreads();
    }
    return sw[0];
}
// <u, v> of the real forms, one sample, and v + al u: every product and sum rounded on its own (contraction off in these two
// bodies; the round-to-nearest intrinsics of this platform are plain * and +, which the default contraction mode fuses), so that
// the updates have the bits of the host loop's NumPy expressions on the same inputs.
__device__ __forceinline__ double lm_redot(double2 u, double2 v) {
#pragma clang fp contract(off)
    return u.x * v.x + u.y * v.y;
}
__device__ __forceinline__ double2 lm_axpy(double al, double2 u, double2 v) {
#pragma clang fp contract(off)
    return make_double2(v.x + al * u.x, v.y + al * u.y);
}
__device__ __forceinline__ bool lm_goes_on(int ncg, int cg, double rr, double rtol, double gg) {
    return ncg < cg && rr > rtol * gg;
}
// Launches k_lm_init (simgn.hip) on npulse workgroups: p holds b; d = 0, r = b, rr = gg = <b, b> and the first run flag.
void lm_init_launch(hipStream_t st, int npulse, const VjpPulseDev* vp, const double* mu, int cg, double rtol, const double2* p,
                    double2* d, double2* r, LmState* state);
// Launch k_bloch_lm_step (blochgn.hip) on npulse workgroups, one CG iteration of every running pulse from the partials of its sweep,
// and k_bloch_lm_trial on the T samples, the input rows at b1 + d; arguments as the kernels take them.
void bloch_lm_step_launch(hipStream_t st, int npulse, const double2* part, const VjpPulseDev* vp, const double* scales, int nscale,
                          const double* in, const BlochPulseDev* pulses, int cg, double rtol, double2* p, double2* d, double2* r,
                          double2* hp, LmState* state);
void bloch_lm_trial_launch(hipStream_t st, const double* in, const double2* d, long T, double* trial);
// The sections the schedule's fused calls add after train_stage (blochtrainschedgn.hip sched_gn_stage, t* null for gn; moved here so
// that the schedule's device step stages through the same code): the weights and targets, the repetitions' factors, the partial and
// checkpoint descriptors, the loss partials' offsets and the fold's table at ndir directions.
struct SchedGnCall {
    TrainStaged Ts;
    size_t o_we = 0, o_te = 0, o_rw = 0, o_wf = 0, o_tf = 0, o_vp = 0, o_ck = 0, o_lp = 0, o_fb = 0;
    long PE = 0, npart = 0, nck = 0, nlp = 0, nfold = 0;      // per direction: double2 partials, checkpoint doubles of one state
};
// mag: w, t, wf and tf hold two planes each, (xy, z), and the sections are two planes long.
void sched_gn_stage(SchedGnCall& Cl, int npulse, int nscale, const int* ntr, const long* roff, int ebcast, int ndir,
                    const double* const w[3], const double* const t[3], const double* rw, const double* const wf[3],
                    const double* const tf[3], bool mag = false);
// Launch k_bloch_train_run_sched_lsq (mag: k_bloch_train_run_sched_lsq_mag; no dL / dm0) and k_bloch_train_sched_gn_fold (one direction, with the loss sum) of
// blochtrainschedgn.hip for the schedule's device step (blochtrainschedlm.hip); arguments as the kernels take them.
void train_sched_lsq_launch(hipStream_t st, long nblk, const double* ws, const double* dws, const double2* rep, const int* gidx,
                            const double* rw, const BlochPulseDev* pulses, const TrainPulseDev* trains, const SimBlock* blocks,
                            const VjpPulseDev* vp, const BlochCkDev* cks, const long* lp, const double* m0, int demod, int ebcast,
                            const double* we, const double* te, long PE, const double* wf, const double* tf, long PO, double* ck,
                            double2* part, double* lpart, bool mag = false);
// Launch the magnitude twins of the two lsq walks (blochtrainmag.hip) on nblk workgroups; arguments as the kernels take
// them, the weights and targets two planes (xy, z) each.
void train_run_lsq_mag_launch(hipStream_t st, long nblk, const double* ws, const double2* rep, const int* gidx, const double* rw,
                              const BlochPulseDev* pulses, const TrainPulseDev* trains, const SimBlock* blocks, const BlochCkDev* cks,
                              const long* lp, const double* m0, int demod, int ebcast, const double* we, const double* te, long PE,
                              const double* wf, const double* tf, long PO, double* ck, double* cw, double* gmx, double* gmy,
                              double* gmz, double* lpart);
void train_sched_lsq_mag_launch(hipStream_t st, long nblk, const double* ws, const double* dws, const double2* rep, const int* gidx,
                                const double* rw, const BlochPulseDev* pulses, const TrainPulseDev* trains, const SimBlock* blocks,
                                const VjpPulseDev* vp, const BlochCkDev* cks, const long* lp, const double* m0, int demod, int ebcast,
                                const double* we, const double* te, long PE, const double* wf, const double* tf, long PO, double* ck,
                                double2* part, double* gmx, double* gmy, double* gmz, double* lpart);
void train_sched_gn_fold_launch(hipStream_t st, long nfold, const double2* part, long NP, const VjpPulseDev* vp, const SimBlock* blocks,
                                int nscale, double2* out, const double* lpart, const long* lp, double* loss);

// The adjoint's sections of one call (simgrad.hip, simgradg.hip): the cotangents, the partial descriptors and the fold kernel's table.
struct VjpSections {
    size_t o_ca = 0, o_cb = 0, o_vp = 0, o_fb = 0;
    long nfold = 0, npart = 0;                                  // workgroups of the fold; double2 entries of the partials
};
// Adds and fills the adjoint's sections of S (after the forward sections: pointers into S taken before this are stale).
inline VjpSections vjp_stage(Staging& S, int npulse, const long* roff, const std::vector<int>& ntime,
                             const std::vector<long>& npoint, int nscale, long O, const double* ca_re, const double* ca_im,
                             const double* cb_re, const double* cb_im) {
    VjpSections V;
    std::vector<VjpPulseDev> vp(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int nch = int((npoint[p] + 255) / 256);
        vp[p] = VjpPulseDev{roff[p], V.npart, ntime[p], nch};
        V.npart += (long)nscale * nch * ntime[p];
        V.nfold += (ntime[p] + 255) / 256;
    }
    V.o_ca = S.add((size_t)O * 16);
    V.o_cb = S.add((size_t)O * 16);
    V.o_vp = S.add(npulse * sizeof(VjpPulseDev));
    V.o_fb = S.add(V.nfold * sizeof(SimBlock));
    pack_cplx(O, ca_re, ca_im, S.at<double2>(V.o_ca));
    pack_cplx(O, cb_re, cb_im, S.at<double2>(V.o_cb));
    std::copy(vp.begin(), vp.end(), S.at<VjpPulseDev>(V.o_vp));
    SimBlock* fb = S.at<SimBlock>(V.o_fb);
    for (int p = 0; p < npulse; ++p)
        for (int c = 0; c < (ntime[p] + 255) / 256; ++c) *fb++ = SimBlock{p, 0, c, 0};
    return V;
}

}  // namespace mbfir
