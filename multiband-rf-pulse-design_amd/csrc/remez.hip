// Batched Parks-McClellan (Remez exchange) on the device for dzlp.m / dzmp.m: real symmetric type I (odd) and type II (even)
// filters of 3 to 2047 taps, one workgroup of 256 threads per design, the whole exchange inside one launch.  Grid, barycentric
// solve, exchange and tap recovery are described in DESIGN.md section 8e.  The exchange is fp64, the tap recovery double-double,
// and every reduction runs in a fixed order, so a design gives the same bits alone or inside any batch.  LDS: x, gamma, C and, for
// the tap recovery, the low parts of gamma and C (5 x 1025 doubles) and small slots; global scratch per design (offset table from
// the host): f, x, D, W, E (5 G doubles), two index lists (2 G ints), the next extremal set (L + 1 ints) and the cosine table
// (2 L - 1 doubles).
#include "dev_common.h"
#include "dd_dev.h"
#include "pulse.h"
#include <cstring>

namespace mbfir {

namespace {

constexpr int RZ_THREADS = 256;
constexpr int RZ_LMAX = 1024;                // numtaps <= 2047

struct RemezJobDev {
    int numtaps, nband, L, G;
    int density, maxiter;
    long scr;                                // byte offset of this design's scratch
    long out;                                // double offset of its taps (numtaps) and extremal frequencies (L + 1)
    int band;                                // first entry of its bands in the band table (6 doubles each)
};

struct RemezScratch {
    double *f, *x, *D, *W, *E, *cs;
    int *cand, *alt, *next;
};

__device__ RemezScratch carve(char* base, int G, int L) {
    RemezScratch s;
    double* d = reinterpret_cast<double*>(base);
    s.f = d; s.x = d + G; s.D = d + 2 * (size_t)G; s.W = d + 3 * (size_t)G; s.E = d + 4 * (size_t)G;
    s.cs = d + 5 * (size_t)G;
    int* ip = reinterpret_cast<int*>(s.cs + (2 * L - 1));
    s.cand = ip; s.alt = ip + G; s.next = ip + 2 * (size_t)G;
    return s;
}

// 1 / d to full double precision without the IEEE division sequence: v_rcp_f64 and two Newton steps (fma).
__device__ __forceinline__ double rcp_nr(double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = fma(-d, r, 1.0);
    r = fma(r, e, r);
    e = fma(-d, r, 1.0);
    return fma(r, e, r);
}

// (h, l) += (a, b): double-double accumulation (two-sum of the high parts, low parts added).
__device__ __forceinline__ void dd_add(double& h, double& l, double a, double b) {
    const double s = h + a, bb = s - h, e = (h - (s - bb)) + (a - bb);
    l += e + b;
    h = s + l;
    l = l - (h - s);
}

// Barycentric interpolant at x through the L + 1 nodes in LDS; *hit = node index when x is a node (then C_k), else -1.
__device__ __forceinline__ double bary(double x, const double* sx, const double* sg, const double* sc, int n1, int* hit) {
    double num = 0.0, den = 0.0;
    int h = -1;
    for (int k = 0; k < n1; ++k) {
        const double d = x - sx[k];
        h = d == 0.0 ? k : h;
        const double tg = sg[k] * rcp_nr(d);
        den += tg;
        num = fma(tg, sc[k], num);
    }
    *hit = h;
    return h >= 0 ? sc[h] : num / den;
}

// The same interpolant with double-double weights (sg, sgl), node values (sc, scl), differences and sums.  For the tap recovery
// only: where the extremal set leaves a transition band empty the terms cancel, and fp64 weights and sums
// leave about 1e-14 in the taps, which a weight ratio of 1e4 turns into more than 1e-8 |delta| of the certificate.
__device__ __forceinline__ double bary_dd(double x, const double* sx, const double* sg, const double* sgl, const double* sc,
                                          const double* scl, int n1) {
    dd num = dd_make(0.0), den = dd_make(0.0);
    int h = -1;
    for (int k = 0; k < n1; ++k) {
        const dd d = two_sum(x, -sx[k]);                     // exact
        h = d.h == 0.0 ? k : h;
        const dd tg = dd_div(dd_make(sg[k], sgl[k]), d);
        den = dd_add(den, tg);
        num = dd_add(num, dd_mul(tg, dd_make(sc[k], scl[k])));
    }
    if (h >= 0) return sc[h] + scl[h];
    const dd q = dd_div(num, den);
    return q.h + q.l;
}

// Candidate test of grid point j in pass 1: a local extremum of E inside its band with |E| >= |delta|.
__device__ __forceinline__ bool is_extremum(const double* E, const int* bstart, int nb_plus1, int j, double adelta) {
    const double e = E[j];
    if (!(fabs(e) >= adelta) || e == 0.0) return false;
    // band of j: bstart is ascending, bstart[nband] = G
    int b = 0;
    while (b + 1 < nb_plus1 && bstart[b + 1] <= j) ++b;
    const double s = e > 0.0 ? 1.0 : -1.0;
    if (j > bstart[b] && !(s * e >= s * E[j - 1])) return false;
    if (j + 1 < bstart[b + 1] && !(s * e > s * E[j + 1])) return false;
    return true;
}

// Pass 2: candidate i of the list survives when it is the largest of its run of equal sign (the first of equal ones).
__device__ __forceinline__ bool run_winner(const double* E, const int* cand, int m, int i) {
    const double e = E[cand[i]], a = fabs(e);
    const bool pos = e > 0.0;
    for (int j = i - 1; j >= 0; --j) {
        const double ej = E[cand[j]];
        if ((ej > 0.0) != pos) break;
        if (fabs(ej) >= a) return false;
    }
    for (int j = i + 1; j < m; ++j) {
        const double ej = E[cand[j]];
        if ((ej > 0.0) != pos) break;
        if (fabs(ej) > a) return false;
    }
    return true;
}

// Ordered stream compaction over [0, n): thread t owns the contiguous chunk t; keep(i) decides, out receives src[i] (or i when
// src is null).  Returns the count.
template <class Keep>
__device__ int compact(int n, const int* src, int* out, int* sscan, Keep keep) {
    const int tid = threadIdx.x, chunk = (n + RZ_THREADS - 1) / RZ_THREADS;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += keep(i) ? 1 : 0;
    sscan[tid] = c;
    __syncthreads();
    if (tid == 0) {                                          // 256 entries, fixed order
        int run = 0;
        for (int t = 0; t < RZ_THREADS; ++t) { const int v = sscan[t]; sscan[t] = run; run += v; }
        sscan[RZ_THREADS] = run;
    }
    __syncthreads();
    int w = sscan[tid];
    for (int i = lo; i < hi; ++i)
        if (keep(i)) out[w++] = src ? src[i] : i;
    __syncthreads();
    return sscan[RZ_THREADS];
}

__global__ __launch_bounds__(RZ_THREADS) void k_remez(const RemezJobDev* __restrict__ jobs, const double* __restrict__ bands,
                                                     char* __restrict__ scratch, double* __restrict__ out, double* __restrict__ rec) {
    __shared__ double sx[RZ_LMAX + 1], sg[RZ_LMAX + 1], sc[RZ_LMAX + 1];
    __shared__ double sgl[RZ_LMAX + 1], scl[RZ_LMAX + 1];    // low parts of gamma and C in the tap recovery (double-double)
    __shared__ int sext[RZ_LMAX + 1];
    __shared__ int sscan[RZ_THREADS + 1];
    __shared__ int sbs[65];                                  // band starts (nband <= 64) and G
    __shared__ double sred[RZ_THREADS / 64 + 17];
    __shared__ double sdd[2 * RZ_THREADS];                   // double-double partial sums of sum gamma D
    __shared__ double sdd2[2 * RZ_THREADS];                  // and, in the tap recovery, of sum gamma (-1)^k / W
    __shared__ int sflag[4];

    const RemezJobDev J = jobs[blockIdx.x];
    const int tid = threadIdx.x, L = J.L, G = J.G, n1 = L + 1, nb = J.nband;
    const bool type2 = (J.numtaps & 1) == 0;
    const double* bt = bands + (size_t)J.band * 6;
    RemezScratch S = carve(scratch + J.scr, G, L);

    // ---- dense grid -----------------------------------------------------------------------------------------
    if (tid == 0) {
        int s = 0;
        for (int b = 0; b < nb; ++b) { sbs[b] = s; s += int(bt[6 * b + 5]); }
        sbs[nb] = G;                                         // type II may end one short of s (f = 1 dropped)
    }
    __syncthreads();
    const double delf = 1.0 / double(J.density * L);
    for (int j = tid; j < G; j += RZ_THREADS) {
        int b = 0;
        while (b + 1 < nb && sbs[b + 1] <= j) ++b;
        const double* q = bt + 6 * b;
        const double lo = q[0], hi = q[1];
        const int i = j - sbs[b], k = int(q[5]);
        const double f = i == k - 1 ? hi : lo + double(i) * delf;
        double D = hi > lo ? q[2] + (q[3] - q[2]) * ((f - lo) / (hi - lo)) : q[2];
        double W = q[4];
        if (type2) {
            const double c = cospi(0.5 * f);
            D = D / c;
            W = W * c;
        }
        S.f[j] = f; S.x[j] = cospi(f); S.D[j] = D; S.W[j] = W;
    }
    for (int k = tid; k < n1; k += RZ_THREADS) sext[k] = int((long)k * (G - 1) / L);   // evenly spaced start
    __syncthreads();

    int status = 1, iters = 0;
    double delta = 0.0;
    for (int it = 1; it <= J.maxiter; ++it) {
        iters = it;
        if (it > 1) {
            for (int k = tid; k < n1; k += RZ_THREADS) sext[k] = S.next[k];
            __syncthreads();
        }
        for (int k = tid; k < n1; k += RZ_THREADS) sx[k] = S.x[sext[k]];
        __syncthreads();
        // barycentric weights: thread per node, exponent kept in an int
        int emax_loc = -100000;
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const double xk = sx[k];
            double p = 1.0;
            int ex = 0;
            for (int j0 = 0; j0 < n1; j0 += 16) {
                const int j1 = min(n1, j0 + 16);
                for (int j = j0; j < j1; ++j)
                    if (j != k) p *= 2.0 * (xk - sx[j]);
                int e;
                p = frexp(p, &e);
                ex += e;
            }
            // gamma_k = (1 / p) 2^-ex; 1 / p in (1, 2]: keep the exponent apart until the common shift is known
            sg[k] = 1.0 / p;
            sc[k] = double(-ex);                             // (sc holds the exponent until C is formed)
            emax_loc = max(emax_loc, -ex);
        }
        double em = block_max(double(emax_loc), sred);
        const int emax = int(em);
        for (int k = tid; k < n1; k += RZ_THREADS) sg[k] = ldexp(sg[k], int(sc[k]) - emax);
        __syncthreads();
        // delta and the interpolation values.  sum gamma D cancels heavily (its terms alternate in sign, and the sum is delta
        // times the cancellation-free sum gamma (-1)^k / W): summed in double-double, or delta keeps only a few digits and the
        // interpolant a spurious degree-L part that the taps cannot represent.
        double nh = 0.0, nl = 0.0, pd = 0.0;
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const int g = sext[k];
            const double sgn = (k & 1) ? -1.0 : 1.0;
            const double p = sg[k] * S.D[g], pe = fma(sg[k], S.D[g], -p);
            dd_add(nh, nl, p, pe);
            pd += sg[k] * sgn / S.W[g];
        }
        sdd[tid] = nh;
        sdd[RZ_THREADS + tid] = nl;
        const double den = block_sum(pd, sred);              // (its barriers also publish sdd)
        if (tid == 0) {                                      // fixed order
            double h = 0.0, l = 0.0;
            for (int t = 0; t < RZ_THREADS; ++t) dd_add(h, l, sdd[t], sdd[RZ_THREADS + t]);
            sred[RZ_THREADS / 64 + 16] = (h + l) / den;
        }
        __syncthreads();
        delta = sred[RZ_THREADS / 64 + 16];
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const int g = sext[k];
            const double sgn = (k & 1) ? -1.0 : 1.0;
            sc[k] = S.D[g] - sgn * delta / S.W[g];
        }
        __syncthreads();
        if (!isfinite(delta)) { status = 2; break; }
        // error on the grid
        for (int j = tid; j < G; j += RZ_THREADS) {
            int hit;
            const double A = bary(S.x[j], sx, sg, sc, n1, &hit);
            S.E[j] = hit >= 0 ? ((hit & 1) ? -delta : delta) : S.W[j] * (S.D[j] - A);
        }
        __syncthreads();
        // exchange
        const double ad = fabs(delta);
        const double* E = S.E;
        const int m1 = compact(G, nullptr, S.cand, sscan, [&](int j) { return is_extremum(E, sbs, nb + 1, j, ad); });
        const int* cand = S.cand;
        const int m2 = compact(m1, cand, S.alt, sscan, [&](int i) { return run_winner(E, cand, m1, i); });
        if (m2 < n1) { status = 2; break; }
        if (tid == 0) {
            int lo = 0, hi = m2 - 1;
            while (hi - lo > L) {
                if (fabs(E[S.alt[lo]]) < fabs(E[S.alt[hi]])) ++lo;
                else --hi;
            }
            sflag[0] = lo;
        }
        __syncthreads();
        const int lo = sflag[0];
        int changed = 0;
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const int g = S.alt[lo + k];
            S.next[k] = g;
            changed |= g != sext[k];
        }
        changed = __syncthreads_or(changed);
        if (!changed) { status = 0; break; }
    }

    // ---- taps from P on the cosine grid ----------------------------------------------------------------------
    // The weights of the last solved set once more in double-double (exact differences, exponent pulled out every 16 factors as
    // above), then delta and the node values from these weights, for bary_dd.  Delta has to be redone with them: the interpolant
    // through D - (-1)^k delta / W has degree L - 1 only for the delta of its own weights, and the fp64 delta would leave a
    // degree-L part of the size of its own error.  The delta reported is the iteration's fp64 one, which the exchange used.
    {
        int emax_loc = -100000;
        int* sex = S.alt;                                    // (the candidate lists are no longer needed)
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const double xk = sx[k];
            dd p = dd_make(1.0);
            int ex = 0;
            for (int j0 = 0; j0 < n1; j0 += 16) {
                const int j1 = min(n1, j0 + 16);
                for (int j = j0; j < j1; ++j)
                    if (j != k) { const dd d = two_sum(xk, -sx[j]); p = dd_mul(p, dd_make(2.0 * d.h, 2.0 * d.l)); }
                int e;
                p.h = frexp(p.h, &e);
                p.l = ldexp(p.l, -e);
                ex += e;
            }
            const dd g = dd_div(dd_make(1.0), p);
            sg[k] = g.h;
            sgl[k] = g.l;
            sex[k] = -ex;
            emax_loc = max(emax_loc, -ex);
        }
        const int emax = int(block_max(double(emax_loc), sred));
        for (int k = tid; k < n1; k += RZ_THREADS) {
            sg[k] = ldexp(sg[k], sex[k] - emax);
            sgl[k] = ldexp(sgl[k], sex[k] - emax);
        }
        __syncthreads();
        dd nm = dd_make(0.0), dn = dd_make(0.0);
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const int g = sext[k];
            const dd gk = dd_make(sg[k], sgl[k]);
            nm = dd_add(nm, dd_mul_d(gk, S.D[g]));
            const dd q = dd_div(gk, dd_make(S.W[g]));
            dn = (k & 1) ? dd_sub(dn, q) : dd_add(dn, q);
        }
        sdd[tid] = nm.h; sdd[RZ_THREADS + tid] = nm.l;
        sdd2[tid] = dn.h; sdd2[RZ_THREADS + tid] = dn.l;
        __syncthreads();
        if (tid == 0) {                                      // fixed order
            dd a = dd_make(0.0), b = dd_make(0.0);
            for (int t = 0; t < RZ_THREADS; ++t) {
                a = dd_add(a, dd_make(sdd[t], sdd[RZ_THREADS + t]));
                b = dd_add(b, dd_make(sdd2[t], sdd2[RZ_THREADS + t]));
            }
            const dd q = dd_div(a, b);
            sred[0] = q.h; sred[1] = q.l;
        }
        __syncthreads();
        const dd dl = dd_make(sred[0], sred[1]);
        for (int k = tid; k < n1; k += RZ_THREADS) {
            const int g = sext[k];
            const dd q = dd_div(dl, dd_make(S.W[g]));
            const dd c = (k & 1) ? dd_add(dd_make(S.D[g]), q) : dd_sub(dd_make(S.D[g]), q);
            sc[k] = c.h; scl[k] = c.l;
        }
        __syncthreads();
    }
    const int M = 2 * L - 1;
    double* P = S.D;                                         // D and W are no longer needed
    double* a = S.W;
    for (int m = tid; m < M; m += RZ_THREADS) S.cs[m] = cospi(2.0 * double(m) / double(M));
    for (int j = tid; j < L; j += RZ_THREADS) P[j] = bary_dd(cospi(2.0 * double(j) / double(M)), sx, sg, sgl, sc, scl, n1);
    __syncthreads();
    for (int k = tid; k < L; k += RZ_THREADS) {
        double s = 0.0;
        int idx = 0;
        for (int j = 1; j < L; ++j) {
            idx += k;
            if (idx >= M) idx -= M;
            s = fma(P[j], S.cs[idx], s);
        }
        const double v = (P[0] + 2.0 * s) / double(M);
        a[k] = k == 0 ? v : 2.0 * v;
    }
    __syncthreads();
    double* h = out + J.out;
    if (!type2) {
        for (int k = tid; k < L; k += RZ_THREADS) {
            if (k == 0) h[L - 1] = a[0];
            else { h[L - 1 - k] = 0.5 * a[k]; h[L - 1 + k] = 0.5 * a[k]; }
        }
    } else {
        for (int n = 1 + tid; n <= L; n += RZ_THREADS) {     // b_n: cos(w / 2) cos(k w) = (cos((k + 1/2) w) + cos((k - 1/2) w)) / 2
            double b;
            if (n == 1) b = a[0] + (L > 1 ? 0.5 * a[1] : 0.0);
            else if (n < L) b = 0.5 * (a[n - 1] + a[n]);
            else b = 0.5 * a[L - 1];
            h[L - n] = 0.5 * b;
            h[L - 1 + n] = 0.5 * b;
        }
    }
    double* fe = h + J.numtaps;
    for (int k = tid; k < n1; k += RZ_THREADS) fe[k] = S.f[sext[k]];
    if (tid == 0) {
        rec[4 * blockIdx.x] = double(status);
        rec[4 * blockIdx.x + 1] = double(iters);
        rec[4 * blockIdx.x + 2] = delta;
        rec[4 * blockIdx.x + 3] = double(G);
    }
}

}  // namespace

int remez_grid_counts(int numtaps, int nband, const double* edges, int density, int* counts) {
    const int L = (numtaps & 1) ? (numtaps + 1) / 2 : numtaps / 2;
    const double delf = 1.0 / double(density * L);
    int G = 0;
    for (int b = 0; b < nband; ++b) {
        int k = int((edges[2 * b + 1] - edges[2 * b]) / delf + 0.5);
        if (k < 1) k = 1;
        counts[b] = k;
        G += k;
    }
    if ((numtaps & 1) == 0 && edges[2 * nband - 1] == 1.0) --G;    // type II: omega = pi is not on the grid
    return G;
}

void remez_run(int device, void* stream, int njobs, const RemezJobHost* jobs, int density, int maxiter) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<RemezJobDev> jd(njobs);
    std::vector<double> bt;
    size_t scr = 0, outn = 0;
    for (int q = 0; q < njobs; ++q) {
        const RemezJobHost& h = jobs[q];
        std::vector<int> cnt(h.nband);
        RemezJobDev& d = jd[q];
        d.numtaps = h.numtaps; d.nband = h.nband;
        d.L = (h.numtaps & 1) ? (h.numtaps + 1) / 2 : h.numtaps / 2;
        d.G = remez_grid_counts(h.numtaps, h.nband, h.edges, density, cnt.data());
        d.density = density; d.maxiter = maxiter;
        d.band = int(bt.size() / 6);
        for (int b = 0; b < h.nband; ++b) {
            const double v[6] = {h.edges[2 * b], h.edges[2 * b + 1], h.desired[2 * b], h.desired[2 * b + 1], h.weight[b], double(cnt[b])};
            bt.insert(bt.end(), v, v + 6);
        }
        d.scr = (long)scr;
        const size_t bytes = (size_t)(5 * (size_t)d.G + 2 * d.L - 1) * 8 + (2 * (size_t)d.G + d.L + 1) * 4;
        scr += (size_t)round_up((long)bytes, 256);
        d.out = (long)outn;
        outn += (size_t)h.numtaps + d.L + 1;
    }
    DevBuf djobs(jd.size() * sizeof(RemezJobDev)), dbands(bt.size() * 8), dscr(scr), dout(outn * 8), drec((size_t)njobs * 32);
    MBFIR_HIP(hipMemcpyAsync(djobs.p, jd.data(), jd.size() * sizeof(RemezJobDev), hipMemcpyHostToDevice, st));
    MBFIR_HIP(hipMemcpyAsync(dbands.p, bt.data(), bt.size() * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_remez, dim3(njobs), dim3(RZ_THREADS), 0, st, djobs.as<RemezJobDev>(), dbands.as<double>(), dscr.as<char>(),
                       dout.as<double>(), drec.as<double>());
    MBFIR_HIP(hipGetLastError());
    std::vector<double> ho(outn), hr((size_t)njobs * 4);
    MBFIR_HIP(hipMemcpyAsync(ho.data(), dout.p, outn * 8, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipMemcpyAsync(hr.data(), drec.p, (size_t)njobs * 32, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipStreamSynchronize(st));
    MBFIR_HIP(hipGetLastError());
    for (int q = 0; q < njobs; ++q) {
        const RemezJobHost& h = jobs[q];
        const double* o = ho.data() + jd[q].out;
        std::memcpy(h.h, o, (size_t)h.numtaps * 8);
        if (h.ext) std::memcpy(h.ext, o + h.numtaps, (size_t)(jd[q].L + 1) * 8);
        *h.status = int(hr[4 * q]);
        *h.iterations = int(hr[4 * q + 1]);
        *h.delta = hr[4 * q + 2];
    }
}

}  // namespace mbfir
