// Root-flip search on the device: score every candidate of a root-flip set of one beta polynomial and keep the best
// (fir_flip_zero.m:56-102 with the beta-tap peak, rf_tools/mex5/minpeakrf.c with the RF peak).
//   candidate = common polynomial c0 (the roots that never flip) times nz linear factors (x - z_j), z_j either the root or its
//   reflection 1 / conj(root), chosen by a bit of an explicit mask or of the candidate index itself;
//   scale     = DC rule sum(beta) = target (fir_flip_zero.m:83) or npoly's max|FFT_nn(beta)| = 1 then * bsf (npoly.code.c);
//   score     = max_k |beta_k|, or max_k |rf_k| with rf = ab2rf(b2a(beta), beta): b2a.m:15-32 (8 n padding, clip at max|B| >= 1,
//               mag2mp window) and ab2rf.m:14-29, the chain of slr.hip / oracle.slr.b2rf;
//   winner    = (peak, index) arg-min over all candidates, ties to the lowest (or highest) index, non-finite peaks never win.
// One workgroup per candidate (grid-stride over candidates), 64 threads up to n = 64 (one wave: the barriers are free), 256 above.
// The length-8n transforms, all for any n:
//   bf   = fft(beta, 8n)             direct, n inputs            8 n^2 complex multiply-adds
//   xlf  = fft(xl), k <= 4n kept     8 sub-DFTs of length n      8 n^2 real x complex
//   xlaf = ifft(xlfp)                8 sub-DFTs, ~n/2 inputs     4 n^2
//   aca  = fft(afa)(0:n-1) / 8n      direct, n outputs           8 n^2
// then the n-step recursion (n^2 / 2 complex rotations).  The sub-DFTs combine in place: output m = r + n s (s = 0..7) needs
// exactly the 8 sub-DFT values at r, so the thread that owns r reads its 8 slots and overwrites them.
// Twiddles exp(-2 pi i m / 8n) and exp(-2 pi i m / nn) are seeded exactly (sincospi of the integer phase, as k_dft_any) into a
// table, indexed by phases kept reduced by integer arithmetic.
// Working set per candidate (double2): Y 8n, X 4n + 1, beta 2 x n (+ the tables 8n + nn when they fit): in LDS when it fits,
// else in a per-workgroup global scratch (n up to 1024).
#include "dev_common.h"
#include "pulse.h"
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace mbfir {

namespace {

struct FlipParams {
    int n, nz, nn, words;          // taps, flip factors, npoly FFT length (power of two >= n), mask words per candidate
    long ncand;
    const double2* c0;             // n - nz coefficients of the common polynomial (c0[0] leading)
    const double2* zr;             // nz: factor roots when not flipped
    const double2* zf;             // nz: ... when flipped
    const unsigned* masks;         // ncand * words (bit j of candidate c = factor j flipped), or null = enumerate
    const int* ebit;               // enumeration: factor j flipped iff bit (ebit[j] >> 1) of c equals ebit[j] & 1
    int scale_rule;                // 0 DC (sum(beta) = target), 1 npoly * bsf (target.x)
    double2 target;
    int criterion;                 // 0 beta taps, 1 RF
    int tie_high;                  // equal peaks go to the highest index (minpeakrf's <=)
    const double2* tw;             // 8n + nn twiddles
    double* peaks;                 // ncand or null
    double* blk_p;                 // per workgroup: best peak ...
    long* blk_i;                   // ... and its index (-1: none finite)
    double2* scratch;              // mode 2: per-workgroup working set of `stride` double2
    long stride;
    const long* pick;              // non-null: build candidate *pick only and write its beta to beta_out
    double2* beta_out;
};

// Stage stores of the test hook's extra launch (k_flip_score<kMode, true>, mbfir_test_flip_stages): workgroups stride over the nsel selected
// candidates sel[s] and store block s of every array.  The search kernels are compiled without them (kDump = false).
struct FlipDump {
    const long* sel;
    long nsel;
    double2* beta;                 // n: after the build and scaling
    double* bf;                    // 8n: |bf| after the clip scale
    double* xl;                    // 8n
    double2* xlfp;                 // 4n + 1: the windowed spectrum
    double2* afa;                  // 8n
    double2* a;                    // n
    double* theta;                 // n: theta[i - 1] of recursion step i (|rf_i| = 2 theta_i)
    double* peak;                  // 1
};

// What a kernel takes: the search's parameters alone, or with the stage stores behind them (the same kernarg layout up to there).
struct FlipDumpParams : FlipParams { FlipDump d; };
template <bool kDump> using FlipArgs = std::conditional_t<kDump, FlipDumpParams, FlipParams>;

// the launch's work items and the candidate behind item s: every candidate, or the selected ones
__device__ __forceinline__ long flip_count(const FlipParams& p) { return p.ncand; }
__device__ __forceinline__ long flip_count(const FlipDumpParams& p) { return p.d.nsel; }
__device__ __forceinline__ long flip_cand(const FlipParams&, long s) { return s; }
__device__ __forceinline__ long flip_cand(const FlipDumpParams& p, long s) { return p.d.sel[s]; }

constexpr int RED = 16;            // double2 of LDS for the block reductions (17 doubles used)

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)
__device__ __forceinline__ double2 cdiv2(double2 a, double2 b) {
    const double d = b.x * b.x + b.y * b.y;
    return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
__device__ __forceinline__ double finite_or_inf(double v) { return v <= 1.79769313486231570e308 ? v : INFINITY; }   // NaN, inf -> inf

// better (p1, i1) than (p2, i2): a recorded candidate (i >= 0) with a smaller peak, equal peaks by index
__device__ __forceinline__ bool flip_better(double p1, long i1, double p2, long i2, int tie_high) {
    const long d = tie_high ? i1 - i2 : i2 - i1;
    return i1 >= 0 && (i2 < 0 || p1 < p2 || (p1 == p2 && d > 0));
}

// beta of candidate c into Bt (ping-pong of 2 x n); returns the buffer that holds it.  Scaled by the rule.
__device__ __forceinline__ double2* flip_build(const FlipParams& p, long c, double2* Bt, double* red, const double2* tw) {
    const int n = p.n, nz = p.nz, n0 = n - nz, T = blockDim.x, tid = threadIdx.x;
    for (int k = tid; k < n; k += T) Bt[k] = k < n0 ? p.c0[k] : make_double2(0, 0);
    __syncthreads();
    int cur = 0;
    for (int j = 0; j < nz; ++j) {                         // coef(2:deg+2) -= z coef(1:deg+1), flipzero.py's order
        int fl;
        if (p.masks) fl = (p.masks[c * p.words + (j >> 5)] >> (j & 31)) & 1;
        else fl = ((c >> (p.ebit[j] >> 1)) & 1) == (p.ebit[j] & 1);
        const double2 z = fl ? p.zf[j] : p.zr[j];
        const double2* src = Bt + cur * n;
        double2* dst = Bt + (cur ^ 1) * n;
        for (int k = tid; k < n; k += T) {
            double2 v = src[k];
            if (k >= 1) {
                const double2 zb = cmul(z, src[k - 1]);
                v = make_double2(v.x - zb.x, v.y - zb.y);
            }
            dst[k] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    double2* b = Bt + cur * n;
    if (p.scale_rule == 0) {                               // fir_flip_zero.m:83  coef *= sum(h) / sum(coef)
        double sr = 0, si = 0;
        for (int k = tid; k < n; k += T) { sr += b[k].x; si += b[k].y; }
        sr = block_sum(sr, red);
        si = block_sum(si, red);
        const double2 f = cdiv2(p.target, make_double2(sr, si));
        for (int k = tid; k < n; k += T) b[k] = cmul(b[k], f);
        __syncthreads();
        return b;
    }
    const int nn = p.nn;                                   // npoly.code.c: b /= max|fft(b, nn)|, then minpeakrf.c: b *= bsf
    const double2* w = tw + 8 * n;
    double m = 0;
    for (int k = tid; k < nn; k += T) {
        double2 acc = make_double2(0, 0);
        int ph = 0;
        for (int j = 0; j < n; ++j) {
            const double2 t = cmul(b[j], w[ph]);
            acc.x += t.x; acc.y += t.y;
            ph += k; ph -= ph >= nn ? nn : 0;
        }
        m = fmax(m, hypot(acc.x, acc.y));
    }
    m = block_max(m, red);
    for (int k = tid; k < n; k += T) b[k] = make_double2(b[k].x / m * p.target.x, b[k].y / m * p.target.x);
    __syncthreads();
    return b;
}

// max_k |rf_k| of rf = ab2rf(b2a(b), b); valid in thread 0.  Y: 8n, X: 4n + 1 double2 of working space.
template <bool kDump>
__device__ __forceinline__ double flip_rf_peak(const FlipArgs<kDump>& p, const double2* b, double2* Y, double2* X, double* red, const double2* tw,
                                               long s_) {
    const int n = p.n, N = 8 * n, T = blockDim.x, tid = threadIdx.x;
    double* Xd = reinterpret_cast<double*>(X);             // N reals
    // bf = fft(b, N); |bf| -> Xd, clip (b2a.m:24-28), xl = log(sqrt(1 - |bf|^2))
    double m = 0;
    for (int k = tid; k < N; k += T) {
        double2 acc = make_double2(0, 0);
        int ph = 0;
        for (int j = 0; j < n; ++j) {
            const double2 t = cmul(b[j], tw[ph]);
            acc.x += t.x; acc.y += t.y;
            ph += k; ph -= ph >= N ? N : 0;
        }
        const double a = hypot(acc.x, acc.y);
        Xd[k] = a;
        m = fmax(m, a);
    }
    m = block_max(m, red);
    const double sc = m >= 1.0 ? 1.0 / (1e-8 + m) : 1.0;
    for (int k = tid; k < N; k += T) {
        const double a = Xd[k] * sc;
        Xd[k] = log(sqrt(1.0 - a * a));
        if constexpr (kDump) { p.d.bf[s_ * N + k] = a; p.d.xl[s_ * N + k] = Xd[k]; }
    }
    __syncthreads();
    // xlf = fft(xl): sub-DFT q = m2 n + k1 over the samples 8 m1 + m2
    for (int q = tid; q < N; q += T) {
        const int m2 = q / n, k1 = q - m2 * n;
        double2 acc = make_double2(0, 0);
        int ph = 0;
        for (int m1 = 0; m1 < n; ++m1) {
            const double v = Xd[8 * m1 + m2];
            const double2 w = tw[8 * ph];
            acc.x += v * w.x; acc.y += v * w.y;
            ph += k1; ph -= ph >= n ? n : 0;
        }
        Y[q] = acc;
    }
    __syncthreads();
    // combine, keep k <= N/2 and window (mag2mp.m:26-29): xlfp -> X[0 .. 4n]
    for (int r = tid; r < n; r += T) {
        double2 y[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) y[t] = Y[t * n + r];
        for (int s = 0; s <= 4; ++s) {
            const int k = r + n * s;
            if (k > 4 * n) break;
            double2 acc = y[0];
#pragma unroll
            for (int t = 1; t < 8; ++t) {
                const double2 v = cmul(y[t], tw[(t * k) % N]);
                acc.x += v.x; acc.y += v.y;
            }
            const double g = (k == 0 || k == 4 * n) ? 1.0 : 2.0;
            X[k] = make_double2(g * acc.x, g * acc.y);
            if constexpr (kDump) p.d.xlfp[s_ * (4 * n + 1) + k] = X[k];
        }
    }
    __syncthreads();
    // xlaf = ifft(xlfp): sub-DFT q = k2 n + m1 over the nonzero inputs 8 k1 + k2 <= 4n
    for (int q = tid; q < N; q += T) {
        const int k2 = q / n, m1 = q - k2 * n, kmax = (4 * n - k2) / 8;
        double2 acc = make_double2(0, 0);
        int ph = 0;
        for (int k1 = 0; k1 <= kmax; ++k1) {
            const double2 v = cmulc(X[8 * k1 + k2], tw[8 * ph]);
            acc.x += v.x; acc.y += v.y;
            ph += m1; ph -= ph >= n ? n : 0;
        }
        Y[q] = acc;
    }
    __syncthreads();
    // combine in place, afa = exp(xlaf) at Y[m] (mag2mp.m:31)
    const double invN = 1.0 / N;
    for (int r = tid; r < n; r += T) {
        double2 y[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) y[t] = Y[t * n + r];
        for (int s = 0; s < 8; ++s) {
            const int mm = r + n * s;
            double2 acc = y[0];
#pragma unroll
            for (int t = 1; t < 8; ++t) {
                const double2 v = cmulc(y[t], tw[(t * mm) % N]);
                acc.x += v.x; acc.y += v.y;
            }
            const double re = acc.x * invN, im = acc.y * invN;
            double sn, cs;
            sincos(im, &sn, &cs);
            const double e = exp(re);
            Y[mm] = make_double2(e * cs, e * sn);
            if constexpr (kDump) p.d.afa[s_ * N + mm] = Y[mm];
        }
    }
    __syncthreads();
    // aca = fft(afa)(0 : n-1) / N, a = aca(n:-1:1) -> X[0 .. n)   (b2a.m:30-32)
    for (int k = tid; k < n; k += T) {
        double2 acc = make_double2(0, 0);
        int ph = 0;
        for (int j = 0; j < N; ++j) {
            const double2 t = cmul(Y[j], tw[ph]);
            acc.x += t.x; acc.y += t.y;
            ph += k; ph -= ph >= N ? N : 0;
        }
        X[n - 1 - k] = make_double2(acc.x * invN, acc.y * invN);
        if constexpr (kDump) p.d.a[s_ * n + n - 1 - k] = X[n - 1 - k];
    }
    __syncthreads();
    // inverse SLR recursion (ab2rf.m:14-29), polynomials ping-pong in Y; |rf_i| = 2 theta_i
    double2* A = Y;
    double2* B = Y + 2 * n;
    for (int k = tid; k < n; k += T) { A[k] = X[k]; B[k] = b[k]; }
    __syncthreads();
    double thmax = 0;
    int cur = 0;
    for (int i = n; i >= 1; --i) {
        const double2 ai = A[cur * n + i - 1], bi = B[cur * n + i - 1];
        const double2 q = cdiv2(bi, ai);
        const double c = sqrt(1.0 / (1.0 + (q.x * q.x + q.y * q.y)));
        const double2 s = make_double2(c * q.x, -c * q.y);                 // conj(c b / a)
        if (tid == 0) {
            const double th = atan2(hypot(s.x, s.y), c);
            thmax = th <= thmax ? thmax : finite_or_inf(th);
            if constexpr (kDump) p.d.theta[s_ * n + i - 1] = th;
        }
        const double2 ms = make_double2(-s.x, s.y);                        // -conj(s)
        const double2* Ac = A + cur * n;
        const double2* Bc = B + cur * n;
        double2* An = A + (cur ^ 1) * n;
        double2* Bn = B + (cur ^ 1) * n;
        for (int k = tid; k < i; k += T) {
            const double2 ak = Ac[k], bk = Bc[k];
            const double2 sb = cmul(s, bk), msa = cmul(ms, ak);
            if (k >= 1) An[k - 1] = make_double2(c * ak.x + sb.x, c * ak.y + sb.y);
            if (k < i - 1) Bn[k] = make_double2(msa.x + c * bk.x, msa.y + c * bk.y);
        }
        __syncthreads();
        cur ^= 1;
    }
    return 2.0 * thmax;
}

// kMode 0: working set and twiddles in LDS; 1: working set in LDS, twiddles from global; 2: both in global memory.
// kDump (a compile-time property, so the search kernels carry no trace of it): score the candidates p.d.sel[] and store every stage.
template <int kMode, bool kDump>
__global__ __launch_bounds__(256) void k_flip_score(FlipArgs<kDump> p) {
    extern __shared__ __attribute__((aligned(16))) double2 smem[];
    const int n = p.n, N = 8 * n, T = blockDim.x, tid = threadIdx.x;
    double* red = reinterpret_cast<double*>(smem);
    double2* W = kMode == 2 ? p.scratch + (size_t)blockIdx.x * p.stride : smem + RED;
    double2* Y = W;
    double2* X = Y + N;
    double2* Bt = X + 4 * n + 1;
    const double2* tw = p.tw;
    if (kMode == 0) {
        double2* tl = Bt + 2 * n;
        for (int m = tid; m < N + p.nn; m += T) tl[m] = p.tw[m];
        __syncthreads();
        tw = tl;
    }
    if constexpr (!kDump) {
        if (p.pick) {                                      // the winner's beta
            const long c = *p.pick;
            if (c < 0) return;
            const double2* b = flip_build(p, c, Bt, red, tw);
            for (int k = tid; k < n; k += T) p.beta_out[k] = b[k];
            return;
        }
    }
    double bp = INFINITY;
    long bi = -1;
    for (long s = blockIdx.x; s < flip_count(p); s += gridDim.x) {                   // s: the candidate, or the selected one's place
        const double2* b = flip_build(p, flip_cand(p, s), Bt, red, tw);
        if constexpr (kDump)
            for (int k = tid; k < n; k += T) p.d.beta[s * n + k] = b[k];
        double pk;
        if (p.criterion == 0) {
            double m = 0;
            for (int k = tid; k < n; k += T) m = fmax(m, finite_or_inf(hypot(b[k].x, b[k].y)));
            pk = block_max(m, red);
        } else {
            pk = flip_rf_peak<kDump>(p, b, Y, X, red, tw, s);
        }
        if (tid == 0) {
            if constexpr (kDump) {
                p.d.peak[s] = pk;
            } else {
                if (p.peaks) p.peaks[s] = pk;
                const long ci = pk < INFINITY ? s : -1;
                if (flip_better(pk, ci, bp, bi, p.tie_high)) { bp = pk; bi = ci; }
            }
        }
        __syncthreads();                                   // the next candidate reuses the working set
    }
    if constexpr (!kDump)
        if (tid == 0) { p.blk_p[blockIdx.x] = bp; p.blk_i[blockIdx.x] = bi; }
}

// arg-min over the workgroups' bests; (peak, index) is a total order, so the result does not depend on the reduction order
__global__ __launch_bounds__(256) void k_flip_argmin(const double* __restrict__ bp, const long* __restrict__ bi, int nb, int tie_high,
                                                     long* __restrict__ win_i, double* __restrict__ win_p) {
    __shared__ double sp[256];
    __shared__ long si[256];
    double p = INFINITY;
    long i = -1;
    for (int b = threadIdx.x; b < nb; b += 256)
        if (flip_better(bp[b], bi[b], p, i, tie_high)) { p = bp[b]; i = bi[b]; }
    sp[threadIdx.x] = p;
    si[threadIdx.x] = i;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h && flip_better(sp[threadIdx.x + h], si[threadIdx.x + h], sp[threadIdx.x], si[threadIdx.x], tie_high)) {
            sp[threadIdx.x] = sp[threadIdx.x + h];
            si[threadIdx.x] = si[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { *win_i = si[0]; *win_p = sp[0]; }
}

// tw[m] = exp(-2 pi i m / N) (m < N), tw[N + m] = exp(-2 pi i m / nn) (m < nn); exact seeds
__global__ void k_flip_twiddles(double2* __restrict__ tw, int N, int nn) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    double s, c;
    if (m < N) {
        sincospi(2.0 * double(m) / double(N), &s, &c);
        tw[m] = make_double2(c, -s);
    } else if (m < N + nn) {
        sincospi(2.0 * double(m - N) / double(nn), &s, &c);
        tw[m] = make_double2(c, -s);
    }
}

template <int kMode>
int flip_blocks(int threads, size_t lds, int ncu) {
    if (lds > 65536)
        MBFIR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_flip_score<kMode, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per = 0;
    MBFIR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_flip_score<kMode, false>, threads, lds));
    return per * ncu;
}

// The hook's part of flip_search_run: the report, the search launch's per-workgroup bests, and one more scoring launch over
// hook.sel through the instantiation that stores every stage (same mode, threads and LDS; nbd workgroups).
void flip_stage_launch(const FlipStages& hook, const FlipParams& p, int mode, int threads, size_t lds, int nb, int nbd, int ldsmax,
                       hipStream_t st) {
    const size_t n = p.n, N = 8 * n, ns = hook.nsel;
    const long rep[8] = {mode, threads, nb, (long)lds, p.stride, ldsmax, p.nn, p.words};
    std::copy(rep, rep + 8, hook.report);
    MBFIR_HIP(hipMemcpyAsync(hook.blk_p, p.blk_p, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipMemcpyAsync(hook.blk_i, p.blk_i, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    if (ns == 0) { MBFIR_HIP(hipStreamSynchronize(st)); return; }
    const bool rf = p.criterion == 1;
    DevBuf dsel(ns * 8), dbe(ns * n * 16), dbf(rf ? ns * N * 8 : 8), dxl(rf ? ns * N * 8 : 8), dxf(rf ? ns * (4 * n + 1) * 16 : 16),
        daf(rf ? ns * N * 16 : 16), da(rf ? ns * n * 16 : 16), dth(rf ? ns * n * 8 : 8), dpk(ns * 8);
    MBFIR_HIP(hipMemcpyAsync(dsel.p, hook.sel, ns * 8, hipMemcpyHostToDevice, st));
    FlipDumpParams q{};
    static_cast<FlipParams&>(q) = p;
    q.peaks = nullptr;
    q.d = FlipDump{dsel.as<long>(), (long)ns, dbe.as<double2>(), dbf.as<double>(), dxl.as<double>(), dxf.as<double2>(),
                   daf.as<double2>(), da.as<double2>(), dth.as<double>(), dpk.as<double>()};
    auto go = [&](auto kernel) {
        if (lds > 65536)
            MBFIR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(nbd), dim3(threads), lds, st, q);
    };
    if (mode == 0) go(&k_flip_score<0, true>);
    else if (mode == 1) go(&k_flip_score<1, true>);
    else go(&k_flip_score<2, true>);
    MBFIR_HIP(hipGetLastError());
    MBFIR_HIP(hipMemcpyAsync(hook.beta, dbe.p, ns * n * 16, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipMemcpyAsync(hook.peak, dpk.p, ns * 8, hipMemcpyDeviceToHost, st));
    if (rf) {
        MBFIR_HIP(hipMemcpyAsync(hook.bf, dbf.p, ns * N * 8, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipMemcpyAsync(hook.xl, dxl.p, ns * N * 8, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipMemcpyAsync(hook.xlfp, dxf.p, ns * (4 * n + 1) * 16, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipMemcpyAsync(hook.afa, daf.p, ns * N * 16, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipMemcpyAsync(hook.a, da.p, ns * n * 16, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipMemcpyAsync(hook.theta, dth.p, ns * n * 8, hipMemcpyDeviceToHost, st));
    }
    MBFIR_HIP(hipStreamSynchronize(st));
}

}  // namespace

// Host side of mbfir_flip_search and of mbfir_test_flip_stages (include/mbfir.h): arguments already checked.  Returns the winner
// (-1: no finite peak).  hook == nullptr is the public call: mode and workgroups as computed here, no stage launch.
long flip_search_run(int device, void* stream, int n, int nz, const double* c0_re, const double* c0_im, const double* z_re,
                     const double* z_im, const double* zf_re, const double* zf_im, long ncand, const unsigned* masks,
                     const int* enum_bits, int scale_rule, double s_re, double s_im, int criterion, int tie_high, double* peaks,
                     double* beta_re, double* beta_im, double* winner_peak, const FlipStages* hook) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = 8 * n, n0 = n - nz, words = (nz + 31) / 32;
    int nn = 1;
    while (nn < n) nn <<= 1;
    std::vector<double2> hc(n0 + 2 * nz);
    pack_cplx(n0, c0_re, c0_im, hc.data());
    pack_cplx(nz, z_re, z_im, hc.data() + n0);
    pack_cplx(nz, zf_re, zf_im, hc.data() + n0 + nz);
    std::vector<int> eb(nz > 0 ? nz : 1);
    for (int j = 0; j < nz; ++j) eb[j] = enum_bits ? enum_bits[j] : (nz - 1 - j) << 1;     // combination_2power (fir_flip_zero.m:153-160)

    int ncu = 0, ldsmax = 0;
    MBFIR_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    MBFIR_HIP(hipDeviceGetAttribute(&ldsmax, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    const int threads = n <= 64 ? 64 : 256;
    const size_t work = (size_t)(14 * n + 1) * 16, red = RED * 16, tabs = (size_t)(N + nn) * 16;
    int mode = 2;
    size_t lds = red;
    if (red + work + tabs <= (size_t)ldsmax) { mode = 0; lds = red + work + tabs; }
    else if (red + work <= (size_t)ldsmax) { mode = 1; lds = red + work; }
    if (hook && hook->force_mode >= 0) {
        const size_t need = hook->force_mode == 0 ? red + work + tabs : hook->force_mode == 1 ? red + work : red;
        if (need > (size_t)ldsmax)
            throw std::invalid_argument("forced mode " + std::to_string(hook->force_mode) + " needs " + std::to_string(need) +
                                        " bytes of LDS, the device gives " + std::to_string(ldsmax));
        mode = hook->force_mode;
        lds = need;
    }
    int maxb = mode == 0 ? flip_blocks<0>(threads, lds, ncu) : mode == 1 ? flip_blocks<1>(threads, lds, ncu) : flip_blocks<2>(threads, lds, ncu);
    if (mode == 2) maxb = std::min(maxb, 2 * ncu);                 // bounds the global scratch (229 KB per workgroup at n = 1024)
    if (hook && hook->max_blocks > 0) maxb = std::min(maxb, hook->max_blocks);
    const int nb = (int)std::max(1L, std::min<long>(ncand, std::max(maxb, 1)));
    const int nsel = hook ? hook->nsel : 0;
    const int nbd = std::max(1, std::min(nsel, std::max(maxb, 1)));  // workgroups of the stage launch

    DevBuf dc(hc.size() * 16), deb(eb.size() * 4), dtw(tabs), dm(masks ? (size_t)ncand * words * 4 : 4),
        dpk(peaks ? (size_t)ncand * 8 : 8), dbp((size_t)nb * 8), dbi((size_t)nb * 8), dwin(16), dbeta((size_t)n * 16),
        dscr(mode == 2 ? (size_t)std::max(nb, nbd) * (14 * n + 1) * 16 : 16);
    MBFIR_HIP(hipMemcpyAsync(dc.p, hc.data(), hc.size() * 16, hipMemcpyHostToDevice, st));
    MBFIR_HIP(hipMemcpyAsync(deb.p, eb.data(), eb.size() * 4, hipMemcpyHostToDevice, st));
    if (masks) MBFIR_HIP(hipMemcpyAsync(dm.p, masks, (size_t)ncand * words * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_flip_twiddles, dim3(cdiv(N + nn, 256)), dim3(256), 0, st, dtw.as<double2>(), N, nn);

    FlipParams p{};
    p.n = n; p.nz = nz; p.nn = nn; p.words = words; p.ncand = ncand;
    p.c0 = dc.as<double2>(); p.zr = p.c0 + n0; p.zf = p.zr + nz;
    p.masks = masks ? dm.as<unsigned>() : nullptr;
    p.ebit = deb.as<int>();
    p.scale_rule = scale_rule; p.target = make_double2(s_re, s_im); p.criterion = criterion; p.tie_high = tie_high;
    p.tw = dtw.as<double2>();
    p.peaks = peaks ? dpk.as<double>() : nullptr;
    p.blk_p = dbp.as<double>(); p.blk_i = dbi.as<long>();
    p.scratch = dscr.as<double2>(); p.stride = 14 * n + 1;
    p.pick = nullptr; p.beta_out = nullptr;
    auto launch = [&](int grid, const FlipParams& q) {
        if (mode == 0) hipLaunchKernelGGL((k_flip_score<0, false>), dim3(grid), dim3(threads), lds, st, q);
        else if (mode == 1) hipLaunchKernelGGL((k_flip_score<1, false>), dim3(grid), dim3(threads), lds, st, q);
        else hipLaunchKernelGGL((k_flip_score<2, false>), dim3(grid), dim3(threads), lds, st, q);
    };
    launch(nb, p);
    long* win_i = dwin.as<long>();
    double* win_p = reinterpret_cast<double*>(win_i + 1);
    hipLaunchKernelGGL(k_flip_argmin, dim3(1), dim3(256), 0, st, p.blk_p, p.blk_i, nb, tie_high, win_i, win_p);
    FlipParams q = p;                                               // the winner's beta (criterion not needed)
    q.pick = win_i; q.beta_out = dbeta.as<double2>(); q.peaks = nullptr;
    launch(1, q);
    MBFIR_HIP(hipGetLastError());
    if (hook) flip_stage_launch(*hook, p, mode, threads, lds, nb, nbd, ldsmax, st);
    long hw[2];
    std::vector<double2> hb(n);
    MBFIR_HIP(hipMemcpyAsync(hw, dwin.p, 16, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipMemcpyAsync(hb.data(), dbeta.p, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    if (peaks) MBFIR_HIP(hipMemcpyAsync(peaks, dpk.p, (size_t)ncand * 8, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipStreamSynchronize(st));
    MBFIR_HIP(hipGetLastError());
    const long w = hw[0];
    double wp;
    memcpy(&wp, &hw[1], 8);
    if (winner_peak) *winner_peak = wp;
    if (w >= 0 && beta_re) unpack_cplx(n, hb.data(), beta_re, beta_im);
    return w;
}

}  // namespace mbfir
