// Inverse SLR step on the device: beta polynomial -> minimum-phase alpha -> RF pulse,
// the restatement of b2a.m:15-32 (with mag2mp.m:21-31) and ab2rf.m:14-29 as dzrf_mb.m:239-240 calls them.
//   b2a   : DFTs of length blp = 8 n (any n: direct O(blp^2) DFT, twiddles by rotation recurrence with an
//           exact sincospi seed every 256 terms), elementwise steps in between
//   ab2rf : the n-step inverse SLR recursion in one workgroup, the two polynomials in LDS (ping-pong)
// k_ab2rf / k_b2rf_batch share ab2rf_recursion, and k_abr_batch / k_abr2_batch share abr_step: one definition each.  The forward
// simulators exist once, as batch kernels: a single pulse is the batch of one pulse at scale 1.0 (mbfir_abr, mbfir_abr2, mbfir_bloch).
// abr_step, the descriptors AbrPulseDev / Abr2PulseDev and the host Staging are in sim_dev.h, which simgrad.hip (the adjoints) shares.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <algorithm>
#include <cmath>

namespace mbfir {

__device__ __forceinline__ double2 cmul2(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// out[k] = scale * sum_j in[j] exp(sign * 2 pi i j k / N); one thread per k, input staged through LDS
constexpr int DFT_TILE = 256;
__global__ __launch_bounds__(256) void k_dft_any(const double2* __restrict__ in, double2* __restrict__ out, int N, int sign,
                                                 double scale) {
    __shared__ double2 tile[DFT_TILE];
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int kk = k < N ? k : 0;
    double sw, cw;
    sincospi(2.0 * double(kk) / double(N), &sw, &cw);
    sw *= sign;
    double2 acc = make_double2(0, 0);
    for (int j0 = 0; j0 < N; j0 += DFT_TILE) {
        const int j = j0 + threadIdx.x;
        __syncthreads();
        tile[threadIdx.x] = j < N ? in[j] : make_double2(0, 0);
        __syncthreads();
        const long ph = ((long)kk * j0) % N;              // exact phase of the tile's first term
        double s, c;
        sincospi(2.0 * double(ph) / double(N), &s, &c);
        s *= sign;
        const int cnt = min(DFT_TILE, N - j0);
        for (int q = 0; q < cnt; ++q) {
            const double2 v = tile[q];
            acc.x += v.x * c - v.y * s;
            acc.y += v.x * s + v.y * c;
            const double cn = c * cw - s * sw;
            s = s * cw + c * sw;
            c = cn;
        }
    }
    if (k < N) out[k] = make_double2(acc.x * scale, acc.y * scale);
}

// B0 = [b ; zeros] (length N)
__global__ void k_slr_pad(const double* __restrict__ b_re, const double* __restrict__ b_im, int n, int N, double2* __restrict__ B0) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) B0[i] = i < n ? make_double2(b_re[i], b_im[i]) : make_double2(0, 0);
}
// xl = log(sqrt(1 - |bf|^2)) with bf scaled by 1 / (1e-8 + max|bf|) when max|bf| >= 1     (b2a.m:24-29, mag2mp.m:24)
__global__ __launch_bounds__(1024) void k_slr_logmag(const double2* __restrict__ bf, int N, double2* __restrict__ xl) {
    __shared__ double sh[17];
    double m = 0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) m = fmax(m, hypot(bf[i].x, bf[i].y));
    m = block_max(m, sh);
    const double sc = m >= 1.0 ? 1.0 / (1e-8 + m) : 1.0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const double re = bf[i].x * sc, im = bf[i].y * sc;
        xl[i] = make_double2(log(sqrt(1.0 - (re * re + im * im))), 0.0);
    }
}
// keep DC and N/2, double 1 .. N/2-1, zero the rest                                        (mag2mp.m:26-29)
__global__ void k_slr_window(double2* __restrict__ x, int N) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double2 v = x[i];
    if (i >= 1 && i < N / 2) v = make_double2(2 * v.x, 2 * v.y);
    else if (i > N / 2) v = make_double2(0, 0);
    x[i] = v;
}
// a = exp(xlaf)                                                                            (mag2mp.m:31)
__global__ void k_slr_exp(double2* __restrict__ x, int N) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double2 v = x[i];
    double s, c;
    sincos(v.y, &s, &c);
    const double e = exp(v.x);
    x[i] = make_double2(e * c, e * s);
}
// aca(n:-1:1)                                                                              (b2a.m:31-32)
__global__ void k_slr_out(const double2* __restrict__ aca, int n, double* __restrict__ a_il) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a_il[2 * i] = aca[n - 1 - i].x; a_il[2 * i + 1] = aca[n - 1 - i].y; }
}

// The n-step inverse SLR recursion (ab2rf.m:14-29) in one workgroup of NT threads, shared by k_ab2rf and k_b2rf_batch.  A / B: the
// two polynomials in LDS, each with its ping-pong twin pp entries further on (the recursion starts in A / B, filled and synchronised
// by the caller); cs: two double2 of LDS; rf: the n samples of the pulse.
template <int NT>
__device__ __forceinline__ void ab2rf_recursion(double2* A, double2* B, int pp, int n, double2* cs, double2* __restrict__ rf) {
    const int tid = threadIdx.x;
    int cur = 0;
    for (int i = n; i >= 1; --i) {
        const double2* Ac = A + cur * pp;
        const double2* Bc = B + cur * pp;
        double2* An = A + (cur ^ 1) * pp;
        double2* Bn = B + (cur ^ 1) * pp;
        if (tid == 0) {
            const double2 ai = Ac[i - 1], bi = Bc[i - 1];
            const double den = ai.x * ai.x + ai.y * ai.y;
            const double2 q = make_double2((bi.x * ai.x + bi.y * ai.y) / den, (bi.y * ai.x - bi.x * ai.y) / den);   // b / a
            const double c = sqrt(1.0 / (1.0 + (q.x * q.x + q.y * q.y)));
            const double2 s = make_double2(c * q.x, -c * q.y);                                                      // conj(c b / a)
            const double theta = atan2(hypot(s.x, s.y), c), psi = atan2(s.y, s.x);
            rf[i - 1] = make_double2(2 * theta * cos(psi), 2 * theta * sin(psi));
            cs[0] = make_double2(c, 0);
            cs[1] = s;
        }
        __syncthreads();
        const double c = cs[0].x;
        const double2 s = cs[1], ms = make_double2(-s.x, s.y);                                                      // -conj(s)
        for (int k = tid; k < i; k += NT) {
            const double2 ak = Ac[k], bk = Bc[k];
            const double2 sb = cmul2(s, bk), msa = cmul2(ms, ak);
            if (k >= 1) An[k - 1] = make_double2(c * ak.x + sb.x, c * ak.y + sb.y);     // ac = acn(2:i)
            if (k < i - 1) Bn[k] = make_double2(msa.x + c * bk.x, msa.y + c * bk.y);    // bc = bcn(1:i-1)
        }
        __syncthreads();
        cur ^= 1;
    }
}

// inverse SLR recursion; a_il / b_il / rf_il interleaved (re, im), which is the double2 layout; n <= SLR_MAXN
constexpr int SLR_MAXN = 2048;
__global__ __launch_bounds__(1024) void k_ab2rf(const double* __restrict__ a_il, const double* __restrict__ b_il, int n,
                                                double* __restrict__ rf_il) {
    __shared__ double2 A[2][SLR_MAXN], B[2][SLR_MAXN];
    __shared__ double2 cs[2];                             // (c, 0), s
    for (int i = threadIdx.x; i < n; i += 1024) {
        A[0][i] = make_double2(a_il[2 * i], a_il[2 * i + 1]);
        B[0][i] = make_double2(b_il[2 * i], b_il[2 * i + 1]);
    }
    __syncthreads();
    ab2rf_recursion<1024>(A[0], B[0], SLR_MAXN, n, cs, reinterpret_cast<double2*>(rf_il));
}

// ------------------------------------------------------------------------------------------------
// Bloch-equation simulation with relaxation: bloch_simulation/blochC.c calcrotmat (:171-236),
// blochsim (:283-418), blochsimfz (:422-512).  One thread per (off-resonance, position) pair -- the reference's
// two outer loops -- and the time loop inside; the per-sample quantities (rotation components of the pulse,
// gradient, interval, E1, E2) are staged through LDS 256 samples at a time.
//   mode bit 0: steady state (propagate A, B with M' = A M + B, then M = (I - A)^-1 B), bit 1: record every sample.
// LDS row of sample t = (rotx, roty, gx, gy, gz (each * gamma * dt), dt * TWOPI, e1, e2); pos3 = (x, y, z) per position.
// Rot3, bloch_rotmat, rot_vec, BLOCH_CH, BLOCH_IN, BlochPulseDev and the host staging (bloch_stage) are in sim_dev.h, which blochgrad.hip
// (the adjoint) shares.

// ------------------------------------------------------------------------------------------------
// Batched simulators: P pulses x S transmit-gain scales in one launch.  Workgroup blockIdx.x -> (pulse, scale, chunk of 256 points)
// through the host-built block table (sim_block_table), the pulses with the most samples first.  Each workgroup stages only its
// own pulse's samples through LDS, 256 at a time, so a thread's bits depend only on its own (pulse, scale, point) and the fixed
// time order.  These are the only forward simulators: the single-pulse calls run them with one pulse at scale 1.0.  Four rules
// fix the bits callers have had since the single-pulse kernels these replaced, and are kept for that reason: a pulse without g
// gets 2 pi / n per sample (and gy = 0 in 2D), the 2D angle is fma(x, gx, y gy), the Bloch rotx is ((-(re s)) gamma) dt, and
// E1 / E2 come from the host's exp.

// One thread per position.  rf (interleaved) is scaled while it is staged; g holds one weight per sample of every pulse (the host
// writes 2 pi / n where a pulse has none).  Output: S x nx per pulse, scale-major.
__global__ __launch_bounds__(256) void k_abr_batch(const double* __restrict__ rf_il, const double* __restrict__ g,
                                                   const double* __restrict__ x, const double* __restrict__ scales,
                                                   const AbrPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                   int mode, double* __restrict__ a_il, double* __restrict__ b_il) {
    __shared__ double2 srf[256];
    __shared__ double sg[256];
    const SimBlock bk = blocks[blockIdx.x];
    const AbrPulseDev P = pulses[bk.pulse];
    const double sc = scales[bk.scale];
    const int n = P.n, i = bk.chunk * 256 + threadIdx.x;
    const double xv = i < P.nx ? x[P.x_off + i] : 0.0;
    double2 a = make_double2(1, 0), b = make_double2(0, 0);
    for (int m0 = 0; m0 < n; m0 += 256) {
        __syncthreads();
        const int mm = m0 + threadIdx.x;
        if (mm < n) {
            const long t = P.r_off + mm;
            srf[threadIdx.x] = make_double2(rf_il[2 * t] * sc, rf_il[2 * t + 1] * sc);
            sg[threadIdx.x] = g[t];
        }
        __syncthreads();
        const int cnt = min(256, n - m0);
        for (int q = 0; q < cnt; ++q) {
            const CayleyKlein ck = abr_step(mode, srf[q], xv * sg[q], a, b);
            a = ck.a; b = ck.b;
        }
    }
    if (i < P.nx) {
        const long o = P.o_off + (long)bk.scale * P.nx + i;
        a_il[2 * o] = a.x; a_il[2 * o + 1] = a.y; b_il[2 * o] = b.x; b_il[2 * o + 1] = b.y;
    }
}

// in[t] = (b1 re, b1 im, gx, gy, gz (each * gamma * dt), dt * TWOPI, e1, e2, dt) per sample of every pulse.  The thread that
// stages sample t forms rotx = ((-(re s)) gamma) dt and roty = ((im s) gamma) dt (blochC.c:332-333, products in this order) for
// the workgroup's scale s, so the LDS tile holds the rows of the pulse b1 s.  m0: (x, y, z) of every (scale, frequency,
// position) block of every pulse; output S x nf x npos x ntout per pulse, scale-major.
__global__ __launch_bounds__(256) void k_bloch_batch(const double* __restrict__ in, const double* __restrict__ df,
                                                     const double* __restrict__ pos3, const double* __restrict__ scales,
                                                     const BlochPulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                     const double* __restrict__ m0, int mode, double* __restrict__ mx,
                                                     double* __restrict__ my, double* __restrict__ mz) {
    __shared__ double sst[BLOCH_CH][8];
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const double sc = scales[bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos;
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 256 + threadIdx.x;
    const bool live = pair < npair;
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    const int ntout = (mode & 2) ? ntime : 1;
    const long blk = (long)bk.scale * npair + pair, o0 = P.o_off + blk * ntout;
    double m[3] = {0, 0, 1};
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
    for (int pass = (mode & 1) ? 0 : 1; pass < 2; ++pass) {
        if (pass == 1 && mode == 1) break;                               // steady state only
        double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, B[3] = {0, 0, 0};
        for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
            __syncthreads();
            const int cnt = min(BLOCH_CH, ntime - t0);
            if ((int)threadIdx.x < cnt) {
                const double* s = in + BLOCH_IN * (P.t_off + t0 + threadIdx.x);
                const double dt = s[8];
                sst[threadIdx.x][0] = ((-(s[0] * sc)) * gamma) * dt;      // rotx of the pulse b1 s
                sst[threadIdx.x][1] = ((s[1] * sc) * gamma) * dt;         // roty
                for (int e = 2; e < 8; ++e) sst[threadIdx.x][e] = s[e];
            }
            __syncthreads();
            if (!live) continue;
            for (int q = 0; q < cnt; ++q) {
                const double* s = sst[q];
                const double rotz = -((s[2] * px + s[3] * py + s[4] * pz) + dfv * s[5]);
                Rot3 R;
                bloch_rotmat(s[0], s[1], rotz, R);
                const double e1 = s[6], e2 = s[7];
                if (pass == 0) {
                    double c[3], o[3];
                    for (int j = 0; j < 3; ++j) {                        // A <- D R A, column by column
                        c[0] = A[3 * j]; c[1] = A[3 * j + 1]; c[2] = A[3 * j + 2];
                        rot_vec(R, c, o);
                        A[3 * j] = e2 * o[0]; A[3 * j + 1] = e2 * o[1]; A[3 * j + 2] = e1 * o[2];
                    }
                    rot_vec(R, B, o);
                    B[0] = e2 * o[0]; B[1] = e2 * o[1]; B[2] = e1 * o[2] + (1 - e1);
                } else {
                    double o[3];
                    rot_vec(R, m, o);
                    m[0] = e2 * o[0]; m[1] = e2 * o[1]; m[2] = e1 * o[2] + (1 - e1);
                    if (mode & 2) { mx[o0 + t0 + q] = m[0]; my[o0 + t0 + q] = m[1]; mz[o0 + t0 + q] = m[2]; }
                }
            }
        }
        if (pass == 0 && live) {
            // M = (I - A)^-1 B by the adjugate (the reference's invmat)
            double K[9];
            for (int e = 0; e < 9; ++e) K[e] = ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0) - A[e];
            const double c00 = K[4] * K[8] - K[7] * K[5], c01 = K[7] * K[2] - K[1] * K[8], c02 = K[1] * K[5] - K[4] * K[2];
            const double det = K[0] * c00 + K[3] * c01 + K[6] * c02;
            const double inv[9] = {c00 / det, c01 / det, c02 / det,
                                   (K[6] * K[5] - K[3] * K[8]) / det, (K[0] * K[8] - K[6] * K[2]) / det, (K[3] * K[2] - K[0] * K[5]) / det,
                                   (K[3] * K[7] - K[6] * K[4]) / det, (K[6] * K[1] - K[0] * K[7]) / det, (K[0] * K[4] - K[3] * K[1]) / det};
            for (int i = 0; i < 3; ++i) m[i] = inv[i] * B[0] + inv[3 + i] * B[1] + inv[6 + i] * B[2];
        }
    }
    if (live && !(mode & 2)) { mx[o0] = m[0]; my[o0] = m[1]; mz[o0] = m[2]; }
}

// work: 3 * 8n double2.  a_il / rf_il: device arrays of 2n doubles (interleaved).
static void slr_b2a_launch(const double* b_re, const double* b_im, int n, double* work, double* a_il, hipStream_t st) {
    const int N = 8 * n;
    double2* B0 = reinterpret_cast<double2*>(work);
    double2* B1 = B0 + N;
    double2* B2 = B1 + N;
    const dim3 g(cdiv(N, 256)), b(256);
    hipLaunchKernelGGL(k_slr_pad, g, b, 0, st, b_re, b_im, n, N, B0);
    hipLaunchKernelGGL(k_dft_any, g, b, 0, st, B0, B1, N, -1, 1.0);              // bf = fft(bcp)
    hipLaunchKernelGGL(k_slr_logmag, dim3(1), dim3(1024), 0, st, B1, N, B2);     // xl
    hipLaunchKernelGGL(k_dft_any, g, b, 0, st, B2, B0, N, -1, 1.0);              // xlf = fft(xl)
    hipLaunchKernelGGL(k_slr_window, g, b, 0, st, B0, N);
    hipLaunchKernelGGL(k_dft_any, g, b, 0, st, B0, B2, N, +1, 1.0 / N);          // xlaf = ifft(xlfp)
    hipLaunchKernelGGL(k_slr_exp, g, b, 0, st, B2, N);                           // afa
    hipLaunchKernelGGL(k_dft_any, g, b, 0, st, B2, B1, N, -1, 1.0 / N);          // aca = fft(afa) / blp
    hipLaunchKernelGGL(k_slr_out, dim3(cdiv(n, 256)), b, 0, st, B1, n, a_il);
}
static void slr_ab2rf_launch(const double* a_il, const double* b_il, int n, double* rf_il, hipStream_t st) {
    if (n > SLR_MAXN) throw HipError("ab2rf: more than 2048 taps");
    hipLaunchKernelGGL(k_ab2rf, dim3(1), dim3(1024), 0, st, a_il, b_il, n, rf_il);
}

// ------------------------------------------------------------------------------------------------
// Batched inverse SLR: count independent polynomials of n taps -> count RF pulses, rf = ab2rf(b2a(b), b) as the launches above
// compute it (b2a.m:15-32 with its 8 n padding and the max|bf| >= 1 rescale, mag2mp.m:21-31, ab2rf.m:14-29), one workgroup per
// polynomial (grid-stride over the batch), all in one launch.  The length-N = 8n transforms are direct, with k_dft_any's twiddles
// (exact sincospi seed at every 256th term, rotation recurrence in between), but only over the terms that can be non-zero:
//   bf   = fft(b, N)                 n inputs, N outputs
//   xlfp = window(fft(xl))           N real inputs, outputs k <= N/2 (the window zeroes the rest)
//   afa  = exp(ifft(xlfp))           N/2 + 1 inputs, N outputs
//   aca  = fft(afa)(0 : n-1) / N     N inputs, n outputs (the only ones b2a.m keeps)
// bf / xl / afa and xlfp live in a per-workgroup global scratch of 2N double2; b, alpha and the ab2rf ping-pong in LDS
// (4 MAXN double2: A0 | B0 | A1 | B1, the DFT input tile borrowing A1 | B1 until the recursion starts).  Every reduction runs in a
// fixed order inside the workgroup, so a pulse's bits depend on neither count nor its place in the batch.
constexpr int B2RF_SEED = 256;

// out(k), k < nout: sum_{j < nin} in[j] exp(sign 2 pi i j k / N), handed to emit(k, acc); tile: NT double2 of LDS
template <int NT, bool REAL, class Emit>
__device__ __forceinline__ void wg_dft(const double2* in, int nin, int N, int nout, int sign, double2* tile, Emit emit) {
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < nout; k0 += NT) {
        const int k = k0 + tid;
        const int kk = k < nout ? k : 0;
        double sw, cw;
        sincospi(2.0 * double(kk) / double(N), &sw, &cw);
        sw *= sign;
        double2 acc = make_double2(0, 0);
        for (int j0 = 0; j0 < nin; j0 += NT) {
            const int cnt = min(NT, nin - j0);
            __syncthreads();
            if (tid < cnt) tile[tid] = in[j0 + tid];
            __syncthreads();
            for (int q0 = 0; q0 < cnt; q0 += B2RF_SEED) {
                const long ph = ((long)kk * (j0 + q0)) % N;          // exact phase of the run's first term
                double s, c;
                sincospi(2.0 * double(ph) / double(N), &s, &c);
                s *= sign;
                const int qe = min(cnt, q0 + B2RF_SEED);
                for (int q = q0; q < qe; ++q) {
                    const double2 v = tile[q];
                    if (REAL) {
                        acc.x += v.x * c;
                        acc.y += v.x * s;
                    } else {
                        acc.x += v.x * c - v.y * s;
                        acc.y += v.x * s + v.y * c;
                    }
                    const double cn = c * cw - s * sw;
                    s = s * cw + c * sw;
                    c = cn;
                }
            }
        }
        if (k < nout) emit(k, acc);
    }
}

// b / rf: count x n double2 (row-major); work: gridDim.x x 2N double2
template <int MAXN, int NT>
__global__ __launch_bounds__(NT) void k_b2rf_batch(const double2* __restrict__ b, int n, int count, double2* __restrict__ work,
                                                   double2* __restrict__ rf) {
    __shared__ double2 L[4 * MAXN];
    __shared__ double red[17];
    __shared__ double2 cs[2];                             // (c, 0), s of the current recursion step
    const int N = 8 * n, tid = threadIdx.x;
    double2* A0 = L;
    double2* B0 = L + MAXN;
    double2* tile = L + 2 * MAXN;                         // NT <= 2 MAXN
    double2* X0 = work + (size_t)blockIdx.x * 2 * N;
    double2* X1 = X0 + N;
    const double invN = 1.0 / N;
    for (int p = blockIdx.x; p < count; p += gridDim.x) {
        __syncthreads();                                  // the previous pulse's recursion is done with L
        for (int i = tid; i < n; i += NT) B0[i] = b[(size_t)p * n + i];
        double m = 0;
        wg_dft<NT, false>(B0, n, N, N, -1, tile, [&](int k, double2 v) {         // bf = fft(bcp)         (b2a.m:22-23)
            X0[k] = v;
            m = fmax(m, hypot(v.x, v.y));
        });
        m = block_max(m, red);
        const double sc = m >= 1.0 ? 1.0 / (1e-8 + m) : 1.0;                    // (b2a.m:25-28)
        for (int k = tid; k < N; k += NT) {                                     // xl (mag2mp.m:24); each k is this thread's own
            const double re = X0[k].x * sc, im = X0[k].y * sc;
            X0[k] = make_double2(log(sqrt(1.0 - (re * re + im * im))), 0.0);
        }
        wg_dft<NT, true>(X0, N, N, N / 2 + 1, -1, tile, [&](int k, double2 v) {  // xlfp               (mag2mp.m:25-29)
            const double g = (k == 0 || k == N / 2) ? 1.0 : 2.0;
            X1[k] = make_double2(g * v.x, g * v.y);
        });
        wg_dft<NT, false>(X1, N / 2 + 1, N, N, +1, tile, [&](int k, double2 v) { // afa = exp(ifft(xlfp)) (mag2mp.m:30-31)
            double s, c;
            sincos(v.y * invN, &s, &c);
            const double e = exp(v.x * invN);
            X0[k] = make_double2(e * c, e * s);
        });
        wg_dft<NT, false>(X0, N, N, n, -1, tile, [&](int k, double2 v) {         // aca(n:-1:1)        (b2a.m:30-32)
            A0[n - 1 - k] = make_double2(v.x * invN, v.y * invN);
        });
        __syncthreads();
        ab2rf_recursion<NT>(A0, B0, 2 * MAXN, n, cs, rf + (size_t)p * n);
    }
}

// The (MAXN, NT) tiers of k_b2rf_batch: f(kernel, NT) for the smallest tier that holds n taps
template <class F>
static auto with_b2rf_tier(int n, F f) {
    if (n <= 128) return f(k_b2rf_batch<128, 256>, 256);
    if (n <= 512) return f(k_b2rf_batch<512, 256>, 256);
    if (n <= 1024) return f(k_b2rf_batch<1024, 512>, 512);
    return f(k_b2rf_batch<2048, 512>, 512);
}
// Sizing, and an enqueue on a caller-owned scratch (no synchronisation).  The grid is what can be resident, which bounds the scratch.
static int b2rf_batch_grid(int device, int n, int count) {
    int ncu = 0, per = 0;
    MBFIR_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    with_b2rf_tier(n, [&](auto kernel, int nt) { MBFIR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, nt, 0)); });
    return std::max(1, std::min(count, std::max(per, 1) * ncu));
}
// work: grid x 2 (8 n) double2
static void b2rf_batch_enqueue(hipStream_t st, int grid, int n, int count, const double2* b, double2* work, double2* rf) {
    with_b2rf_tier(n, [&](auto kernel, int nt) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(nt), 0, st, b, n, count, work, rf); });
    MBFIR_HIP(hipGetLastError());
}

// Host side of mbfir_b2rf_batch (arguments checked): host planes in, host planes out.
void slr_b2rf_batch_run(int device, void* stream, int n, int count, const double* b_re, const double* b_im, double* rf_re,
                        double* rf_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 2 || n > SLR_MAXN || count < 1) throw HipError("b2rf_batch: bad sizes");
    const size_t tot = (size_t)n * count;
    std::vector<double2> h(tot);
    pack_cplx(tot, b_re, b_im, h.data());
    DevBuf db(tot * sizeof(double2)), drf(tot * sizeof(double2));
    MBFIR_HIP(hipMemcpyAsync(db.p, h.data(), tot * sizeof(double2), hipMemcpyHostToDevice, st));
    const int grid = b2rf_batch_grid(device, n, count);
    DevBuf work((size_t)grid * 2 * 8 * n * sizeof(double2));
    b2rf_batch_enqueue(st, grid, n, count, db.as<double2>(), work.as<double2>(), drf.as<double2>());
    MBFIR_HIP(hipMemcpyAsync(h.data(), drf.p, tot * sizeof(double2), hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipStreamSynchronize(st));                  // the buffers are freed on return
    MBFIR_HIP(hipGetLastError());
    unpack_cplx(tot, h.data(), rf_re, rf_im);
}

// ------------------------------------------------------------------------------------------------
// 2D inverse SLR (dzepse.m:39-49) for count complex m x n matrices r (rows: spatial samples, columns: spectral samples), all on one
// stream with the intermediates on the device:
//   stage 1   rn1(q, :) = b2rf(r(q, :))                   k_b2rf_batch, count m polynomials of n taps
//   middle    p2_j = fftcp(s_j, 2m)(m/2 : 3m/2 - 1) / 2m  k_slr2d_mid, s_j(q) = sin(|rn1(q, j)| / 2) exp(-i arg rn1(q, j))
//                                                         (literal: dzepse.m:45's sin(conj(rn1(q, j)) / 2))
//   stage 2   rf2(j, :) = b2rf(p2_j)                      k_b2rf_batch, count n polynomials of m taps
//   rn2(q, j) = conj(rf2(j, q))                            k_slr2d_out
// s is the beta of a hard pulse of angle |theta| about the axis arg theta; for a real theta it is dzepse's sin(conj(theta) / 2).
// dzepse's own stage-1 angles are not real (its spatial profile carries a half-sample phase ramp), and there the two forms differ
// by up to 4e-3 of max|rf|: `literal` selects dzepse's form, for parity with it.

// Middle stage, one workgroup per (matrix, column) w = c n + j (grid-stride).  fftcp pads s with m/2 zeros on each side, so the
// middle m samples of its centred 2m-point DFT are the direct centred sum over the m non-zero inputs:
//   p2_j(r) = 1/2m sum_q s(q) exp(-2 pi i (q - m/2)(r - m/2) / 2m),  q, r = 0 .. m-1.
// The twiddle index (q - m/2)(r - m/2) is reduced mod 2m in exact integer steps; the table holds exp(-i pi p / m) for p < m (one
// sincospi each, in LDS), and p >= m is the negated entry p - m.  The column gather (m loads of stride n) is read once into LDS
// against m^2 complex products; the output row p2_j is written contiguously, which is stage 2's row-major layout.
template <int MAXM, int NT>
__global__ __launch_bounds__(NT) void k_slr2d_mid(const double2* __restrict__ rn1, int m, int n, long total, int literal,
                                                  double2* __restrict__ p2) {
    __shared__ double2 tw[MAXM];
    __shared__ double2 s[MAXM];
    const int tid = threadIdx.x, M2 = 2 * m, half = m / 2;
    for (int p = tid; p < m; p += NT) {
        double sn, cs;
        sincospi(double(p) / double(m), &sn, &cs);
        tw[p] = make_double2(cs, -sn);
    }
    const double inv = 1.0 / double(M2);
    for (long w = blockIdx.x; w < total; w += gridDim.x) {
        const long c = w / n;
        const double2* col = rn1 + (size_t)c * m * n + (w - c * n);
        __syncthreads();                                  // the previous column's sums are done with s
        for (int q = tid; q < m; q += NT) {
            const double2 t = col[(size_t)q * n];
            const double th = hypot(t.x, t.y);
            double2 v = make_double2(0, 0);
            if (literal) {                                    // sin(a + i b) = sin a cosh b + i cos a sinh b, a + i b = conj(t) / 2
                double sa, ca;
                sincos(0.5 * t.x, &sa, &ca);
                v = make_double2(sa * cosh(0.5 * t.y), -(ca * sinh(0.5 * t.y)));
            } else if (th > 0) {
                const double sh = sin(0.5 * th);
                v = make_double2(sh * (t.x / th), -(sh * (t.y / th)));
            }
            s[q] = v;
        }
        __syncthreads();
        double2* out = p2 + (size_t)w * m;
        for (int r = tid; r < m; r += NT) {
            const int b = r - half;                                   // in [-m/2, m/2)
            const int step = b < 0 ? b + M2 : b;                      // b mod 2m
            int ph = (int)((((long)(-half) * b) % M2 + M2) % M2);     // (q - m/2)(r - m/2) mod 2m at q = 0
            double2 acc = make_double2(0, 0);
            for (int q = 0; q < m; ++q) {
                const double2 v = s[q];
                const bool neg = ph >= m;
                const double2 e = tw[neg ? ph - m : ph];
                const double ex = neg ? -e.x : e.x, ey = neg ? -e.y : e.y;
                acc.x += v.x * ex - v.y * ey;
                acc.y += v.x * ey + v.y * ex;
                ph += step;
                if (ph >= M2) ph -= M2;
            }
            out[r] = make_double2(acc.x * inv, acc.y * inv);
        }
    }
}

// rn2(c, q, j) = conj(rf2(c, j, q)): count n x m matrices -> m x n, 32 x 32 tiles through LDS so that both the reads and the
// writes run along rows (grid-stride over the tiles).
__global__ __launch_bounds__(256) void k_slr2d_out(const double2* __restrict__ rf2, int m, int n, long ntile, double2* __restrict__ rn2) {
    __shared__ double2 t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int tm = (m + 31) / 32, tn = (n + 31) / 32;
    for (long w = blockIdx.x; w < ntile; w += gridDim.x) {
        const long c = w / ((long)tm * tn);
        const int rest = (int)(w - c * tm * tn), bj = rest / tm, bq = rest - bj * tm;
        const double2* src = rf2 + (size_t)c * n * m;
        double2* dst = rn2 + (size_t)c * m * n;
        __syncthreads();
        for (int y = ty; y < 32; y += 8) {
            const int j = 32 * bj + y, q = 32 * bq + tx;
            if (j < n && q < m) t[y][tx] = src[(size_t)j * m + q];
        }
        __syncthreads();
        for (int y = ty; y < 32; y += 8) {
            const int q = 32 * bq + y, j = 32 * bj + tx;
            if (q < m && j < n) {
                const double2 v = t[tx][y];
                dst[(size_t)q * n + j] = make_double2(v.x, -v.y);
            }
        }
    }
}

template <int MAXM>
static void slr2d_mid_enqueue(hipStream_t st, const double2* rn1, int m, int n, long total, int literal, double2* p2) {
    const int grid = (int)std::min(total, 1L << 20);
    hipLaunchKernelGGL((k_slr2d_mid<MAXM, 256>), dim3(grid), dim3(256), 0, st, rn1, m, n, total, literal, p2);
    MBFIR_HIP(hipGetLastError());
}

// Host side of mbfir_slr2d_batch (arguments checked): host planes in (count x m x n row-major), host planes out (same layout).
void slr_slr2d_batch_run(int device, void* stream, int m, int n, int count, const double* r_re, const double* r_im, double* out_re,
                         double* out_im, int literal) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 2 || n > SLR_MAXN || m < 2 || m > SLR_MAXN || m % 2 || count < 1 || (long)count * std::max(m, n) > INT32_MAX)
        throw HipError("slr2d_batch: bad sizes");
    const size_t tot = (size_t)m * n * count;
    std::vector<double2> h(tot);
    pack_cplx(tot, r_re, r_im, h.data());
    const int rows1 = count * m, rows2 = count * n;
    const int g1 = b2rf_batch_grid(device, n, rows1), g2 = b2rf_batch_grid(device, m, rows2);
    DevBuf d0(tot * sizeof(double2)), d1(tot * sizeof(double2));
    DevBuf work(std::max((size_t)g1 * 16 * n, (size_t)g2 * 16 * m) * sizeof(double2));
    double2* x0 = d0.as<double2>();
    double2* x1 = d1.as<double2>();
    MBFIR_HIP(hipMemcpyAsync(x0, h.data(), tot * sizeof(double2), hipMemcpyHostToDevice, st));
    b2rf_batch_enqueue(st, g1, n, rows1, x0, work.as<double2>(), x1);                 // rn1: count m rows of n
    if (m <= 128) slr2d_mid_enqueue<128>(st, x1, m, n, rows2, literal, x0);           // p2: count n rows of m
    else if (m <= 512) slr2d_mid_enqueue<512>(st, x1, m, n, rows2, literal, x0);
    else slr2d_mid_enqueue<2048>(st, x1, m, n, rows2, literal, x0);
    b2rf_batch_enqueue(st, g2, m, rows2, x0, work.as<double2>(), x1);                 // rf2: count n rows of m
    const long ntile = (long)count * ((m + 31) / 32) * ((n + 31) / 32);
    hipLaunchKernelGGL(k_slr2d_out, dim3((int)std::min(ntile, 1L << 20)), dim3(256), 0, st, x1, m, n, ntile, x0);
    MBFIR_HIP(hipGetLastError());
    MBFIR_HIP(hipMemcpyAsync(h.data(), x0, tot * sizeof(double2), hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipStreamSynchronize(st));                  // the buffers are freed on return
    MBFIR_HIP(hipGetLastError());
    unpack_cplx(tot, h.data(), out_re, out_im);
}

// 2D forward simulation (abrm.m:39-57), both models: one workgroup per (pulse, scale, chunk of 256 points) through the block table
// of the other batched simulators, one thread per point i = k ny + j at (x_k, y_j).  rf (interleaved) is scaled while it is staged;
// gx / gy hold one weight per sample of every pulse (the host writes 2 pi / n and 0 where a pulse has none).  mode 0 is one rotation
// about (Re rf, Im rf, x gx + y gy) per sample, mode 1 the hard-pulse model with that precession angle.  Output: S x nx x ny per
// pulse, scale-major.  The precession angle is defined as fma(x, gx, y gy): left as x gx + y gy the compiler may fuse the other
// product, and callers' bits would move.
__global__ __launch_bounds__(256) void k_abr2_batch(const double* __restrict__ rf_il, const double* __restrict__ gx,
                                                    const double* __restrict__ gy, const double* __restrict__ x,
                                                    const double* __restrict__ y, const double* __restrict__ scales,
                                                    const Abr2PulseDev* __restrict__ pulses, const SimBlock* __restrict__ blocks,
                                                    int mode, double* __restrict__ a_il, double* __restrict__ b_il) {
    __shared__ double2 srf[256];
    __shared__ double sgx[256], sgy[256];
    const SimBlock bk = blocks[blockIdx.x];
    const Abr2PulseDev P = pulses[bk.pulse];
    const double sc = scales[bk.scale];
    const int n = P.n, ny = P.ny;
    const long i = (long)bk.chunk * 256 + threadIdx.x, tot = (long)P.nx * ny;
    const bool live = i < tot;
    const long kx = live ? i / ny : 0;
    const double xv = x[P.x_off + kx], yv = y[P.y_off + (live ? i - kx * ny : 0)];
    double2 a = make_double2(1, 0), b = make_double2(0, 0);
    for (int m0 = 0; m0 < n; m0 += 256) {
        __syncthreads();
        const int mm = m0 + threadIdx.x;
        if (mm < n) {
            const long t = P.r_off + mm;
            srf[threadIdx.x] = make_double2(rf_il[2 * t] * sc, rf_il[2 * t + 1] * sc);
            sgx[threadIdx.x] = gx[t];
            sgy[threadIdx.x] = gy[t];
        }
        __syncthreads();
        const int cnt = min(256, n - m0);
        for (int q = 0; q < cnt; ++q) {
            const CayleyKlein ck = abr_step(mode, srf[q], fma(xv, sgx[q], yv * sgy[q]), a, b);
            a = ck.a; b = ck.b;
        }
    }
    if (live) {
        const long o = P.o_off + (long)bk.scale * tot + i;
        a_il[2 * o] = a.x; a_il[2 * o + 1] = a.y; b_il[2 * o] = b.x; b_il[2 * o + 1] = b.y;
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_b2a / mbfir_ab2rf / mbfir_b2rf (pulse.h; arguments checked).

void slr_run(int device, void* stream, int n, const double* b_re, const double* b_im, const double* a_in_re, const double* a_in_im,
             double* a_re, double* a_im, double* rf_re, double* rf_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)n;
    DevBuf db(2 * N * 8), dbil(2 * N * 8), da(2 * N * 8), drf(2 * N * 8), dw(a_in_re ? 8 : 48 * N * 8);
    std::vector<double2> h(N);
    MBFIR_HIP(hipMemcpyAsync(db.p, b_re, N * 8, hipMemcpyHostToDevice, st));
    MBFIR_HIP(hipMemcpyAsync(db.as<double>() + N, b_im, N * 8, hipMemcpyHostToDevice, st));
    if (a_in_re) {
        pack_cplx(N, a_in_re, a_in_im, h.data());
        MBFIR_HIP(hipMemcpyAsync(da.p, h.data(), 2 * N * 8, hipMemcpyHostToDevice, st));
        MBFIR_HIP(hipStreamSynchronize(st));
    } else {
        slr_b2a_launch(db.as<double>(), db.as<double>() + N, n, dw.as<double>(), da.as<double>(), st);
    }
    if (a_re) {
        MBFIR_HIP(hipMemcpyAsync(h.data(), da.p, 2 * N * 8, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipStreamSynchronize(st));
        unpack_cplx(N, h.data(), a_re, a_im);
    }
    if (rf_re) {
        std::vector<double2> hb(N);
        pack_cplx(N, b_re, b_im, hb.data());
        MBFIR_HIP(hipMemcpyAsync(dbil.p, hb.data(), 2 * N * 8, hipMemcpyHostToDevice, st));
        slr_ab2rf_launch(da.as<double>(), dbil.as<double>(), n, drf.as<double>(), st);
        MBFIR_HIP(hipMemcpyAsync(h.data(), drf.p, 2 * N * 8, hipMemcpyDeviceToHost, st));
        MBFIR_HIP(hipStreamSynchronize(st));
        unpack_cplx(N, h.data(), rf_re, rf_im);
    }
    MBFIR_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Host side of the forward simulators (mbfir_bloch_batch / mbfir_abr_batch / mbfir_abr2_batch, and mbfir_bloch / mbfir_abr /
// mbfir_abr2 as their batch of one; arguments checked by api.cpp): every input in one staging buffer of 256-byte-aligned sections,
// one upload, one launch, one download.  The staging functions (bloch_stage, abr_stage, abr2_stage) are shared with the derivative
// calls' files, which add their own sections.

long sim_block_table(int npulse, const int* ntime, const long* npoint, int nscale, SimBlock* out) {
    long k = 0;
    for (int p = 0; p < npulse; ++p) k += (npoint[p] + 255) / 256 * nscale;
    if (!out) return k;
    // Longest pulses first: workgroups are handed out roughly in blockIdx order, and a long pulse's workgroups started last would
    // run on alone after the short ones have drained (the longest-processing-time-first rule).
    std::vector<int> order(npulse);
    for (int p = 0; p < npulse; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ntime[a] > ntime[b]; });
    long w = 0;
    for (int p : order) {
        const long nch = (npoint[p] + 255) / 256;
        for (int s = 0; s < nscale; ++s)
            for (long c = 0; c < nch; ++c) out[w++] = SimBlock{p, s, int(c), 0};
    }
    return k;
}

constexpr double TWOPI_REF = 6.283185;                      // blochC.c:6, the reference's truncated constant
void bloch_stage(BlochStaged& B, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                 const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                 const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff, const double* dx,
                 const double* dy, const double* dz, int nscale, const double* scales, int mode, const double* m0x,
                 const double* m0y, const double* m0z) {
    std::vector<BlochPulseDev>& pd = B.pd;
    std::vector<int>& nt = B.ntime;
    std::vector<long>& npair = B.npair;
    pd.resize(npulse);
    nt.resize(npulse);
    npair.resize(npulse);
    long M = 0, O = 0;                                       // m0 blocks, output entries
    for (int p = 0; p < npulse; ++p) {
        const int fg = nfgrid == 1 ? 0 : p, pg = npgrid == 1 ? 0 : p;
        BlochPulseDev& d = pd[p];
        d.t_off = toff[p]; d.f_off = foff[fg]; d.p_off = poff[pg]; d.m_off = M; d.o_off = O;
        d.ntime = nt[p] = int(toff[p + 1] - toff[p]);
        d.nf = int(foff[fg + 1] - foff[fg]);
        d.npos = int(poff[pg + 1] - poff[pg]);
        d.pad = 0;
        d.gamma = gamma[p];
        npair[p] = (long)d.nf * d.npos;
        M += nscale * npair[p];
        O += nscale * npair[p] * ((mode & 2) ? d.ntime : 1);
    }
    B.M = M;
    B.O = O;
    const long T = toff[npulse], F = foff[nfgrid], NP = poff[npgrid];
    Staging& S = B.S;
    const size_t o_in = B.o_in = S.add(T * BLOCH_IN * 8), o_df = B.o_df = S.add(F * 8), o_pos = B.o_pos = S.add(NP * 24),
                 o_m0 = B.o_m0 = S.add(M * 24);
    S.add_tables(npulse, pd.data(), sizeof(BlochPulseDev), nt.data(), npair.data(), nscale, scales);
    double* in = S.at<double>(o_in);
    for (int p = 0; p < npulse; ++p) {
        const bool one = tsoff[p + 1] - tsoff[p] == 1;
        const double g = gamma[p];
        for (long t = toff[p]; t < toff[p + 1]; ++t) {
            const double dt = tsteps[tsoff[p] + (one ? 0 : t - toff[p])];
            double* s = in + BLOCH_IN * t;
            s[0] = b1_re[t];
            s[1] = b1_im[t];
            s[2] = (gx ? gx[t] : 0.0) * g * dt;                 // gradient terms of rotz (blochC.c:317-319, :330)
            s[3] = (gy ? gy[t] : 0.0) * g * dt;
            s[4] = (gz ? gz[t] : 0.0) * g * dt;
            s[5] = TWOPI_REF * dt;
            s[6] = std::exp(-dt / t1[p]);                       // :460-464
            s[7] = std::exp(-dt / t2[p]);
            s[8] = dt;
        }
    }
    std::copy(df, df + F, S.at<double>(o_df));
    double* pos = S.at<double>(o_pos);                       // (x, y, z) per position, a null axis as zeros
    for (long q = 0; q < NP; ++q) {
        pos[3 * q] = dx ? dx[q] : 0.0; pos[3 * q + 1] = dy ? dy[q] : 0.0; pos[3 * q + 2] = dz ? dz[q] : 0.0;
    }
    double* m0 = S.at<double>(o_m0);                         // the initial magnetisation sits at the first sample of each output block
    for (int p = 0; p < npulse; ++p) {
        const long ntout = (mode & 2) ? nt[p] : 1;
        for (long b = 0; b < nscale * npair[p]; ++b) {
            const long o = pd[p].o_off + b * ntout, m = 3 * (pd[p].m_off + b);
            m0[m] = m0x ? m0x[o] : 0.0; m0[m + 1] = m0x ? m0y[o] : 0.0; m0[m + 2] = m0x ? m0z[o] : 1.0;
        }
    }
}

void bloch_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im, const double* gx,
                     const double* gy, const double* gz, const long* tsoff, const double* tsteps, const double* t1, const double* t2,
                     const double* gamma, int nfgrid, const long* foff, const double* df, int npgrid, const long* poff,
                     const double* dx, const double* dy, const double* dz, int nscale, const double* scales, int mode, double* mx,
                     double* my, double* mz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    BlochStaged B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, mode, mx, my, mz);
    Staging& S = B.S;
    const long O = B.O;
    S.upload(3 * (size_t)O * 8, st);
    double* out = S.dev<double>(S.o_out);
    hipLaunchKernelGGL(k_bloch_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(B.o_in), S.dev<const double>(B.o_df),
                       S.dev<const double>(B.o_pos), S.dev<const double>(S.o_sc), S.dev<const BlochPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const double>(B.o_m0), mode, out, out + O, out + 2 * O);
    std::vector<double> h(3 * (size_t)O);
    S.download(h.data(), h.size() * 8, st);
    std::copy(h.begin(), h.begin() + O, mx);
    std::copy(h.begin() + O, h.begin() + 2 * O, my);
    std::copy(h.begin() + 2 * O, h.end(), mz);
}

void abr_stage(AbrStaged& A, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g, int nxgrid,
               const long* xoff, const double* x, int nscale, const double* scales) {
    std::vector<AbrPulseDev> pd(npulse);
    A.ntime.resize(npulse);
    A.npoint.resize(npulse);
    A.O = 0;
    for (int p = 0; p < npulse; ++p) {
        const int xg = nxgrid == 1 ? 0 : p;
        pd[p] = AbrPulseDev{roff[p], xoff[xg], A.O, int(roff[p + 1] - roff[p]), int(xoff[xg + 1] - xoff[xg])};
        A.ntime[p] = pd[p].n;
        A.npoint[p] = pd[p].nx;
        A.O += nscale * A.npoint[p];
    }
    const long R = roff[npulse], X = xoff[nxgrid];
    Staging& S = A.S;
    A.o_rf = S.add(R * 16); A.o_g = S.add(R * 8); A.o_x = S.add(X * 8);
    S.add_tables(npulse, pd.data(), sizeof(AbrPulseDev), A.ntime.data(), A.npoint.data(), nscale, scales);
    pack_cplx(R, rf_re, rf_im, S.at<double2>(A.o_rf));
    double* gw = S.at<double>(A.o_g);
    for (int p = 0; p < npulse; ++p)
        for (long t = roff[p]; t < roff[p + 1]; ++t) gw[t] = g ? g[t] : 2.0 * M_PI / pd[p].n;     // a null g is 2 pi / n per sample
    std::copy(x, x + X, S.at<double>(A.o_x));
}

void abr_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* g,
                   int nxgrid, const long* xoff, const double* x, int nscale, const double* scales, int mode, double* a_re,
                   double* a_im, double* b_re, double* b_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbrStaged A;
    abr_stage(A, npulse, roff, rf_re, rf_im, g, nxgrid, xoff, x, nscale, scales);
    Staging& S = A.S;
    const long O = A.O;                                         // output entries of a (and of b)
    S.upload(4 * (size_t)O * 8, st);
    double2* out = S.dev<double2>(S.o_out);                     // a: O entries, then b: O entries
    hipLaunchKernelGGL(k_abr_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf), S.dev<const double>(A.o_g),
                       S.dev<const double>(A.o_x), S.dev<const double>(S.o_sc), S.dev<const AbrPulseDev>(S.o_pd),
                       S.dev<const SimBlock>(S.o_bk), mode, reinterpret_cast<double*>(out), reinterpret_cast<double*>(out + O));
    std::vector<double2> h(2 * (size_t)O);
    S.download(h.data(), h.size() * 16, st);
    unpack_cplx(O, h.data(), a_re, a_im);
    unpack_cplx(O, h.data() + O, b_re, b_im);
}

void abr2_stage(Abr2Staged& A, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff, const double* y,
                int nscale, const double* scales) {
    std::vector<Abr2PulseDev> pd(npulse);
    A.ntime.resize(npulse);
    A.npoint.resize(npulse);
    A.O = 0;
    for (int p = 0; p < npulse; ++p) {
        const int xg = nxgrid == 1 ? 0 : p, yg = nygrid == 1 ? 0 : p;
        pd[p] = Abr2PulseDev{roff[p], xoff[xg], yoff[yg], A.O, int(roff[p + 1] - roff[p]), int(xoff[xg + 1] - xoff[xg]),
                             int(yoff[yg + 1] - yoff[yg]), 0};
        A.ntime[p] = pd[p].n;
        A.npoint[p] = (long)pd[p].nx * pd[p].ny;
        A.O += nscale * A.npoint[p];
    }
    const long R = roff[npulse], X = xoff[nxgrid], Y = yoff[nygrid];
    Staging& S = A.S;
    A.o_rf = S.add(R * 16); A.o_gx = S.add(R * 8); A.o_gy = S.add(R * 8); A.o_x = S.add(X * 8); A.o_y = S.add(Y * 8);
    S.add_tables(npulse, pd.data(), sizeof(Abr2PulseDev), A.ntime.data(), A.npoint.data(), nscale, scales);
    pack_cplx(R, rf_re, rf_im, S.at<double2>(A.o_rf));
    double* gxw = S.at<double>(A.o_gx);
    double* gyw = S.at<double>(A.o_gy);
    for (int p = 0; p < npulse; ++p)
        for (long t = roff[p]; t < roff[p + 1]; ++t) {
            gxw[t] = gx ? gx[t] : 2.0 * M_PI / pd[p].n;         // a null gx is 2 pi / n per sample, a null gy is 0
            gyw[t] = gy ? gy[t] : 0.0;
        }
    std::copy(x, x + X, S.at<double>(A.o_x));
    std::copy(y, y + Y, S.at<double>(A.o_y));
}

void abr2_batch_run(int device, void* stream, int npulse, const long* roff, const double* rf_re, const double* rf_im, const double* gx,
                    const double* gy, int nxgrid, const long* xoff, const double* x, int nygrid, const long* yoff, const double* y,
                    int nscale, const double* scales, int mode, double* a_re, double* a_im, double* b_re, double* b_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Abr2Staged A;
    abr2_stage(A, npulse, roff, rf_re, rf_im, gx, gy, nxgrid, xoff, x, nygrid, yoff, y, nscale, scales);
    Staging& S = A.S;
    const long O = A.O;                                         // output entries of a (and of b)
    S.upload(4 * (size_t)O * 8, st);
    double2* out = S.dev<double2>(S.o_out);                     // a: O entries, then b: O entries
    hipLaunchKernelGGL(k_abr2_batch, dim3((unsigned)S.nblk), dim3(256), 0, st, S.dev<const double>(A.o_rf), S.dev<const double>(A.o_gx),
                       S.dev<const double>(A.o_gy), S.dev<const double>(A.o_x), S.dev<const double>(A.o_y), S.dev<const double>(S.o_sc),
                       S.dev<const Abr2PulseDev>(S.o_pd), S.dev<const SimBlock>(S.o_bk), mode, reinterpret_cast<double*>(out),
                       reinterpret_cast<double*>(out + O));
    std::vector<double2> h(2 * (size_t)O);
    S.download(h.data(), h.size() * 16, st);
    unpack_cplx(O, h.data(), a_re, a_im);
    unpack_cplx(O, h.data() + O, b_re, b_im);
}

}  // namespace mbfir
