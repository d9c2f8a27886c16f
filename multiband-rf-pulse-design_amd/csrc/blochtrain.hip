// The echo-by-echo transient of a pulse train: N repetitions of one period of the Bloch simulator with relaxation,
// repetition k played at the RF amplitude gains[k] and the RF phase phi_k, gradients and timing the same every repetition.  One
// period at RF phase 0 is the affine map m -> A m + meq B (k_bloch_batch's pass 0, with the recovery term (1 - e1) scaled by meq), and
// rotating the RF phase by phi conjugates it by a rotation about z, so that with (A_e, B_e) the map of the period's first `echo`
// samples
//     u = Z(+phi_k) m_k,   echo_k = Z(-phi_k) (A_e u + meq B_e),   m_{k+1} = Z(-phi_k) (A u + meq B)
// with Z(th) = [[cos th, -sin th, 0], [sin th, cos th, 0], [0, 0, 1]] (rotx = -Re b1, roty = +Im b1: b1 e^{i phi} turns the axis by
// Z(-phi)).  Two kernels, both one 256-thread workgroup per 256 points and one thread per point, no atomics:
//   k_bloch_train_prop: one sweep over the period's samples per (scale, distinct gain) accumulates (A, B) and snapshots (A_e, B_e);
//   k_bloch_train_run:  per (scale, point) walks the repetitions, about sixty flops each.
// The 24 doubles of a (combination, point) lie plane by plane, [combination][entry][point], so both kernels read and write them
// coalesced.  cos phi_k, sin phi_k, the distinct gains and the products scale x gain are formed on the host in float64: they are
// inputs of the recursion, like E1 and E2.  There is no matrix inverse here and no bit relation to mode 1.  The descriptor, the
// repetition's helpers and the staging are in sim_dev.h, shared with the train's adjoint (blochtrainvjp.hip).
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

// blocks: (pulse, combination, chunk).  ws receives the planes.
__global__ __launch_bounds__(256) void k_bloch_train_prop(const double* __restrict__ in, const double* __restrict__ df,
                                                          const double* __restrict__ pos3, const double* __restrict__ amp,
                                                          const BlochPulseDev* __restrict__ pulses,
                                                          const TrainPulseDev* __restrict__ trains,
                                                          const SimBlock* __restrict__ blocks, double* __restrict__ ws) {
    __shared__ double sst[BLOCH_CH][8];
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const double sc = amp[Tr.a_off + bk.scale], gamma = P.gamma;
    const int ntime = P.ntime, npos = P.npos, echo = Tr.echo;
    const long npair = (long)P.nf * npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;                                       // a thread past the end of the grid sweeps the first point
    const int fi = live ? int(pair / npos) : 0, pi = live ? int(pair - (long)fi * npos) : 0;
    const double dfv = df[P.f_off + fi];
    const double* pp = pos3 + 3 * (P.p_off + pi);
    const double px = pp[0], py = pp[1], pz = pp[2];
    double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, B[3] = {0, 0, 0};
    double Ae[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Be[3] = {0, 0, 0};        // echo = 0: (I, 0)
    for (int t0 = 0; t0 < ntime; t0 += BLOCH_CH) {
        bloch_ss_stage(sst, in, P.t_off, ntime, t0, sc, gamma);
        const int cnt = min(BLOCH_CH, ntime - t0);
        for (int q = 0; q < cnt; ++q) {
            const double* s = sst[q];
            Rot3 R;
            bloch_rotmat(s[0], s[1], bloch_rotz(s, px, py, pz, dfv), R);
            const double e1 = s[6], e2 = s[7];
            double c[3], o[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {                                 // A <- D R A, column by column
                c[0] = A[3 * j]; c[1] = A[3 * j + 1]; c[2] = A[3 * j + 2];
                rot_vec(R, c, o);
                A[3 * j] = e2 * o[0]; A[3 * j + 1] = e2 * o[1]; A[3 * j + 2] = e1 * o[2];
            }
            rot_vec(R, B, o);
            B[0] = e2 * o[0]; B[1] = e2 * o[1]; B[2] = e1 * o[2] + (1 - e1);
            if (t0 + q + 1 == echo) {                                     // uniform over the workgroup
#pragma unroll
                for (int e = 0; e < 9; ++e) Ae[e] = A[e];
                Be[0] = B[0]; Be[1] = B[1]; Be[2] = B[2];
            }
        }
    }
    if (!live) return;
    double* w = ws + Tr.w_off + (long)bk.scale * TRAIN_ENT * npair + pair;
#pragma unroll
    for (int e = 0; e < 9; ++e) w[e * npair] = A[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) w[(9 + e) * npair] = B[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) w[(12 + e) * npair] = Ae[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) w[(21 + e) * npair] = Be[e];
}

// blocks: (pulse, scale, chunk), the forward simulators' table.  rep = (cos phi_k, sin phi_k) and gidx = the gain index of every
// repetition of every pulse, staged through LDS 256 repetitions at a time.  m0 as k_bloch_batch's.  ex / ey / ez (null: not
// wanted): S x ntr x npair per pulse; fx / fy / fz (null: not wanted): m after the last repetition, S x npair per pulse.
__global__ __launch_bounds__(256) void k_bloch_train_run(const double* __restrict__ ws, const double2* __restrict__ rep,
                                                         const int* __restrict__ gidx, const BlochPulseDev* __restrict__ pulses,
                                                         const TrainPulseDev* __restrict__ trains,
                                                         const SimBlock* __restrict__ blocks, const double* __restrict__ m0,
                                                         int demod, double* __restrict__ ex, double* __restrict__ ey,
                                                         double* __restrict__ ez, double* __restrict__ fx, double* __restrict__ fy,
                                                         double* __restrict__ fz) {
    __shared__ double2 scs[256];
    __shared__ int sgi[256];
    const int tid = threadIdx.x;
    const SimBlock bk = blocks[blockIdx.x];
    const BlochPulseDev P = pulses[bk.pulse];
    const TrainPulseDev Tr = trains[bk.pulse];
    const int ntr = Tr.ntr, G = Tr.ngain;
    const double meq = Tr.meq;
    const long npair = (long)P.nf * P.npos, pair = (long)bk.chunk * 256 + tid;
    const bool live = pair < npair;
    const long blk = (long)bk.scale * npair + pair;
    const double* wb = ws + Tr.w_off + (long)bk.scale * G * TRAIN_ENT * npair + (live ? pair : 0);
    double m[3] = {0, 0, 1}, W[TRAIN_ENT];
    if (live) { const double* mi = m0 + 3 * (P.m_off + blk); m[0] = mi[0]; m[1] = mi[1]; m[2] = mi[2]; }
    if (G == 1) {                                                         // one distinct gain: the planes are loaded once
#pragma unroll
        for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wb[e * npair];
    }
    double* eo = ex ? ex + Tr.e_off + (long)bk.scale * ntr * npair + pair : nullptr;
    const long dy = ey - ex, dz = ez - ex;                                // the three planes are laid out alike
    for (int k0 = 0; k0 < ntr; k0 += 256) {
        __syncthreads();
        const int cnt = min(256, ntr - k0);
        if (tid < cnt) { scs[tid] = rep[Tr.r_off + k0 + tid]; sgi[tid] = gidx[Tr.r_off + k0 + tid]; }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const double c = scs[q].x, s = scs[q].y;
            if (G != 1) {
                const double* wg = wb + (long)sgi[q] * TRAIN_ENT * npair;
#pragma unroll
                for (int e = 0; e < TRAIN_ENT; ++e) W[e] = wg[e * npair];
            }
            double e[3], n[3];
            train_zp(c, s, m);                                            // u = Z(+phi) m
            train_affine(W + 12, W + 21, meq, m, e);
            train_affine(W, W + 9, meq, m, n);
            if (!demod) train_zm(c, s, e);
            train_zm(c, s, n);
            m[0] = n[0]; m[1] = n[1]; m[2] = n[2];
            if (eo) {
                double* o = eo + (long)(k0 + q) * npair;
                o[0] = e[0]; o[dy] = e[1]; o[dz] = e[2];
            }
        }
    }
    if (live && fx) {
        const long o = P.o_off + blk;
        fx[o] = m[0]; fy[o] = m[1]; fz[o] = m[2];
    }
}

// ------------------------------------------------------------------------------------------------
// Host side of mbfir_bloch_train_batch and mbfir_bloch_prop_batch (arguments checked by api.cpp): the forward call's staging
// (bloch_stage, mode 0: m0 per (scale, frequency, position)) plus the amplitudes, the train descriptors, the repetition tables and
// the propagator kernel's block table; one upload, the launches, one download.  The output region is the echo planes (3 E), the
// final planes (3 O), then the propagators' planes, which stay on the device unless the caller is mbfir_bloch_prop_batch.
void train_launch_prop(TrainStaged& Ts, hipStream_t st, double* ws, const double* in) {
    Staging& S = Ts.B.S;
    hipLaunchKernelGGL(k_bloch_train_prop, dim3((unsigned)Ts.nprop), dim3(256), 0, st, in ? in : S.dev<const double>(Ts.B.o_in),
                       S.dev<const double>(Ts.B.o_df), S.dev<const double>(Ts.B.o_pos), S.dev<const double>(Ts.o_amp),
                       S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr), S.dev<const SimBlock>(Ts.o_pb), ws);
}

// ntr / echo / meq / ngain per pulse; goff, gains, roff, cosphi, sinphi, gidx may be null for the propagator call (one gain of 1,
// no repetitions).
void train_stage(TrainStaged& Ts, int npulse, int nscale, const double* scales, const int* ntr, const long* roff,
                 const double* cosphi, const double* sinphi, const int* gidx, const long* goff, const double* gains, const int* echo,
                 const double* meq) {
    BlochStaged& B = Ts.B;
    Staging& S = B.S;
    Ts.tr.resize(npulse);
    long ncomb = 0, R = 0;
    std::vector<int> ncmb(npulse);
    for (int p = 0; p < npulse; ++p) {
        const int G = goff ? int(goff[p + 1] - goff[p]) : 1, n = ntr ? ntr[p] : 0;
        Ts.tr[p] = TrainPulseDev{Ts.W, ncomb, R, Ts.E, n, G, echo[p], 0, meq ? meq[p] : 1.0};
        ncmb[p] = nscale * G;
        Ts.W += (long)ncmb[p] * TRAIN_ENT * B.npair[p];
        Ts.E += (long)nscale * n * B.npair[p];
        ncomb += ncmb[p];
        R += n;
        Ts.nprop += (B.npair[p] + 255) / 256 * ncmb[p];
    }
    Ts.o_amp = S.add(ncomb * 8);
    Ts.o_tr = S.add(npulse * sizeof(TrainPulseDev));
    Ts.o_rep = S.add((R ? R : 1) * 16);
    Ts.o_gi = S.add((R ? R : 1) * 4);
    Ts.o_pb = S.add(Ts.nprop * sizeof(SimBlock));
    double* amp = S.at<double>(Ts.o_amp);
    for (int p = 0; p < npulse; ++p)
        for (int s = 0; s < nscale; ++s)
            for (int g = 0; g < Ts.tr[p].ngain; ++g) *amp++ = goff ? scales[s] * gains[goff[p] + g] : scales[s];
    std::copy(Ts.tr.begin(), Ts.tr.end(), S.at<TrainPulseDev>(Ts.o_tr));
    double2* rp = S.at<double2>(Ts.o_rep);
    int* gi = S.at<int>(Ts.o_gi);
    for (long k = 0; k < R; ++k) { rp[k] = make_double2(cosphi[k], sinphi[k]); gi[k] = gidx[k]; }
    // kernel 1's table: the forward table's order (the longest periods first), a pulse's combinations in place of its scales
    const SimBlock* fb = S.at<SimBlock>(S.o_bk);
    SimBlock* pb = S.at<SimBlock>(Ts.o_pb);
    for (long w = 0; w < S.nblk; ++w) {
        if (fb[w].scale != 0 || fb[w].chunk != 0) continue;              // the first workgroup of each pulse, in launch order
        const int p = fb[w].pulse;
        const int nch = int((B.npair[p] + 255) / 256);
        for (int c = 0; c < ncmb[p]; ++c)
            for (int k = 0; k < nch; ++k) *pb++ = SimBlock{p, c, k, 0};
    }
}

void bloch_train_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                           const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                           const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                           int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                           const double* scales, const int* ntr, const long* roff, const double* cosphi, const double* sinphi,
                           const int* gidx, const long* goff, const double* gains, const int* echo, const double* meq, int demod,
                           const double* m0x, const double* m0y, const double* m0z, double* ex, double* ey, double* ez, double* fx,
                           double* fy, double* fz) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, m0x, m0y, m0z);
    train_stage(Ts, npulse, nscale, scales, ntr, roff, cosphi, sinphi, gidx, goff, gains, echo, meq);
    Staging& S = B.S;
    const size_t E = ex ? (size_t)Ts.E : 0, O = fx ? (size_t)B.O : 0;
    S.upload((3 * E + 3 * O + (size_t)Ts.W) * 8, st);
    double* out = S.dev<double>(S.o_out);
    double* pf = out + 3 * E;
    double* ws = pf + 3 * O;
    train_launch_prop(Ts, st, ws);
    hipLaunchKernelGGL(k_bloch_train_run, dim3((unsigned)S.nblk), dim3(256), 0, st, ws, S.dev<const double2>(Ts.o_rep),
                       S.dev<const int>(Ts.o_gi), S.dev<const BlochPulseDev>(S.o_pd), S.dev<const TrainPulseDev>(Ts.o_tr),
                       S.dev<const SimBlock>(S.o_bk), S.dev<const double>(B.o_m0), demod, ex ? out : nullptr,
                       ex ? out + E : nullptr, ex ? out + 2 * E : nullptr, fx ? pf : nullptr, fx ? pf + O : nullptr,
                       fx ? pf + 2 * O : nullptr);
    std::vector<double> h(3 * E + 3 * O);
    S.download(h.data(), h.size() * 8, st);
    if (ex) {
        std::copy(h.begin(), h.begin() + E, ex);
        std::copy(h.begin() + E, h.begin() + 2 * E, ey);
        std::copy(h.begin() + 2 * E, h.begin() + 3 * E, ez);
    }
    if (fx) {
        const double* hf = h.data() + 3 * E;
        std::copy(hf, hf + O, fx);
        std::copy(hf + O, hf + 2 * O, fy);
        std::copy(hf + 2 * O, hf + 3 * O, fz);
    }
}

void bloch_prop_batch_run(int device, void* stream, int npulse, const long* toff, const double* b1_re, const double* b1_im,
                          const double* gx, const double* gy, const double* gz, const long* tsoff, const double* tsteps,
                          const double* t1, const double* t2, const double* gamma, int nfgrid, const long* foff, const double* df,
                          int npgrid, const long* poff, const double* dx, const double* dy, const double* dz, int nscale,
                          const double* scales, const int* echo, double* a, double* b, double* ae, double* be) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainStaged Ts;
    BlochStaged& B = Ts.B;
    bloch_stage(B, npulse, toff, b1_re, b1_im, gx, gy, gz, tsoff, tsteps, t1, t2, gamma, nfgrid, foff, df, npgrid, poff, dx, dy, dz,
                nscale, scales, 0, nullptr, nullptr, nullptr);
    train_stage(Ts, npulse, nscale, scales, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, echo, nullptr);
    Staging& S = B.S;
    S.upload((size_t)Ts.W * 8, st);
    train_launch_prop(Ts, st, S.dev<double>(S.o_out));
    std::vector<double> h((size_t)Ts.W);
    S.download(h.data(), h.size() * 8, st);
    // planes [scale][entry][point] of pulse p -> a / ae (9) and b / be (3) per (scale, point), pulse p from its mode-0 offset
    for (int p = 0; p < npulse; ++p) {
        const long np = B.npair[p], o_off = B.pd[p].o_off;
        for (int s = 0; s < nscale; ++s) {
            const double* w = h.data() + Ts.tr[p].w_off + (long)s * TRAIN_ENT * np;
            for (long q = 0; q < np; ++q) {
                const long o = o_off + (long)s * np + q;
                for (int e = 0; e < 9; ++e) { a[9 * o + e] = w[e * np + q]; ae[9 * o + e] = w[(12 + e) * np + q]; }
                for (int e = 0; e < 3; ++e) { b[3 * o + e] = w[(9 + e) * np + q]; be[3 * o + e] = w[(21 + e) * np + q]; }
            }
        }
    }
}

}  // namespace mbfir
