// K7: tap extraction of the arbitrary-phase designer -- autocorrelation -> minimum-phase taps by
// FFT spectral factorisation, the device restatement of fir_ap_cvx.m:185-186 (reshape),
// :264-284 (fmp2) and :294-304 (mag2mp).  Three FFTs of length lp = 8*2^ceil(log2(2n-1))
// (<= 65536): one workgroup, in-place radix-2 on global scratch, twiddles by sincospi.
#include "dev_common.h"
#include "pulse.h"

namespace mbfir {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// In-place FFT of length n = 2^logn; sign = -1 forward, +1 inverse (unscaled).
__device__ void fft_inplace(double2* a, int n, int logn, int sign) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < n; i += nt) {
        int j = int(__brev((unsigned)i) >> (32 - logn));
        if (i < j) { double2 t = a[i]; a[i] = a[j]; a[j] = t; }
    }
    __syncthreads();
    for (int s = 1; s <= logn; ++s) {
        const int m = 1 << s, half = m >> 1;
        for (int idx = tid; idx < n / 2; idx += nt) {
            int j = idx & (half - 1);
            int k = (idx >> (s - 1)) << s;
            double sn, cs;
            sincospi(2.0 * double(j) / double(m), &sn, &cs);
            double2 w = make_double2(cs, sign * sn);
            double2 u = a[k + j], t = cmul(w, a[k + j + half]);
            a[k + j] = make_double2(u.x + t.x, u.y + t.y);
            a[k + j + half] = make_double2(u.x - t.x, u.y - t.y);
        }
        __syncthreads();
    }
}

// Stage stores of the test hook (mbfir_test_specfact_stages, include/mbfir.h): where the kDump instantiations leave what the
// chain otherwise overwrites in place.  Each pointer is one lane's block; the production instantiations never touch them.
struct SpecDump {
    double2* hpf;    // lp: B0 as the first transform leaves it
    double* xl;      // lp
    double2* xlfp;   // lp: the windowed transform of xl
    double2* a;      // lp: exp(xlaf)
    double* lift;    // 1: what k_fmp subtracts from real(hpf) (k_specfact: 0)
};

// The chain both kernels share from the spectrum on (mag2mp and the last transform): B0 holds the transform of fftshift(hp),
// m taps leave through hout.  lift is subtracted from real(hpf) before the root (k_specfact: 0, which changes no bit).
template <bool kDump>
__device__ __forceinline__ void cepstral_taps(double2* __restrict__ B0, int lp, int loglp, double lift, int m,
                                              double* __restrict__ hout, const SpecDump& dump) {
    double2* __restrict__ B1 = B0 + lp;
    double2* __restrict__ B2 = B0 + 2 * lp;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int hlp = lp / 2;
    if (kDump) {
        for (int i = tid; i < lp; i += nt) dump.hpf[i] = B0[i];
        if (tid == 0) dump.lift[0] = lift;
    }
    // xl = log(sqrt(abs(hpf)))                                                   :281,296  (fmp.m:20, mag2mp.m)
    for (int i = tid; i < lp; i += nt) {
        const double2 v = B0[(i + hlp) & (lp - 1)];
        const double xl = log(sqrt(hypot(v.x - lift, v.y)));
        B1[i] = make_double2(xl, 0.0);
        if (kDump) dump.xl[i] = xl;
    }
    __syncthreads();
    fft_inplace(B1, lp, loglp, -1);                      // xlf                             :297
    for (int i = tid; i < lp; i += nt) {                 // :298-301  keep DC and lp/2, double the positive, zero the negative
        double2 v = B1[i];
        if (i >= 1 && i < hlp) v = make_double2(2 * v.x, 2 * v.y);
        else if (i > hlp) v = make_double2(0, 0);
        B1[i] = v;
        if (kDump) dump.xlfp[i] = v;
    }
    __syncthreads();
    fft_inplace(B1, lp, loglp, +1);                      // xlaf * lp                        :302
    const double inv = 1.0 / double(lp);
    for (int i = tid; i < lp; i += nt) {                 // a = exp(xlaf)                    :303
        const double2 v = B1[i];
        double e = exp(v.x * inv), sn, cs;
        sincos(v.y * inv, &sn, &cs);
        const double2 a = make_double2(e * cs, e * sn);
        B1[i] = a;
        if (kDump) dump.a[i] = a;
    }
    __syncthreads();
    for (int i = tid; i < lp; i += nt) {                 // fftshift(conj(hpfmp))            :282  (fmp.m:21)
        const double2 v = B1[(i + hlp) & (lp - 1)];
        B2[i] = make_double2(v.x, -v.y);
    }
    __syncthreads();
    fft_inplace(B2, lp, loglp, +1);                      // hpmp = ifft(...)
    for (int i = tid; i < m; i += nt) {                  // hmp = hpmp(1:(l+1)/2)            :283  (fmp.m:22)
        hout[2 * i] = B2[i].x * inv;
        hout[2 * i + 1] = B2[i].y * inv;
    }
}

template <class T>
__device__ __forceinline__ T* lane_ptr(T* p, size_t off) {
    return (T*)((const char*)p + off);
}

// blockIdx.x = design of a lock-step unit: every pointer moves by blockIdx.x * lane_bytes
template <bool kDump>
__global__ __launch_bounds__(1024) void k_specfact(const double* __restrict__ x, int n, int lp, int loglp,
                                                   double2* __restrict__ B0, double* __restrict__ hout, size_t lane_bytes,
                                                   SpecDump dump) {
    {
        const size_t off = (size_t)blockIdx.x * lane_bytes;
        x = lane_ptr(x, off);
        B0 = lane_ptr(B0, off);
        hout = lane_ptr(hout, off);
        if (kDump) {
            dump.hpf = lane_ptr(dump.hpf, off); dump.xl = lane_ptr(dump.xl, off); dump.xlfp = lane_ptr(dump.xlfp, off);
            dump.a = lane_ptr(dump.a, off); dump.lift = lane_ptr(dump.lift, off);
        }
    }
    const int tid = threadIdx.x, nt = blockDim.x;
    const int l = 2 * n - 1;
    const int pad_lo = (lp - l + 1) / 2;                 // ceil((lp-l)/2)            :273
    const int hlp = lp / 2;
    // B0 = fftshift(hp), hp = [zeros r zeros], r two-sided Hermitian              :185-186,273
    for (int i = tid; i < lp; i += nt) {
        int q = (i + hlp) & (lp - 1);                    // index into hp
        int t = q - pad_lo;
        double2 v = make_double2(0, 0);
        if (t >= 0 && t < l) {
            int lag = t - (n - 1);
            int al = lag < 0 ? -lag : lag;
            double re = x[al];
            double im = al == 0 ? 0.0 : x[n - 1 + al];
            v = make_double2(re, lag < 0 ? -im : im);
        }
        B0[i] = v;
    }
    __syncthreads();
    fft_inplace(B0, lp, loglp, -1);                      // hpf = fftshift(B0)               :274
    cepstral_taps<kDump>(B0, lp, loglp, 0.0, n, hout, dump);
}

int specfact_lp(int n) {
    int l = 2 * n - 1, p = 1;
    while (p < l) p <<= 1;                               // 2^ceil(log2(l))                  :272
    return 8 * p;
}

template <bool kDump>
static void specfact_launch_t(const double* x, int n, double* work, double* hout, hipStream_t st, int nlanes, size_t lane_bytes,
                              const SpecDump& dump) {
    int lp = specfact_lp(n), loglp = 0;
    while ((1 << loglp) < lp) ++loglp;
    hipLaunchKernelGGL(k_specfact<kDump>, dim3(nlanes), dim3(1024), 0, st, x, n, lp, loglp, reinterpret_cast<double2*>(work), hout,
                       lane_bytes, dump);
}
void specfact_launch(const double* x, int n, double* work, double* hout, hipStream_t st, int nlanes, size_t lane_bytes) {
    specfact_launch_t<false>(x, n, work, hout, st, nlanes, lane_bytes, SpecDump{});
}

// fmp.m (rf_tools/fmp.m:12-23, called by dzmp.m): an equiripple linear-phase filter h (odd length l <= 2047) -> its minimum-phase
// factor, (l + 1) / 2 taps.  The steps of K7 above from the spectrum on, with two differences: the zero-padded h itself is
// transformed (:16-18), and the spectrum is lifted by its most negative real part before the root (:19,
// hpfs = hpf - 1.000001 min(real(hpf))).  One workgroup, lp = 8 * 2^ceil(log2(l)) <= 16384.
template <bool kDump>
__global__ __launch_bounds__(1024) void k_fmp(const double2* __restrict__ h, int l, int lp, int loglp, double2* __restrict__ B0,
                                              double* __restrict__ hout, SpecDump dump) {
    __shared__ double sred[17];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int pad_lo = (lp - l + 1) / 2;                 // ceil((lp-l)/2)                   :17
    const int hlp = lp / 2;
    for (int i = tid; i < lp; i += nt) {                 // B0 = fftshift(hp)                :17-18
        const int t = ((i + hlp) & (lp - 1)) - pad_lo;
        B0[i] = t >= 0 && t < l ? h[t] : make_double2(0, 0);
    }
    __syncthreads();
    fft_inplace(B0, lp, loglp, -1);                      // hpf = fftshift(B0)               :18
    double mn = INFINITY;                                // min(real(hpf)): exact whatever the order
    for (int i = tid; i < lp; i += nt) mn = fmin(mn, B0[i].x);
    mn = -block_max(-mn, sred);
    const double lift = mn * 1.000001;                   // :19
    cepstral_taps<kDump>(B0, lp, loglp, lift, (l + 1) / 2, hout, dump);
}

static int fmp_lp(int l) {
    int p = 1;
    while (p < l) p <<= 1;                               // 2^ceil(log2(l))                  :16
    return 8 * p;
}

template <bool kDump>
static void fmp_launch(const double* h_il, int l, double* work, double* hout, hipStream_t st, const SpecDump& dump = SpecDump{}) {
    int lp = fmp_lp(l), loglp = 0;
    while ((1 << loglp) < lp) ++loglp;
    hipLaunchKernelGGL(k_fmp<kDump>, dim3(1), dim3(1024), 0, st, reinterpret_cast<const double2*>(h_il), l, lp, loglp,
                       reinterpret_cast<double2*>(work), hout, dump);
}

// Host side of mbfir_fmp (pulse.h; arguments checked).
void fmp_run(int device, void* stream, int l, const double* h_re, const double* h_im, double* out_re, double* out_im) {
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int lp = fmp_lp(l), m = (l + 1) / 2;
    std::vector<double2> h(l), o(m);
    pack_cplx(l, h_re, h_im, h.data());
    DevBuf dh(h.size() * 16), dw(6 * (size_t)lp * 8), dout(o.size() * 16);
    MBFIR_HIP(hipMemcpyAsync(dh.p, h.data(), h.size() * 16, hipMemcpyHostToDevice, st));
    fmp_launch<false>(dh.as<double>(), l, dw.as<double>(), dout.as<double>(), st);
    MBFIR_HIP(hipGetLastError());
    MBFIR_HIP(hipMemcpyAsync(o.data(), dout.p, o.size() * 16, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipStreamSynchronize(st));
    MBFIR_HIP(hipGetLastError());
    unpack_cplx(m, o.data(), out_re, out_im);
}

// Host side of mbfir_test_specfact_stages (include/mbfir.h says what layout holds; arguments checked).  One device arena of nlanes
// lanes, every double of it `fill` before the inputs go in; each block of a lane is followed by at least `guard` doubles nothing
// may write (rounded up so that every block starts on 16 bytes), `extra` more end the lane.  The launch is specfact_launch's /
// fmp_launch's own, through the instantiation that also stores the stages, with the lane stride as the only lane argument.
void specfact_stages_run(int device, void* stream, int kind, int n, int nlanes, const double* in_re, const double* in_im, int guard,
                         double fill, long extra, long* layout, double* raw) {
    const int lp = kind == 0 ? specfact_lp(n) : fmp_lp(n), m = kind == 0 ? n : (n + 1) / 2;
    const long nin = kind == 0 ? 2L * n - 1 : 2L * n;
    const long size[8] = {nin, 6L * lp, 2L * m, 2L * lp, lp, 2L * lp, 2L * lp, 1};   // in, work, h, hpf, xl, xlfp, a, lift
    long off[8], at = 0;
    for (int b = 0; b < 8; ++b) { off[b] = at; at += (size[b] + guard + 1) & ~1L; }
    const long stride = at + ((extra + 1) & ~1L);
    layout[0] = lp; layout[1] = stride;
    for (int b = 0; b < 8; ++b) { layout[2 + b] = off[b]; layout[10 + b] = size[b]; }
    if (!raw) return;
    MBFIR_HIP(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t total = (size_t)nlanes * stride;
    std::vector<double> img(total, fill);
    for (int b = 0; b < nlanes; ++b) {
        double* dst = img.data() + (size_t)b * stride + off[0];
        if (kind == 0) std::copy(in_re + (size_t)b * nin, in_re + (size_t)(b + 1) * nin, dst);
        else pack_cplx(n, in_re, in_im, reinterpret_cast<double2*>(dst));
    }
    DevBuf d(total * 8);
    double* base = d.as<double>();
    MBFIR_HIP(hipMemcpyAsync(base, img.data(), total * 8, hipMemcpyHostToDevice, st));
    const SpecDump dump{reinterpret_cast<double2*>(base + off[3]), base + off[4], reinterpret_cast<double2*>(base + off[5]),
                        reinterpret_cast<double2*>(base + off[6]), base + off[7]};
    if (kind == 0) specfact_launch_t<true>(base + off[0], n, base + off[1], base + off[2], st, nlanes, (size_t)stride * 8, dump);
    else fmp_launch<true>(base + off[0], n, base + off[1], base + off[2], st, dump);
    MBFIR_HIP(hipGetLastError());
    MBFIR_HIP(hipMemcpyAsync(raw, base, total * 8, hipMemcpyDeviceToHost, st));
    MBFIR_HIP(hipStreamSynchronize(st));
    MBFIR_HIP(hipGetLastError());
}

}  // namespace mbfir
