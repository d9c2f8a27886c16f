// What the batched Cayley-Klein simulators (slr.hip: k_abr_batch, k_abr2_batch), their adjoints (simgrad.hip) and their tangents
// (simjvp.hip) share: the step of the forward model, the helpers of its derivative, the per-pulse descriptors, and the host staging
// of one call.  Moved here from slr.hip and simgrad.hip token for token.
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

}  // namespace mbfir
