// pfhe_fft.hip — torus FFT tables (FullComplex64FftTable) and the TFHE external product in the Fourier domain
// (primus_fft, primus_lattice::tfhe).  include/pfhe.h: pfhe_fft_*, pfhe_tfhe_*, pfhe_tfhe32_*.
//
// Every transform runs at N/2 complex points.  For real x and Y = FFT_N(x_j psi^j), psi = e^{i pi/N}:
//   Y[(1 - k) mod N] = conj(Y[k])                                       (the odd entries are redundant)
//   Y[2m] = FFT_{N/2}((x_m + i x_{m+N/2}) e^{i pi m/N}),  m < N/2       (the folded negacyclic transform)
// The reference's inverse takes Re of the full inverse, which equals the folded inverse of the Hermitian part
// H[2m] = (Y[2m] + conj(Y[(1 - 2m) mod N])) / 2 on any spectrum; the standalone inverse forms H from both entries.
//
// One workgroup per polynomial, the N/2-point transform in LDS: a radix-2 decimation-in-frequency forward (natural in,
// bit-reversed out) and a decimation-in-time inverse (bit-reversed in, natural out), so no permutation pass is needed.
// LDS index i is stored at i + i/16 (one 16-byte slot of padding per 16) to spread the power-of-two strides over banks.
// Twiddles are the host's cis(pi j / N), j < N (complex64/table.rs:76-81, one rounding of the angle): the butterfly of
// span h uses e^{-+2 pi i j / 2h} = cis(-+pi (j N/h) / N).
//
// The external product (tfhe/external_product.rs:36-93): per input row r and level l, the signed digits of
// init_carry_slice + decompose_iter (decompose/primitive/basis.rs, common.rs) go through a forward half transform and
// are multiplied into k+1 half-spectrum accumulators with the key's Hermitian part (K[2m] + conj(K[(1-2m) mod N])) / 2 —
// the digits are real, so Re(ifft(D K)) = ifft(D Herm(K)) for any key — then k+1 folded inverses and the torus wrap.
//   fused   (k = 1, N <= 2^11): one launch, a workgroup per ciphertext; digits, digit spectrum and accumulators on chip
//            (accumulators in registers), the key read from L2;
//   general (every other shape): key Hermitian part, digit transforms, one multiply-accumulate kernel and the batched
//            inverse over plan-owned scratch.
// Summation order is fixed (rows, then levels); no atomics: results do not depend on batch size or chunking.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <vector>

#include "pfhe_capi_internal.hpp"
#include "pfhe_plan_guard.hpp"
#include "pfhe_staging.hpp"

using namespace pfhe;

struct pfhe_fft {
    int device = 0;
    u32 log_n = 0;
    size_t n = 0;
    double2 *tw = nullptr;  // device: cis(pi j / N), j < N
    ~pfhe_fft() {
        if (!tw) return;
        DeviceGuard g(device);
        (void)counted_free(tw);
    }
};

// TfheFftContext<T> + ApproxSignedBasis<T> (power-of-two modulus): the shape of the product and its device scratch.
template <class W>
struct TfhePlanCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the plan)
    PlanGuard guard;                // one holder at a time (&mut TfheFftContext), successive calls ordered across streams
    u32 k = 1, log_basis = 0, ell = 0, drop_bits = 0;
    size_t chunk = 1;
    bool fused = false;
    // general form only: digit spectra (chunk x (k+1) x ell x N/2), accumulators (chunk x (k+1) x N/2) and the key's
    // Hermitian part ((k+1) x ell x (k+1) x N/2), complex f64
    double2 *spec = nullptr, *acc = nullptr, *keyh = nullptr;
    size_t scratch = 0;
    ~TfhePlanCore() {
        if (!fft) return;
        DeviceGuard g(fft->device);
        for (double2 *b : {spec, acc, keyh})
            if (b) (void)counted_free(b);
    }
};
struct pfhe_tfhe_plan : TfhePlanCore<u64> {};
struct pfhe_tfhe32_plan : TfhePlanCore<u32> {};

namespace pfhe {
namespace {

constexpr u32 kMaxLogN = 14;
constexpr int kThreads = 256;
constexpr u32 kFusedMaxLogN = 11;
constexpr int kFusedPer = (1 << (kFusedMaxLogN - 1)) / kThreads;  // half-spectrum slots per thread in the fused kernel

__device__ __forceinline__ u32 lpad(u32 i) { return i + (i >> 4); }
__host__ __device__ inline size_t lds_bytes(u32 log_n) {
    const u32 m = 1u << (log_n - 1);
    return (size_t)(m + (m >> 4) + 1) * sizeof(double2);
}
__device__ __forceinline__ u32 bitrev(u32 i, u32 log_m) { return log_m ? __brev(i) >> (32 - log_m) : 0u; }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// forward, natural order in, bit-reversed out: spans M/2 .. 1, twiddle e^{-2 pi i j / 2h} after the difference
__device__ void fft_dif(double2 *x, u32 log_m, u32 log_n, const double2 *__restrict__ tw) {
    const u32 half = (1u << log_m) >> 1;
    for (u32 lh = log_m; lh-- > 0;) {
        const u32 h = 1u << lh;
        for (u32 b = threadIdx.x; b < half; b += blockDim.x) {
            const u32 j = b & (h - 1);
            const u32 i0 = ((b >> lh) << (lh + 1)) + j, i1 = i0 + h;
            const double2 a = x[lpad(i0)], c = x[lpad(i1)];
            double2 w = tw[j << (log_n - lh)];
            w.y = -w.y;
            x[lpad(i0)] = cadd(a, c);
            x[lpad(i1)] = cmul(csub(a, c), w);
        }
        __syncthreads();
    }
}

// inverse (unscaled), bit-reversed in, natural out: spans 1 .. M/2, twiddle e^{+2 pi i j / 2h} before the sum
__device__ void fft_dit(double2 *x, u32 log_m, u32 log_n, const double2 *__restrict__ tw) {
    const u32 half = (1u << log_m) >> 1;
    for (u32 lh = 0; lh < log_m; ++lh) {
        const u32 h = 1u << lh;
        for (u32 b = threadIdx.x; b < half; b += blockDim.x) {
            const u32 j = b & (h - 1);
            const u32 i0 = ((b >> lh) << (lh + 1)) + j, i1 = i0 + h;
            const double2 a = x[lpad(i0)], c = cmul(x[lpad(i1)], tw[j << (log_n - lh)]);
            x[lpad(i0)] = cadd(a, c);
            x[lpad(i1)] = csub(a, c);
        }
        __syncthreads();
    }
}

// TorusFftValue::into_f64_centered
__device__ __forceinline__ double centre(u32 x) { return (double)(int)x; }
__device__ __forceinline__ double centre(u64 x) { return (double)(long long)x; }

// TorusFftValue::from_f64_wrapping_rounded: round half away from zero, then `as i64 as u32` (saturating at +-2^63) or
// `as i128 as u64` (saturating at +-2^127, otherwise exact mod 2^64); NaN gives 0
template <class W>
__device__ __forceinline__ W to_torus(double v);
template <>
__device__ __forceinline__ u32 to_torus<u32>(double v) {
    const double r = round(v);
    if (r != r) return 0u;
    if (r >= 0x1p63) return 0xffffffffu;
    if (r <= -0x1p63) return 0u;
    return (u32)(u64)(long long)r;
}
template <>
__device__ __forceinline__ u64 to_torus<u64>(double v) {
    const double r = round(v);
    if (r != r) return 0ull;
    if (fabs(r) < 0x1p63) return (u64)(long long)r;
    if (r >= 0x1p127) return ~0ull;
    if (r <= -0x1p127) return 0ull;
    const u64 bits = (u64)__double_as_longlong(r);  // 2^63 <= |r| < 2^127: r = mant * 2^e, 11 <= e < 75
    const int e = (int)((bits >> 52) & 0x7ff) - 1075;
    const u64 mag = e >= 64 ? 0ull : ((bits & 0xfffffffffffffull) | (1ull << 52)) << e;
    return r < 0 ? 0ull - mag : mag;
}

// one OnceSignedDecomposer step (common.rs:219-274) on a power-of-two modulus: the digit as its centred f64 value
template <class W>
__device__ __forceinline__ double digit_step(W v, u32 shift, u32 log_basis, u32 &carry) {
    const W B = (W)1 << log_basis;
    const W temp = ((v >> shift) & (B - 1)) + (W)carry;
    const W cmask = log_basis == 1 ? (W)2 : (B | (B >> 1));
    const bool nc = (temp & cmask) != 0;
    carry = nc ? 1u : 0u;
    if (!nc) return (double)temp;
    return temp > B - 1 ? 0.0 : -(double)(B - temp);  // temp + (2^BITS - B), reinterpreted as signed
}
template <class W>
__device__ __forceinline__ u32 init_carry(W v, u32 drop_bits) {
    return drop_bits ? (u32)((v >> (drop_bits - 1)) & 1) : 0u;
}

struct Shape {
    u32 log_n, k, log_basis, ell, drop_bits;
};

// ---------------- standalone batched transforms ----------------

// forward_torus_slice: count polynomials of N words -> count x N complex (the reference's full layout)
template <class W>
__global__ __launch_bounds__(kThreads) void fft_forward_kernel(const W *__restrict__ in, double2 *__restrict__ out,
                                                               const double2 *__restrict__ tw, u32 log_n) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_f[];
    const u32 n = 1u << log_n, m = n >> 1, log_m = log_n - 1;
    const W *x = in + (size_t)blockIdx.x * n;
    double2 *y = out + (size_t)blockIdx.x * n;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x)
        lds_f[lpad(i)] = cmul(make_double2(centre(x[i]), centre(x[i + m])), tw[i]);
    __syncthreads();
    fft_dif(lds_f, log_m, log_n, tw);
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const double2 v = lds_f[lpad(bitrev(i, log_m))];
        y[2 * i] = v;
        y[(n + 1 - 2 * i) & (n - 1)] = make_double2(v.x, -v.y);
    }
}

// inverse_torus_slice (FULL: count x N complex in the reference's layout, Hermitian part formed here) or the
// product's accumulators (!FULL: count x N/2 half-spectrum values, natural order)
template <class W, bool FULL>
__global__ __launch_bounds__(kThreads) void fft_inverse_kernel(const double2 *__restrict__ in, W *__restrict__ out,
                                                               const double2 *__restrict__ tw, u32 log_n) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_i[];
    const u32 n = 1u << log_n, m = n >> 1, log_m = log_n - 1;
    W *x = out + (size_t)blockIdx.x * n;
    if constexpr (FULL) {
        const double2 *y = in + (size_t)blockIdx.x * n;
        for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
            const double2 a = y[2 * i], b = y[(n + 1 - 2 * i) & (n - 1)];
            lds_i[lpad(bitrev(i, log_m))] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
        }
    } else {
        const double2 *y = in + (size_t)blockIdx.x * m;
        for (u32 i = threadIdx.x; i < m; i += blockDim.x) lds_i[lpad(bitrev(i, log_m))] = y[i];
    }
    __syncthreads();
    fft_dit(lds_i, log_m, log_n, tw);
    const double scale = 1.0 / (double)m;  // exact: a power of two
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const double2 t = tw[i];
        const double2 v = cmul(lds_i[lpad(i)], make_double2(t.x, -t.y));
        x[i] = to_torus<W>(v.x * scale);
        x[i + m] = to_torus<W>(v.y * scale);
    }
}

// ---------------- the general product ----------------

// the key's Hermitian part, natural order: keyh[p][i] = (K[p][2i] + conj(K[p][(1 - 2i) mod N])) / 2
__global__ __launch_bounds__(kThreads) void tfhe_key_herm_kernel(const double2 *__restrict__ key, double2 *__restrict__ keyh,
                                                                 u32 log_n, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, m = n >> 1;
    const u64 p = t >> (log_n - 1);
    const u32 i = (u32)(t & (m - 1));
    const double2 a = key[p * n + 2 * i], b = key[p * n + ((n + 1 - 2 * i) & (n - 1))];
    keyh[t] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
}

// one workgroup per digit polynomial (ciphertext e, row r, level l): its digits (the carry chain from level 0), the
// forward half transform, written in natural order to spec[((e (k+1) + r) ell + l) N/2 + i]
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_digit_fwd_kernel(const W *__restrict__ in, double2 *__restrict__ spec,
                                                                  const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_d[];
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1;
    const u32 lvl = blockIdx.x % s.ell;
    const u64 poly = blockIdx.x / s.ell;  // e * (k+1) + r
    const W *x = in + poly * n;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const W v0 = x[i], v1 = x[i + m];
        u32 c0 = init_carry(v0, s.drop_bits), c1 = init_carry(v1, s.drop_bits);
        double d0 = 0.0, d1 = 0.0;
        for (u32 l = 0; l <= lvl; ++l) {
            const u32 shift = s.drop_bits + l * s.log_basis;
            d0 = digit_step(v0, shift, s.log_basis, c0);
            d1 = digit_step(v1, shift, s.log_basis, c1);
        }
        lds_d[lpad(i)] = cmul(make_double2(d0, d1), tw[i]);
    }
    __syncthreads();
    fft_dif(lds_d, log_m, s.log_n, tw);
    double2 *out = spec + (u64)blockIdx.x * m;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) out[i] = lds_d[lpad(bitrev(i, log_m))];
}

// acc[e][c][i] = sum over r, l (in that order) of spec[e][r][l][i] * keyh[r][l][c][i]
__global__ __launch_bounds__(kThreads) void tfhe_mulacc_kernel(const double2 *__restrict__ spec,
                                                               const double2 *__restrict__ keyh, double2 *__restrict__ acc,
                                                               u32 log_n, u32 k, u32 ell, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 m = 1u << (log_n - 1), rows = k + 1;
    const u32 i = (u32)(t & (m - 1));
    const u64 ec = t >> (log_n - 1);
    const u32 c = (u32)(ec % rows);
    const u64 e = ec / rows;
    const double2 *sp = spec + e * rows * ell * m + i;
    const double2 *kh = keyh + (u64)c * m + i;
    double2 a = make_double2(0.0, 0.0);
    for (u32 rl = 0; rl < rows * ell; ++rl) a = cadd(a, cmul(sp[(u64)rl * m], kh[(u64)rl * rows * m]));
    acc[t] = a;
}

// ---------------- the fused product (k = 1, N <= 2^11) ----------------

// one workgroup per ciphertext.  Thread t owns coefficient pairs (i, i + N/2) and half-spectrum slots i for
// i = t + 256 u; the accumulators of both output rows stay in its registers.  The key is read in natural order (even
// entries and their mirrored odd partners), the digit spectrum from LDS at the bit-reversed position.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_fused_kernel(const W *__restrict__ in, const double2 *__restrict__ key,
                                                              W *__restrict__ out, const double2 *__restrict__ tw, Shape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_p[];
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1;
    const W *x = in + (u64)blockIdx.x * 2 * n;
    W *o = out + (u64)blockIdx.x * 2 * n;
    double2 acc0[kFusedPer], acc1[kFusedPer];
#pragma unroll
    for (int u = 0; u < kFusedPer; ++u) acc0[u] = acc1[u] = make_double2(0.0, 0.0);
    for (u32 r = 0; r < 2; ++r) {
        // the words are re-read at every level (L1 hits) and only the carries stay in registers: bit u of carry0 /
        // carry1 is the carry of coefficient i / i + N/2 of slot u
        const W *xr = x + r * n;
        u32 carry0 = 0, carry1 = 0;
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            if (i < m) {
                carry0 |= init_carry(xr[i], s.drop_bits) << u;
                carry1 |= init_carry(xr[i + m], s.drop_bits) << u;
            }
        }
        for (u32 l = 0; l < s.ell; ++l) {
            const u32 shift = s.drop_bits + l * s.log_basis;
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kThreads;
                if (i < m) {
                    u32 c0 = (carry0 >> u) & 1, c1 = (carry1 >> u) & 1;
                    const double d0 = digit_step(xr[i], shift, s.log_basis, c0);
                    const double d1 = digit_step(xr[i + m], shift, s.log_basis, c1);
                    carry0 = (carry0 & ~(1u << u)) | (c0 << u);
                    carry1 = (carry1 & ~(1u << u)) | (c1 << u);
                    lds_p[lpad(i)] = cmul(make_double2(d0, d1), tw[i]);
                }
            }
            __syncthreads();
            fft_dif(lds_p, log_m, s.log_n, tw);
            const double2 *k0 = key + (u64)((r * s.ell + l) * 2) * n, *k1 = k0 + n;
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kThreads;
                if (i < m) {
                    const double2 d = lds_p[lpad(bitrev(i, log_m))];
                    const u32 j = (n + 1 - 2 * i) & (n - 1);
                    const double2 a0 = k0[2 * i], b0 = k0[j], a1 = k1[2 * i], b1 = k1[j];
                    acc0[u] = cadd(acc0[u], cmul(d, make_double2(0.5 * (a0.x + b0.x), 0.5 * (a0.y - b0.y))));
                    acc1[u] = cadd(acc1[u], cmul(d, make_double2(0.5 * (a1.x + b1.x), 0.5 * (a1.y - b1.y))));
                }
            }
            __syncthreads();  // the next level overwrites the digit spectrum
        }
    }
    const double scale = 1.0 / (double)m;
#pragma unroll
    for (u32 c = 0; c < 2; ++c) {
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            if (i < m) lds_p[lpad(bitrev(i, log_m))] = c ? acc1[u] : acc0[u];
        }
        __syncthreads();
        fft_dit(lds_p, log_m, s.log_n, tw);
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            if (i < m) {
                const double2 t = tw[i];
                const double2 v = cmul(lds_p[lpad(i)], make_double2(t.x, -t.y));
                o[c * n + i] = to_torus<W>(v.x * scale);
                o[c * n + i + m] = to_torus<W>(v.y * scale);
            }
        }
        __syncthreads();  // the second row reuses the buffer
    }
}

}  // namespace
}  // namespace pfhe

namespace {

// kernels with more than 64 KiB of LDS need the attribute once per device (pfhe_fft_create sets it)
template <class W>
int set_lds_attributes(size_t bytes) {
    if (bytes <= 64 * 1024) return PFHE_OK;
    const void *kerns[] = {reinterpret_cast<const void *>(fft_forward_kernel<W>),
                           reinterpret_cast<const void *>(fft_inverse_kernel<W, true>),
                           reinterpret_cast<const void *>(fft_inverse_kernel<W, false>),
                           reinterpret_cast<const void *>(tfhe_digit_fwd_kernel<W>)};
    for (const void *k : kerns) PFHE_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PFHE_OK;
}

template <class W>
int forward_dev(const pfhe_fft *f, const W *in, size_t len_in, double *out, size_t len_out, hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % f->n != 0 || len_out != len_in) {
        set_last_error("fft forward: input must be count*N words and output count*N complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_in == 0) return PFHE_OK;
    if (!in || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(in);
    PFHE_REQUIRE_ALIGNED(out);
    const u64 count = len_in / f->n;
    if (count > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    hipLaunchKernelGGL(fft_forward_kernel<W>, dim3((u32)count), dim3(kThreads), lds_bytes(f->log_n), s, in, (double2 *)out,
                       f->tw, f->log_n);
    PFHE_HIP(hipGetLastError());
    return PFHE_OK;
}

template <class W>
int inverse_dev(const pfhe_fft *f, const double *in, size_t len_in, W *out, size_t len_out, hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % f->n != 0 || len_out != len_in) {
        set_last_error("fft inverse: input must be count*N complex values and output count*N words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_in == 0) return PFHE_OK;
    if (!in || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(in);
    PFHE_REQUIRE_ALIGNED(out);
    const u64 count = len_in / f->n;
    if (count > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    hipLaunchKernelGGL((fft_inverse_kernel<W, true>), dim3((u32)count), dim3(kThreads), lds_bytes(f->log_n), s,
                       (const double2 *)in, out, f->tw, f->log_n);
    PFHE_HIP(hipGetLastError());
    return PFHE_OK;
}

// host forms: staged through the pooled context (in, out are host pointers)
template <class In, class Out, class DevFn>
int host_form(const pfhe_fft *f, const In *in, size_t in_bytes, Out *out, size_t out_bytes, size_t len_in, size_t len_out,
              DevFn dev) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    if ((!in && in_bytes) || (!out && out_bytes)) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in % f->n != 0 || len_out != len_in) return PFHE_ERR_BAD_LENGTH;
    if (len_in == 0) return PFHE_OK;
    DeviceGuard g(f->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    HostStage st(f->device);
    if (!st.ok()) return PFHE_ERR_HIP;
    void *a = nullptr, *b = nullptr;
    PFHE_TRY(st.upload(in, in_bytes, &a));
    PFHE_TRY(st.alloc(out_bytes, &b));
    PFHE_TRY(dev((const In *)a, (Out *)b, st.stream()));
    PFHE_TRY(st.download(out, b, out_bytes));
    return st.finish();
}

// ---------------- plans ----------------

constexpr const char *kPlanBusy = "TFHE product plan in use by another thread (one plan per thread, like &mut TfheFftContext)";

// ApproxSignedBasis::new (basis.rs:47-177) with modulus None: its assert!s become PFHE_ERR_BAD_ARGUMENT (log_basis = BITS
// overflows the basis there too); decompose_length 0 = the full length BITS / log_basis
int basis_shape(u32 bits, u32 log_basis, size_t length, u32 &ell, u32 &drop) {
    if (log_basis == 0 || log_basis >= bits) {
        set_last_error("log_basis must be in 1..BITS-1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const u32 full = bits / log_basis;
    if (length > full) {
        set_last_error("decompose_length exceeds BITS / log_basis");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    ell = length ? (u32)length : full;
    drop = bits - ell * log_basis;
    return PFHE_OK;
}

constexpr size_t kMaxGlweDimension = 64;
constexpr size_t kDefaultScratchBytes = 256ull << 20;

template <class P>
int plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t chunk,
                P **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    using W = typename std::conditional<std::is_same<P, pfhe_tfhe_plan>::value, u64, u32>::type;
    u32 ell = 0, drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), log_basis, decompose_length, ell, drop));
    if (glwe_dimension > kMaxGlweDimension) {
        set_last_error("glwe_dimension above 64 is not supported");
        return PFHE_ERR_UNSUPPORTED;
    }
    if (!fft) return PFHE_ERR_BAD_ARGUMENT;
    auto p = std::make_unique<P>();
    p->k = (u32)glwe_dimension;
    p->log_basis = log_basis;
    p->ell = ell;
    p->drop_bits = drop;
    // the form follows N and k alone
    p->fused = p->k == 1 && fft->log_n <= kFusedMaxLogN;
    const size_t m = fft->n / 2, rows = glwe_dimension + 1;
    const size_t per_ct = p->fused ? 0 : (rows * ell + rows) * m * sizeof(double2);
    p->chunk = chunk ? chunk : (per_ct ? std::max<size_t>(1, kDefaultScratchBytes / per_ct) : 65536);
    p->chunk = std::min<size_t>(p->chunk, p->fused ? 0x7fffffffull : 0x7fffffffull / (rows * ell));
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    p->fft = fft;
    if (!p->fused) {
        const size_t sizes[] = {p->chunk * rows * ell * m, p->chunk * rows * m, rows * ell * rows * m};
        double2 **bufs[] = {&p->spec, &p->acc, &p->keyh};
        for (int i = 0; i < 3; ++i) {
            void *b = nullptr;
            PFHE_HIP(counted_malloc(&b, sizes[i] * sizeof(double2)));
            *bufs[i] = (double2 *)b;
            p->scratch += sizes[i] * sizeof(double2);
        }
    }
    PFHE_TRY(p->guard.init(fft->device));
    *out = p.release();
    return PFHE_OK;
}

template <class W, class P>
int product_impl(P *p, const W *in, const double2 *key, W *out, u64 batch, hipStream_t s) {
    const pfhe_fft &f = *p->fft;
    const u32 rows = p->k + 1, m = (u32)(f.n / 2);
    const Shape sh{f.log_n, p->k, p->log_basis, p->ell, p->drop_bits};
    const size_t glwe = (size_t)rows * f.n;
    if (!p->fused) {
        const u64 kt = (u64)rows * p->ell * rows * m;
        hipLaunchKernelGGL(tfhe_key_herm_kernel, dim3((u32)((kt + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, key,
                           p->keyh, f.log_n, kt);
        PFHE_HIP(hipGetLastError());
    }
    for (u64 done = 0; done < batch; done += p->chunk) {
        const u64 cur = std::min<u64>(p->chunk, batch - done);
        const W *x = in + done * glwe;
        W *o = out + done * glwe;
        if (p->fused) {
            hipLaunchKernelGGL(tfhe_fused_kernel<W>, dim3((u32)cur), dim3(kThreads), lds_bytes(f.log_n), s, x, key, o, f.tw, sh);
            PFHE_HIP(hipGetLastError());
            continue;
        }
        hipLaunchKernelGGL(tfhe_digit_fwd_kernel<W>, dim3((u32)(cur * rows * p->ell)), dim3(kThreads), lds_bytes(f.log_n), s,
                           x, p->spec, f.tw, sh);
        PFHE_HIP(hipGetLastError());
        const u64 at = cur * rows * m;
        hipLaunchKernelGGL(tfhe_mulacc_kernel, dim3((u32)((at + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p->spec,
                           p->keyh, p->acc, f.log_n, p->k, p->ell, at);
        PFHE_HIP(hipGetLastError());
        hipLaunchKernelGGL((fft_inverse_kernel<W, false>), dim3((u32)(cur * rows)), dim3(kThreads), lds_bytes(f.log_n), s,
                           p->acc, o, f.tw, f.log_n);
        PFHE_HIP(hipGetLastError());
    }
    return PFHE_OK;
}

template <class W, class P>
int product_dev(P *p, const W *in, size_t len_in, const double *key, size_t len_key, W *out, size_t len_out,
                hipStream_t s) {
    if (!p || !p->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(p->guard, kPlanBusy);
    const pfhe_fft &f = *p->fft;
    const size_t rows = p->k + 1, glwe = rows * f.n, key_len = rows * p->ell * rows * f.n;
    if (len_in % glwe != 0 || len_out != len_in || len_key != key_len) {
        set_last_error("TFHE external product: input / output must be batch*(k+1)*N words and the key "
                       "(k+1)*ell*(k+1)*N complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_in / glwe;
    if (batch == 0) return PFHE_OK;
    if (!in || !key || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(in);
    PFHE_REQUIRE_ALIGNED(key);
    PFHE_REQUIRE_ALIGNED(out);
    const uintptr_t a0 = (uintptr_t)in, o0 = (uintptr_t)out, bytes = (uintptr_t)len_in * sizeof(W);
    // in place is safe: the fused form reads a ciphertext wholly before its workgroup writes it, the general form reads a
    // chunk's input in the digit launch and writes its output in the inverse launch
    if (a0 < o0 + bytes && o0 < a0 + bytes && a0 != o0) {
        set_last_error("TFHE external product: input and output must be the same buffer or disjoint");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    DeviceGuard g(f.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return ordered_on(p->guard, s, [&] { return product_impl<W>(p, in, (const double2 *)key, out, batch, s); });
}

template <class W, class P>
int product_host(P *p, const W *in, size_t len_in, const double *key, size_t len_key, W *out, size_t len_out) {
    if (!p || !p->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(p->guard, kPlanBusy);
    if ((!in && len_in) || (!key && len_key) || (!out && len_out)) return PFHE_ERR_BAD_ARGUMENT;
    const pfhe_fft &f = *p->fft;
    const size_t rows = p->k + 1, glwe = rows * f.n, key_len = rows * p->ell * rows * f.n;
    if (len_in % glwe != 0 || len_out != len_in || len_key != key_len) return PFHE_ERR_BAD_LENGTH;
    if (len_in == 0) return PFHE_OK;
    DeviceGuard g(f.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    HostStage st(f.device);
    if (!st.ok()) return PFHE_ERR_HIP;
    void *a = nullptr, *k = nullptr, *o = nullptr;
    PFHE_TRY(st.upload(in, len_in * sizeof(W), &a));
    PFHE_TRY(st.upload(key, len_key * 2 * sizeof(double), &k));
    PFHE_TRY(st.alloc(len_out * sizeof(W), &o));
    PFHE_TRY(product_dev<W>(p, (const W *)a, len_in, (const double *)k, len_key, (W *)o, len_out, st.stream()));
    PFHE_TRY(st.download(out, o, len_out * sizeof(W)));
    return st.finish();
}

}  // namespace

extern "C" {

int pfhe_fft_create(uint32_t log_n, int device, pfhe_fft **out) {
    PFHE_GUARD_BEGIN
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (log_n == 0 || log_n > kMaxLogN) {
        set_last_error("FFT tables cover 1 <= log N <= 14 (the N/2-point transform of a polynomial lives in LDS)");
        return PFHE_ERR_UNSUPPORTED;
    }
    PFHE_TRY(capi_check_device(device));
    auto f = std::make_unique<pfhe_fft>();
    f->device = device;
    f->log_n = log_n;
    f->n = (size_t)1 << log_n;
    std::vector<double2> tw(f->n);
    const double nf = (double)f->n;
    for (size_t j = 0; j < f->n; ++j) {
        const double a = M_PI * (double)j / nf;  // Complex64::cis(PI * j as f64 / n_f64)
        tw[j] = make_double2(std::cos(a), std::sin(a));
    }
    DeviceGuard g(device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    void *d = nullptr;
    PFHE_HIP(counted_malloc(&d, f->n * sizeof(double2)));
    f->tw = (double2 *)d;
    PFHE_HIP(hipMemcpy(f->tw, tw.data(), f->n * sizeof(double2), hipMemcpyHostToDevice));
    PFHE_TRY(set_lds_attributes<u64>(lds_bytes(log_n)));
    PFHE_TRY(set_lds_attributes<u32>(lds_bytes(log_n)));
    *out = f.release();
    return PFHE_OK;
    PFHE_GUARD_END
}
void pfhe_fft_destroy(pfhe_fft *fft) { delete fft; }
size_t pfhe_fft_poly_length(const pfhe_fft *fft) { return fft ? fft->n : 0; }
size_t pfhe_fft_fourier_length(const pfhe_fft *fft) { return fft ? fft->n : 0; }

int pfhe_fft_forward_torus_dev(const pfhe_fft *fft, const uint64_t *input_dev, size_t len_input, double *output_dev,
                               size_t len_output, void *stream) {
    PFHE_GUARD_BEGIN
    return forward_dev<u64>(fft, (const u64 *)input_dev, len_input, output_dev, len_output, (hipStream_t)stream);
    PFHE_GUARD_END
}
int pfhe_fft_forward_torus32_dev(const pfhe_fft *fft, const uint32_t *input_dev, size_t len_input, double *output_dev,
                                 size_t len_output, void *stream) {
    PFHE_GUARD_BEGIN
    return forward_dev<u32>(fft, input_dev, len_input, output_dev, len_output, (hipStream_t)stream);
    PFHE_GUARD_END
}
int pfhe_fft_inverse_torus_dev(const pfhe_fft *fft, const double *input_dev, size_t len_input, uint64_t *output_dev,
                               size_t len_output, void *stream) {
    PFHE_GUARD_BEGIN
    return inverse_dev<u64>(fft, input_dev, len_input, (u64 *)output_dev, len_output, (hipStream_t)stream);
    PFHE_GUARD_END
}
int pfhe_fft_inverse_torus32_dev(const pfhe_fft *fft, const double *input_dev, size_t len_input, uint32_t *output_dev,
                                 size_t len_output, void *stream) {
    PFHE_GUARD_BEGIN
    return inverse_dev<u32>(fft, input_dev, len_input, output_dev, len_output, (hipStream_t)stream);
    PFHE_GUARD_END
}

int pfhe_fft_forward_torus_slice(const pfhe_fft *fft, const uint64_t *input, size_t len_input, double *output,
                                 size_t len_output) {
    PFHE_GUARD_BEGIN
    return host_form(fft, input, len_input * 8, output, len_output * 16, len_input, len_output,
                     [&](const uint64_t *a, double *b, hipStream_t s) {
                         return forward_dev<u64>(fft, (const u64 *)a, len_input, b, len_output, s);
                     });
    PFHE_GUARD_END
}
int pfhe_fft_forward_torus32_slice(const pfhe_fft *fft, const uint32_t *input, size_t len_input, double *output,
                                   size_t len_output) {
    PFHE_GUARD_BEGIN
    return host_form(fft, input, len_input * 4, output, len_output * 16, len_input, len_output,
                     [&](const uint32_t *a, double *b, hipStream_t s) {
                         return forward_dev<u32>(fft, a, len_input, b, len_output, s);
                     });
    PFHE_GUARD_END
}
int pfhe_fft_inverse_torus_slice(const pfhe_fft *fft, const double *input, size_t len_input, uint64_t *output,
                                 size_t len_output) {
    PFHE_GUARD_BEGIN
    return host_form(fft, input, len_input * 16, output, len_output * 8, len_input, len_output,
                     [&](const double *a, uint64_t *b, hipStream_t s) {
                         return inverse_dev<u64>(fft, a, len_input, (u64 *)b, len_output, s);
                     });
    PFHE_GUARD_END
}
int pfhe_fft_inverse_torus32_slice(const pfhe_fft *fft, const double *input, size_t len_input, uint32_t *output,
                                   size_t len_output) {
    PFHE_GUARD_BEGIN
    return host_form(fft, input, len_input * 16, output, len_output * 4, len_input, len_output,
                     [&](const double *a, uint32_t *b, hipStream_t s) {
                         return inverse_dev<u32>(fft, a, len_input, b, len_output, s);
                     });
    PFHE_GUARD_END
}

int pfhe_tfhe_plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                          size_t chunk, pfhe_tfhe_plan **out) {
    PFHE_GUARD_BEGIN
    return plan_create(fft, glwe_dimension, log_basis, decompose_length, chunk, out);
    PFHE_GUARD_END
}
void pfhe_tfhe_plan_destroy(pfhe_tfhe_plan *plan) { delete plan; }
int pfhe_tfhe_plan_in_use(const pfhe_tfhe_plan *plan) {
    return plan ? plan->guard.in_use() : 0;
}
size_t pfhe_tfhe_plan_scratch_bytes(const pfhe_tfhe_plan *plan) { return plan ? plan->scratch : 0; }
int pfhe_tfhe_external_product_to_dev(pfhe_tfhe_plan *plan, const uint64_t *input_dev, size_t len_input,
                                      const double *key_dev, size_t len_key, uint64_t *output_dev, size_t len_output,
                                      void *stream) {
    PFHE_GUARD_BEGIN
    return product_dev<u64>(plan, (const u64 *)input_dev, len_input, key_dev, len_key, (u64 *)output_dev, len_output,
                            (hipStream_t)stream);
    PFHE_GUARD_END
}
int pfhe_tfhe_external_product_to(pfhe_tfhe_plan *plan, const uint64_t *input, size_t len_input, const double *key,
                                  size_t len_key, uint64_t *output, size_t len_output) {
    PFHE_GUARD_BEGIN
    return product_host<u64>(plan, (const u64 *)input, len_input, key, len_key, (u64 *)output, len_output);
    PFHE_GUARD_END
}

int pfhe_tfhe32_plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                            size_t chunk, pfhe_tfhe32_plan **out) {
    PFHE_GUARD_BEGIN
    return plan_create(fft, glwe_dimension, log_basis, decompose_length, chunk, out);
    PFHE_GUARD_END
}
void pfhe_tfhe32_plan_destroy(pfhe_tfhe32_plan *plan) { delete plan; }
int pfhe_tfhe32_plan_in_use(const pfhe_tfhe32_plan *plan) {
    return plan ? plan->guard.in_use() : 0;
}
size_t pfhe_tfhe32_plan_scratch_bytes(const pfhe_tfhe32_plan *plan) { return plan ? plan->scratch : 0; }
int pfhe_tfhe32_external_product_to_dev(pfhe_tfhe32_plan *plan, const uint32_t *input_dev, size_t len_input,
                                        const double *key_dev, size_t len_key, uint32_t *output_dev, size_t len_output,
                                        void *stream) {
    PFHE_GUARD_BEGIN
    return product_dev<u32>(plan, input_dev, len_input, key_dev, len_key, output_dev, len_output, (hipStream_t)stream);
    PFHE_GUARD_END
}
int pfhe_tfhe32_external_product_to(pfhe_tfhe32_plan *plan, const uint32_t *input, size_t len_input, const double *key,
                                    size_t len_key, uint32_t *output, size_t len_output) {
    PFHE_GUARD_BEGIN
    return product_host<u32>(plan, input, len_input, key, len_key, output, len_output);
    PFHE_GUARD_END
}

}  // extern "C"
