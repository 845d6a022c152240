// pfhe_pack_fft.hip — the packing key switch in the Fourier domain (include/pfhe.h: pfhe_tfhe{,32}_packfft_plan_*,
// _packfft_key_dev, _pack_keyswitch_fft*).  The exact call of pfhe_pack.hip multiplies every digit into a key word; here
// the count digits of one key row (j, l) become ONE real polynomial that meets the row in the Fourier domain:
//     D_{j,l}(X) = sum_{i < count} d_l(a_{e,i,j}) X^i                                 (zero from count on)
//     ACC_c      = sum_j sum_l FFT(D_{j,l}) * Herm(FFT(PKSK[j][l][c]))               c = 0..k
//     out_e      = (0, ..., 0, sum_i b_{e,i} X^i) - IFFT(ACC_c)                       mod 2^BITS, X^N + 1
// which is the external product of pfhe_fft.hip with in_dimension * ell rows instead of (k+1) * ell, on the same device
// code (pfhe_fft_device.hpp): the folded N/2-point transforms, digit_step / init_carry, cmac_fixed and to_torus, thread t
// owning the half-spectrum slots t + 256 u.  Approximate as that product is: f64 rounding, exact while the sums stay
// below 2^53.
//
//   key        the even entries of a real polynomial's spectrum ARE its Hermitian part, so the Fourier packing key is the
//              half spectrum in natural order, in_dimension x ell x (k+1) x N/2 complex values: half the bytes of the
//              reference's full layout and no Hermitian pass per call (tfhe_pack_key_fwd_kernel, one workgroup per
//              key polynomial);
//   accumulate a workgroup owns one group e and one SLICE of kPackFftSlice consecutive mask words, all levels: the slice's
//              words of all count ciphertexts are staged once through LDS (global reads run along j), then row after row
//              the digits, the forward transform and the multiply-accumulate into K1 = k+1 register accumulators per
//              owned slot; the K1 partial half spectra go to plan scratch at [e][slice][c][i];
//   finish     a workgroup per (e, c) adds the slices' partials in ascending slice order, runs the folded inverse and
//              writes b - to_torus(v) with wrapping arithmetic.
// The slice width is a constant of the build, so the order of every sum is fixed by (in_dimension, ell) alone: a group's
// words do not depend on the batch, the chunk or the device, and a call is repeatable.  No atomics.
// Shapes: 1 <= log N <= 11 and 1 <= k <= 3 (the register / LDS form of the fused product); the exact call serves the rest.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// Mask words per slice.  A workgroup's cost is slice * ell transforms against one write of K1 half spectra, and a group
// gives in_dimension / slice workgroups: 4 keeps the partials at 1 / (4 ell) of the key traffic, fills the device from one
// group of 630 words alone (158 workgroups), and keeps the staged words at 4 N words of LDS.
constexpr u32 kPackFftSlice = 4;
constexpr u32 kPackFftMaxK = 3;
constexpr size_t kPackFftDefaultBytes = 256ull << 20;
constexpr size_t kPackFftMaxChunk = 65535;  // a chunk is the y extent of the accumulate grid

struct PackFftShape {
    u32 log_n, k, in_dim, count, log_basis, ell, drop_bits, slices;
};

// bytes of the staged words behind the transform buffer
template <class W>
__host__ __device__ inline size_t packfft_lds_bytes(u32 log_n, u32 count) {
    return lds_bytes(log_n) + (size_t)count * kPackFftSlice * sizeof(W);
}

// ---------------- the key ----------------

// one workgroup per key polynomial: the forward folded transform of the centred words, natural order, N/2 values
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_pack_key_fwd_kernel(const W *__restrict__ pksk, double2 *__restrict__ fkey,
                                                                     const double2 *__restrict__ tw, u32 log_n) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_k[];
    const u32 n = 1u << log_n, m = n >> 1, log_m = log_n - 1;
    const W *x = pksk + (u64)blockIdx.x * n;
    double2 *y = fkey + (u64)blockIdx.x * m;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x)
        lds_k[lpad(i)] = cmul(make_double2(centre(x[i]), centre(x[i + m])), tw[i]);
    __syncthreads();
    fft_dif(lds_k, log_m, log_n, tw);
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) y[i] = lds_k[lpad(bitrev(i, log_m))];
}

// ---------------- slice accumulate ----------------

// grid (slices, groups of the chunk).  tile[i * kPackFftSlice + jj] is mask word j0 + jj of ciphertext i < count; a
// coefficient from count on has the word 0, whose digits and carries are 0.
template <class W, int K1>
__global__ __launch_bounds__(kThreads) void tfhe_packfft_accumulate_kernel(const W *__restrict__ lwe_in,
                                                                           const double2 *__restrict__ fkey,
                                                                           double2 *__restrict__ partial,
                                                                           const double2 *__restrict__ tw, PackFftShape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_a[];
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1;
    W *tile = reinterpret_cast<W *>(reinterpret_cast<char *>(lds_a) + lds_bytes(s.log_n));
    const u32 slice = blockIdx.x;
    const u64 e = blockIdx.y;
    const u32 j0 = slice * kPackFftSlice, jcur = min(kPackFftSlice, s.in_dim - j0);
    const u64 in_stride = (u64)s.in_dim + 1;
    const W *lwe = lwe_in + e * s.count * in_stride + j0;
    // consecutive threads, consecutive mask words of one ciphertext
    for (u32 p = threadIdx.x; p < s.count * jcur; p += kThreads) {
        const u32 i = p / jcur, jj = p - i * jcur;
        tile[i * kPackFftSlice + jj] = lwe[(u64)i * in_stride + jj];
    }
    __syncthreads();

    double2 acc[K1][kFusedPer];
#pragma unroll
    for (int c = 0; c < K1; ++c)
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) acc[c][u] = make_double2(0.0, 0.0);

    for (u32 jj = 0; jj < jcur; ++jj) {
        // bit u of carry0 / carry1: the carry of coefficient i / i + N/2 of slot u, as fused_accumulate_rows keeps them
        u32 carry0 = 0, carry1 = 0;
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            if (i < m) {
                const W lo = i < s.count ? tile[i * kPackFftSlice + jj] : (W)0;
                const W hi = i + m < s.count ? tile[(i + m) * kPackFftSlice + jj] : (W)0;
                carry0 |= init_carry(lo, s.drop_bits) << u;
                carry1 |= init_carry(hi, s.drop_bits) << u;
            }
        }
        for (u32 l = 0; l < s.ell; ++l) {
            const u32 shift = s.drop_bits + l * s.log_basis;
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kThreads;
                if (i < m) {
                    const W lo = i < s.count ? tile[i * kPackFftSlice + jj] : (W)0;
                    const W hi = i + m < s.count ? tile[(i + m) * kPackFftSlice + jj] : (W)0;
                    u32 c0 = (carry0 >> u) & 1, c1 = (carry1 >> u) & 1;
                    const double d0 = digit_step(lo, shift, s.log_basis, c0);
                    const double d1 = digit_step(hi, shift, s.log_basis, c1);
                    carry0 = (carry0 & ~(1u << u)) | (c0 << u);
                    carry1 = (carry1 & ~(1u << u)) | (c1 << u);
                    lds_a[lpad(i)] = cmul(make_double2(d0, d1), tw[i]);
                }
            }
            __syncthreads();
            fft_dif(lds_a, log_m, s.log_n, tw);
            const double2 *kp = fkey + ((u64)(j0 + jj) * s.ell + l) * K1 * m;
#pragma unroll
            for (int u = 0; u < kFusedPer; ++u) {
                const u32 i = threadIdx.x + u * kThreads;
                if (i < m) {
                    const double2 d = lds_a[lpad(bitrev(i, log_m))];
#pragma unroll
                    for (int c = 0; c < K1; ++c) acc[c][u] = cmac_fixed(acc[c][u], d, kp[(u32)c * m + i]);
                }
            }
            __syncthreads();  // the next row overwrites the digit spectrum
        }
    }

    double2 *out = partial + (e * s.slices + slice) * K1 * m;
#pragma unroll
    for (int c = 0; c < K1; ++c)
#pragma unroll
        for (int u = 0; u < kFusedPer; ++u) {
            const u32 i = threadIdx.x + u * kThreads;
            if (i < m) out[(u32)c * m + i] = acc[c][u];
        }
}

// ---------------- reduce and inverse ----------------

// one workgroup per (e, c): the slices' partials in ascending order, the folded inverse, out = [body] - to_torus(v)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_packfft_finish_kernel(const double2 *__restrict__ partial,
                                                                       const W *__restrict__ lwe_in, W *__restrict__ glwe_out,
                                                                       const double2 *__restrict__ tw, PackFftShape s) {
    extern __shared__ __attribute__((aligned(16))) double2 lds_f[];
    const u32 n = 1u << s.log_n, m = n >> 1, log_m = s.log_n - 1, k1 = s.k + 1;
    const u64 e = blockIdx.x / k1;
    const u32 c = blockIdx.x % k1;
    const double2 *p = partial + (e * s.slices * k1 + c) * m;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        double2 a = p[i];
        // the adds stay in ascending order; unrolled so that the loads of several slices are in flight together
#pragma unroll 8
        for (u32 sl = 1; sl < s.slices; ++sl) a = cadd(a, p[(u64)sl * k1 * m + i]);
        lds_f[lpad(bitrev(i, log_m))] = a;
    }
    __syncthreads();
    fft_dit(lds_f, log_m, s.log_n, tw);
    const double scale = 1.0 / (double)m;  // exact: a power of two
    const u64 in_stride = (u64)s.in_dim + 1;
    const W *body = lwe_in + e * s.count * in_stride + s.in_dim;
    W *o = glwe_out + (e * k1 + c) * n;
    const bool is_body = c == s.k;
    for (u32 i = threadIdx.x; i < m; i += blockDim.x) {
        const double2 t = tw[i];
        const double2 v = cmul(lds_f[lpad(i)], make_double2(t.x, -t.y));
        const W b0 = is_body && i < s.count ? body[(u64)i * in_stride] : (W)0;
        const W b1 = is_body && i + m < s.count ? body[(u64)(i + m) * in_stride] : (W)0;
        o[i] = b0 - to_torus<W>(v.x * scale);
        o[i + m] = b1 - to_torus<W>(v.y * scale);
    }
}

}  // namespace
}  // namespace pfhe

// The plan: the shape, and the partial half spectra of `chunk` groups — chunk x slices x (k+1) x N/2 complex values,
// allocated at creation.
template <class W>
struct TfhePackFftCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the plan)
    pfhe::PlanGuard guard;          // one holder at a time, successive calls ordered across streams
    pfhe::Shape shape{};
    size_t in_dim = 0, slices = 0, chunk = 1;
    double2 *partial = nullptr;
    pfhe::DeviceBuffers bufs;
};
struct pfhe_tfhe_packfft_plan : TfhePackFftCore<pfhe::u64> {};
struct pfhe_tfhe32_packfft_plan : TfhePackFftCore<pfhe::u32> {};

namespace {

constexpr const char *kPackFftBusy = "Fourier packing plan in use by another thread (one plan per thread)";

template <class W, int K1>
const void *accumulate_kernel() {
    return reinterpret_cast<const void *>(tfhe_packfft_accumulate_kernel<W, K1>);
}

template <class W, class P>
int packfft_plan_create(const pfhe_fft *fft, size_t k, size_t in_dimension, uint32_t log_basis, size_t decompose_length,
                        size_t chunk, P **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    u32 ell = 0, drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), log_basis, decompose_length, ell, drop));
    if (k > kPackFftMaxK) {
        set_last_error("Fourier packing: glwe_dimension above 3 is not supported (the exact packing key switch serves it)");
        return PFHE_ERR_UNSUPPORTED;
    }
    if (!fft) return PFHE_ERR_BAD_ARGUMENT;
    if (fft->log_n > kFusedMaxLogN) {
        set_last_error("Fourier packing: log N above 11 is not supported (the exact packing key switch serves it)");
        return PFHE_ERR_UNSUPPORTED;
    }
    PFHE_TRY(require_glwe_dimension(k, "Fourier packing: glwe_dimension must be in 1..3 and in_dimension in 1..2^31-2"));
    PFHE_TRY(require_lwe_dimension(in_dimension, "Fourier packing: glwe_dimension must be in 1..3 and in_dimension in 1..2^31-2"));
    auto p = std::make_unique<P>();
    p->shape = Shape{fft->log_n, (u32)k, log_basis, ell, drop};
    p->in_dim = in_dimension;
    p->slices = (in_dimension + kPackFftSlice - 1) / kPackFftSlice;
    const size_t per_group = p->slices * (k + 1) * (fft->n / 2);  // complex values
    p->chunk = chunk ? chunk : std::max<size_t>(1, kPackFftDefaultBytes / (per_group * sizeof(double2)));
    p->chunk = std::min(p->chunk, kPackFftMaxChunk);
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    p->fft = fft;
    // the staged words of a full packing pass 64 KiB of dynamic LDS at u64, N = 2^11
    const size_t lds = packfft_lds_bytes<W>(fft->log_n, (u32)fft->n);
    if (lds > 64 * 1024) {
        for (const void *kern : {accumulate_kernel<W, 2>(), accumulate_kernel<W, 3>(), accumulate_kernel<W, 4>()})
            PFHE_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    p->bufs.bind(fft->device);
    PFHE_TRY(p->bufs.add(p->partial, p->chunk * per_group));
    PFHE_TRY(p->guard.init(fft->device));
    *out = p.release();
    return PFHE_OK;
}

template <class W>
size_t packfft_key_rows(const TfhePackFftCore<W> *p) {
    return p->in_dim * p->shape.ell * (p->shape.k + 1);
}

template <class W>
int packfft_key_dev(TfhePackFftCore<W> *p, const W *pksk, size_t len_pksk, double *fkey, size_t len_fkey, hipStream_t s) {
    if (!p || !p->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(p->guard, kPackFftBusy);
    const pfhe_fft &f = *p->fft;
    const size_t polys = packfft_key_rows(p);
    if (len_pksk != polys * f.n || len_fkey != polys * (f.n / 2)) {
        set_last_error("Fourier packing key: pksk must be in_dimension*ell*(k+1)*N words and fkey in_dimension*ell*(k+1)*N/2 "
                       "complex values");
        return PFHE_ERR_BAD_LENGTH;
    }
    const StageBuf bufs[] = {stage_in(pksk, len_pksk * sizeof(W)), stage_out(fkey, len_fkey * sizeof(double2))};
    return stateless_call(
        f.device, Form::kDevice, bufs, "Fourier packing key: the output must not overlap the input", s,
        [&](void *const *d, hipStream_t st) {
            return launch_groups(tfhe_pack_key_fwd_kernel<W>, polys, lds_bytes(f.log_n), st, (const W *)d[0], (double2 *)d[1], f.tw,
                                 f.log_n);
        },
        [&]() -> int {
            PFHE_REQUIRE_ALIGNED(fkey);
            return PFHE_OK;
        });
}

template <class W>
int packfft_launch(TfhePackFftCore<W> *p, const W *lwe_in, const double2 *fkey, W *glwe_out, u32 count, u64 batch,
                   hipStream_t s) {
    const pfhe_fft &f = *p->fft;
    const Shape &sh = p->shape;
    const PackFftShape ps{sh.log_n, sh.k, (u32)p->in_dim, count, sh.log_basis, sh.ell, sh.drop_bits, (u32)p->slices};
    const u64 in_words = (u64)count * (p->in_dim + 1), out_words = (u64)(sh.k + 1) * f.n;
    const size_t lds = packfft_lds_bytes<W>(sh.log_n, count);
    const auto kernel = sh.k == 1 ? tfhe_packfft_accumulate_kernel<W, 2>
                        : sh.k == 2 ? tfhe_packfft_accumulate_kernel<W, 3>
                                    : tfhe_packfft_accumulate_kernel<W, 4>;
    // chunk after chunk: a chunk's partials are consumed by its finish launch before the next chunk overwrites them
    for (u64 done = 0; done < batch; done += p->chunk) {
        const u32 cur = (u32)std::min<u64>(p->chunk, batch - done);
        const W *x = lwe_in + done * in_words;
        PFHE_TRY(launch_grid(kernel, dim3(ps.slices, cur), lds, s, x, fkey, p->partial, f.tw, ps));
        PFHE_TRY(launch_groups(tfhe_packfft_finish_kernel<W>, (u64)cur * (sh.k + 1), lds_bytes(sh.log_n), s, p->partial, x,
                               glwe_out + done * out_words, f.tw, ps));
    }
    return PFHE_OK;
}

// count, the three lengths, the empty batch, then null pointers and (device form) the overlap: the exact call's order
template <class W>
int packfft_keyswitch(Form form, TfhePackFftCore<W> *p, const W *lwe_in, size_t len_in, size_t count, const double *fkey,
                      size_t len_fkey, W *glwe_out, size_t len_out, hipStream_t s) {
    if (!p || !p->fft) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(p->guard, kPackFftBusy);
    const pfhe_fft &f = *p->fft;
    if (count == 0 || count > f.n) {
        set_last_error("Fourier packing key switch: count must be in 1..N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const size_t group = count * (p->in_dim + 1), glwe = (p->shape.k + 1) * f.n;
    if (len_in % group != 0 || len_fkey != packfft_key_rows(p) * (f.n / 2) || len_out != len_in / group * glwe) {
        set_last_error("Fourier packing key switch: lwe_in must be batch*count*(in_dimension+1) words, fkey "
                       "in_dimension*ell*(k+1)*N/2 complex values and glwe_out batch*(k+1)*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_in == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(fkey, len_fkey * sizeof(double2)),
                             stage_out(glwe_out, len_out * sizeof(W))};
    return stateless_call(
        f.device, form, bufs, "Fourier packing key switch: the output must not overlap an input", s,
        [&](void *const *d, hipStream_t st) {
            return ordered_on(p->guard, st, [&] {
                return packfft_launch<W>(p, (const W *)d[0], (const double2 *)d[1], (W *)d[2], (u32)count, len_in / group, st);
            });
        },
        [&]() -> int {
            if (form == Form::kDevice) PFHE_REQUIRE_ALIGNED(fkey);
            return PFHE_OK;
        });
}

}  // namespace

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_PACKFFT_FAMILY(P, CW, W)                                                                                  \
    PFHE_ENTRY(P##_packfft_plan_create, (const pfhe_fft *fft, size_t glwe_dimension, size_t in_dimension,              \
                uint32_t log_basis, size_t decompose_length, size_t chunk, P##_packfft_plan **out),                    \
               packfft_plan_create<W>(fft, glwe_dimension, in_dimension, log_basis, decompose_length, chunk, out))     \
    PFHE_HANDLE_TRIO(P##_packfft_plan, P##_packfft_plan, h->bufs.bytes())                                              \
    PFHE_ENTRY(P##_packfft_key_dev, (P##_packfft_plan *plan, const CW *pksk_dev, size_t len_pksk, double *fkey_dev,    \
                size_t len_fkey, void *stream),                                                                        \
               packfft_key_dev<W>(plan, (const W *)pksk_dev, len_pksk, fkey_dev, len_fkey, (hipStream_t)stream))       \
    PFHE_ENTRY(P##_pack_keyswitch_fft_dev, (P##_packfft_plan *plan, const CW *lwe_in_dev, size_t len_in, size_t count, \
                const double *fkey_dev, size_t len_fkey, CW *glwe_out_dev, size_t len_out, void *stream),              \
               packfft_keyswitch<W>(Form::kDevice, plan, (const W *)lwe_in_dev, len_in, count, fkey_dev, len_fkey,     \
                                    (W *)glwe_out_dev, len_out, (hipStream_t)stream))                                  \
    PFHE_ENTRY(P##_pack_keyswitch_fft, (P##_packfft_plan *plan, const CW *lwe_in, size_t len_in, size_t count,         \
                const double *fkey, size_t len_fkey, CW *glwe_out, size_t len_out),                                    \
               packfft_keyswitch<W>(Form::kHost, plan, (const W *)lwe_in, len_in, count, fkey, len_fkey,               \
                                    (W *)glwe_out, len_out, nullptr))

extern "C" {

PFHE_PACKFFT_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_PACKFFT_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_PACKFFT_FAMILY

}  // extern "C"
