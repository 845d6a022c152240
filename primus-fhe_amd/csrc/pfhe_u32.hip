// pfhe_u32.hip — the u32 / low-q tables: U32NttTable (primus_ntt/src/ntt/prime32/table.rs) and
// U32DcrtTable (primus_ntt/src/dcrt/prime32.rs) behind the C ABI (include/pfhe.h, "u32 tables").
//
// The transforms run the same strided / block kernels as the 64-bit path, instantiated with
// B32Arith (pfhe_ntt_device.hpp): a 64-bit word carries two adjacent u32 coefficients, so a
// polynomial of N coefficients is transformed as N/2 words plus one intra-word stage.  This file
// holds the streaming kernels on u32 data (pointwise products, monomial transforms, synthetic fill)
// with their launchers, and the extern "C" entry points only the u32 tables have.  The entry points
// the four tables share are in pfhe_capi.hip, table construction in pfhe_tables.cpp.
#include <cstdio>

#include "pfhe_capi_internal.hpp"
#include "pfhe_common.hpp"
#include "pfhe_handles.hpp"
#include "pfhe_modmath.hpp"
#include "pfhe_ntt_device.hpp"
#include "pfhe_pointwise.hpp"

namespace pfhe {

namespace {

constexpr int kThreads = 256;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

u32 grid_for(u64 items) {
    u64 g = (items + kThreads - 1) / kThreads;
    const u64 cap = 0x7fffffffull;  // one workgroup per 256 items streams fastest (see pfhe_elementwise.hip)
    if (g > cap) g = cap;
    return (u32)(g ? g : 1);
}

// x mod q for x < 2^62, q < 2^30; bar = floor(2^64 / q).  The estimate floor(x*bar / 2^64) is the
// true quotient or one less.
__device__ __forceinline__ u32 red64(u64 x, u32 q, u64 bar) {
    const u64 r = x - mulhi64(x, bar) * q;
    return (u32)(r >= q ? r - q : r);
}

// MODE 0: acc = acc*b; MODE 1: acc = a*b + acc — BarrettModulus<u32>::reduce_mul / reduce_mul_add
// on every limb (primus_modulus/src/barrett/ops.rs), canonical in and out.
template <int MODE>
__global__ __launch_bounds__(kThreads) void pointwise32_kernel(u32 *acc, const u32 *a, const u32 *__restrict__ b,
                                                               const NttPrime *__restrict__ primes, u32 L, u32 log_n,
                                                               u64 len, u64 len_b) {
    const u64 nvec = len >> 2;
    for (u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (u64)gridDim.x * blockDim.x) {
        const u64 i = v << 2;
        const NttPrime *P = primes + (u32)((i >> log_n) % L);
        const u32 q = (u32)P->q;
        const u64 bar = P->bar_lo;
        const u64 ib = len_b != len ? i % len_b : i;
        const u32x4 x = *reinterpret_cast<const u32x4 *>((MODE == 0 ? acc : a) + i);
        const u32x4 y = *reinterpret_cast<const u32x4 *>(b + ib);
        u32x4 r;
        if constexpr (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = red64((u64)x[e] * y[e], q, bar);
        } else {
            const u32x4 z = *reinterpret_cast<const u32x4 *>(acc + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = red64((u64)x[e] * y[e] + z[e], q, bar);
        }
        *reinterpret_cast<u32x4 *>(acc + i) = r;
    }
}

// scalar form for polynomials shorter than one vector (N < 4)
template <int MODE>
__global__ void pointwise32_small_kernel(u32 *acc, const u32 *a, const u32 *__restrict__ b,
                                         const NttPrime *__restrict__ primes, u32 L, u32 log_n, u64 len, u64 len_b) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (u64)gridDim.x * blockDim.x) {
        const NttPrime *P = primes + (u32)((i >> log_n) % L);
        const u64 x = (u64)(MODE == 0 ? acc : a)[i] * b[len_b != len ? i % len_b : i] + (MODE == 1 ? acc[i] : 0u);
        acc[i] = red64(x, (u32)P->q, P->bar_lo);
    }
}

// NTT of coeff * X^degree (table.rs:376-470): out[i] = coeff * psi^((2*brv(i)+1)*degree mod 2N);
// psi^k for k < N is the low half of the packed forward table at brv(k), psi^(k+N) = -psi^k.
__global__ __launch_bounds__(kThreads) void monomial32_kernel(u32 *__restrict__ out,
                                                              const NttPrime *__restrict__ primes, u32 L, u32 log_n,
                                                              u64 degree, MonomialScalars sc) {
    const u64 n = 1ull << log_n;
    const u64 total = n * L;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) {
        const u32 limb = (u32)(t >> log_n);
        const u32 i = (u32)(t & (n - 1));
        const NttPrime *P = primes + limb;
        const u32 q = (u32)P->q;
        const u32 r = log_n == 0 ? 0u : (__brev(i) >> (32 - log_n));
        const u64 idx = ((2ull * r + 1) * degree) & (2 * n - 1);
        const u32 k = (u32)(idx & (n - 1));
        const u32 kb = log_n == 0 ? 0u : (__brev(k) >> (32 - log_n));
        u32 w = (u32)P->fwd_w[kb];
        if (idx >= n) w = q - w;
        out[t] = red64((u64)w * (u32)sc.value[limb], q, P->bar_lo);
    }
}

__device__ __forceinline__ u64 splitmix64(u64 seed, u64 i) {
    u64 z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(kThreads) void fill_uniform32_kernel(u32 *__restrict__ dst, u64 len,
                                                                  const NttPrime *__restrict__ primes, u32 L,
                                                                  u32 log_n, u64 seed) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (u64)gridDim.x * blockDim.x) {
        const u64 q = primes[(u32)((i >> log_n) % L)].q;
        dst[i] = (u32)mulhi64(splitmix64(seed, i), q);
    }
}

}  // namespace

// The u32 launchers of the tables' host layer (pfhe_handles.hpp); validation is the shared templates' (pfhe_capi.hip).
int launch_pointwise(const TableSet &t, int mode, u32 *acc, const u32 *a, const u32 *b, u64 len, u64 len_b, hipStream_t s) {
    if (t.log_n >= 2) {
        const dim3 grid(grid_for(len / 4)), block(kThreads);
        if (mode == 0) hipLaunchKernelGGL(pointwise32_kernel<0>, grid, block, 0, s, acc, a, b, t.primes_dev, t.L, t.log_n, len, len_b);
        else hipLaunchKernelGGL(pointwise32_kernel<1>, grid, block, 0, s, acc, a, b, t.primes_dev, t.L, t.log_n, len, len_b);
    } else {
        const dim3 grid(grid_for(len)), block(kThreads);
        if (mode == 0) hipLaunchKernelGGL(pointwise32_small_kernel<0>, grid, block, 0, s, acc, a, b, t.primes_dev, t.L, t.log_n, len, len_b);
        else hipLaunchKernelGGL(pointwise32_small_kernel<1>, grid, block, 0, s, acc, a, b, t.primes_dev, t.L, t.log_n, len, len_b);
    }
    PFHE_HIP(hipGetLastError());
    return PFHE_OK;
}

int launch_monomial(u32 *out, const NttPrime *primes, u32 L, u32 log_n, u64 degree, const MonomialScalars &sc, hipStream_t s) {
    hipLaunchKernelGGL(monomial32_kernel, dim3(grid_for((u64)L << log_n)), dim3(kThreads), 0, s, out, primes, L, log_n, degree, sc);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PFHE_OK : hip_fail(e, "monomial transform", __FILE__, __LINE__);
}

}  // namespace pfhe

using namespace pfhe;

extern "C" {

int pfhe_dcrt32_fill_uniform_dev(const pfhe_dcrt32 *table, uint32_t *dst_dev, size_t len, uint64_t seed,
                                 void *stream) {
    PFHE_GUARD_BEGIN
    if (!table || (!dst_dev && len)) return PFHE_ERR_BAD_ARGUMENT;
    if (len == 0) return PFHE_OK;
    const TableSet &t = *table->t;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    hipLaunchKernelGGL(fill_uniform32_kernel, dim3(grid_for(len)), dim3(kThreads), 0, (hipStream_t)stream, dst_dev,
                       (u64)len, t.primes_dev, t.L, t.log_n, seed);
    PFHE_HIP(hipGetLastError());
    return PFHE_OK;
    PFHE_GUARD_END
}

/* profiling hooks: the passes of one transform, as for the 64-bit tables */
int pfhe_dcrt32_transform_num_passes(const pfhe_dcrt32 *table) {
    if (!table) return 0;
    return table->t->log_n <= 4 ? 1 : ntt_num_passes(table->t->log_n - 1, kArithB32);
}
const char *pfhe_dcrt32_transform_pass_name(const pfhe_dcrt32 *table, int inverse, int index) {
    static thread_local char buf[kPassNameCap];
    buf[0] = 0;
    if (!table) return buf;
    if (table->t->log_n <= 4) {
        std::snprintf(buf, sizeof buf, "ntt32_tiny_kernel");
        return buf;
    }
    char inner[96];
    ntt_pass_name(table->t->log_n - 1, inverse != 0, index, inner, sizeof inner, kArithB32);
    std::snprintf(buf, sizeof buf, "u32:%s", inner);
    return buf;
}
int pfhe_dcrt32_transform_form(const pfhe_dcrt32 *table, size_t len, int inverse, char *name, size_t cap, int *launches) {
    if (!table || !name || cap == 0 || !launches) return PFHE_ERR_BAD_ARGUMENT;
    const TableSet &t = *table->t;
    if (len % (t.n * t.L) != 0) return PFHE_ERR_BAD_LENGTH;
    if (t.log_n <= 4) {
        std::snprintf(name, cap, "ntt32_tiny_kernel");
        *launches = 1;
        return PFHE_OK;
    }
    char inner[96];
    *launches = ntt_transform_form(t.L, t.log_n - 1, kArithB32, len / t.n, inverse != 0, t.tune, inner, sizeof inner);
    std::snprintf(name, cap, "u32:%s", inner);
    return PFHE_OK;
}
int pfhe_dcrt32_transform_pass_dev(const pfhe_dcrt32 *table, uint32_t *poly_dev, size_t len, int inverse, int index,
                                   int lazy, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table || (!poly_dev && len)) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(poly_dev);
    const TableSet &t = *table->t;
    if (len % (t.n * t.L) != 0) return PFHE_ERR_BAD_LENGTH;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    if (t.log_n <= 4) {
        if (index != 0) return PFHE_ERR_BAD_ARGUMENT;
        return ntt32_transform_dev(t.primes_dev, t.L, t.log_n, poly_dev, len / t.n, inverse != 0, lazy != 0,
                                   (hipStream_t)stream);
    }
    return ntt_pass_dev(t.primes_dev, t.L, t.log_n - 1, kArithB32, reinterpret_cast<u64 *>(poly_dev), len / t.n,
                        inverse != 0, index, lazy != 0, (hipStream_t)stream);
    PFHE_GUARD_END
}

}  // extern "C"
