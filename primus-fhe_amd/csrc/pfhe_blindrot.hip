// pfhe_blindrot.hip — the element-wise glue of a batched blind rotation, and the per-ciphertext monomial product.
//
// One step of the blind-rotation (CMUX) loop, per ciphertext e with its own exponent r = exps[e] (mod 2N):
//   D     = X^r * ACC - ACC          CrtGlwe::mul_monic_monomial_assign (glwe/crt.rs:76-114) + sub_element_wise_assign
//   E     = coeff_form(D (x) BSK_i)  CrtGlwe::mul_dcrt_ggsw_to (glwe/crt.rs:200-227) + DcrtGlwe::write_coeff_form
//   ACC  += E                        add_element_wise_assign (macros/mod.rs:410)
// The product is the external product's own launch sequence; everything else of a step is ONE launch of
// blindrot_glue_kernel, which forms ACC' = ACC + E and, for the next step, D' = X^r' * ACC' - ACC'.  The rotated
// source word ACC'[(j - r) mod N] is gathered as ACC + E at that index straight from global memory, so ACC' is written
// to a different buffer than the one it is read from (the caller ping-pongs between two).
// Canonical residues in, canonical residues out; WT = u64 (pfhe_dcrt) or u32 (pfhe_dcrt32) words.
#include "pfhe_capi_internal.hpp"
#include "pfhe_modmath.hpp"
#include "pfhe_rns.hpp"
#include "../../include/pfhe.h"

namespace pfhe {

namespace {

constexpr int kGlueThreads = 256;

// what one launch writes: ACC' (STORE_ACC), and D' (ROT == kRotSub: X^r ACC' - ACC') or X^r ACC' alone (ROT == kRotOnly)
enum GlueRot : int { kRotNone = 0, kRotSub = 1, kRotOnly = 2 };

// One thread per coefficient.  Coefficient i of the flat batch belongs to polynomial p = i >> log_n =
// (element * polys_per_exp + row) * L + limb; element e = p / (polys_per_exp * L) takes exponent exps[e * exp_stride].
// X^r (crt/mul.rs:102-127): out[j] = +-in[(j - r) mod N], the wrapped part negated; r >= N negates the other part.
template <class WT, bool ADD_E, bool STORE_ACC, int ROT>
__global__ __launch_bounds__(kGlueThreads) void blindrot_glue_kernel(const WT *__restrict__ acc, const WT *__restrict__ e_in,
                                                                   WT *__restrict__ acc_out, WT *__restrict__ d_out,
                                                                   const u32 *__restrict__ exps, u32 exp_stride,
                                                                   u32 polys_per_exp, const NttPrime *__restrict__ primes,
                                                                   u32 L, u32 log_n, u64 total) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u32 n = 1u << log_n, mask = n - 1;
    const u64 p = i >> log_n;
    const u64 q = primes[(u32)(p % L)].q;
    const u64 a = ADD_E ? add_mod((u64)acc[i], (u64)e_in[i], q) : (u64)acc[i];
    if constexpr (STORE_ACC) acc_out[i] = (WT)a;
    if constexpr (ROT != kRotNone) {
        const u64 el = p / ((u64)polys_per_exp * L);
        const u32 r = exps[el * exp_stride] & (2 * n - 1);  // the device form takes every exponent modulo 2N
        const bool high = r >= n;
        const u32 rot = high ? r - n : r;
        const u32 j = (u32)(i & mask);
        const u64 src = (i - j) + ((j - rot) & mask);
        const u64 s = ADD_E ? add_mod((u64)acc[src], (u64)e_in[src], q) : (u64)acc[src];
        const u64 x = ((j < rot) != high) ? (s ? q - s : 0) : s;
        d_out[i] = (WT)(ROT == kRotSub ? sub_mod(x, a, q) : x);
    }
}

template <class WT, bool ADD_E, bool STORE_ACC, int ROT>
int launch_glue(const WT *acc, const WT *e_in, WT *acc_out, WT *d_out, const u32 *exps, u32 exp_stride, u32 polys_per_exp,
                const NttPrime *primes, u32 L, u32 log_n, u64 total, hipStream_t s) {
    if (total == 0) return PFHE_OK;
    const u64 grid = (total + kGlueThreads - 1) / kGlueThreads;
    if (grid > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    hipLaunchKernelGGL((blindrot_glue_kernel<WT, ADD_E, STORE_ACC, ROT>), dim3((u32)grid), dim3(kGlueThreads), 0, s, acc, e_in,
                       acc_out, d_out, exps, exp_stride, polys_per_exp, primes, L, log_n, total);
    PFHE_HIP(hipGetLastError());
    return PFHE_OK;
}

}  // namespace

template <class WT>
int blindrot_glue_dev(const TableSet &t, BlindRotGlue mode, const WT *acc, const WT *e_in, WT *acc_out, WT *d_out,
                      const u32 *exps, u32 exp_stride, u32 polys_per_exp, u64 elements, hipStream_t s) {
    const u64 total = elements * polys_per_exp * t.L * t.n;
    switch (mode) {
        case BlindRotGlue::kFirst:
            return launch_glue<WT, false, false, kRotSub>(acc, nullptr, nullptr, d_out, exps, exp_stride, polys_per_exp,
                                                          t.primes_dev, t.L, t.log_n, total, s);
        case BlindRotGlue::kFirstCopy:
            return launch_glue<WT, false, true, kRotSub>(acc, nullptr, acc_out, d_out, exps, exp_stride, polys_per_exp,
                                                         t.primes_dev, t.L, t.log_n, total, s);
        case BlindRotGlue::kStep:
            return launch_glue<WT, true, true, kRotSub>(acc, e_in, acc_out, d_out, exps, exp_stride, polys_per_exp,
                                                        t.primes_dev, t.L, t.log_n, total, s);
        case BlindRotGlue::kLast:
            return launch_glue<WT, true, true, kRotNone>(acc, e_in, acc_out, nullptr, exps, exp_stride, polys_per_exp,
                                                         t.primes_dev, t.L, t.log_n, total, s);
        case BlindRotGlue::kMonomial:
            return launch_glue<WT, false, false, kRotOnly>(acc, nullptr, nullptr, d_out, exps, exp_stride, polys_per_exp,
                                                           t.primes_dev, t.L, t.log_n, total, s);
    }
    return PFHE_ERR_BAD_ARGUMENT;
}
template int blindrot_glue_dev<u64>(const TableSet &, BlindRotGlue, const u64 *, const u64 *, u64 *, u64 *, const u32 *, u32,
                                   u32, u64, hipStream_t);
template int blindrot_glue_dev<u32>(const TableSet &, BlindRotGlue, const u32 *, const u32 *, u32 *, u32 *, const u32 *, u32,
                                   u32, u64, hipStream_t);

}  // namespace pfhe

namespace {

using namespace pfhe;

// X^{exps[e]} * element e for `polys_per_exp` RNS polynomials per element; out must not overlap a (the rotation reads
// a[(j - r) mod N] while other threads write out[j])
template <class WT>
int monomial_each(const TableSet &t, const WT *a, size_t len, const uint32_t *exps, size_t polys_per_exp, WT *out,
                  hipStream_t s) {
    const size_t unit = polys_per_exp * t.L * t.n;
    if (polys_per_exp == 0 || polys_per_exp > 0xffffffffull || len % unit != 0) {
        set_last_error("mul_monomial_each: len must be a whole number of elements of polys_per_exp * L * N words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    if (!a || !exps || !out) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(a);
    PFHE_REQUIRE_ALIGNED(out);
    const uintptr_t a0 = (uintptr_t)a, o0 = (uintptr_t)out, bytes = (uintptr_t)len * sizeof(WT);
    if (a0 < o0 + bytes && o0 < a0 + bytes) {
        set_last_error("mul_monomial_each_to needs non-overlapping buffers");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    DeviceGuard guard(t.device);
    if (!guard.ok) return PFHE_ERR_NO_DEVICE;
    return blindrot_glue_dev<WT>(t, BlindRotGlue::kMonomial, a, nullptr, nullptr, out, exps, 1, (u32)polys_per_exp,
                                 len / unit, s);
}

}  // namespace

extern "C" {

int pfhe_dcrt_mul_monomial_each_to_dev(const pfhe_dcrt *table, const uint64_t *a_dev, size_t len, const uint32_t *exps_dev,
                                       size_t polys_per_exp, uint64_t *out_dev, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table) return PFHE_ERR_BAD_ARGUMENT;
    return monomial_each<u64>(*capi_table_of(table), (const u64 *)a_dev, len, exps_dev, polys_per_exp, (u64 *)out_dev,
                              (hipStream_t)stream);
    PFHE_GUARD_END
}

int pfhe_dcrt32_mul_monomial_each_to_dev(const pfhe_dcrt32 *table, const uint32_t *a_dev, size_t len,
                                         const uint32_t *exps_dev, size_t polys_per_exp, uint32_t *out_dev, void *stream) {
    PFHE_GUARD_BEGIN
    if (!table) return PFHE_ERR_BAD_ARGUMENT;
    return monomial_each<u32>(*capi_table32_of(table), a_dev, len, exps_dev, polys_per_exp, out_dev, (hipStream_t)stream);
    PFHE_GUARD_END
}

}  // extern "C"
