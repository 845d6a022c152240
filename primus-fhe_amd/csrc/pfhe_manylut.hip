// pfhe_manylut.hip — the three exact steps that let ONE blind rotation serve several look-ups (many-LUT), and the strided
// modulus switch's entry point (include/pfhe.h: pfhe_tfhe{,32}_modswitch_stride_dev).  The bootstrap handle
// (pfhe_bootstrap.hip, log_luts) and the circuit bootstrap handle (pfhe_cbs.hip, shared_rotation) queue them through the
// launches declared in pfhe_tfhe_handles.hpp.  Each generalises a kernel of one of those files, which stays as it is:
//
//   strided modulus switch    switch_rounded (pfhe_tfhe_exact_device.hpp) at stride 2^v, reduced modulo 2N: round(w 2N /
//                             2^v / 2^BITS) with ties up, times 2^v.  v = 0 is what tfhe_modswitch_kernel writes; with
//                             body_offset = 2^(BITS-2) it is what tfhe_cbs_modswitch_kernel writes, the exponents of an
//                             input written once.
//   patterned accumulator     ACC_e = X^{neg_b[e]} TV, TV the trivial GLWE whose body coefficient c is -g_{c mod 2^v}/2 for
//                             c mod 2^v < levels and 0 otherwise, written from constants with MonomialShift's sign as
//                             tfhe_cbs_acc_init_kernel does (v = 0, levels = 1: that kernel's words).
//   multi-index extraction    tfhe_sample_extract_kernel at every index h < count of every accumulator, row e count + h,
//                             with g_h/2 added to the body when the circuit bootstrap asks for it.
// Exact integer arithmetic modulo 2^BITS; one thread per word written, no LDS, no atomics, no scratch memory.
#include <cstdint>

#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// one thread per word of the batch: word i of ciphertext e goes to exps[e n + i] (i < n) or, with body_offset added before
// the switch and negated after it, to neg_b[e] (i = n)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_modswitch_stride_kernel(const W *__restrict__ lwe, u32 *__restrict__ exps,
                                                                         u32 *__restrict__ neg_b, u32 n, u32 log_n,
                                                                         u32 log_stride, W body_offset, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u64 e = t / (n + 1);
    const u32 i = (u32)(t - e * (n + 1));
    if (i < n)
        exps[e * n + i] = switch_rounded<W>(lwe[t], log_n, log_stride) & ((2u << log_n) - 1);
    else
        neg_b[e] = ((2u << log_n) - (switch_rounded<W>((W)(lwe[t] + body_offset), log_n, log_stride) & ((2u << log_n) - 1))) &
                   ((2u << log_n) - 1);
}

// ACC_e = X^{neg_b[e]} TV, one thread per accumulator word: the mask polynomials are 0; body coefficient j holds
// -+TV[(j - rot) mod N], whose level is (j - rot) mod 2^v and whose value is -g_level/2 = -2^(half_shift + level log_basis),
// or 0 for a level the basis does not have
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_pattern_acc_init_kernel(W *__restrict__ acc, const u32 *__restrict__ neg_b,
                                                                         u32 k, u32 log_n, u32 log_stride, u32 levels,
                                                                         u32 log_basis, u32 half_shift, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 poly = t >> log_n, e = poly / (k + 1);
    if (poly - e * (k + 1) != k) {
        acc[t] = 0;
        return;
    }
    const MonomialShift x(neg_b[e], n);
    const u32 j = (u32)(t & (n - 1));
    const u32 level = (j - x.rot) & ((1u << log_stride) - 1);
    const W v = level < levels ? (W)0 - ((W)1 << (half_shift + level * log_basis)) : (W)0;
    acc[t] = x.apply(j, v);
}

// one thread per output word: row a = e count + h is accumulator e extracted at index h, out[jN + i] =
// extract_word(A_j, h, N, i), out[kN] = B[h], plus 2^(half_shift + h log_basis) when add_half is set
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_multi_extract_kernel(const W *__restrict__ glwe, W *__restrict__ lwe, u32 k,
                                                                      u32 log_n, u32 count, u32 add_half, u32 log_basis,
                                                                      u32 half_shift, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 out_len = ((u64)k << log_n) + 1;
    const u64 a = t / out_len, c = t - a * out_len;
    const u64 e = a / count;
    const u32 h = (u32)(a - e * count);
    const W *ct = glwe + e * ((u64)(k + 1) << log_n);
    if (c == out_len - 1) {
        const W b = ct[((u64)k << log_n) + h];
        lwe[t] = add_half ? b + ((W)1 << (half_shift + h * log_basis)) : b;
        return;
    }
    const u32 i = (u32)(c & (n - 1));
    lwe[t] = extract_word(ct + (c - i), h, n, i);
}

}  // namespace

// ---------------- launches (arguments already checked: log_stride <= log_n, count <= N, levels g_l/2 are words) ----------------

template <class W>
int launch_modswitch_stride(const W *lwe, u32 n, u32 log_n, u32 log_stride, W body_offset, u32 *exps, u32 *neg_b, u64 batch,
                            hipStream_t s) {
    return launch_flat(tfhe_modswitch_stride_kernel<W>, batch * ((u64)n + 1), s, lwe, exps, neg_b, n, log_n, log_stride,
                       body_offset);
}

template <class W>
int launch_pattern_acc_init(W *acc, const u32 *neg_b, u32 k, u32 log_n, u32 log_stride, u32 levels, u32 log_basis,
                            u32 half_shift, u64 batch, hipStream_t s) {
    return launch_flat(tfhe_pattern_acc_init_kernel<W>, (batch * (k + 1)) << log_n, s, acc, neg_b, k, log_n, log_stride, levels,
                       log_basis, half_shift);
}

template <class W>
int launch_multi_extract(const W *glwe, W *lwe, u32 k, u32 log_n, u32 count, bool add_half, u32 log_basis, u32 half_shift,
                         u64 batch, hipStream_t s) {
    return launch_flat(tfhe_multi_extract_kernel<W>, batch * count * (((u64)k << log_n) + 1), s, glwe, lwe, k, log_n, count,
                       (u32)add_half, log_basis, half_shift);
}

template int launch_modswitch_stride<u32>(const u32 *, u32, u32, u32, u32, u32 *, u32 *, u64, hipStream_t);
template int launch_modswitch_stride<u64>(const u64 *, u32, u32, u32, u64, u32 *, u32 *, u64, hipStream_t);
template int launch_pattern_acc_init<u32>(u32 *, const u32 *, u32, u32, u32, u32, u32, u32, u64, hipStream_t);
template int launch_pattern_acc_init<u64>(u64 *, const u32 *, u32, u32, u32, u32, u32, u32, u64, hipStream_t);
template int launch_multi_extract<u32>(const u32 *, u32 *, u32, u32, u32, bool, u32, u32, u64, hipStream_t);
template int launch_multi_extract<u64>(const u64 *, u64 *, u32, u32, u32, bool, u32, u32, u64, hipStream_t);

namespace {

// pfhe_tfhe*_modswitch_dev's refusals in its order, the stride's right behind log_n's
template <class W>
int modswitch_stride_dev(int device, const W *lwe, size_t len_lwe, size_t lwe_dimension, uint32_t log_n, uint32_t log_stride,
                         uint32_t *exps, size_t len_exps, uint32_t *neg_b, size_t len_neg_b, hipStream_t s) {
    if (log_n == 0 || log_n > kMaxLogN) {
        set_last_error("strided modulus switch: log_n must be in 1..14");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (log_stride > log_n) {
        set_last_error("strided modulus switch: log_stride must be at most log_n");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (lwe_dimension == 0 || lwe_dimension >= 0xffffffffull) {
        set_last_error("strided modulus switch: lwe_dimension must be in 1..2^32-2");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (len_lwe % (lwe_dimension + 1) != 0 || len_neg_b != len_lwe / (lwe_dimension + 1) ||
        len_exps != len_neg_b * lwe_dimension) {
        set_last_error("strided modulus switch: lwe must be batch*(n+1) words, exps batch*n and neg_b batch exponents");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_lwe == 0) return PFHE_OK;
    // no overlap message: this step refuses none, as the plain switch
    const StageBuf bufs[] = {stage_in(lwe, len_lwe * sizeof(W)), stage_out(exps, len_exps * sizeof(u32)),
                             stage_out(neg_b, len_neg_b * sizeof(u32))};
    return stateless_call(
        device, Form::kDevice, bufs, nullptr, s,
        [&](void *const *d, hipStream_t st) {
            return launch_modswitch_stride<W>((const W *)d[0], (u32)lwe_dimension, log_n, log_stride, (W)0, (u32 *)d[1],
                                              (u32 *)d[2], len_neg_b, st);
        },
        [&] { return capi_check_device(device); });
}

}  // namespace
}  // namespace pfhe

// The entry point of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_MANYLUT_FAMILY(P, CW, W)                                                                                   \
    PFHE_ENTRY(P##_modswitch_stride_dev, (int device, const CW *lwe_dev, size_t len_lwe, size_t lwe_dimension,          \
                uint32_t log_n, uint32_t log_stride, uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev,          \
                size_t len_neg_b, void *stream),                                                                        \
               modswitch_stride_dev<W>(device, (const W *)lwe_dev, len_lwe, lwe_dimension, log_n, log_stride, exps_dev, \
                                       len_exps, neg_b_dev, len_neg_b, (hipStream_t)stream))

extern "C" {

PFHE_MANYLUT_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_MANYLUT_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_MANYLUT_FAMILY

}  // extern "C"
