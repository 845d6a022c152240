// pfhe_tfhe_stages.hip — the exact stages around a blind rotation, ONE kernel per stage, and the strided modulus switch's
// entry point (include/pfhe.h: pfhe_tfhe{,32}_modswitch_stride_dev).  The bootstrap handle
// (pfhe_bootstrap.hip), the circuit bootstrap handle (pfhe_cbs.hip), bit extraction (pfhe_bitext.hip), the look-up
// (pfhe_lut.hip) and the stateless entry points queue them through the launches declared in pfhe_tfhe_handles.hpp; what
// differs between plain, many-LUT and shared-rotation use is in the arguments:
//
//   modulus switch            switch_rounded (pfhe_tfhe_exact_device.hpp) at stride 2^v, reduced modulo 2N: round(w 2N /
//                             2^v / 2^BITS) with ties up, times 2^v; the body with body_offset added first and negated after.
//                             The exponents of an input are written `copies` times, once per accumulator the rotation sees.
//                             plain (0, 0, 1); circuit bootstrap (0, 2^(BITS-2), levels); strided (v, offset, 1).
//   accumulator, caller's     ACC_e = X^{neg_b[e]} TV_e, the rotation of pfhe_tfhe*_mul_monomial_each_to_dev with the test
//                             vector read in place (one shared by the batch, or one per ciphertext).
//   accumulator, constants    ACC_a = X^{neg_b[e]} TV, e = a / per_input, TV the trivial GLWE whose body coefficient c is
//                             -g_level/2 at level = a mod per_input + c mod 2^v, 0 where the basis has no such level.
//                             one per level (per_input = levels, v = 0); one per input (per_input = 1; bit extraction's
//                             single constant is that form with levels = 1).
//   sample extraction         output row a is accumulator a / per_acc at index first_index + a mod per_acc, with
//                             g_{a mod level_period}/2 added to the body when the rule asks for it; SUB stores src - row
//                             instead (bit extraction's running ciphertext).
// Exact integer arithmetic modulo 2^BITS; one thread per word written, no LDS, no atomics, no scratch memory.
#include <cstdint>

#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// one thread per word of the batch: word i of ciphertext e goes to exps[(e copies + c) n + i] for every c < copies (i < n)
// or, with body_offset added before the switch and negated after it, to neg_b[e] (i = n)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_modswitch_kernel(const W *__restrict__ lwe, u32 *__restrict__ exps,
                                                                  u32 *__restrict__ neg_b, u32 n, u32 log_n, u32 log_stride,
                                                                  W body_offset, u32 copies, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u64 e = t / (n + 1);
    const u32 i = (u32)(t - e * (n + 1));
    const u32 two_n_mask = (2u << log_n) - 1;
    if (i < n) {
        const u32 v = switch_rounded<W>(lwe[t], log_n, log_stride) & two_n_mask;
        for (u32 c = 0; c < copies; ++c) exps[(e * copies + c) * n + i] = v;
    } else {
        neg_b[e] = ((2u << log_n) - (switch_rounded<W>((W)(lwe[t] + body_offset), log_n, log_stride) & two_n_mask)) & two_n_mask;
    }
}

// ACC_e = X^{neg_b[e]} TV_e (MonomialShift), one thread per accumulator word.  tv_stride: words between the test vectors of
// consecutive ciphertexts, 0 when one is shared by the batch.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_acc_init_kernel(const W *__restrict__ tv, W *__restrict__ acc,
                                                                 const u32 *__restrict__ neg_b, u32 rows, u32 log_n,
                                                                 u64 tv_stride, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n, j = (u32)(t & (n - 1));
    const u64 poly = t >> log_n, e = poly / rows;
    const u32 row = (u32)(poly - e * rows);
    const MonomialShift x(neg_b[e], n);
    acc[t] = x.apply(j, tv[e * tv_stride + ((u64)row << log_n) + x.source(j)]);
}

// ACC_a = X^{neg_b[e]} TV written from constants, one thread per accumulator word; accumulator a belongs to input e = a /
// per_input and starts at level a mod per_input.  The mask polynomials are 0; body coefficient j holds -+TV[(j - rot) mod N],
// whose level is the base plus (j - rot) mod 2^v and whose value is -g_level/2 = -2^(half_shift + level log_basis), or 0 for a
// level the basis does not have
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_const_acc_init_kernel(W *__restrict__ acc, const u32 *__restrict__ neg_b,
                                                                       u32 k, u32 log_n, u32 per_input, u32 log_stride,
                                                                       u32 levels, u32 log_basis, u32 half_shift, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 poly = t >> log_n, a = poly / (k + 1);
    if (poly - a * (k + 1) != k) {
        acc[t] = 0;
        return;
    }
    const u64 e = a / per_input;
    const MonomialShift x(neg_b[e], n);
    const u32 j = (u32)(t & (n - 1));
    const u32 level = (u32)(a - e * per_input) + ((j - x.rot) & ((1u << log_stride) - 1));
    const W v = level < levels ? (W)0 - ((W)1 << (half_shift + level * log_basis)) : (W)0;
    acc[t] = x.apply(j, v);
}

// one thread per output word: row a is accumulator a / per_acc extracted at index h = first_index + a mod per_acc, row[jN +
// i] = extract_word(A_j, h, N, i), row[kN] = B[h], plus 2^(half_shift + (a mod level_period) log_basis) when add_half is
// set.  SUB: dst[t] = src[t] - that word, and dst may be exactly src (a thread reads and writes one word of them; no
// __restrict__ on the two for that reason); otherwise dst[t] is the word and src is not looked at.
template <class W, bool SUB>
__global__ __launch_bounds__(kThreads) void tfhe_extract_kernel(const W *__restrict__ glwe, const W *src, W *dst, u32 k,
                                                                u32 log_n, ExtractRule r, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 out_len = ((u64)k << log_n) + 1;
    const u64 a = t / out_len, c = t - a * out_len;
    const u64 e = r.per_acc == 1 ? a : a / r.per_acc;  // one index per accumulator: the plain forms pay for no division
    const u32 h = r.first_index + (u32)(a - e * r.per_acc);
    const W *ct = glwe + e * ((u64)(k + 1) << log_n);
    W w;
    if (c == out_len - 1) {
        w = ct[((u64)k << log_n) + h];
        if (r.add_half) w += (W)1 << (r.half_shift + (u32)(a % r.level_period) * r.log_basis);
    } else {
        const u32 i = (u32)(c & (n - 1));
        w = extract_word(ct + (c - i), h, n, i);
    }
    dst[t] = SUB ? (W)(src[t] - w) : w;
}

}  // namespace

// ---------------- launches (arguments already checked: log_stride <= log_n, every index below N, levels g_l/2 are words) ----

template <class W>
int launch_modswitch(const W *lwe, u32 n, u32 log_n, u32 log_stride, W body_offset, u32 copies, u32 *exps, u32 *neg_b,
                     u64 batch, hipStream_t s) {
    return launch_flat(tfhe_modswitch_kernel<W>, batch * ((u64)n + 1), s, lwe, exps, neg_b, n, log_n, log_stride, body_offset,
                       copies);
}

template <class W>
int launch_acc_init(const W *tv, u64 tv_stride, W *acc, const u32 *neg_b, u32 rows, u32 log_n, u64 batch, hipStream_t s) {
    return launch_flat(tfhe_acc_init_kernel<W>, (batch * rows) << log_n, s, tv, acc, neg_b, rows, log_n, tv_stride);
}

template <class W>
int launch_const_acc_init(W *acc, const u32 *neg_b, u32 k, u32 log_n, u32 per_input, u32 log_stride, u32 levels, u32 log_basis,
                          u32 half_shift, u64 accs, hipStream_t s) {
    return launch_flat(tfhe_const_acc_init_kernel<W>, (accs * (k + 1)) << log_n, s, acc, neg_b, k, log_n, per_input, log_stride,
                       levels, log_basis, half_shift);
}

template <class W>
int launch_extract(const W *glwe, const W *src, W *dst, u32 k, u32 log_n, const ExtractRule &rule, u64 rows, hipStream_t s) {
    const u64 total = rows * (((u64)k << log_n) + 1);
    if (src) return launch_flat(tfhe_extract_kernel<W, true>, total, s, glwe, src, dst, k, log_n, rule);
    return launch_flat(tfhe_extract_kernel<W, false>, total, s, glwe, src, dst, k, log_n, rule);
}

#define PFHE_STAGE_LAUNCHES(W)                                                                               \
    template int launch_modswitch<W>(const W *, u32, u32, u32, W, u32, u32 *, u32 *, u64, hipStream_t);      \
    template int launch_acc_init<W>(const W *, u64, W *, const u32 *, u32, u32, u64, hipStream_t);           \
    template int launch_const_acc_init<W>(W *, const u32 *, u32, u32, u32, u32, u32, u32, u32, u64, hipStream_t); \
    template int launch_extract<W>(const W *, const W *, W *, u32, u32, const ExtractRule &, u64, hipStream_t);
PFHE_STAGE_LAUNCHES(u32)
PFHE_STAGE_LAUNCHES(u64)
#undef PFHE_STAGE_LAUNCHES

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
            return launch_modswitch<W>((const W *)d[0], (u32)lwe_dimension, log_n, log_stride, (W)0, 1, (u32 *)d[1], (u32 *)d[2],
                                       len_neg_b, st);
        },
        [&] { return capi_check_device(device); });
}

}  // namespace
}  // namespace pfhe

// The entry point of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_STAGES_FAMILY(P, CW, W)                                                                                    \
    PFHE_ENTRY(P##_modswitch_stride_dev, (int device, const CW *lwe_dev, size_t len_lwe, size_t lwe_dimension,          \
                uint32_t log_n, uint32_t log_stride, uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev,          \
                size_t len_neg_b, void *stream),                                                                        \
               modswitch_stride_dev<W>(device, (const W *)lwe_dev, len_lwe, lwe_dimension, log_n, log_stride, exps_dev, \
                                       len_exps, neg_b_dev, len_neg_b, (hipStream_t)stream))

extern "C" {

PFHE_STAGES_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_STAGES_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_STAGES_FAMILY

}  // extern "C"
