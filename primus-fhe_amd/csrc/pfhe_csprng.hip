// pfhe_csprng.hip — the random layer of the torus side: a position-addressed ChaCha20 stream on the device, four exact samplers
// over it, the fill of whole ciphertext rows (masks uniform, bodies bounded noise), and seeded LWE ciphertexts, whose masks
// are a function of a public seed and the row index and are therefore neither stored nor sent (include/pfhe.h:
// pfhe_csprng_keystream_dev, pfhe_rand{,32}_*; DESIGN.md §26 states the stream and every sampler rule).
//
//   rand_fill_kernel          outputs [offset, offset + n) of one sampler: a thread computes one block, the workgroup's blocks
//                             cross LDS, and a wave stores 64 consecutive outputs at a time
//   rand_rows_kernel          rows of mask_len uniform words and body_len TUniform words in ONE launch (the first workgroups
//                             the masks, the rest the bodies, stored or added), or with the bodies copied: the expansion
//   rand_lwe_seeded_kernel    bodies[r] += <mask(R), key> + noise(R), a wave per row, the mask never leaving registers
// Seeds are kernel arguments: no key is ever written to device global memory, and no message names one.  Exact integer
// arithmetic modulo 2^BITS; no atomics, no scratch memory, no allocation, no generator state: the words of a call depend on
// (seed, position) alone, not on the launch.  Every call goes through stateless_call of pfhe_tfhe_host.hpp.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "pfhe_capi_internal.hpp"
#include "pfhe_csprng_device.hpp"
#include "pfhe_tfhe_host.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

static_assert(kThreads % kRandWave == 0, "whole waves");
constexpr int kRandWaves = kThreads / kRandWave;

// ---------------- one sampler, a flat range ----------------

template <class W, int S>
__global__ __launch_bounds__(kThreads) void rand_fill_kernel(RandSeed seed, u64 offset, W *__restrict__ out, u64 n, u32 b) {
    __shared__ u32 lds[kThreads * kRandLdsPitch];
    const u64 first = offset / RandPerBlock<W, S>::value + (u64)blockIdx.x * kThreads;
    rand_blocks_to_lds(seed, first, lds);
    rand_emit<W, S>(first, offset, offset + n, b, lds, [&](u64 o, u32, W v) { out[o - offset] = v; });
}

// ---------------- rows: masks and bodies in one launch ----------------

enum RowsBody : u32 { kBodyStore = 0, kBodyAdd = 1, kBodyCopy = 2 };

struct RowsShape {
    u64 first_row, rows;
    u32 mask_len, body_len;
    u32 bound_log2, body;  // a RowsBody
    u32 mask_groups;       // workgroups [0, mask_groups) write masks, the rest bodies
};

// Row r of the call is absolute row R = first_row + r.  Its mask is outputs [R mask_len, (R + 1) mask_len) of the uniform
// sampler on the mask stream and its body outputs [R body_len, (R + 1) body_len) of TUniform on the noise stream: both are
// flat ranges of their streams, so a workgroup does what rand_fill_kernel does and only the address differs.  A wave divides
// its first output index by the segment length once (64-bit); an output then needs one 32-bit division.
template <class W>
__global__ __launch_bounds__(kThreads) void rand_rows_kernel(RandSeed mask_seed, RandSeed noise_seed, RowsShape sh,
                                                             const W *__restrict__ bodies, W *__restrict__ out) {
    __shared__ u32 lds[kThreads * kRandLdsPitch];
    const bool body = blockIdx.x >= sh.mask_groups;  // the same for the whole workgroup
    const u64 pitch = (u64)sh.mask_len + sh.body_len;
    if (body && sh.body == kBodyCopy) {
        const u64 i = (u64)(blockIdx.x - sh.mask_groups) * kThreads + threadIdx.x;
        if (i >= sh.rows * sh.body_len) return;
        const u64 r = i / sh.body_len;
        out[r * pitch + sh.mask_len + (i - r * sh.body_len)] = bodies[i];
        return;
    }
    const u32 len = body ? sh.body_len : sh.mask_len;
    const u32 per = body ? RandPerBlock<W, kRandTUniform>::value : RandPerBlock<W, kRandUniform>::value;
    const u64 lo = sh.first_row * len, hi = (sh.first_row + sh.rows) * len;
    const u64 first = lo / per + (u64)(blockIdx.x - (body ? sh.mask_groups : 0)) * kThreads;
    rand_blocks_to_lds(rand_select_seed(!body, mask_seed, noise_seed), first, lds);
    const u64 wave_base = (first + (u64)(threadIdx.x / kRandWave) * kRandWave) * per;
    const u64 base_row = wave_base / len;
    const u32 base_col = (u32)(wave_base - base_row * len);
    W *const origin = out + (body ? sh.mask_len : 0);
    // base_col < 2^31 and local < 2^10: the sum fits a u32.  A row below first_row is never asked for: rand_emit stays in [lo, hi)
    auto place = [&](u32 local) {
        const u32 t = base_col + local, q = t / len;
        return origin + (base_row + q - sh.first_row) * pitch + (t - q * len);
    };
    if (!body) {
        rand_emit<W, kRandUniform>(first, lo, hi, 0, lds, [&](u64, u32 local, W v) { *place(local) = v; });
    } else if (sh.body == kBodyAdd) {
        rand_emit<W, kRandTUniform>(first, lo, hi, sh.bound_log2, lds, [&](u64, u32 local, W v) { *place(local) += v; });
    } else {
        rand_emit<W, kRandTUniform>(first, lo, hi, sh.bound_log2, lds, [&](u64, u32 local, W v) { *place(local) = v; });
    }
}

// ---------------- the seeded LWE encryption ----------------
//
// One wave per row R = first_row + r, kRandWaves rows per workgroup.  The row's mask is W-words [R n, (R + 1) n) of the mask
// stream, which start and end inside a block as a rule: the blocks fb .. fb + nb - 1 that hold them are dealt to the lanes,
// lane l taking blocks l, l + 64, ..., and of each block the lane multiplies the words that belong to the row with their key
// words.  The noise is TUniform output R of the noise stream (body_len 1): one more job, dealt like a block, so that at
// n = 630 it falls to a lane that would otherwise idle.  Sums modulo 2^BITS are order-free: the body is word for word
// fill_rows(add) followed by the LWE body call.
template <class W>
__global__ __launch_bounds__(kThreads) void rand_lwe_seeded_kernel(RandSeed mask_seed, RandSeed noise_seed, u64 first_row, u32 n,
                                                                   u32 b, const W *__restrict__ key, W *__restrict__ bodies,
                                                                   u64 rows) {
    constexpr u32 kPer = RandPerBlock<W, kRandUniform>::value;
    const u32 lane = threadIdx.x % kRandWave;
    const u64 r = (u64)blockIdx.x * kRandWaves + threadIdx.x / kRandWave;
    if (r >= rows) return;  // the whole wave leaves; the kernel has no barrier
    const u64 row = first_row + r, e0 = row * n;
    const u64 fb = e0 / kPer;
    const u32 nb = (u32)((e0 + n - 1) / kPer - fb) + 1;
    W sum = 0;
    for (u32 job = lane; job <= nb; job += kRandWave) {
        const bool noise = job == nb;
        u32 x[16];
        chacha20_block(rand_select_seed(noise, noise_seed, mask_seed), noise ? row / 8 : fb + job, x);
        if (noise) {
            const u32 at = (u32)(row % 8);
            u64 word = 0;
#pragma unroll
            for (u32 j = 0; j < 8; ++j) word = j == at ? (x[2 * j] | (u64)x[2 * j + 1] << 32) : word;
            sum += rand_tuniform<W>(word, b);
        } else {
            const u64 e = (fb + job) * kPer - e0;  // wraps below the row's first word: the test below is unsigned
#pragma unroll
            for (u32 j = 0; j < kPer; ++j) {
                W a;
                if constexpr (sizeof(W) == 8) a = (W)(x[2 * j] | (u64)x[2 * j + 1] << 32);
                else a = (W)x[j];
                if (e + j < n) sum += a * key[e + j];
            }
        }
    }
    sum = rand_wave_sum(sum);
    if (lane == 0) bodies[r] += sum;
}

// ---------------- launches (arguments already checked) ----------------

// workgroups whose blocks cover outputs [lo, hi) at `per` outputs a block, hi > lo
inline u64 groups_over(u64 lo, u64 hi, u32 per) { return ((hi - 1) / per - lo / per + 1 + kThreads - 1) / kThreads; }

template <class W, int S>
int launch_fill(const RandSeed &seed, u64 offset, W *out, u64 n, u32 b, hipStream_t s) {
    return launch_groups(rand_fill_kernel<W, S>, groups_over(offset, offset + n, RandPerBlock<W, S>::value), 0, s, seed, offset,
                         out, n, b);
}

template <class W>
int launch_rows(const RandSeed &mask_seed, const RandSeed &noise_seed, RowsShape sh, const W *bodies, W *out, hipStream_t s) {
    const u64 mask_groups = groups_over(sh.first_row * sh.mask_len, (sh.first_row + sh.rows) * sh.mask_len,
                                        RandPerBlock<W, kRandUniform>::value);
    const u64 body_groups = sh.body == kBodyCopy ? (sh.rows * sh.body_len + kThreads - 1) / kThreads
                                                 : groups_over(sh.first_row * sh.body_len, (sh.first_row + sh.rows) * sh.body_len,
                                                               RandPerBlock<W, kRandTUniform>::value);
    if (mask_groups + body_groups > 0x7fffffffull) {
        set_last_error("random rows: more than 2^31-1 workgroups");
        return PFHE_ERR_BAD_LENGTH;
    }
    sh.mask_groups = (u32)mask_groups;
    return launch_groups(rand_rows_kernel<W>, mask_groups + body_groups, 0, s, mask_seed, noise_seed, sh, bodies, out);
}

// ---------------- the checks every call shares ----------------

// a seed from the caller's host pointers: eight key words and two nonce words (state words 14 and 15)
inline int take_seed(const uint32_t *key, const uint32_t *nonce, RandSeed &seed) {
    if (!key || !nonce) {
        set_last_error("random layer: a null key or nonce");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    std::memcpy(seed.key, key, sizeof seed.key);
    std::memcpy(seed.nonce, nonce, sizeof seed.nonce);
    return PFHE_OK;
}

// the two seeds of a call that draws masks and noise: a seeded ciphertext publishes its mask seed, which must not give the noise
inline int take_seed_pair(const uint32_t *mask_key, const uint32_t *mask_nonce, const uint32_t *noise_key,
                          const uint32_t *noise_nonce, RandSeed &mask, RandSeed &noise) {
    PFHE_TRY(take_seed(mask_key, mask_nonce, mask));
    PFHE_TRY(take_seed(noise_key, noise_nonce, noise));
    if (std::memcmp(&mask, &noise, sizeof mask) == 0) {
        set_last_error("random layer: the mask stream and the noise stream must differ in key or nonce");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    return PFHE_OK;
}

template <class W>
int require_bound(uint32_t bound_log2) {
    if (bound_log2 <= 8 * sizeof(W) - 2) return PFHE_OK;
    set_last_error("TUniform: bound_log2 must be in 0..BITS-2");
    return PFHE_ERR_BAD_ARGUMENT;
}

// outputs [first * len, (first + count) * len) of a stream: refused when the end passes kRandMaxIndex
inline int require_index_range(size_t first, size_t count, size_t len) {
    u64 end = 0, hi = 0;
    if (!__builtin_add_overflow((u64)first, (u64)count, &end) && !__builtin_mul_overflow(end, (u64)len, &hi) &&
        hi <= kRandMaxIndex)
        return PFHE_OK;
    set_last_error("random layer: the last output index must not exceed 2^64 - 2^20");
    return PFHE_ERR_BAD_LENGTH;
}

constexpr const char *kRowRange = "random rows: mask_len and body_len must be in 1..2^31-2";

// ---------------- the entry points ----------------

template <class W, int S>
int rand_fill_dev(int device, const uint32_t *key, const uint32_t *nonce, size_t offset, uint32_t bound_log2, W *out, size_t n,
                  hipStream_t s) {
    RandSeed seed;
    PFHE_TRY(take_seed(key, nonce, seed));
    if (S == kRandTUniform) PFHE_TRY(require_bound<W>(bound_log2));
    PFHE_TRY(require_index_range(offset, n, 1));
    if (n == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_out(out, n * sizeof(W))};
    return stateless_call(
        device, Form::kDevice, bufs, nullptr, s,
        [&](void *const *d, hipStream_t st) { return launch_fill<W, S>(seed, offset, (W *)d[0], n, bound_log2, st); },
        [&] { return capi_check_device(device); });
}

template <class W>
int rand_fill_rows_dev(int device, const uint32_t *mask_key, const uint32_t *mask_nonce, const uint32_t *noise_key,
                       const uint32_t *noise_nonce, size_t first_row, size_t mask_len, size_t body_len, uint32_t bound_log2,
                       int add, W *out, size_t len_out, hipStream_t s) {
    RandSeed mask, noise;
    PFHE_TRY(take_seed_pair(mask_key, mask_nonce, noise_key, noise_nonce, mask, noise));
    PFHE_TRY(require_bound<W>(bound_log2));
    PFHE_TRY(require_lwe_dimension(mask_len, kRowRange));
    PFHE_TRY(require_lwe_dimension(body_len, kRowRange));
    const size_t pitch = mask_len + body_len, rows = len_out / pitch;
    if (len_out % pitch != 0) {
        set_last_error("random rows: out must be rows*(mask_len+body_len) words");
        return PFHE_ERR_BAD_LENGTH;
    }
    PFHE_TRY(require_index_range(first_row, rows, std::max(mask_len, body_len)));
    if (rows == 0) return PFHE_OK;
    const RowsShape sh{first_row, rows, (u32)mask_len, (u32)body_len, bound_log2, add ? kBodyAdd : kBodyStore, 0};
    const StageBuf bufs[] = {stage_inout(out, len_out * sizeof(W))};
    return stateless_call(
        device, Form::kDevice, bufs, nullptr, s,
        [&](void *const *d, hipStream_t st) { return launch_rows<W>(mask, noise, sh, nullptr, (W *)d[0], st); },
        [&] { return capi_check_device(device); });
}

template <class W>
int rand_lwe_encrypt_seeded(Form form, int device, const uint32_t *mask_key, const uint32_t *mask_nonce,
                            const uint32_t *noise_key, const uint32_t *noise_nonce, size_t first_row, const W *lwe_key,
                            size_t dimension, uint32_t bound_log2, W *bodies, size_t rows, hipStream_t s) {
    RandSeed mask, noise;
    PFHE_TRY(take_seed_pair(mask_key, mask_nonce, noise_key, noise_nonce, mask, noise));
    PFHE_TRY(require_bound<W>(bound_log2));
    PFHE_TRY(require_lwe_dimension(dimension, "seeded LWE encryption: dimension must be in 1..2^31-2"));
    PFHE_TRY(require_index_range(first_row, rows, dimension));
    if (rows == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(lwe_key, dimension * sizeof(W)), stage_inout(bodies, rows * sizeof(W))};
    return stateless_call(
        device, form, bufs, "seeded LWE encryption: the key must not overlap the bodies", s,
        [&](void *const *d, hipStream_t st) {
            return launch_groups(rand_lwe_seeded_kernel<W>, ((u64)rows + kRandWaves - 1) / kRandWaves, 0, st, mask, noise,
                                 (u64)first_row, (u32)dimension, bound_log2, (const W *)d[0], (W *)d[1], (u64)rows);
        },
        [&] {
            if (((u64)rows + kRandWaves - 1) / kRandWaves > 0x7fffffffull) {
                set_last_error("seeded LWE encryption: more than 2^31-1 workgroups");
                return (int)PFHE_ERR_BAD_LENGTH;
            }
            return capi_check_device(device);
        });
}

template <class W>
int rand_seeded_expand(Form form, int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row,
                       size_t mask_len, size_t body_len, const W *bodies, size_t len_bodies, W *out, size_t len_out,
                       hipStream_t s) {
    RandSeed mask;
    PFHE_TRY(take_seed(mask_key, mask_nonce, mask));
    PFHE_TRY(require_lwe_dimension(mask_len, kRowRange));
    PFHE_TRY(require_lwe_dimension(body_len, kRowRange));
    const size_t pitch = mask_len + body_len, rows = len_bodies / body_len;
    if (len_bodies % body_len != 0 || len_out % pitch != 0 || len_out / pitch != rows) {
        set_last_error("seeded expansion: bodies must be rows*body_len words and out rows*(mask_len+body_len)");
        return PFHE_ERR_BAD_LENGTH;
    }
    PFHE_TRY(require_index_range(first_row, rows, mask_len));
    if (rows == 0) return PFHE_OK;
    const RowsShape sh{first_row, rows, (u32)mask_len, (u32)body_len, 0, kBodyCopy, 0};
    const StageBuf bufs[] = {stage_in(bodies, len_bodies * sizeof(W)), stage_out(out, len_out * sizeof(W))};
    return stateless_call(
        device, form, bufs, "seeded expansion: out must not overlap the bodies", s,
        [&](void *const *d, hipStream_t st) { return launch_rows<W>(mask, RandSeed{}, sh, (const W *)d[0], (W *)d[1], st); },
        [&] { return capi_check_device(device); });
}

}  // namespace
}  // namespace pfhe

// The entry points of one word width.  P: pfhe_rand / pfhe_rand32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_RAND_SAMPLER(P, CW, W, NAME, S)                                                                              \
    PFHE_ENTRY(P##_##NAME##_dev, (int device, const uint32_t *key, const uint32_t *nonce, size_t offset, CW *out_dev,     \
                size_t n, void *stream),                                                                                  \
               rand_fill_dev<W, S>(device, key, nonce, offset, 0, (W *)out_dev, n, (hipStream_t)stream))
#define PFHE_RAND_FAMILY(P, CW, W)                                                                                        \
    PFHE_RAND_SAMPLER(P, CW, W, uniform, kRandUniform)                                                                    \
    PFHE_RAND_SAMPLER(P, CW, W, binary, kRandBinary)                                                                      \
    PFHE_RAND_SAMPLER(P, CW, W, ternary, kRandTernary)                                                                    \
    PFHE_ENTRY(P##_tuniform_dev, (int device, const uint32_t *key, const uint32_t *nonce, size_t offset,                  \
                uint32_t bound_log2, CW *out_dev, size_t n, void *stream),                                                \
               rand_fill_dev<W, kRandTUniform>(device, key, nonce, offset, bound_log2, (W *)out_dev, n,                   \
                                               (hipStream_t)stream))                                                      \
    PFHE_ENTRY(P##_fill_rows_dev, (int device, const uint32_t *mask_key, const uint32_t *mask_nonce,                      \
                const uint32_t *noise_key, const uint32_t *noise_nonce, size_t first_row, size_t mask_len,               \
                size_t body_len, uint32_t bound_log2, int add, CW *out_dev, size_t len_out, void *stream),               \
               rand_fill_rows_dev<W>(device, mask_key, mask_nonce, noise_key, noise_nonce, first_row, mask_len, body_len, \
                                     bound_log2, add, (W *)out_dev, len_out, (hipStream_t)stream))                        \
    PFHE_ENTRY(P##_lwe_encrypt_seeded_dev, (int device, const uint32_t *mask_key, const uint32_t *mask_nonce,             \
                const uint32_t *noise_key, const uint32_t *noise_nonce, size_t first_row, const CW *lwe_key_dev,         \
                size_t dimension, uint32_t bound_log2, CW *bodies_dev, size_t rows, void *stream),                       \
               rand_lwe_encrypt_seeded<W>(Form::kDevice, device, mask_key, mask_nonce, noise_key, noise_nonce, first_row, \
                                          (const W *)lwe_key_dev, dimension, bound_log2, (W *)bodies_dev, rows,           \
                                          (hipStream_t)stream))                                                           \
    PFHE_ENTRY(P##_lwe_encrypt_seeded, (int device, const uint32_t *mask_key, const uint32_t *mask_nonce,                 \
                const uint32_t *noise_key, const uint32_t *noise_nonce, size_t first_row, const CW *lwe_key,             \
                size_t dimension, uint32_t bound_log2, CW *bodies, size_t rows),                                         \
               rand_lwe_encrypt_seeded<W>(Form::kHost, device, mask_key, mask_nonce, noise_key, noise_nonce, first_row,   \
                                          (const W *)lwe_key, dimension, bound_log2, (W *)bodies, rows, nullptr))         \
    PFHE_ENTRY(P##_seeded_expand_dev, (int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row, \
                size_t mask_len, size_t body_len, const CW *bodies_dev, size_t len_bodies, CW *out_dev, size_t len_out,  \
                void *stream),                                                                                            \
               rand_seeded_expand<W>(Form::kDevice, device, mask_key, mask_nonce, first_row, mask_len, body_len,          \
                                     (const W *)bodies_dev, len_bodies, (W *)out_dev, len_out, (hipStream_t)stream))      \
    PFHE_ENTRY(P##_seeded_expand, (int device, const uint32_t *mask_key, const uint32_t *mask_nonce, size_t first_row,    \
                size_t mask_len, size_t body_len, const CW *bodies, size_t len_bodies, CW *out, size_t len_out),         \
               rand_seeded_expand<W>(Form::kHost, device, mask_key, mask_nonce, first_row, mask_len, body_len,            \
                                     (const W *)bodies, len_bodies, (W *)out, len_out, nullptr))

extern "C" {

// raw u32 stream words [word_offset, word_offset + n_words): the uniform sampler at the u32 width under its plain name
PFHE_ENTRY(pfhe_csprng_keystream_dev, (int device, const uint32_t *key, const uint32_t *nonce, size_t word_offset,
            uint32_t *out_dev, size_t n_words, void *stream),
           rand_fill_dev<u32, kRandUniform>(device, key, nonce, word_offset, 0, out_dev, n_words, (hipStream_t)stream))

PFHE_RAND_FAMILY(pfhe_rand, uint64_t, u64)
PFHE_RAND_FAMILY(pfhe_rand32, uint32_t, u32)
#undef PFHE_RAND_FAMILY
#undef PFHE_RAND_SAMPLER

}  // extern "C"
