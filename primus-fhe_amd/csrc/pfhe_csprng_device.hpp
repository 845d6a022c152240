// pfhe_csprng_device.hpp — the device side of the random layer (pfhe_csprng.hip): the ChaCha20 block function,
// the position-addressed stream and the four exact samplers over it.  Device code only, in a header so that a kernel that
// consumes the stream in registers (the seeded LWE encryption) shares it with the kernels that store it.
//
// The stream: the 20-round block function of RFC 8439 on the state
//     words 0..3 "expand 32-byte k", 4..11 the key, 12 / 13 the block counter (low / high), 14 / 15 the nonce (low / high);
// u32 stream word j is little-endian word j mod 16 of block j div 16, u64 stream word j is u32 words 2j (low half) and 2j + 1.
// Every sampler consumes a fixed number of stream words per output, so output i is a closed form of (key, nonce, i): there is
// no generator state and no rejection, and any launch can produce any sub-range.
//
// A seed travels to a kernel BY VALUE, as a kernel argument: the library never writes a key to device global memory.  A block
// lives in 16 registers with constant indices; nothing here uses scratch memory.
#pragma once

#include "pfhe_common.hpp"

namespace pfhe {

// the ten words of a stream's identity: the key and the nonce (state words 4..11 and 14..15)
struct RandSeed {
    u32 key[8];
    u32 nonce[2];
};

enum RandSampler : int { kRandUniform = 0, kRandBinary = 1, kRandTernary = 2, kRandTUniform = 3 };

constexpr u64 kRandMaxIndex = ~0ull - (1ull << 20) + 1;  // 2^64 - 2^20: no call reaches an output index above this one
constexpr int kRandWave = 64;
constexpr int kRandBlockWords = 16;  // u32 words of a ChaCha block
constexpr int kRandLdsPitch = kRandBlockWords + 1;  // a block's words in LDS, one word of padding (bank = lane + word)

// outputs one block yields: one per stream word of the output's width (uniform), per u64 stream word (TUniform, both widths),
// per bit (binary), per two bits (ternary)
template <class W, int S>
struct RandPerBlock {
    static constexpr u32 value = S == kRandUniform    ? 64 / sizeof(W)
                                 : S == kRandTUniform ? 8
                                 : S == kRandBinary   ? 512
                                                      : 256;
};

#define PFHE_CHACHA_QR(a, b, c, d)                 \
    x[a] += x[b];                                  \
    x[d] = __builtin_rotateleft32(x[d] ^ x[a], 16); \
    x[c] += x[d];                                  \
    x[b] = __builtin_rotateleft32(x[b] ^ x[c], 12); \
    x[a] += x[b];                                  \
    x[d] = __builtin_rotateleft32(x[d] ^ x[a], 8);  \
    x[c] += x[d];                                  \
    x[b] = __builtin_rotateleft32(x[b] ^ x[c], 7);

// block `counter` of the stream of `seed`: x[j] is u32 stream word 16 counter + j
__device__ __forceinline__ void chacha20_block(const RandSeed &seed, u64 counter, u32 (&x)[16]) {
    const u32 in[16] = {0x61707865u,  0x3320646eu,  0x79622d32u,  0x6b206574u,  seed.key[0],   seed.key[1],
                        seed.key[2],  seed.key[3],  seed.key[4],  seed.key[5],  seed.key[6],   seed.key[7],
                        (u32)counter, (u32)(counter >> 32), seed.nonce[0], seed.nonce[1]};
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = in[j];
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        PFHE_CHACHA_QR(0, 4, 8, 12)
        PFHE_CHACHA_QR(1, 5, 9, 13)
        PFHE_CHACHA_QR(2, 6, 10, 14)
        PFHE_CHACHA_QR(3, 7, 11, 15)
        PFHE_CHACHA_QR(0, 5, 10, 15)
        PFHE_CHACHA_QR(1, 6, 11, 12)
        PFHE_CHACHA_QR(2, 7, 8, 13)
        PFHE_CHACHA_QR(3, 4, 9, 14)
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] += in[j];
}
#undef PFHE_CHACHA_QR

// `a` where `first`, else `b`, word by word (ten selects; no memory)
__device__ __forceinline__ RandSeed rand_select_seed(bool first, const RandSeed &a, const RandSeed &b) {
    RandSeed s;
#pragma unroll
    for (int j = 0; j < 8; ++j) s.key[j] = first ? a.key[j] : b.key[j];
    s.nonce[0] = first ? a.nonce[0] : b.nonce[0];
    s.nonce[1] = first ? a.nonce[1] : b.nonce[1];
    return s;
}

// TUniform(b) from one u64 stream word: r its low b + 2 bits, (r >> 1) + (r & 1) - 2^b modulo 2^BITS.  0 <= b <= BITS - 2; the
// mask is a right shift of all ones, since 1 << (b + 2) does not exist at b = 62, and r + 1 is never formed.
template <class W>
__device__ __forceinline__ W rand_tuniform(u64 word, u32 b) {
    const u64 r = word & (~0ull >> (62 - b));
    return (W)((r >> 1) + (r & 1) - (1ull << b));
}

template <class W>
__device__ __forceinline__ W rand_ternary(u32 two_bits) {
    return two_bits == 2 ? (W)1 : two_bits == 3 ? (W) ~(W)0 : (W)0;
}

// Output `local` (counted from the first output of the wave's first block) from the wave's 64 blocks in LDS, block l at
// l * kRandLdsPitch.
template <class W, int S>
__device__ __forceinline__ W rand_sample_lds(const u32 *blocks, u32 local, u32 b) {
    auto word = [&](u32 j) { return blocks[j + j / kRandBlockWords]; };
    if constexpr (S == kRandBinary) {
        return (W)((word(local >> 5) >> (local & 31)) & 1u);
    } else if constexpr (S == kRandTernary) {
        return rand_ternary<W>((word(local >> 4) >> (2 * (local & 15))) & 3u);
    } else if constexpr (S == kRandTUniform) {
        return rand_tuniform<W>(word(2 * local) | (u64)word(2 * local + 1) << 32, b);
    } else if constexpr (sizeof(W) == 8) {
        return (W)(word(2 * local) | (u64)word(2 * local + 1) << 32);
    } else {
        return (W)word(local);
    }
}

// A workgroup's share of a stream, in two steps so that a kernel may pick the seed and the sampler by workgroup.
//
// rand_blocks_to_lds: thread t computes block first_block + t and lays it into LDS (kThreads * kRandLdsPitch words); ends in
// a barrier, so every thread of the workgroup calls it.
__device__ __forceinline__ void rand_blocks_to_lds(const RandSeed &seed, u64 first_block, u32 *lds) {
    u32 x[16];
    chacha20_block(seed, first_block + threadIdx.x, x);
    u32 *mine = lds + threadIdx.x * kRandLdsPitch;
#pragma unroll
    for (int j = 0; j < 16; ++j) mine[j] = x[j];
    __syncthreads();
}

// rand_emit: the outputs of sampler S in [lo, hi) that the wave's 64 blocks hold, lane l taking every 64th, so that a wave
// hands store(o, local, value) 64 consecutive outputs at a time (coalesced whatever the alignment of lo).  `local` counts from
// the wave's first output, whose absolute index the caller can form as (first_block + 64 wave) * per_block.  The host keeps
// hi at or below kRandMaxIndex, so no index of a workgroup's blocks wraps.
template <class W, int S, class Store>
__device__ __forceinline__ void rand_emit(u64 first_block, u64 lo, u64 hi, u32 b, const u32 *lds, Store &&store) {
    constexpr u32 kPer = RandPerBlock<W, S>::value, kSpan = kRandWave * kPer;
    const u32 lane = threadIdx.x % kRandWave, wave = threadIdx.x / kRandWave;
    const u64 base = (first_block + (u64)wave * kRandWave) * kPer;
    if (hi <= base || (lo > base && lo - base >= kSpan)) return;
    const u32 from = lo > base ? (u32)(lo - base) : 0, to = hi - base < kSpan ? (u32)(hi - base) : kSpan;
    const u32 *blocks = lds + wave * kRandWave * kRandLdsPitch;
    for (u32 local = from + lane; local < to; local += kRandWave) store(base + local, local, rand_sample_lds<W, S>(blocks, local, b));
}

template <class W>
__device__ __forceinline__ W rand_wave_sum(W v) {
#pragma unroll
    for (int d = kRandWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kRandWave);
    return v;
}

}  // namespace pfhe
