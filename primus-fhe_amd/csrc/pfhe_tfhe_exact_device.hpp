// pfhe_tfhe_exact_device.hpp — the exact (integer, modulo 2^BITS) device code the torus-side stages share: the rules of the
// stages around a blind rotation, one definition each, and the tile of the two key-switch GEMMs.
//
//   switch_rounded   the modulus switch to multiples of 2^v, which its callers reduce modulo 2N; v = 0 is the plain switch:
//                    tfhe_modswitch_kernel (pfhe_tfhe_stages.hip) and the switch that tfhe_bitext_keyswitch_kernel
//                    (pfhe_bitext.hip) does on the words it has just stored.
//   extract_word     a mask word of sample extraction at index h: tfhe_extract_kernel (pfhe_tfhe_stages.hip), every form of
//                    it.  tfhe_extract_first_few_kernel (pfhe_pack.hip), which writes another layout, keeps its own two-case
//                    form for index 0, a[0] or -a[N - i].
//   KsShape          the LWE key switch as its two kernels take it: tfhe_keyswitch_kernel (pfhe_bootstrap.hip) and
//                    tfhe_bitext_keyswitch_kernel (pfhe_bitext.hip).
//   ks_tile_sums     the group loop of tfhe_keyswitch_kernel (pfhe_bootstrap.hip), tfhe_pfks_kernel (pfhe_cbs.hip) and
//                    tfhe_bitext_keyswitch_kernel (pfhe_bitext.hip).
// MonomialShift, the negacyclic rule X^r p of the accumulator kernels (pfhe_tfhe_stages.hip) and of the rotated differences
// (pfhe_fft.hip, pfhe_lut.hip), sits in pfhe_fft_device.hpp beside rotated_diff, which needs it; it is included from there.
// Every function is inlined into its kernels.  The forms (what is a member, the order of parameters, what is left to the
// caller) are the ones with which the kernels that were not merged compile to the instructions they had with the rule
// written out (profiles/tfhe_exact_a_kernel_identity.txt, profiles/tfhe_stages_a_kernel_identity.txt).
#pragma once

#include <algorithm>

#include "pfhe_fft_device.hpp"

namespace pfhe {

// ---------------- the stage rules ----------------

// The modulus switch of one word before its reduction modulo 2N: round(w 2N / 2^v / 2^BITS) with ties up, times 2^v, computed
// without overflow; sw_v(w) = switch_rounded(w, log_n, v) & (2N-1), a multiple of 2^v below 2N (a word that rounds up to 2N
// wraps to 0).  v = 0 is the plain switch.  The reference has no modulus switching; the rule is this project's own.
template <class W>
__device__ __forceinline__ u32 switch_rounded(W w, u32 log_n, u32 log_stride) {
    const u32 drop = 8 * sizeof(W) - log_n - 2 + log_stride;  // at most BITS - 2: log_stride <= log_n
    return (u32)(((w >> drop) + 1) >> 1) << log_stride;
}

// word i of the LWE mask that sample extraction at index h takes from the mask polynomial a of N words
// (Rlwe::extract_lwe_with_index, primus_lattice/src/rlwe/coeff.rs:194-227): a[h - i] for i <= h, -a[N + h - i] above
template <class W>
__device__ __forceinline__ W extract_word(const W *a, u32 h, u32 n, u32 i) {
    return i <= h ? a[h - i] : (W)0 - a[n + h - i];
}

// ---------------- the key-switch tile ----------------
//
// A small integer GEMM: M input ciphertexts, K = words * ell key rows, `cols` output columns.  One workgroup owns kKsTileM
// ciphertexts x kKsTileN columns; a thread owns kKsRows ciphertexts (its wave's) x kKsCols columns (its lane's, kKsLanes
// apart) and keeps their sums in registers.  The workgroup walks the input words in groups of `ki`: first every
// (ciphertext, word) pair of the group gets its ell signed digits from ONE thread, which writes them to LDS as words; then
// every thread streams the group's key rows, coalesced along the columns and kKsUnroll rows in flight at a time, against
// the digits of its ciphertexts, which all lanes of a wave read from the same LDS address (a broadcast).  ki * ell <=
// kKsMaxRows bounds the LDS at kKsMaxRows * kKsTileM words: 8 KiB for u32, 16 KiB for u64, a constant of the design.
constexpr int kKsLanes = 64, kKsWaves = kFftThreads / kKsLanes;
constexpr int kKsRows = 8, kKsCols = 2;
constexpr int kKsTileM = kKsWaves * kKsRows, kKsTileN = kKsLanes * kKsCols;
constexpr u32 kKsMaxRows = 64;
constexpr int kKsUnroll = 4;

// The LWE key switch as its kernels take it (tfhe_keyswitch_kernel, tfhe_bitext_keyswitch_kernel): the two dimensions, the
// basis, and ki
struct KsShape {
    u32 in_dim, out_dim, log_basis, ell, drop_bits, ki;
};

// ki: input words of one group
inline u32 ks_group_words(u32 ell) { return std::max<u32>(1, std::min<u32>(kKsMaxRows / ell, kFftThreads / kKsTileM)); }

// acc[r][c] += sum over the `words` first words j of input row r0 + wave kKsRows + r (row m starts at in + m stride; rows
// from `total` on count as 0) and the levels l of d_l(word j) * key[c][(j ell + l) cols].  dig: kKsMaxRows * kKsTileM words
// of LDS, [word of the group][level][ciphertext of the tile].  The LWE key switch passes stride = words + 1 (the body is not
// decomposed), the private one stride = words (it is).  shift: every word is shifted left by it, as a wrapping word, before
// its digits are taken (pfhe_bitext.hip; 0 everywhere else, where the shift folds away).
template <class W>
__device__ __forceinline__ void ks_tile_sums(W *dig, const W *__restrict__ in, u64 stride, u32 words, u64 r0, u64 total,
                                             const W *const (&key)[kKsCols], u32 cols, u32 log_basis, u32 ell, u32 drop_bits,
                                             u32 ki, W (&acc)[kKsRows][kKsCols], u32 shift = 0) {
    const u32 wave = threadIdx.x / kKsLanes;
    // the pair this thread decomposes in every group: word ii of the group, ciphertext ei of the tile
    const u32 ii = threadIdx.x % ki, ei = threadIdx.x / ki;
    for (u32 i0 = 0; i0 < words; i0 += ki) {
        if (ei < (u32)kKsTileM) {
            const bool live = r0 + ei < total && i0 + ii < words;
            const W v = live ? (W)(in[(r0 + ei) * stride + i0 + ii] << shift) : (W)0;
            u32 carry = init_carry(v, drop_bits);
            for (u32 l = 0; l < ell; ++l)
                dig[(ii * ell + l) * kKsTileM + ei] = digit_word(v, drop_bits + l * log_basis, log_basis, carry);
        }
        __syncthreads();
        const u32 rows = min(ki, words - i0) * ell;
        const u64 key_row = (u64)i0 * ell;
        u32 row = 0;
        // kKsUnroll rows at a time: all their key words are requested before the first is used
        for (; row + kKsUnroll <= rows; row += kKsUnroll) {
            W kv[kKsUnroll][kKsCols];
#pragma unroll
            for (int u = 0; u < kKsUnroll; ++u)
#pragma unroll
                for (int c = 0; c < kKsCols; ++c) kv[u][c] = key[c][(key_row + row + u) * cols];
#pragma unroll
            for (int u = 0; u < kKsUnroll; ++u)
#pragma unroll
                for (int r = 0; r < kKsRows; ++r) {
                    const W d = dig[(row + u) * kKsTileM + wave * kKsRows + r];
#pragma unroll
                    for (int c = 0; c < kKsCols; ++c) acc[r][c] += d * kv[u][c];
                }
        }
        for (; row < rows; ++row) {
            W kv[kKsCols];
#pragma unroll
            for (int c = 0; c < kKsCols; ++c) kv[c] = key[c][(key_row + row) * cols];
#pragma unroll
            for (int r = 0; r < kKsRows; ++r) {
                const W d = dig[row * kKsTileM + wave * kKsRows + r];
#pragma unroll
                for (int c = 0; c < kKsCols; ++c) acc[r][c] += d * kv[c];
            }
        }
        __syncthreads();  // the next group overwrites the digits
    }
}

}  // namespace pfhe
