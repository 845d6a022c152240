// pfhe_pack.hip — from LWE ciphertexts back to a GLWE and out again: the packing key switch, its key, and the multi-message
// sample extraction (include/pfhe.h: pfhe_tfhe{,32}_pack_keyswitch*, _pksk_generate_dev, _sample_extract_first_few*,
// _multimsg_extract*).
//
//   packing key switch   out_e = (0, ..., 0, sum_i b_{e,i} X^i) - sum_i X^i sum_j sum_l d_l(a_{e,i,j}) PKSK[j][l] modulo
//                        2^BITS and X^N + 1, with the digits of ApproxSignedBasis exactly as the LWE key switch forms them
//                        (init_carry / digit_word of pfhe_fft_device.hpp).  No reference counterpart.
//   packing key          row (j, l) of the caller's randomness becomes a GLWE encryption of key_in[j] 2^(drop + l log_basis):
//                        the GLWE body call of pfhe_keygen.hip on all rows, then the message term on coefficient 0.
//   first few            Rlwe::extract_first_few_lwe (primus_lattice/src/rlwe/coeff.rs:231-260) per mask polynomial: the
//                        MultiMsgLwe layout, [a_0, -a_{N-1}, ..., -a_1] per mask polynomial, then b_0 .. b_{count-1}.
//   expansion            MultiMsgLwe::extract_rlwe_mode (lwe/multiple_message.rs:250-263) for every index below count.
// Every step is exact integer arithmetic modulo 2^BITS; no atomics, no scratch memory, nothing allocated by a call.
// Launches and host forms go through pfhe_tfhe_host.hpp; the packing key switch keeps its own 2-D grid.
#include <algorithm>
#include <cstdint>

#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// ---------------- the packing key switch ----------------
//
// Per key row (j, l) and component the work is acc -= D (*) K, D = sum_{i < count} d_l(a_{e,i,j}) X^i: a negacyclic
// product of a count-term digit polynomial with a key polynomial.  The index scheme is the GLWE body kernel's with the
// roles swapped: the sums stay in registers, the KEY polynomial is what is staged in LDS, and the digit is a broadcast.
//
// A 256-thread workgroup owns one output GLWE e, one component and a tile of T = min(N, 64 U) coefficients; lane t of
// every wave owns the U consecutive coefficients c0 + t U + u.  The count ciphertexts are walked in blocks of J (a
// multiple of U, at most kPackMaxJ) and, inside a block, the mask words in groups of ki: first every (ciphertext, mask
// word) pair of the group gets its ell digits from one thread, written to LDS as words, dig[row of the group][i]; then,
// key row after key row, the window of the row that the tile needs against the block is staged as
//     win[y] = E[lo + y],   E[x] = -K[x] for x < N and K[x - N] otherwise,   lo = N + c0 - i_block - J,
// so that X^i K at coefficient c is E[N + c - i] with the sign already in place.  The four waves split the block's
// ciphertexts; a wave walks its share U at a time: ONE aligned U-word LDS read of the window (the other half of the 2U
// words it needs is the previous step's) and one U-word broadcast of digits feed U x U multiply-adds.  A window of at
// most kPackSide words (few ciphertexts per block) leaves room for four: then four key rows are staged side by side per
// pair of barriers and every wave takes one row and all of the block's ciphertexts, instead of a quarter of them against
// one row.  The next window is already on its way from memory into registers while the current one is multiplied.  At
// the end the four partial sums meet in LDS (the window's own words) and thread t writes coefficient c0 + t.
//
// LDS: kPackWin window words + kPackDig digit words, a constant of the design (21 KiB for u32, 42 KiB for u64).
constexpr int kPackLanes = 64, kPackWaves = kThreads / kPackLanes;
constexpr u32 kPackMaxJ = 1024;                                // ciphertexts per block
constexpr u32 kPackMaxT = 256;                                 // coefficients per tile (U = 4)
constexpr u32 kPackWin = kPackMaxT + kPackMaxJ;                // window words
constexpr u32 kPackDig = 4096;                                 // digit words: ki * ell * J of them are used
constexpr int kPackStage = (int)(kPackWin / kThreads);         // window words a thread carries from memory to LDS
constexpr u32 kPackSide = kPackWin / kPackWaves;               // the longest window that is staged four rows side by side
static_assert(kPackWin % kThreads == 0 && kPackWaves * kPackMaxT <= kPackWin, "the partial sums reuse the window");
static_assert(kPackSide % 4 == 0, "a row of a side-by-side stage starts on a vector boundary");

struct PackShape {
    u32 in_dim, k, log_n, count, log_basis, ell, drop_bits;
    u32 tile;     // T
    u32 block_j;  // J
    u32 ki;       // mask words per group of digits
};

template <class W, int U>
__global__ __launch_bounds__(kThreads) void tfhe_pack_keyswitch_kernel(const W *__restrict__ lwe_in,
                                                                       const W *__restrict__ pksk, W *__restrict__ glwe_out,
                                                                       PackShape s) {
    typedef W Vec __attribute__((ext_vector_type(U)));
    __shared__ __align__(32) W win[kPackWin];
    __shared__ __align__(32) W dig[kPackDig];  // [row of the group][ciphertext of the block], rows block_j apart
    const u32 n = 1u << s.log_n, mask = n - 1;
    const u32 tid = threadIdx.x, lane = tid % kPackLanes, wave = tid / kPackLanes;
    const u32 tiles = n / s.tile;
    const u32 comp = blockIdx.x / tiles, c0 = (blockIdx.x % tiles) * s.tile;
    const u64 e = blockIdx.y;
    const u64 in_stride = (u64)s.in_dim + 1, row_stride = (u64)(s.k + 1) << s.log_n;
    const W *lwe = lwe_in + e * s.count * in_stride;
    const W *key = pksk + ((u64)comp << s.log_n);
    const bool owner = lane * U < s.tile;  // for N < 64 U the other lanes only help with the staging
    const u32 count_pad = (s.count + U - 1) / U * U;

    W acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0;

    for (u32 ib = 0; ib < count_pad; ib += s.block_j) {
        const u32 jlen = min(s.block_j, count_pad - ib);  // a multiple of U
        const u32 lo = n + c0 - ib - jlen, span = s.tile + jlen;
        for (u32 j0 = 0; j0 < s.in_dim; j0 += s.ki) {
            const u32 kcur = min(s.ki, s.in_dim - j0), rows = kcur * s.ell;
            // the first window leaves memory before the digits are formed.  Word x of a stage is word x of the one row's
            // window, or, side by side, word x % kPackSide of row x / kPackSide of the stage
            const W *krow = key + (u64)j0 * s.ell * row_stride;
            const bool side = span <= kPackSide;
            const u32 per_stage = side ? kPackWaves : 1;
            W stage[kPackStage];
            auto load_stage = [&](u32 r) {
#pragma unroll
                for (int q = 0; q < kPackStage; ++q) {
                    const u32 x = tid + q * kThreads;
                    const u32 sr = side ? x / kPackSide : 0, y = side ? x % kPackSide : x;
                    stage[q] = y < span && r + sr < rows ? krow[(u64)(r + sr) * row_stride + ((lo + y) & mask)] : (W)0;
                }
            };
            load_stage(0);
            // digits: pair p is mask word p % kcur of the group (consecutive threads, consecutive words) and ciphertext
            // p / kcur of the block; a ciphertext past count has the digits 0
            for (u32 p = tid; p < kcur * jlen; p += kThreads) {
                const u32 jj = p % kcur, ii = p / kcur;
                const W v = ib + ii < s.count ? lwe[(u64)(ib + ii) * in_stride + j0 + jj] : (W)0;
                u32 carry = init_carry(v, s.drop_bits);
                for (u32 l = 0; l < s.ell; ++l)
                    dig[(jj * s.ell + l) * s.block_j + ii] = digit_word(v, s.drop_bits + l * s.log_basis, s.log_basis, carry);
            }
            for (u32 r = 0; r < rows; r += per_stage) {
#pragma unroll
                for (int q = 0; q < kPackStage; ++q) {
                    const u32 x = tid + q * kThreads;
                    const u32 y = side ? x % kPackSide : x;
                    if (y < span) win[x] = lo + y < n ? (W)0 - stage[q] : stage[q];
                }
                __syncthreads();  // the window (and, for r = 0, the digits) are in LDS
                if (r + per_stage < rows) load_stage(r + per_stage);
                // this wave's row and its ciphertexts of the block, [i_begin, i_end), both multiples of U: side by side
                // its own row and all of them, otherwise the one row and a quarter
                const u32 row = side ? r + wave : r;
                if (owner && row < rows) {
                    const u32 share = side ? jlen : ((jlen + kPackWaves - 1) / kPackWaves + U - 1) / U * U;
                    const u32 i_begin = side ? 0 : min(jlen, wave * share), i_end = min(jlen, i_begin + share);
                    if (i_begin < i_end) {
                        const W *d = dig + row * s.block_j;
                        const W *wrow = side ? win + wave * kPackSide : win;
                        u32 q = lane * U + jlen - i_begin;  // wrow[q + u - v] is E[N + c - i] for i = ib + i_begin + v
                        Vec high = *reinterpret_cast<const Vec *>(wrow + q);
                        for (u32 i0 = i_begin; i0 < i_end; i0 += U, q -= U) {
                            const Vec low = *reinterpret_cast<const Vec *>(wrow + q - U);
                            const Vec dv = *reinterpret_cast<const Vec *>(d + i0);
                            W w[2 * U];
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                w[u] = low[u];
                                w[U + u] = high[u];
                            }
#pragma unroll
                            for (int v = 0; v < U; ++v)
#pragma unroll
                                for (int u = 0; u < U; ++u) acc[u] += dv[v] * w[U + u - v];
                            high = low;
                        }
                    }
                }
                __syncthreads();  // the next stage overwrites the window, the next group the digits
            }
        }
    }

    // the four partial sums of every coefficient meet in the window's words
    if (owner) {
#pragma unroll
        for (int u = 0; u < U; ++u) win[wave * kPackMaxT + lane * U + u] = acc[u];
    }
    __syncthreads();
    if (tid < s.tile) {
        W sum = 0;
#pragma unroll
        for (int w = 0; w < kPackWaves; ++w) sum += win[w * kPackMaxT + tid];
        const u32 c = c0 + tid;
        const W b = comp == s.k && c < s.count ? lwe[(u64)c * in_stride + s.in_dim] : (W)0;
        glwe_out[e * row_stride + ((u64)comp << s.log_n) + c] = b - sum;
    }
}

// ---------------- the packing key's message term ----------------

// one thread per key row (j, l): coefficient 0 of the body gets key_in[j] 2^(drop + l log_basis)
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_pksk_add_message_kernel(W *__restrict__ pksk, const W *__restrict__ key_in,
                                                                         u32 k, u32 log_n, u32 ell, u32 log_basis, u32 drop,
                                                                         u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 l = (u32)(t % ell);
    pksk[((t * (k + 1) + k) << log_n)] += key_in[t / ell] << (drop + l * log_basis);
}

// ---------------- multi-message extraction ----------------

// one thread per output word: out[jN + i] = A_j[0] (i = 0) or -A_j[N - i], out[kN + h] = B[h] for h < count
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_extract_first_few_kernel(const W *__restrict__ glwe, W *__restrict__ multi,
                                                                          u32 k, u32 log_n, u32 count, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 mask_len = (u64)k << log_n, out_len = mask_len + count;
    const u64 e = t / out_len, c = t - e * out_len;
    const W *ct = glwe + e * ((u64)(k + 1) << log_n);
    if (c >= mask_len) {
        multi[t] = ct[c];  // B[c - kN]: the body polynomial follows the masks
        return;
    }
    const u32 i = (u32)(c & (n - 1));
    multi[t] = i == 0 ? ct[c] : (W)0 - ct[c - i + (n - i)];
}

// one thread per output word of ciphertext h of group e: the mask polynomial rotated right by h with its first h words
// negated, and the body b_h
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_multimsg_extract_kernel(const W *__restrict__ multi, W *__restrict__ lwe,
                                                                         u32 k, u32 log_n, u32 count, u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 n = 1u << log_n;
    const u64 mask_len = (u64)k << log_n, out_len = mask_len + 1;
    const u64 ct = t / out_len, c = t - ct * out_len;
    const u64 e = ct / count;
    const u32 h = (u32)(ct - e * count);
    const W *src = multi + e * (mask_len + count);
    if (c == mask_len) {
        lwe[t] = src[mask_len + h];
        return;
    }
    const u32 i = (u32)(c & (n - 1));
    const W *m = src + (c - i);
    lwe[t] = i < h ? (W)0 - m[n - h + i] : m[i - h];
}

// ---------------- launches (arguments already checked) ----------------

inline PackShape pack_shape(u32 in_dim, u32 k, u32 log_n, u32 count, u32 log_basis, u32 ell, u32 drop) {
    const u32 n = 1u << log_n;
    const u32 per = n >= 4 ? 4 : 2;  // U
    PackShape sh{in_dim, k, log_n, count, log_basis, ell, drop, 0, 0, 0};
    sh.tile = std::min<u32>(n, kPackLanes * per);
    const u32 count_pad = (count + per - 1) / per * per;
    sh.block_j = std::min<u32>(std::min<u32>(count_pad, kPackMaxJ), kPackDig / ell / per * per);
    sh.ki = std::max<u32>(1, std::min<u32>(in_dim, kPackDig / (ell * sh.block_j)));
    return sh;
}

template <class W>
int launch_pack_keyswitch(const W *lwe_in, const W *pksk, W *glwe_out, PackShape sh, u64 batch, hipStream_t s) {
    const u32 n = 1u << sh.log_n;
    const u32 gx = (sh.k + 1) * (n / sh.tile);
    const u64 in_words = (u64)sh.count * ((u64)sh.in_dim + 1), out_words = (u64)(sh.k + 1) << sh.log_n;
    return launch_y_slices(batch, [&](u64 done, u32 cur) {
        return launch_grid(n >= 4 ? tfhe_pack_keyswitch_kernel<W, 4> : tfhe_pack_keyswitch_kernel<W, 2>, dim3(gx, cur), 0, s,
                           lwe_in + done * in_words, pksk, glwe_out + done * out_words, sh);
    });
}

template <class W>
int launch_pksk_message(W *pksk, const W *key_in, u32 k, u32 log_n, u32 ell, u32 log_basis, u32 drop, u64 rows,
                        hipStream_t s) {
    return launch_flat(tfhe_pksk_add_message_kernel<W>, rows, s, pksk, key_in, k, log_n, ell, log_basis, drop);
}

template <class W>
int launch_extract_first_few(const W *glwe, W *multi, u32 k, u32 log_n, u32 count, u64 batch, hipStream_t s) {
    return launch_flat(tfhe_extract_first_few_kernel<W>, batch * (((u64)k << log_n) + count), s, glwe, multi, k, log_n, count);
}

template <class W>
int launch_multimsg_extract(const W *multi, W *lwe, u32 k, u32 log_n, u32 count, u64 batch, hipStream_t s) {
    return launch_flat(tfhe_multimsg_extract_kernel<W>, batch * count * (((u64)k << log_n) + 1), s, multi, lwe, k, log_n,
                       count);
}

// ---------------- the entry points ----------------

// tfhe_keyswitch_dimensions' refusals, then count (which needs the table's N)
template <class W>
int pack_check(const pfhe_fft *f, size_t k, size_t len_in, size_t in_dimension, size_t count, size_t len_pksk,
               uint32_t log_basis, size_t decompose_length, size_t len_out, PackShape &sh) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(tfhe_keyswitch_dimensions<W>("packing key switch: glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2", f, k, in_dimension, log_basis, decompose_length, ell, drop));
    if (count == 0 || count > f->n) {
        set_last_error("packing key switch: count must be in 1..N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const size_t group = count * (in_dimension + 1), glwe = (k + 1) * f->n;
    if (len_in % group != 0 || len_pksk != in_dimension * ell * glwe || len_out != len_in / group * glwe) {
        set_last_error("packing key switch: lwe_in must be batch*count*(in_dimension+1) words, pksk in_dimension*ell*(k+1)*N "
                       "and glwe_out batch*(k+1)*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    sh = pack_shape((u32)in_dimension, (u32)k, f->log_n, (u32)count, log_basis, ell, drop);
    return PFHE_OK;
}

template <class W>
int pack_keyswitch(Form form, const pfhe_fft *f, size_t k, const W *lwe_in, size_t len_in, size_t in_dimension, size_t count,
                   const W *pksk, size_t len_pksk, uint32_t log_basis, size_t decompose_length, W *glwe_out, size_t len_out,
                   hipStream_t s) {
    PackShape sh{};
    PFHE_TRY(pack_check<W>(f, k, len_in, in_dimension, count, len_pksk, log_basis, decompose_length, len_out, sh));
    if (len_in == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(pksk, len_pksk * sizeof(W)),
                             stage_out(glwe_out, len_out * sizeof(W))};
    return stateless_call(f->device, form, bufs, "packing key switch: the output must not overlap an input", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_pack_keyswitch<W>((const W *)d[0], (const W *)d[1], (W *)d[2], sh,
                                                              len_in / (count * (in_dimension + 1)), st);
                          });
}

template <class W>
int pksk_generate_dev(const pfhe_fft *f, size_t k, const W *key_in, size_t in_dimension, const W *glwe_key, size_t len_glwe_key,
                      uint32_t log_basis, size_t decompose_length, W *pksk, size_t len, hipStream_t s) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(tfhe_keyswitch_dimensions<W>("packing key: glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2", f, k, in_dimension, log_basis, decompose_length, ell, drop));
    if (len_glwe_key != k * f->n || len != in_dimension * ell * (k + 1) * f->n) {
        set_last_error("packing key: glwe_key must be k*N words and pksk in_dimension*ell*(k+1)*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    const StageBuf bufs[] = {stage_in(key_in, in_dimension * sizeof(W)), stage_in(glwe_key, len_glwe_key * sizeof(W)),
                             stage_inout(pksk, len * sizeof(W))};
    return stateless_call(
        f->device, Form::kDevice, bufs, "packing key: the keys must not overlap pksk", s,
        [&](void *const *d, hipStream_t st) {
            PFHE_TRY(glwe_body_add(f, k, (W *)d[2], len, (const W *)d[1], len_glwe_key, st));
            return launch_pksk_message<W>((W *)d[2], (const W *)d[0], (u32)k, f->log_n, ell, log_basis, drop,
                                          (u64)in_dimension * ell, st);
        },
        [&] { return in_dimension * ell > 0x7fffffffull ? PFHE_ERR_BAD_LENGTH : PFHE_OK; });
}

// the table, the dimension and count as pfhe_tfhe_sample_extract checks its table, dimension and index
inline int multimsg_dimensions(const pfhe_fft *f, size_t k, size_t count) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(require_glwe_dimension(k, "multi-message extraction: glwe_dimension must be in 1..64"));
    if (count == 0 || count > f->n) {
        set_last_error("multi-message extraction: count must be in 1..N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    return PFHE_OK;
}

template <class W>
int first_few(Form form, const pfhe_fft *f, size_t k, const W *glwe, size_t len_glwe, size_t count, W *multi, size_t len_multi,
              hipStream_t s) {
    PFHE_TRY(multimsg_dimensions(f, k, count));
    const size_t in_words = (k + 1) * f->n, out_words = k * f->n + count;
    if (len_glwe % in_words != 0 || len_multi != len_glwe / in_words * out_words) {
        set_last_error("multi-message extraction: glwe must be batch*(k+1)*N words and multi batch*(k*N+count)");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_glwe == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(glwe, len_glwe * sizeof(W)), stage_out(multi, len_multi * sizeof(W))};
    return stateless_call(f->device, form, bufs, "multi-message extraction: the output must not overlap the input", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_extract_first_few<W>((const W *)d[0], (W *)d[1], (u32)k, f->log_n, (u32)count,
                                                                 len_glwe / in_words, st);
                          });
}

template <class W>
int multimsg_extract(Form form, const pfhe_fft *f, size_t k, const W *multi, size_t len_multi, size_t count, W *lwe,
                     size_t len_lwe, hipStream_t s) {
    PFHE_TRY(multimsg_dimensions(f, k, count));
    const size_t in_words = k * f->n + count, out_words = count * (k * f->n + 1);
    if (len_multi % in_words != 0 || len_lwe != len_multi / in_words * out_words) {
        set_last_error("multi-message expansion: multi must be batch*(k*N+count) words and lwe batch*count*(k*N+1)");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_multi == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(multi, len_multi * sizeof(W)), stage_out(lwe, len_lwe * sizeof(W))};
    return stateless_call(f->device, form, bufs, "multi-message expansion: the output must not overlap the input", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_multimsg_extract<W>((const W *)d[0], (W *)d[1], (u32)k, f->log_n, (u32)count,
                                                                len_multi / in_words, st);
                          });
}

}  // namespace
}  // namespace pfhe

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_PACK_FAMILY(P, CW, W)                                                                                       \
    PFHE_ENTRY(P##_pack_keyswitch_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *lwe_in_dev, size_t len_in, \
                size_t in_dimension, size_t count, const CW *pksk_dev, size_t len_pksk, uint32_t log_basis,              \
                size_t decompose_length, CW *glwe_out_dev, size_t len_out, void *stream),                                \
               pack_keyswitch<W>(Form::kDevice, fft, glwe_dimension, (const W *)lwe_in_dev, len_in, in_dimension, count, \
                                 (const W *)pksk_dev, len_pksk, log_basis, decompose_length, (W *)glwe_out_dev, len_out, \
                                 (hipStream_t)stream))                                                                   \
    PFHE_ENTRY(P##_pack_keyswitch, (const pfhe_fft *fft, size_t glwe_dimension, const CW *lwe_in, size_t len_in,         \
                size_t in_dimension, size_t count, const CW *pksk, size_t len_pksk, uint32_t log_basis,                  \
                size_t decompose_length, CW *glwe_out, size_t len_out),                                                  \
               pack_keyswitch<W>(Form::kHost, fft, glwe_dimension, (const W *)lwe_in, len_in, in_dimension, count,       \
                                 (const W *)pksk, len_pksk, log_basis, decompose_length, (W *)glwe_out, len_out,         \
                                 nullptr))                                                                               \
    PFHE_ENTRY(P##_pksk_generate_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *key_in_dev,                 \
                size_t in_dimension, const CW *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,                    \
                size_t decompose_length, CW *pksk_dev, size_t len_pksk, void *stream),                                   \
               pksk_generate_dev<W>(fft, glwe_dimension, (const W *)key_in_dev, in_dimension, (const W *)glwe_key_dev,   \
                                    len_glwe_key, log_basis, decompose_length, (W *)pksk_dev, len_pksk,                  \
                                    (hipStream_t)stream))                                                                \
    PFHE_ENTRY(P##_sample_extract_first_few_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *glwe_dev,        \
                size_t len_glwe, size_t count, CW *multi_dev, size_t len_multi, void *stream),                           \
               first_few<W>(Form::kDevice, fft, glwe_dimension, (const W *)glwe_dev, len_glwe, count, (W *)multi_dev,    \
                            len_multi, (hipStream_t)stream))                                                             \
    PFHE_ENTRY(P##_sample_extract_first_few, (const pfhe_fft *fft, size_t glwe_dimension, const CW *glwe,                \
                size_t len_glwe, size_t count, CW *multi, size_t len_multi),                                             \
               first_few<W>(Form::kHost, fft, glwe_dimension, (const W *)glwe, len_glwe, count, (W *)multi, len_multi,   \
                            nullptr))                                                                                    \
    PFHE_ENTRY(P##_multimsg_extract_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *multi_dev,               \
                size_t len_multi, size_t count, CW *lwe_dev, size_t len_lwe, void *stream),                              \
               multimsg_extract<W>(Form::kDevice, fft, glwe_dimension, (const W *)multi_dev, len_multi, count,           \
                                   (W *)lwe_dev, len_lwe, (hipStream_t)stream))                                          \
    PFHE_ENTRY(P##_multimsg_extract, (const pfhe_fft *fft, size_t glwe_dimension, const CW *multi, size_t len_multi,     \
                size_t count, CW *lwe, size_t len_lwe),                                                                  \
               multimsg_extract<W>(Form::kHost, fft, glwe_dimension, (const W *)multi, len_multi, count, (W *)lwe,       \
                                   len_lwe, nullptr))

extern "C" {

PFHE_PACK_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_PACK_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_PACK_FAMILY

}  // extern "C"
