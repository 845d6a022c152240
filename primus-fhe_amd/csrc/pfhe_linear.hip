// pfhe_linear.hip — the leveled step between two bootstraps: a batched linear layer with clear integer weights on LWE
// ciphertexts (include/pfhe.h: pfhe_lwe{,32}_linear*).  DESIGN.md §25 states the rule.
//
//   out[e][o][c] = sum_{i < in_features} W[o][i] in[e][i][c] + [c = dimension] bias[o]      (mod 2^BITS)
//
// word for word out_features chains of Lwe::add_mul_scalar_assign (primus_lattice/src/lwe/single_message.rs:262-268) per
// input vector e.  A GEMM modulo 2^BITS: M = out_features, K = in_features, dimension + 1 columns, once per vector.
//
//   lwe_linear_kernel      word weights (the reference's `scalar: T`): the register tile of the key switch
//                          (pfhe_tfhe_exact_device.hpp) with the weights where the digits are, on the vector ALU.
//   lwe_linear_i8_kernel   int8 weights: every word split into its bytes, one i32 matrix-core accumulator per byte plane
//                          (v_mfma_i32_16x16x64_i8), the planes folded into words at least every 2^16 input rows.
// Exact integer arithmetic modulo 2^BITS; no atomics, no scratch memory, no allocation.  Both forms of a call go through
// stateless_call of pfhe_tfhe_host.hpp.
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "pfhe_capi_internal.hpp"
#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_host.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// ---------------- word weights ----------------
//
// One workgroup owns kKsWaves * R outputs x kKsTileN columns of one input vector; a thread owns R outputs (its wave's) x
// kKsCols columns (its lane's, kKsLanes apart) and keeps their sums in registers.  The workgroup walks the inputs in groups
// of kKsMaxRows: first the group's weights go to LDS as [input of the group][output of the tile] (read coalesced along the
// inputs; the pitch is odd, so the writes of a wave fall into different banks), then every thread streams the group's
// ciphertext rows, coalesced along the columns and kKsUnroll rows in flight at a time, against the weights of its outputs,
// which all lanes of a wave read from one LDS address.  R is the tile's only parameter: the words do not depend on it.

template <class W, int R>
__global__ __launch_bounds__(kThreads) void lwe_linear_kernel(const W *__restrict__ lwe_in, const W *__restrict__ weights,
                                                              const W *__restrict__ bias, W *__restrict__ lwe_out, u32 row,
                                                              u32 in_features, u32 out_features, u32 col_tiles, u32 first_tile) {
    constexpr int kTile = kKsWaves * R, kPitch = kTile + 1;
    __shared__ W wts[kKsMaxRows * kPitch];
    const u32 lane = threadIdx.x % kKsLanes, wave = threadIdx.x / kKsLanes;
    const u64 e = blockIdx.x / col_tiles;
    const u32 c0 = (u32)(blockIdx.x - e * col_tiles) * kKsTileN + lane;
    const u32 o0 = (first_tile + blockIdx.y) * kTile;
    W acc[R][kKsCols] = {};
    // the columns of this thread; a column past the end reads the last one instead (its sums are never stored), so that no
    // load of the inner loop sits behind a branch
    const W *x[kKsCols];
#pragma unroll
    for (int c = 0; c < kKsCols; ++c) x[c] = lwe_in + e * in_features * row + min(c0 + c * kKsLanes, row - 1);
    // the weights this thread stages in every group: input ii of the group, outputs oo, oo + kKsWaves, ...
    const u32 ii = threadIdx.x % kKsMaxRows, oo = threadIdx.x / kKsMaxRows;
    for (u32 i0 = 0; i0 < in_features; i0 += kKsMaxRows) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const u32 o = oo + j * (kThreads / kKsMaxRows);
            const bool live = o0 + o < out_features && i0 + ii < in_features;
            wts[ii * kPitch + o] = live ? weights[(u64)(o0 + o) * in_features + i0 + ii] : (W)0;
        }
        __syncthreads();
        const u32 rows = min(kKsMaxRows, in_features - i0);
        u32 r0 = 0;
        // kKsUnroll rows at a time: all their words are requested before the first is used
        for (; r0 + kKsUnroll <= rows; r0 += kKsUnroll) {
            W xv[kKsUnroll][kKsCols];
#pragma unroll
            for (int u = 0; u < kKsUnroll; ++u)
#pragma unroll
                for (int c = 0; c < kKsCols; ++c) xv[u][c] = x[c][(size_t)u * row];
#pragma unroll
            for (int u = 0; u < kKsUnroll; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const W w = wts[(r0 + u) * kPitch + wave * R + r];
#pragma unroll
                    for (int c = 0; c < kKsCols; ++c) acc[r][c] += w * xv[u][c];
                }
#pragma unroll
            for (int c = 0; c < kKsCols; ++c) x[c] += (size_t)kKsUnroll * row;
        }
        for (; r0 < rows; ++r0) {
            W xv[kKsCols];
#pragma unroll
            for (int c = 0; c < kKsCols; ++c) xv[c] = x[c][0];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const W w = wts[r0 * kPitch + wave * R + r];
#pragma unroll
                for (int c = 0; c < kKsCols; ++c) acc[r][c] += w * xv[c];
            }
#pragma unroll
            for (int c = 0; c < kKsCols; ++c) x[c] += row;
        }
        __syncthreads();  // the next group overwrites the weights
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32 o = o0 + wave * R + r;
        if (o >= out_features) continue;
#pragma unroll
        for (int c = 0; c < kKsCols; ++c) {
            const u32 col = c0 + c * kKsLanes;
            if (col >= row) continue;
            const W b = bias && col == row - 1 ? bias[o] : (W)0;  // the body's thread adds the bias
            lwe_out[(e * out_features + o) * row + col] = acc[r][c] + b;
        }
    }
}

// ---------------- int8 weights, on the matrix cores ----------------
//
// x = sum_b x_b 2^(8b) with unsigned bytes x_b, so  sum_i W[o][i] x[i] = sum_b 2^(8b) sum_i W[o][i] x_b[i].  The i8 MFMA
// takes signed bytes: it is fed x_b - 128 (x_b ^ 0x80), and sum_i W[o][i] 128 comes back through one more accumulator
// against a plane of ones, times 0x80..80 as a word.  v_mfma_i32_16x16x64_i8: A = 16 outputs x 64 inputs of weights, B =
// 64 inputs x 16 columns of one byte plane, D = 16 x 16 i32.  A and B take their k index from the lane and the byte in the
// same way, so only "A's row and B's column are lane & 15" and the C/D map (column lane & 15, rows 4 (lane >> 4) + reg)
// matter; tests/test_gpu_lwe_linear.py checks both with asymmetric data.
//
// One workgroup owns 16 MT outputs x 64 columns of one input vector, a wave 16 MT outputs x 16 columns.  Per step of 64
// inputs: the workgroup stages the weights into LDS (bytes past either end are zero); a lane loads the 16 words of its
// column and its quarter of the step (a row past the end is clamped: its weights are zero), transposes their bytes into
// plane fragments with v_perm_b32, and issues BITS/8 + 1 MFMAs per 16 outputs.  Every product is at most 2^14 in
// magnitude, so an accumulator stays below 2^30 for kFoldSteps steps (2^16 inputs); then the planes are folded into the
// word sums, wrapping, and cleared.  Nothing relies on an i32 overflow.

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kI8Step = 64;       // inputs per MFMA
constexpr int kI8Pitch = 64 + 16; // bytes between two outputs' weights in LDS: 16-byte aligned, rows 20 banks apart
constexpr u32 kFoldSteps = 1024;  // 2^16 inputs between two folds

template <class W>
__device__ __forceinline__ W sign_extended(int v) {
    return (W)(typename std::make_signed<W>::type)v;
}

// byte b of four words -> one dword of plane b, in the words' order, for b = 0..3
__device__ __forceinline__ void transpose_bytes(const u32 (&w)[4], u32 (&p)[4]) {
    const u32 lo01 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u);
    const u32 lo23 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(w[3], w[2], 0x07030602u);
    p[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    p[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    p[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    p[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

template <class W, int MT>
__global__ __launch_bounds__(kThreads) void lwe_linear_i8_kernel(const W *__restrict__ lwe_in, const int8_t *__restrict__ weights,
                                                                 const W *__restrict__ bias, W *__restrict__ lwe_out, u32 row,
                                                                 u32 in_features, u32 out_features, u32 col_tiles,
                                                                 u32 first_tile) {
    constexpr int kPlanes = sizeof(W), kTile = 16 * MT;
    __shared__ __attribute__((aligned(16))) int8_t wts[kTile * kI8Pitch];
    const u32 lane = threadIdx.x % kKsLanes, wave = threadIdx.x / kKsLanes;
    const u32 lr = lane & 15, lq = lane >> 4;
    const u64 e = blockIdx.x / col_tiles;
    const u32 col = (u32)(blockIdx.x - e * col_tiles) * 64 + wave * 16 + lr;
    const u32 o0 = (first_tile + blockIdx.y) * kTile;
    const W *x = lwe_in + e * in_features * row + min(col, row - 1);
    v4i plane[MT][kPlanes], ones[MT];
    W acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int b = 0; b < kPlanes; ++b) plane[m][b] = v4i{0, 0, 0, 0};
        ones[m] = v4i{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = 0;
    }
    // acc += sum_b plane_b 2^(8b) + ones 0x80..80, and the planes start again
    auto fold = [&] {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                W s = sign_extended<W>(ones[m][r]) * (W)0x8080808080808080ull;
#pragma unroll
                for (int b = 0; b < kPlanes; ++b) s += (W)(sign_extended<W>(plane[m][b][r]) << (8 * b));
                acc[m][r] += s;
            }
#pragma unroll
            for (int b = 0; b < kPlanes; ++b) plane[m][b] = v4i{0, 0, 0, 0};
            ones[m] = v4i{0, 0, 0, 0};
        }
    };
    u32 steps = 0;
    for (u32 i0 = 0; i0 < in_features; i0 += kI8Step) {
        // 16 MT outputs x 64 weight bytes: one dword per thread and 16 outputs
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const u32 o = m * 16 + threadIdx.x / 16, k = (threadIdx.x % 16) * 4;
            u32 packed = 0;
            if (o0 + o < out_features) {
                const int8_t *w = weights + (u64)(o0 + o) * in_features;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + k + j < in_features) packed |= (u32)(uint8_t)w[i0 + k + j] << (8 * j);
            }
            *reinterpret_cast<u32 *>(&wts[o * kI8Pitch + k]) = packed;
        }
        __syncthreads();
        // the 16 words of this lane's column and quarter, all requested before the first is used
        W xv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) xv[j] = x[(u64)min(i0 + lq * 16 + j, in_features - 1) * row];
        v4i a[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) a[m] = *reinterpret_cast<const v4i *>(&wts[(m * 16 + lr) * kI8Pitch + lq * 16]);
        // frag[b][g]: byte b of words 4g .. 4g+3, less 128
        u32 frag[kPlanes][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int h = 0; h < kPlanes / 4; ++h) {
                u32 w[4], p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = (u32)((u64)xv[4 * g + j] >> (32 * h));
                transpose_bytes(w, p);
#pragma unroll
                for (int b = 0; b < 4; ++b) frag[4 * h + b][g] = p[b] ^ 0x80808080u;
            }
        }
        const v4i all_ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int b = 0; b < kPlanes; ++b) {
                const v4i f = {(int)frag[b][0], (int)frag[b][1], (int)frag[b][2], (int)frag[b][3]};
                plane[m][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], f, plane[m][b], 0, 0, 0);
            }
            ones[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], all_ones, ones[m], 0, 0, 0);
        }
        if (++steps == kFoldSteps) {
            fold();
            steps = 0;
        }
        __syncthreads();  // the next step overwrites the weights
    }
    fold();
    if (col >= row) return;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const u32 o = o0 + m * 16 + lq * 4 + r;
            if (o >= out_features) continue;
            const W b = bias && col == row - 1 ? bias[o] : (W)0;
            lwe_out[(e * out_features + o) * row + col] = acc[m][r] + b;
        }
    }
}

// ---------------- launches (arguments already checked) ----------------

struct LinearShape {
    u32 row, in_features, out_features;
    u64 batch;
};

// x: the column tiles of every vector; y: the output tiles, in slices
template <class K, class W, class S>
int launch_linear_tiles(K kernel, u32 tile_outputs, u32 tile_cols, const W *in, const S *weights, const W *bias, W *out,
                        LinearShape sh, hipStream_t s) {
    const u32 col_tiles = (sh.row + tile_cols - 1) / tile_cols;
    const u64 groups = sh.batch * col_tiles;
    return launch_y_slices((sh.out_features + tile_outputs - 1) / tile_outputs, [&](u64 first_tile, u32 tiles) {
        return launch_grid(kernel, dim3((u32)groups, tiles), 0, s, in, weights, bias, out, sh.row, sh.in_features,
                           sh.out_features, col_tiles, (u32)first_tile);
    });
}

// Which R runs.  A larger tile reads every ciphertext row fewer times, a smaller one gives the grid more workgroups, and
// below about two workgroups per compute unit the grid decides (tools/microbench13_linear_tiles.hip, DESIGN.md §25: at batch
// 1 R = 1 is 2 to 3 times faster than R = 8 even at 32 outputs).  So: the largest R whose grid still has kLinMinGroups
// workgroups, never one whose half would hold all the outputs; R = 1 when no grid is that long.
constexpr u64 kLinMinGroups = 512;  // two per compute unit

template <class W, int R>
int launch_linear_r(const W *in, const W *weights, const W *bias, W *out, LinearShape sh, hipStream_t s) {
    return launch_linear_tiles(lwe_linear_kernel<W, R>, kKsWaves * R, kKsTileN, in, weights, bias, out, sh, s);
}

inline int linear_rows_per_thread(LinearShape sh) {
    const u64 groups = sh.batch * ((sh.row + kKsTileN - 1) / kKsTileN);
    for (u32 r = kKsRows; r > 1; r /= 2) {
        const u32 tile = kKsWaves * r;
        if (sh.out_features > tile / 2 && (sh.out_features + tile - 1) / tile * groups >= kLinMinGroups) return (int)r;
    }
    return 1;
}

template <class W>
int launch_linear(const W *in, const W *weights, const W *bias, W *out, LinearShape sh, hipStream_t s) {
    switch (linear_rows_per_thread(sh)) {
        case 8: return launch_linear_r<W, 8>(in, weights, bias, out, sh, s);
        case 4: return launch_linear_r<W, 4>(in, weights, bias, out, sh, s);
        case 2: return launch_linear_r<W, 2>(in, weights, bias, out, sh, s);
        default: return launch_linear_r<W, 1>(in, weights, bias, out, sh, s);
    }
}

template <class W>
int launch_linear(const W *in, const int8_t *weights, const W *bias, W *out, LinearShape sh, hipStream_t s) {
    if (sh.out_features <= 16) return launch_linear_tiles(lwe_linear_i8_kernel<W, 1>, 16, 64, in, weights, bias, out, sh, s);
    return launch_linear_tiles(lwe_linear_i8_kernel<W, 2>, 32, 64, in, weights, bias, out, sh, s);
}

// ---------------- the stateless entry points ----------------

// S: the weights' type, W (the reference's scalar) or int8_t.  The ranges, the lengths, the empty batch; a null pointer, a
// bias pointer with no length; then the tail (an overlap), the gate (a grid too long, the device index) and the device.
template <class W, class S>
int lwe_linear(Form form, int device, const W *lwe_in, size_t len_in, size_t dimension, const S *weights, size_t len_weights,
               size_t in_features, size_t out_features, const W *bias, size_t len_bias, W *lwe_out, size_t len_out,
               hipStream_t s) {
    constexpr const char *kRange = "LWE linear: dimension, in_features and out_features must be in 1..2^31-2";
    PFHE_TRY(require_lwe_dimension(dimension, kRange));
    PFHE_TRY(require_lwe_dimension(in_features, kRange));
    PFHE_TRY(require_lwe_dimension(out_features, kRange));
    const size_t row = dimension + 1, in_words = in_features * row, out_words = out_features * row;  // below 2^62
    const size_t batch = len_in / in_words;
    if (len_in % in_words != 0 || len_weights != out_features * in_features || (len_bias != 0 && len_bias != out_features) ||
        len_out % out_words != 0 || len_out / out_words != batch) {
        set_last_error("LWE linear: lwe_in must be batch*in_features*(dimension+1) words, weights out_features*in_features "
                       "scalars, bias none or out_features words and lwe_out batch*out_features*(dimension+1)");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (batch == 0) return PFHE_OK;
    const LinearShape sh{(u32)row, (u32)in_features, (u32)out_features, batch};
    // a null bias is a buffer of no bytes: it is neither refused nor staged
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(weights, len_weights * sizeof(S)),
                             stage_in(bias, len_bias * sizeof(W)), stage_out(lwe_out, len_out * sizeof(W))};
    // the tail's own first refusal, here so that the bias pointer and its length disagreeing comes right behind it
    PFHE_TRY(refuse_null(bufs));
    if (bias && !len_bias) {
        set_last_error("LWE linear: a bias pointer with len_bias 0");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    return stateless_call(
        device, form, bufs, "LWE linear: the output must not overlap an input", s,
        [&](void *const *d, hipStream_t st) {
            return launch_linear<W>((const W *)d[0], (const S *)d[1], (const W *)d[2], (W *)d[3], sh, st);
        },
        [&] {
            // the column tiles of the whole batch are one grid dimension: tiles of 128 columns (words) or 64 (int8)
            constexpr size_t kTileCols = std::is_same<S, int8_t>::value ? 64 : kKsTileN;
            if (batch > 0x7fffffffull / ((row + kTileCols - 1) / kTileCols)) {
                set_last_error("LWE linear: batch times the column tiles of a ciphertext exceeds 2^31-1 workgroups");
                return (int)PFHE_ERR_BAD_LENGTH;
            }
            return capi_check_device(device);
        });
}

}  // namespace
}  // namespace pfhe

// The entry points of one word width.  P: pfhe_lwe / pfhe_lwe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_LINEAR_FORMS(P, CW, W, NAME, CS, S)                                                                           \
    PFHE_ENTRY(P##_##NAME##_dev, (int device, const CW *lwe_in_dev, size_t len_in, size_t dimension, const CS *weights_dev, \
                size_t len_weights, size_t in_features, size_t out_features, const CW *bias_dev, size_t len_bias,          \
                CW *lwe_out_dev, size_t len_out, void *stream),                                                            \
               lwe_linear<W, S>(Form::kDevice, device, (const W *)lwe_in_dev, len_in, dimension, (const S *)weights_dev,   \
                                len_weights, in_features, out_features, (const W *)bias_dev, len_bias, (W *)lwe_out_dev,   \
                                len_out, (hipStream_t)stream))                                                             \
    PFHE_ENTRY(P##_##NAME, (int device, const CW *lwe_in, size_t len_in, size_t dimension, const CS *weights,              \
                size_t len_weights, size_t in_features, size_t out_features, const CW *bias, size_t len_bias, CW *lwe_out, \
                size_t len_out),                                                                                           \
               lwe_linear<W, S>(Form::kHost, device, (const W *)lwe_in, len_in, dimension, (const S *)weights, len_weights, \
                                in_features, out_features, (const W *)bias, len_bias, (W *)lwe_out, len_out, nullptr))
#define PFHE_LINEAR_FAMILY(P, CW, W)              \
    PFHE_LINEAR_FORMS(P, CW, W, linear, CW, W)    \
    PFHE_LINEAR_FORMS(P, CW, W, linear_i8, int8_t, int8_t)

extern "C" {

PFHE_LINEAR_FAMILY(pfhe_lwe, uint64_t, u64)
PFHE_LINEAR_FAMILY(pfhe_lwe32, uint32_t, u32)
#undef PFHE_LINEAR_FAMILY
#undef PFHE_LINEAR_FORMS

}  // extern "C"
