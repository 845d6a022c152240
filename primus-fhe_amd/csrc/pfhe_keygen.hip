// pfhe_keygen.hip — the ends of the TFHE bootstrap: LWE / GLWE body computation (encryption and phase), the GGSW gadget
// term, and the bootstrapping key (classic and multi-bit layout) and key-switch key in the layouts the existing calls take
// (include/pfhe.h: pfhe_tfhe{,32}_lwe_body_mac*, _glwe_body_mac*, _ggsw_add_gadget_dev, _bsk_generate_dev, _ksk_generate_dev).
//
//   LWE body    b_e <- b_e +- <a_e, s>: Lwe::generate_random_zero_sample (primus_lattice/src/lwe/single_message.rs:94-125) with
//               the caller's randomness already in the buffer (add), or the phase b - <a,s> written into the body slot
//   GLWE body   B_e <- B_e +- sum_j A_{e,j} (*) z_j, negacyclic: Rlwe::generate_random_zero_sample (rlwe/coeff.rs:92-121)
//   gadget      m 2^(drop_bits + l log_basis) onto coefficient 0 of component r of row (r, l) of a torus-form GGSW
//   keys        the three above in a row, then the existing forward transform for the bootstrapping key
// No random number is drawn here: masks and noise are the caller's.  Every step is exact integer arithmetic modulo 2^BITS;
// no atomics, no scratch memory.  The body calls ACCUMULATE into the body slot, so running one twice adds the product twice.
// Launches and host forms go through pfhe_tfhe_host.hpp; the GLWE body keeps its own 2-D grid.
#include <algorithm>
#include <cstdint>

#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

constexpr int kWave = 64, kWavesPerBlock = kThreads / kWave;

// ---------------- LWE body ----------------

template <class W>
__device__ __forceinline__ W wave_sum(W v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// One wave per ciphertext, four ciphertexts per workgroup: lane l sums a[l + 64u] s[l + 64u] (coalesced over the mask), a
// butterfly of shuffles adds the 64 partial sums and lane 0 updates the body.  With row_key (a key-switch key): row (i, j)
// also gets row_key[i] 2^(drop + j log_basis), rows = ell levels per key element.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_lwe_body_mac_kernel(W *__restrict__ lwe, const W *__restrict__ key, u32 dim,
                                                                     u64 batch, int subtract, const W *__restrict__ row_key,
                                                                     u32 ell, u32 log_basis, u32 drop) {
    const u32 lane = threadIdx.x % kWave;
    const u64 e = (u64)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (e >= batch) return;  // the whole wave leaves
    W *ct = lwe + e * ((u64)dim + 1);
    W sum = 0;
    for (u32 i = lane; i < dim; i += kWave) sum += ct[i] * key[i];
    sum = wave_sum(sum);
    if (lane != 0) return;
    W b = subtract ? ct[dim] - sum : ct[dim] + sum;
    if (row_key) b += row_key[e / ell] << (drop + (u32)(e % ell) * log_basis);
    ct[dim] = b;
}

// ---------------- GLWE body ----------------
//
// A 256-thread workgroup owns one ciphertext and a tile of T = min(N, 256 U) output coefficients; thread t owns the
// coefficients i = i0 + t + 256u, u < U, and keeps their sums in registers.  For N < 256 the lanes t >= N stay idle (one
// ciphertext per workgroup whatever N).  Per mask polynomial the key coefficients are walked in blocks of J: the window of
// the mask that the tile needs against such a block, A[(i0 - j0 - J + 1 + x) mod N] for x < L = min(N, T + J - 1), is
// staged in LDS; J = N (the whole polynomial, staged once) while N words fit kGlweLdsBytes, half of that otherwise, so that
// two workgroups fit a CU's 160 KiB either way.  At a given j the lanes read consecutive LDS words; z[j] is the same for
// the whole workgroup, and a zero key coefficient is skipped by all of it.
constexpr size_t kGlweLdsBytes = 64 * 1024;
constexpr int kGlweMaxU = 8;

struct GlweMacShape {
    u32 k, log_n;
    u32 block_j;  // J
    u32 window;   // L
};

template <class W, int U>
__global__ __launch_bounds__(kThreads) void tfhe_glwe_body_mac_kernel(W *__restrict__ glwe, const W *__restrict__ z,
                                                                      GlweMacShape s, int subtract) {
    extern __shared__ __align__(16) unsigned char glwe_mac_lds[];
    W *win = reinterpret_cast<W *>(glwe_mac_lds);
    const u32 n = 1u << s.log_n, mask = n - 1;
    const u32 t = threadIdx.x;
    const u32 i0 = blockIdx.y * (u32)(kThreads * U);
    W *ct = glwe + (u64)blockIdx.x * ((u64)(s.k + 1) << s.log_n);
    W acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0;
    for (u32 c = 0; c < s.k; ++c) {
        const W *a = ct + ((u64)c << s.log_n);
        const W *zc = z + ((u64)c << s.log_n);
        for (u32 j0 = 0; j0 < n; j0 += s.block_j) {
            const u32 base = (i0 - j0 - (s.block_j - 1)) & mask;
            for (u32 x = t; x < s.window; x += kThreads) win[x] = a[(base + x) & mask];
            __syncthreads();
            for (u32 jj = 0; jj < s.block_j; ++jj) {
                const u32 j = j0 + jj;
                const W zj = zc[j];  // the same word for the whole workgroup
                if (zj == 0) continue;
                const W zneg = (W)0 - zj;
                const u32 off = t + (s.block_j - 1 - jj);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const u32 i = i0 + t + u * kThreads;
                    acc[u] += win[(off + u * kThreads) & mask] * (i < j ? zneg : zj);
                }
            }
            __syncthreads();  // the next block overwrites the window
        }
    }
    W *b = ct + ((u64)s.k << s.log_n);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u32 i = i0 + t + u * kThreads;
        if (i < n) b[i] = subtract ? b[i] - acc[u] : b[i] + acc[u];
    }
}

// ---------------- gadget ----------------

// One thread per (GGSW, row r, level l).  g == 0: the message of GGSW q is msgs[q].  g >= 1 (a multi-bit bootstrapping key):
// GGSW q = t 2^g + j gets prod_b (bit b of j ? s : 1 - s) with s = msgs[t g + b], in wrapping words.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_ggsw_add_gadget_kernel(W *__restrict__ ggsw, const W *__restrict__ msgs, u32 k,
                                                                        u32 log_n, u32 ell, u32 log_basis, u32 drop, u32 g,
                                                                        u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 l = (u32)(t % ell);
    const u64 row = t / ell;  // q (k+1) + r
    const u32 r = (u32)(row % (k + 1));
    const u64 q = row / (k + 1);
    W m;
    if (g == 0) {
        m = msgs[q];
    } else {
        const u64 group = q >> g;
        const u32 j = (u32)(q & ((1u << g) - 1));
        m = 1;
        for (u32 b = 0; b < g; ++b) {
            const W sb = msgs[group * g + b];
            m *= ((j >> b) & 1) ? sb : (W)1 - sb;
        }
    }
    ggsw[(((row * ell + l) * (k + 1) + r) << log_n)] += m << (drop + l * log_basis);
}

// ---------------- launches (arguments already checked) ----------------

template <class W>
int launch_lwe_body_mac(W *lwe, const W *key, u32 dim, u64 batch, int subtract, const W *row_key, u32 ell, u32 log_basis,
                        u32 drop, hipStream_t s) {
    return launch_groups(tfhe_lwe_body_mac_kernel<W>, (batch + kWavesPerBlock - 1) / kWavesPerBlock, 0, s, lwe, key, dim, batch,
                         subtract, row_key, ell, log_basis, drop);
}

template <class W, int U>
int launch_glwe_u(W *glwe, const W *z, GlweMacShape sh, u32 tiles, u64 batch, int subtract, hipStream_t s) {
    return launch_grid(tfhe_glwe_body_mac_kernel<W, U>, dim3((u32)batch, tiles), sh.window * sizeof(W), s, glwe, z, sh, subtract);
}

template <class W>
int launch_glwe_body_mac(W *glwe, const W *z, u32 k, u32 log_n, u64 batch, int subtract, hipStream_t s) {
    if (batch > 0x7fffffffull) return PFHE_ERR_BAD_LENGTH;
    const u32 n = 1u << log_n;
    const u32 per_thread = std::min<u32>(std::max<u32>(1, n / kThreads), kGlweMaxU);
    const u32 tile = std::min<u32>(n, per_thread * kThreads);
    const u32 fit = (u32)(kGlweLdsBytes / sizeof(W));
    GlweMacShape sh{k, log_n, 0, 0};
    sh.block_j = n <= fit ? n : fit / 2;
    sh.window = std::min<u32>(n, tile + sh.block_j - 1);
    const u32 tiles = n / tile;
    switch (per_thread) {
    case 1: return launch_glwe_u<W, 1>(glwe, z, sh, tiles, batch, subtract, s);
    case 2: return launch_glwe_u<W, 2>(glwe, z, sh, tiles, batch, subtract, s);
    case 4: return launch_glwe_u<W, 4>(glwe, z, sh, tiles, batch, subtract, s);
    default: return launch_glwe_u<W, 8>(glwe, z, sh, tiles, batch, subtract, s);
    }
}

template <class W>
int launch_gadget(W *ggsw, const W *msgs, u32 k, u32 log_n, u32 ell, u32 log_basis, u32 drop, u32 g, u64 count,
                  hipStream_t s) {
    return launch_flat(tfhe_ggsw_add_gadget_kernel<W>, count * (k + 1) * ell, s, ggsw, msgs, k, log_n, ell, log_basis, drop, g);
}

inline int forward_torus(const pfhe_fft *f, const u64 *in, size_t len, double *out, hipStream_t s) {
    return pfhe_fft_forward_torus_dev(f, (const uint64_t *)in, len, out, len, s);
}
inline int forward_torus(const pfhe_fft *f, const u32 *in, size_t len, double *out, hipStream_t s) {
    return pfhe_fft_forward_torus32_dev(f, in, len, out, len, s);
}

// ---------------- the entry points ----------------

template <class W>
int lwe_body_mac(Form form, int device, W *lwe, size_t len, size_t dimension, const W *key, size_t len_key, int subtract,
                 hipStream_t s) {
    PFHE_TRY(require_lwe_dimension(dimension, "LWE body: dimension must be in 1..2^31-2"));
    if (len_key != dimension || len % (dimension + 1) != 0) {
        set_last_error("LWE body: lwe must be batch*(dimension+1) words and key dimension words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_inout(lwe, len * sizeof(W)), stage_in(key, len_key * sizeof(W))};
    return stateless_call(
        device, form, bufs, "LWE body: the key must not overlap the ciphertexts", s,
        [&](void *const *d, hipStream_t st) {
            return launch_lwe_body_mac<W>((W *)d[0], (const W *)d[1], (u32)dimension, len / (dimension + 1), subtract, nullptr,
                                          1, 0, 0, st);
        },
        [&] { return capi_check_device(device); });
}

template <class W>
int glwe_body_mac(Form form, const pfhe_fft *f, size_t k, W *glwe, size_t len, const W *key, size_t len_key, int subtract,
                  hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(require_glwe_dimension(k, "GLWE body: glwe_dimension must be in 1..64"));
    if (len_key != k * f->n || len % ((k + 1) * f->n) != 0) {
        set_last_error("GLWE body: glwe must be batch*(k+1)*N words and key k*N words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_inout(glwe, len * sizeof(W)), stage_in(key, len_key * sizeof(W))};
    return stateless_call(f->device, form, bufs, "GLWE body: the key must not overlap the ciphertexts", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_glwe_body_mac<W>((W *)d[0], (const W *)d[1], (u32)k, f->log_n,
                                                             len / ((k + 1) * f->n), subtract, st);
                          });
}

// the product plan's checks through the plan's own function, then what a GGSW needs beyond them
template <class W>
int ggsw_shape(const pfhe_fft *f, size_t k, uint32_t log_basis, size_t decompose_length, u32 &ell, u32 &drop) {
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(f, k, log_basis, decompose_length, sh));
    ell = sh.ell;
    drop = sh.drop_bits;
    if (k == 0) {
        set_last_error("GGSW: glwe_dimension must be at least 1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    return PFHE_OK;
}

template <class W>
int ggsw_add_gadget_dev(const pfhe_fft *f, size_t k, uint32_t log_basis, size_t decompose_length, W *ggsw, size_t len,
                        const W *msgs, size_t len_msgs, hipStream_t s) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(ggsw_shape<W>(f, k, log_basis, decompose_length, ell, drop));
    const size_t one = (k + 1) * ell * (k + 1) * f->n;
    if (len % one != 0 || len_msgs != len / one) {
        set_last_error("GGSW gadget: ggsw must be count*(k+1)*ell*(k+1)*N words and messages count words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_inout(ggsw, len * sizeof(W)), stage_in(msgs, len_msgs * sizeof(W))};
    return stateless_call(f->device, Form::kDevice, bufs, "GGSW gadget: the messages must not overlap the GGSWs", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_gadget<W>((W *)d[0], (const W *)d[1], (u32)k, f->log_n, ell, log_basis, drop, 0,
                                                      len_msgs, st);
                          });
}

template <class W>
int bsk_generate_dev(const pfhe_fft *f, size_t k, uint32_t log_basis, size_t decompose_length, size_t grouping, const W *lwe_key,
                     size_t n, const W *glwe_key, size_t len_glwe_key, W *ggsw, size_t len_ggsw, double *bsk, size_t len_bsk,
                     hipStream_t s) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(ggsw_shape<W>(f, k, log_basis, decompose_length, ell, drop));
    if (grouping > kMaxGrouping) {
        set_last_error("bootstrapping key: grouping_factor must be 0 (the classic layout) or in 1..4");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    PFHE_TRY(require_lwe_dimension(n, "bootstrapping key: lwe_dimension must be in 1..2^31-2"));
    if (grouping && n % grouping != 0) {
        set_last_error("bootstrapping key: lwe_dimension must be a multiple of grouping_factor");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const size_t keys = grouping ? (n / grouping) << grouping : n;
    const size_t rows = (k + 1) * ell, glwe = (k + 1) * f->n;
    if (len_glwe_key != k * f->n || len_ggsw != keys * rows * glwe || len_bsk != len_ggsw) {
        set_last_error("bootstrapping key: glwe_key must be k*N words, ggsw_torus keys*(k+1)*ell*(k+1)*N words and bsk_out as "
                       "many complex values, keys = n or (n/g)*2^g");
        return PFHE_ERR_BAD_LENGTH;
    }
    const StageBuf bufs[] = {stage_in(lwe_key, n * sizeof(W)), stage_in(glwe_key, len_glwe_key * sizeof(W)),
                             stage_inout(ggsw, len_ggsw * sizeof(W)), stage_out(bsk, len_bsk * 2 * sizeof(double))};
    PFHE_TRY(refuse_null(bufs));  // ahead of the tail's own: the alignment is judged between the null and the overlap test
    PFHE_REQUIRE_ALIGNED(ggsw);
    PFHE_REQUIRE_ALIGNED(bsk);
    return stateless_call(
        f->device, Form::kDevice, bufs, "bootstrapping key: the outputs must overlap neither each other nor a key", s,
        [&](void *const *d, hipStream_t st) {
            PFHE_TRY(launch_glwe_body_mac<W>((W *)d[2], (const W *)d[1], (u32)k, f->log_n, keys * rows, 0, st));
            PFHE_TRY(launch_gadget<W>((W *)d[2], (const W *)d[0], (u32)k, f->log_n, ell, log_basis, drop, (u32)grouping, keys,
                                      st));
            return forward_torus(f, (const W *)d[2], len_ggsw, (double *)d[3], st);
        },
        [&] { return keys * rows > 0x7fffffffull || len_ggsw / f->n > 0x7fffffffull ? PFHE_ERR_BAD_LENGTH : PFHE_OK; });
}

template <class W>
int ksk_generate_dev(int device, const W *key_in, size_t in_dimension, const W *key_out, size_t out_dimension,
                     uint32_t log_basis, size_t decompose_length, W *ksk, size_t len, hipStream_t s) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), log_basis, decompose_length, ell, drop));
    PFHE_TRY(require_lwe_dimension(in_dimension, "key-switch key: both dimensions must be in 1..2^31-2"));
    PFHE_TRY(require_lwe_dimension(out_dimension, "key-switch key: both dimensions must be in 1..2^31-2"));
    if (len != in_dimension * ell * (out_dimension + 1)) {
        set_last_error("key-switch key: ksk must be in_dimension*ell*(out_dimension+1) words");
        return PFHE_ERR_BAD_LENGTH;
    }
    const StageBuf bufs[] = {stage_in(key_in, in_dimension * sizeof(W)), stage_in(key_out, out_dimension * sizeof(W)),
                             stage_inout(ksk, len * sizeof(W))};
    return stateless_call(
        device, Form::kDevice, bufs, "key-switch key: the keys must not overlap ksk", s,
        [&](void *const *d, hipStream_t st) {
            return launch_lwe_body_mac<W>((W *)d[2], (const W *)d[1], (u32)out_dimension, (u64)in_dimension * ell, 0,
                                          (const W *)d[0], ell, log_basis, drop, st);
        },
        [&] { return capi_check_device(device); });
}

}  // namespace
}  // namespace pfhe

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_KEYGEN_FAMILY(P, CW, W)                                                                                    \
    PFHE_ENTRY(P##_lwe_body_mac_dev, (int device, CW *lwe_dev, size_t len_lwe, size_t dimension, const CW *key_dev,     \
                size_t len_key, int subtract, void *stream),                                                            \
               lwe_body_mac<W>(Form::kDevice, device, (W *)lwe_dev, len_lwe, dimension, (const W *)key_dev, len_key,    \
                               subtract, (hipStream_t)stream))                                                          \
    PFHE_ENTRY(P##_lwe_body_mac, (int device, CW *lwe, size_t len_lwe, size_t dimension, const CW *key, size_t len_key, \
                int subtract),                                                                                          \
               lwe_body_mac<W>(Form::kHost, device, (W *)lwe, len_lwe, dimension, (const W *)key, len_key, subtract,    \
                               nullptr))                                                                                \
    PFHE_ENTRY(P##_glwe_body_mac_dev, (const pfhe_fft *fft, size_t glwe_dimension, CW *glwe_dev, size_t len_glwe,       \
                const CW *key_dev, size_t len_key, int subtract, void *stream),                                         \
               glwe_body_mac<W>(Form::kDevice, fft, glwe_dimension, (W *)glwe_dev, len_glwe, (const W *)key_dev,        \
                                len_key, subtract, (hipStream_t)stream))                                                \
    PFHE_ENTRY(P##_glwe_body_mac, (const pfhe_fft *fft, size_t glwe_dimension, CW *glwe, size_t len_glwe,               \
                const CW *key, size_t len_key, int subtract),                                                           \
               glwe_body_mac<W>(Form::kHost, fft, glwe_dimension, (W *)glwe, len_glwe, (const W *)key, len_key,         \
                                subtract, nullptr))                                                                     \
    PFHE_ENTRY(P##_ggsw_add_gadget_dev, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                \
                size_t decompose_length, CW *ggsw_dev, size_t len_ggsw, const CW *messages_dev, size_t len_messages,    \
                void *stream),                                                                                          \
               ggsw_add_gadget_dev<W>(fft, glwe_dimension, log_basis, decompose_length, (W *)ggsw_dev, len_ggsw,        \
                                      (const W *)messages_dev, len_messages, (hipStream_t)stream))                      \
    PFHE_ENTRY(P##_bsk_generate_dev, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                   \
                size_t decompose_length, size_t grouping_factor, const CW *lwe_key_dev, size_t lwe_dimension,           \
                const CW *glwe_key_dev, size_t len_glwe_key, CW *ggsw_torus_dev, size_t len_ggsw, double *bsk_out_dev,  \
                size_t len_bsk, void *stream),                                                                          \
               bsk_generate_dev<W>(fft, glwe_dimension, log_basis, decompose_length, grouping_factor,                   \
                                   (const W *)lwe_key_dev, lwe_dimension, (const W *)glwe_key_dev, len_glwe_key,        \
                                   (W *)ggsw_torus_dev, len_ggsw, bsk_out_dev, len_bsk, (hipStream_t)stream))           \
    PFHE_ENTRY(P##_ksk_generate_dev, (int device, const CW *key_in_dev, size_t in_dimension, const CW *key_out_dev,     \
                size_t out_dimension, uint32_t log_basis, size_t decompose_length, CW *ksk_dev, size_t len_ksk,         \
                void *stream),                                                                                          \
               ksk_generate_dev<W>(device, (const W *)key_in_dev, in_dimension, (const W *)key_out_dev, out_dimension,  \
                                   log_basis, decompose_length, (W *)ksk_dev, len_ksk, (hipStream_t)stream))

extern "C" {

PFHE_KEYGEN_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_KEYGEN_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_KEYGEN_FAMILY

}  // extern "C"
