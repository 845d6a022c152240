// pfhe_cbs.hip — from an encrypted bit to a GGSW ciphertext: the private functional key switch, its key, and the circuit
// bootstrap handle that runs a blind rotation per level in front of it (include/pfhe.h: pfhe_tfhe{,32}_private_keyswitch*,
// _pfksk_generate_dev, _cbs_*).  No reference counterpart; DESIGN.md §19 states the rules.
//
//   private key switch   out[e][u][l] = - sum_{j <= in_dimension} sum_{t < ell} d_t(c_{e,l,j}) PFKSK[u][j][t] modulo 2^BITS,
//                        c = (a, b): the body word is decomposed as one more mask word (its key is -1).  Row (u, j, t) of the
//                        key encrypts f_u(s'_j g_t), s' = (s_in, -1), f_u(x) = -z_u x for u < k and x on coefficient 0
//                        for u = k, so that the phase of out[e][u][l] is f_u of the input's phase: row (u, l) of a GGSW.
//                        Digits exactly as the LWE key switch forms them (init_carry / digit_word of pfhe_fft_device.hpp).
//   its key              the GLWE body call of pfhe_keygen.hip on all rows of the caller's randomness, then the messages.
//   circuit bootstrap    per input e and level l of the output basis: modulus switch of (a, b + 2^(BITS-2)), ACC_{e,l} =
//                        X^{neg_b[e]} TV_l with TV_l = (0, .., 0, -g_l/2 on every coefficient) written from constants, the
//                        rotation handle on batch * levels accumulators, extraction at index 0 with g_l/2 added to the body,
//                        and the private key switch with levels = ell_cb into the caller's GGSWs.
//   ... with options     (pfhe_tfhe{,32}_cbs_create_with) the rotation is the multi-bit one, and / or ONE rotation
//                        per input serves all levels: the switch to multiples of 2^ceil(log2 ell_cb), TV with -g_l/2 on the
//                        coefficients l mod 2^ceil(log2 ell_cb), extraction of level l at index l.
// The switch, the accumulator and the extraction are the stage kernels of pfhe_tfhe_stages.hip, queued through the launches
// of pfhe_tfhe_handles.hpp with one set of arguments per form; the private key switch and its key are this file's.
// Every step is exact integer arithmetic modulo 2^BITS except the rotation; no atomics, no scratch memory.  Launches and
// the two forms of every call (stateless_call, handle_call) go through pfhe_tfhe_host.hpp; the private key switch keeps
// its own 3-D grid.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// ---------------- the private functional key switch ----------------
//
// The key-switch tile of pfhe_tfhe_exact_device.hpp per key block u (grid.z): M = batch * levels input ciphertexts, K =
// (in_dimension + 1) * ell key rows, (k+1) N columns.  The workgroup walks the input words, body included.  Input row m =
// e * levels + l is stored to out[e][u][l].
constexpr size_t kMaxLevels = 64;

struct PfksShape {
    u32 in_dim, k, log_n, levels, log_basis, ell, drop_bits, ki;
};

template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_pfks_kernel(const W *__restrict__ lwe_in, const W *__restrict__ pfksk,
                                                             W *__restrict__ out, PfksShape s, u64 m0, u64 m_total) {
    __shared__ W dig[kKsMaxRows * kKsTileM];
    const u32 lane = threadIdx.x % kKsLanes, wave = threadIdx.x / kKsLanes;
    const u32 cols = (s.k + 1) << s.log_n, words = s.in_dim + 1;
    const u32 c0 = blockIdx.x * kKsTileN + lane;
    const u64 r0 = m0 + (u64)blockIdx.y * kKsTileM;
    const u32 u = blockIdx.z;
    W acc[kKsRows][kKsCols] = {};
    // the key columns of this thread in block u; a column past the end reads the last one instead (its sums are never
    // stored), so that no load of the inner loop sits behind a branch
    const W *key[kKsCols];
#pragma unroll
    for (int c = 0; c < kKsCols; ++c) key[c] = pfksk + (u64)u * words * s.ell * cols + min(c0 + c * kKsLanes, cols - 1);
    ks_tile_sums(dig, lwe_in, (u64)words, words, r0, m_total, key, cols, s.log_basis, s.ell, s.drop_bits, s.ki, acc);
#pragma unroll
    for (int r = 0; r < kKsRows; ++r) {
        const u64 m = r0 + wave * kKsRows + r;
        if (m >= m_total) continue;
        const u64 e = m / s.levels, l = m - e * s.levels;
        W *dst = out + ((e * (s.k + 1) + u) * s.levels + l) * cols;
#pragma unroll
        for (int c = 0; c < kKsCols; ++c) {
            const u32 col = c0 + c * kKsLanes;
            if (col < cols) dst[col] = (W)0 - acc[r][c];
        }
    }
}

// ---------------- the key's messages ----------------

// Per (j, t): one thread per body coefficient of the k rows (u < k, j, t), which get -s'_j g_t z_u[i], and one for
// coefficient 0 of row (k, j, t), which gets s'_j g_t; s'_j = key_in[j] for j < in_dim and -1 for the body word
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_pfksk_add_message_kernel(W *__restrict__ pfksk, const W *__restrict__ key_in,
                                                                          const W *__restrict__ glwe_key, u32 k, u32 log_n,
                                                                          u32 in_dim, u32 ell, u32 log_basis, u32 drop,
                                                                          u64 total) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u64 per = ((u64)k << log_n) + 1;
    const u64 pair = t / per, q = t - pair * per;
    const u64 j = pair / ell;
    const u32 lvl = (u32)(pair - j * ell);
    const W msg = (j < in_dim ? key_in[j] : (W)0 - (W)1) << (drop + lvl * log_basis);
    const u32 u = (u32)(q >> log_n), i = (u32)(q & ((1u << log_n) - 1));  // q = kN: u = k, i = 0
    W *body = pfksk + (((((u64)u * (in_dim + 1) + j) * ell + lvl) * (k + 1) + k) << log_n);
    if (u == k)
        body[0] += msg;
    else
        body[i] -= msg * glwe_key[((u64)u << log_n) + i];
}

// ---------------- launches (arguments already checked) ----------------

template <class W>
int launch_pfks(const W *lwe_in, const W *pfksk, W *out, PfksShape sh, u64 rows, hipStream_t s) {
    const u32 gx = (((sh.k + 1) << sh.log_n) + kKsTileN - 1) / kKsTileN;
    return launch_y_slices((rows + kKsTileM - 1) / kKsTileM, [&](u64 first_tile, u32 tiles) {
        return launch_grid(tfhe_pfks_kernel<W>, dim3(gx, tiles, sh.k + 1), 0, s, lwe_in, pfksk, out, sh, first_tile * kKsTileM,
                           rows);
    });
}

// ---------------- the stateless entry points ----------------

constexpr const char *kPfksDimensions = "private key switch: glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2";

inline size_t pfksk_words(size_t k, size_t n, size_t in_dimension, size_t ell) {
    return (k + 1) * (in_dimension + 1) * ell * (k + 1) * n;
}

template <class W>
int pfks_check(const pfhe_fft *f, size_t k, size_t len_in, size_t in_dimension, size_t levels, size_t len_pfksk,
               uint32_t log_basis, size_t decompose_length, size_t len_out, PfksShape &sh) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(tfhe_keyswitch_dimensions<W>(kPfksDimensions, f, k, in_dimension, log_basis, decompose_length, ell, drop));
    if (levels == 0 || levels > kMaxLevels) {
        set_last_error("private key switch: levels must be in 1..64");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const size_t group = levels * (in_dimension + 1), ggsw = (k + 1) * levels * (k + 1) * f->n;
    if (len_in % group != 0 || len_pfksk != pfksk_words(k, f->n, in_dimension, ell) || len_out != len_in / group * ggsw) {
        set_last_error("private key switch: lwe_in must be batch*levels*(in_dimension+1) words, pfksk "
                       "(k+1)*(in_dimension+1)*ell*(k+1)*N and out batch*(k+1)*levels*(k+1)*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    sh = PfksShape{(u32)in_dimension, (u32)k, f->log_n, (u32)levels, log_basis, ell, drop, ks_group_words(ell)};
    return PFHE_OK;
}

template <class W>
int private_keyswitch(Form form, const pfhe_fft *f, size_t k, const W *lwe_in, size_t len_in, size_t in_dimension, size_t levels,
                      const W *pfksk, size_t len_pfksk, uint32_t log_basis, size_t decompose_length, W *out, size_t len_out,
                      hipStream_t s) {
    PfksShape sh{};
    PFHE_TRY(pfks_check<W>(f, k, len_in, in_dimension, levels, len_pfksk, log_basis, decompose_length, len_out, sh));
    if (len_in == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(pfksk, len_pfksk * sizeof(W)),
                             stage_out(out, len_out * sizeof(W))};
    return stateless_call(f->device, form, bufs, "private key switch: the output must not overlap an input", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_pfks<W>((const W *)d[0], (const W *)d[1], (W *)d[2], sh, len_in / (in_dimension + 1),
                                                    st);
                          });
}

template <class W>
int pfksk_generate_dev(const pfhe_fft *f, size_t k, const W *key_in, size_t in_dimension, const W *glwe_key, size_t len_glwe_key,
                       uint32_t log_basis, size_t decompose_length, W *pfksk, size_t len, hipStream_t s) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(tfhe_keyswitch_dimensions<W>("private key-switch key: glwe_dimension must be in 1..64 and in_dimension in 1..2^31-2", f, k,
                                in_dimension, log_basis, decompose_length, ell, drop));
    if (len_glwe_key != k * f->n || len != pfksk_words(k, f->n, in_dimension, ell)) {
        set_last_error("private key-switch key: glwe_key must be k*N words and pfksk (k+1)*(in_dimension+1)*ell*(k+1)*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    const StageBuf bufs[] = {stage_in(key_in, in_dimension * sizeof(W)), stage_in(glwe_key, len_glwe_key * sizeof(W)),
                             stage_inout(pfksk, len * sizeof(W))};
    const u64 pairs = ((u64)in_dimension + 1) * ell;
    return stateless_call(
        f->device, Form::kDevice, bufs, "private key-switch key: the keys must not overlap pfksk", s,
        [&](void *const *d, hipStream_t st) {
            PFHE_TRY(glwe_body_add(f, k, (W *)d[2], len, (const W *)d[1], len_glwe_key, st));
            return launch_flat(tfhe_pfksk_add_message_kernel<W>, pairs * (k * f->n + 1), st, (W *)d[2], (const W *)d[0],
                               (const W *)d[1], (u32)k, f->log_n, (u32)in_dimension, ell, log_basis, drop);
        },
        [&] { return pairs * (k + 1) > 0x7fffffffull ? PFHE_ERR_BAD_LENGTH : PFHE_OK; });
}

}  // namespace
}  // namespace pfhe

// ---------------- the circuit bootstrap handle ----------------

// Owns a blind rotation (classic or multi-bit, behind TfheRotation) and, for `chunk` inputs, chunk * ell_cb accumulators (chunk
// with a shared rotation), their switched exponents, neg_b and the chunk * ell_cb extracted LWE ciphertexts: all allocated at
// creation.
template <class W>
struct TfheCbsCore : TfheBootstrapBase<W> {
    u32 cb_log_basis = 0, cb_ell = 0, cb_drop = 0;
    bool shared = false;  // one rotation per input serves all ell_cb levels (many-LUT): chunk accumulators, not chunk * ell_cb
    u32 log_stride = 0;   // shared: ceil(log2 ell_cb), the stride bits of the modulus switch
    PfksShape pf{};
};
struct pfhe_tfhe_cbs_handle : TfheCbsCore<u64> {};
struct pfhe_tfhe32_cbs_handle : TfheCbsCore<u32> {};

namespace {

constexpr const char *kCbsBusy = "TFHE circuit bootstrap handle in use by another thread (one handle per thread)";
constexpr const char *kCbsLengths =
    "TFHE circuit bootstrap: lwe_in must be batch*(n+1) words, bsk n*(k+1)*ell*(k+1)*N complex values, pfksk "
    "(k+1)*(k*N+1)*pfks_ell*(k+1)*N words and ggsw_out batch*(k+1)*cbs_ell*(k+1)*N";
constexpr size_t kCbsDefaultAccBytes = 256ull << 20;

// Everything that decides before the device first: the rotation's own checks in its order, then what is the circuit
// bootstrap's own (the dimensions, the two bases' assert!s, drop_bits of the output basis); then the rotation's create.
// cbs_create_with adds: grouping_factor above 1 makes the rotation the multi-bit one (its range with the rotation's checks,
// then the divisibility, as bootstrap_create refuses them); shared_rotation refuses ell_cb above N last of all
template <class W, class H>
int cbs_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t lwe_dimension,
               uint32_t cbs_log_basis, size_t cbs_decompose_length, uint32_t pfks_log_basis, size_t pfks_decompose_length,
               size_t chunk, H **out, size_t grouping_factor = 1, bool shared = false) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape rot_shape{};
    const std::optional<size_t> grouping = grouping_factor > 1 ? std::optional<size_t>(grouping_factor) : std::nullopt;
    PFHE_TRY(tfhe_bootstrap_check<W>(fft, glwe_dimension, log_basis, decompose_length, grouping, lwe_dimension,
                                     "TFHE circuit bootstrap: lwe_dimension must be a multiple of grouping_factor", rot_shape));
    // a zero glwe_dimension is refused as a zero lwe_dimension is: one message for both
    PFHE_TRY(require_lwe_dimension(glwe_dimension ? lwe_dimension : 0,
                                   "TFHE circuit bootstrap: glwe_dimension must be at least 1 and lwe_dimension in 1..2^31-2"));
    auto h = std::make_unique<H>();
    PFHE_TRY(basis_shape(8 * sizeof(W), cbs_log_basis, cbs_decompose_length, h->cb_ell, h->cb_drop));
    u32 pf_ell = 0, pf_drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), pfks_log_basis, pfks_decompose_length, pf_ell, pf_drop));
    if (h->cb_drop == 0) {
        set_last_error("TFHE circuit bootstrap: the output basis must drop at least one bit (g_l / 2 must be a word)");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (shared && h->cb_ell > fft->n) {
        set_last_error("TFHE circuit bootstrap: a shared rotation serves at most N levels of the output basis");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    h->shared = shared;
    while (shared && (1u << h->log_stride) < h->cb_ell) ++h->log_stride;
    // chunk inputs are chunk * ell_cb accumulators of the rotation, or chunk with a shared one; 0 stays the rotation's default
    const size_t per_input = shared ? 1 : h->cb_ell;
    if (chunk > 0x7fffffffull / h->cb_ell) return PFHE_ERR_BAD_LENGTH;
    TfheRotation<W> *rotation = nullptr;
    PFHE_TRY(tfhe_rotation_create<W>(fft, glwe_dimension, log_basis, decompose_length, grouping, chunk * per_input, &rotation));
    h->rotation.reset(rotation);
    const TfheRotation<W> &rot = *h->rotation;
    h->fft = fft;
    h->k = (u32)glwe_dimension;
    h->n = (u32)lwe_dimension;
    h->cb_log_basis = cbs_log_basis;
    const size_t glwe = rot.glwe, ext = glwe_dimension * fft->n + 1, levels = h->cb_ell;
    h->pf = PfksShape{(u32)(ext - 1), h->k, fft->log_n, h->cb_ell, pfks_log_basis, pf_ell, pf_drop, ks_group_words(pf_ell)};
    h->bsk_len = tfhe_bootstrap_keys(grouping, lwe_dimension) * rot.key_len;
    // chunk 0: what the rotation's default holds, capped at about 256 MiB of accumulators
    h->chunk = chunk ? chunk
                     : std::max<size_t>(1, std::min(rot.chunk, kCbsDefaultAccBytes / (glwe * sizeof(W))) / per_input);
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    const size_t accs = h->chunk * per_input, rows = h->chunk * levels;
    h->bufs.bind(fft->device);
    PFHE_TRY(h->bufs.add(h->acc, accs * glwe));
    PFHE_TRY(h->bufs.add(h->extracted, rows * ext));
    PFHE_TRY(h->bufs.add(h->exps, accs * lwe_dimension));
    PFHE_TRY(h->bufs.add(h->neg_b, h->chunk));
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

template <class W, class H>
int cbs_check(const H *h, size_t len_in, size_t len_bsk, size_t len_pfksk, size_t len_out, u64 &batch) {
    const size_t n = h->fft->n, k = h->k, in_words = (size_t)h->n + 1;
    batch = len_in / in_words;
    if (len_in % in_words != 0 || len_bsk != h->bsk_len || len_pfksk != pfksk_words(k, n, k * n, h->pf.ell) ||
        len_out != batch * (k + 1) * h->cb_ell * (k + 1) * n) {
        set_last_error(kCbsLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    return PFHE_OK;
}

// Both forms refuse alike up to the null test; the device form then looks at its pointers.
template <class W, class H>
int cbs(Form form, H *h, const W *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const W *pfksk, size_t len_pfksk,
        W *ggsw_out, size_t len_out, hipStream_t s) {
    if (!h || !h->rotation) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kCbsBusy);
    u64 batch = 0;
    PFHE_TRY((cbs_check<W>(h, len_in, len_bsk, len_pfksk, len_out, batch)));
    if (batch == 0) return PFHE_OK;
    if (!lwe_in || !bsk || !pfksk || !ggsw_out) return PFHE_ERR_BAD_ARGUMENT;
    if (form == Form::kDevice) {
        PFHE_REQUIRE_ALIGNED(bsk);
        const size_t out_bytes = len_out * sizeof(W);
        if (overlaps(lwe_in, len_in * sizeof(W), ggsw_out, out_bytes) ||
            overlaps(bsk, len_bsk * 2 * sizeof(double), ggsw_out, out_bytes) ||
            overlaps(pfksk, len_pfksk * sizeof(W), ggsw_out, out_bytes)) {
            set_last_error("TFHE circuit bootstrap: the output must not overlap an input");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const pfhe_fft &f = *h->fft;
    const size_t glwe = h->rotation->glwe, in_words = (size_t)h->n + 1;
    const u32 levels = h->cb_ell, half_shift = h->cb_drop - 1;
    const size_t ggsw = (size_t)(h->k + 1) * levels * glwe;
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(bsk, len_bsk * sizeof(double2)),
                             stage_in(pfksk, len_pfksk * sizeof(W)), stage_out(ggsw_out, len_out * sizeof(W))};
    return handle_call(h->guard, f.device, form, bufs, s, [&](void *const *d, hipStream_t st) -> int {
        // chunk after chunk; every stage of a chunk is queued before the next chunk starts.  An input has per_input
        // accumulators, each of which gives per_acc of its `levels` rows: one accumulator with a shared rotation (the switch to
        // multiples of 2^log_stride, the patterned test vector, level l read off coefficient l), one per level without
        // (log_stride 0, every coefficient of TV_l alike, index 0)
        const W *in = (const W *)d[0];
        const u32 per_input = h->shared ? 1 : levels, per_acc = h->shared ? levels : 1;
        for (u64 done = 0; done < batch; done += h->chunk) {
            const u64 cur = std::min<u64>(h->chunk, batch - done), accs = cur * per_input;
            PFHE_TRY(launch_modswitch<W>(in + done * in_words, h->n, f.log_n, h->log_stride, (W)1 << (8 * sizeof(W) - 2), per_input,
                                         h->exps, h->neg_b, cur, st));
            PFHE_TRY(launch_const_acc_init<W>(h->acc, h->neg_b, h->k, f.log_n, per_input, h->log_stride, levels, h->cb_log_basis,
                                              half_shift, accs, st));
            PFHE_TRY(h->rotation->rotate_dev(h->acc, accs * glwe, (const double *)d[1], len_bsk, h->exps, accs * h->n, st));
            PFHE_TRY(launch_extract<W>(h->acc, nullptr, h->extracted, h->k, f.log_n,
                                       ExtractRule{per_acc, 0, levels, 1, h->cb_log_basis, half_shift}, cur * levels, st));
            PFHE_TRY(launch_pfks<W>(h->extracted, (const W *)d[2], (W *)d[3] + done * ggsw, h->pf, cur * levels, st));
        }
        return PFHE_OK;
    });
}

}  // namespace

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_CBS_FAMILY(P, CW, W)                                                                                       \
    PFHE_ENTRY(P##_private_keyswitch_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *lwe_in_dev,            \
                size_t len_in, size_t in_dimension, size_t levels, const CW *pfksk_dev, size_t len_pfksk,               \
                uint32_t log_basis, size_t decompose_length, CW *out_dev, size_t len_out, void *stream),                \
               private_keyswitch<W>(Form::kDevice, fft, glwe_dimension, (const W *)lwe_in_dev, len_in, in_dimension,    \
                                    levels, (const W *)pfksk_dev, len_pfksk, log_basis, decompose_length, (W *)out_dev, \
                                    len_out, (hipStream_t)stream))                                                      \
    PFHE_ENTRY(P##_private_keyswitch, (const pfhe_fft *fft, size_t glwe_dimension, const CW *lwe_in, size_t len_in,     \
                size_t in_dimension, size_t levels, const CW *pfksk, size_t len_pfksk, uint32_t log_basis,              \
                size_t decompose_length, CW *out, size_t len_out),                                                      \
               private_keyswitch<W>(Form::kHost, fft, glwe_dimension, (const W *)lwe_in, len_in, in_dimension, levels,  \
                                    (const W *)pfksk, len_pfksk, log_basis, decompose_length, (W *)out, len_out,        \
                                    nullptr))                                                                           \
    PFHE_ENTRY(P##_pfksk_generate_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *key_in_dev,               \
                size_t in_dimension, const CW *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,                   \
                size_t decompose_length, CW *pfksk_dev, size_t len_pfksk, void *stream),                                \
               pfksk_generate_dev<W>(fft, glwe_dimension, (const W *)key_in_dev, in_dimension,                          \
                                     (const W *)glwe_key_dev, len_glwe_key, log_basis, decompose_length,                \
                                     (W *)pfksk_dev, len_pfksk, (hipStream_t)stream))                                   \
    PFHE_ENTRY(P##_cbs_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                         \
                size_t decompose_length, size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length,     \
                uint32_t pfks_log_basis, size_t pfks_decompose_length, size_t chunk, P##_cbs_handle **out),             \
               cbs_create<W>(fft, glwe_dimension, log_basis, decompose_length, lwe_dimension, cbs_log_basis,            \
                             cbs_decompose_length, pfks_log_basis, pfks_decompose_length, chunk, out))                  \
    PFHE_ENTRY(P##_cbs_create_with, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                    \
                size_t decompose_length, size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length,     \
                uint32_t pfks_log_basis, size_t pfks_decompose_length, size_t grouping_factor, int shared_rotation,     \
                size_t chunk, P##_cbs_handle **out),                                                                    \
               cbs_create<W>(fft, glwe_dimension, log_basis, decompose_length, lwe_dimension, cbs_log_basis,            \
                             cbs_decompose_length, pfks_log_basis, pfks_decompose_length, chunk, out, grouping_factor,  \
                             shared_rotation != 0))                                                                     \
    PFHE_HANDLE_TRIO(P##_cbs, P##_cbs_handle, tfhe_bootstrap_scratch(h))                                                \
    PFHE_ENTRY(P##_cbs_dev, (P##_cbs_handle *h, const CW *lwe_in_dev, size_t len_in, const double *bsk_dev,             \
                size_t len_bsk, const CW *pfksk_dev, size_t len_pfksk, CW *ggsw_out_dev, size_t len_out, void *stream), \
               cbs<W>(Form::kDevice, h, (const W *)lwe_in_dev, len_in, bsk_dev, len_bsk, (const W *)pfksk_dev,          \
                      len_pfksk, (W *)ggsw_out_dev, len_out, (hipStream_t)stream))                                      \
    PFHE_ENTRY(P##_cbs, (P##_cbs_handle *h, const CW *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,         \
                const CW *pfksk, size_t len_pfksk, CW *ggsw_out, size_t len_out),                                       \
               cbs<W>(Form::kHost, h, (const W *)lwe_in, len_in, bsk, len_bsk, (const W *)pfksk, len_pfksk,             \
                      (W *)ggsw_out, len_out, nullptr))

extern "C" {

PFHE_CBS_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_CBS_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_CBS_FAMILY

}  // extern "C"
