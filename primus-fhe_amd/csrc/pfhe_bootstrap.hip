// pfhe_bootstrap.hip — the steps of a TFHE programmable bootstrap around the blind rotation, and the handle that runs
// them in order (include/pfhe.h: pfhe_tfhe{,32}_modswitch_dev, _sample_extract*, _keyswitch*, _bootstrap_*).
//
//   modulus switch     LWE words -> exponents modulo 2N: switch_rounded at stride 2^log_luts (0 without many-LUT),
//                      round(w 2N / 2^BITS) with ties up, reduced modulo 2N.
//   accumulator init   ACC_e = X^{neg_b[e]} TV, the rotation of pfhe_tfhe*_mul_monomial_each_to_dev with the test vector
//                      read in place (one shared by the batch, or one per ciphertext).
//   blind rotation     the classic or the multi-bit handle (pfhe_fft.hip) behind TfheRotation, called as it is.
//   sample extraction  Rlwe::extract_lwe_with_index (primus_lattice/src/rlwe/coeff.rs:194-227) per mask polynomial, at
//                      every index below 2^log_luts (pfhe_tfhe{,32}_bootstrap_create_many_lut; index 0 without).
//   key switch         out = (0, b) - sum_i sum_j d_{i,j} KSK[i][j], a sequence of Lwe::add_mul_scalar_assign
//                      (lwe/single_message.rs:262-268) with the digits of ApproxSignedBasis (init_carry / digit_word of
//                      pfhe_fft_device.hpp, over the product's own digit_step).
// The switch, the accumulator and the extraction are the stage kernels of pfhe_tfhe_stages.hip, queued through the launches
// of pfhe_tfhe_handles.hpp; the key switch's kernel is this file's.
// Every step is exact integer arithmetic modulo 2^BITS except the rotation; no atomics, no scratch memory.  Launches and
// the two forms of every call (stateless_call, handle_call) go through pfhe_tfhe_host.hpp; the key switch keeps its own
// 2-D grid.  The rules of the exact steps and the key switch's tile are pfhe_tfhe_exact_device.hpp's.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// ---------------- key switch ----------------
//
// The key-switch tile of pfhe_tfhe_exact_device.hpp with M = batch, K = in_dimension * ell, out_dimension + 1 columns: the
// workgroup walks the mask words, and the body goes into the last column behind the sums.

template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_keyswitch_kernel(const W *__restrict__ lwe_in, const W *__restrict__ ksk,
                                                                  W *__restrict__ lwe_out, KsShape s, u64 batch) {
    __shared__ W dig[kKsMaxRows * kKsTileM];
    const u32 lane = threadIdx.x % kKsLanes, wave = threadIdx.x / kKsLanes;
    const u32 cols = s.out_dim + 1;
    const u32 c0 = blockIdx.x * kKsTileN + lane;
    const u64 e0 = (u64)blockIdx.y * kKsTileM;
    const u64 in_stride = (u64)s.in_dim + 1;
    W acc[kKsRows][kKsCols] = {};
    // the key columns of this thread; a column past the end reads the last one instead (its sums are never stored), so that
    // no load of the inner loop sits behind a branch
    const W *key[kKsCols];
#pragma unroll
    for (int c = 0; c < kKsCols; ++c) key[c] = ksk + min(c0 + c * kKsLanes, cols - 1);
    ks_tile_sums(dig, lwe_in, in_stride, s.in_dim, e0, batch, key, cols, s.log_basis, s.ell, s.drop_bits, s.ki, acc);
#pragma unroll
    for (int r = 0; r < kKsRows; ++r) {
        const u64 e = e0 + wave * kKsRows + r;
        if (e >= batch) continue;
#pragma unroll
        for (int c = 0; c < kKsCols; ++c) {
            const u32 col = c0 + c * kKsLanes;
            if (col >= cols) continue;
            const W b = col == s.out_dim ? lwe_in[e * in_stride + s.in_dim] : (W)0;
            lwe_out[e * cols + col] = b - acc[r][c];
        }
    }
}

// ---------------- launches (arguments already checked) ----------------

template <class W>
int launch_keyswitch(const W *lwe_in, const W *ksk, W *lwe_out, KsShape sh, u64 batch, hipStream_t s) {
    const u64 gx = ((u64)sh.out_dim + 1 + kKsTileN - 1) / kKsTileN;
    return launch_y_slices((batch + kKsTileM - 1) / kKsTileM, [&](u64 first_tile, u32 tiles) {
        const u64 done = first_tile * kKsTileM, cur = std::min<u64>(batch - done, (u64)tiles * kKsTileM);
        return launch_grid(tfhe_keyswitch_kernel<W>, dim3((u32)gx, tiles), 0, s, lwe_in + done * ((u64)sh.in_dim + 1), ksk,
                           lwe_out + done * ((u64)sh.out_dim + 1), sh, cur);
    });
}

// ---------------- the stateless entry points ----------------

template <class W>
int modswitch_dev(int device, const W *lwe, size_t len_lwe, size_t lwe_dimension, uint32_t log_n, uint32_t *exps,
                  size_t len_exps, uint32_t *neg_b, size_t len_neg_b, hipStream_t s) {
    if (log_n == 0 || log_n > kMaxLogN) {
        set_last_error("modulus switch: log_n must be in 1..14");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (lwe_dimension == 0 || lwe_dimension >= 0xffffffffull) {
        set_last_error("modulus switch: lwe_dimension must be in 1..2^32-2");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (len_lwe % (lwe_dimension + 1) != 0 || len_neg_b != len_lwe / (lwe_dimension + 1) ||
        len_exps != len_neg_b * lwe_dimension) {
        set_last_error("modulus switch: lwe must be batch*(n+1) words, exps batch*n and neg_b batch exponents");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_lwe == 0) return PFHE_OK;
    // no overlap message: this step refuses none
    const StageBuf bufs[] = {stage_in(lwe, len_lwe * sizeof(W)), stage_out(exps, len_exps * sizeof(u32)),
                             stage_out(neg_b, len_neg_b * sizeof(u32))};
    return stateless_call(
        device, Form::kDevice, bufs, nullptr, s,
        [&](void *const *d, hipStream_t st) {
            return launch_modswitch<W>((const W *)d[0], (u32)lwe_dimension, log_n, 0, (W)0, 1, (u32 *)d[1], (u32 *)d[2],
                                       len_neg_b, st);
        },
        [&] { return capi_check_device(device); });
}

template <class W>
int sample_extract(Form form, const pfhe_fft *f, size_t k, const W *glwe, size_t len_glwe, size_t index, W *lwe, size_t len_lwe,
                   hipStream_t s) {
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(require_glwe_dimension(k, "sample extraction: glwe_dimension must be in 1..64"));
    if (index >= f->n) {
        set_last_error("sample extraction: index must be below N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (len_glwe % ((k + 1) * f->n) != 0 || len_lwe != len_glwe / ((k + 1) * f->n) * (k * f->n + 1)) {
        set_last_error("sample extraction: glwe must be batch*(k+1)*N words and lwe batch*(k*N+1)");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (len_glwe == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(glwe, len_glwe * sizeof(W)), stage_out(lwe, len_lwe * sizeof(W))};
    return stateless_call(f->device, form, bufs, "sample extraction: the output must not overlap the input", s,
                          [&](void *const *d, hipStream_t st) {
                              return launch_extract<W>((const W *)d[0], nullptr, (W *)d[1], (u32)k, f->log_n,
                                                       ExtractRule{1, (u32)index, 1, 0, 0, 0}, len_glwe / ((k + 1) * f->n), st);
                          });
}

// ApproxSignedBasis::new's assert!s first, then the dimensions
template <class W>
int keyswitch_shape(size_t in_dimension, size_t out_dimension, uint32_t log_basis, size_t decompose_length, KsShape &sh) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), log_basis, decompose_length, ell, drop));
    PFHE_TRY(require_lwe_dimension(in_dimension, "key switch: both dimensions must be in 1..2^31-2"));
    PFHE_TRY(require_lwe_dimension(out_dimension, "key switch: both dimensions must be in 1..2^31-2"));
    sh = KsShape{(u32)in_dimension, (u32)out_dimension, log_basis, ell, drop,
                 ks_group_words(ell)};
    return PFHE_OK;
}

// ... then the lengths
template <class W>
int keyswitch_check(size_t len_in, size_t in_dimension, size_t len_ksk, size_t out_dimension, uint32_t log_basis,
                    size_t decompose_length, size_t len_out, KsShape &sh) {
    PFHE_TRY(keyswitch_shape<W>(in_dimension, out_dimension, log_basis, decompose_length, sh));
    if (len_in % (in_dimension + 1) != 0 || len_ksk != in_dimension * sh.ell * (out_dimension + 1) ||
        len_out != len_in / (in_dimension + 1) * (out_dimension + 1)) {
        set_last_error("key switch: lwe_in must be batch*(in_dimension+1) words, ksk in_dimension*ell*(out_dimension+1) and "
                       "lwe_out batch*(out_dimension+1)");
        return PFHE_ERR_BAD_LENGTH;
    }
    return PFHE_OK;
}

template <class W>
int keyswitch(Form form, int device, const W *lwe_in, size_t len_in, size_t in_dimension, const W *ksk, size_t len_ksk,
              size_t out_dimension, uint32_t log_basis, size_t decompose_length, W *lwe_out, size_t len_out, hipStream_t s) {
    KsShape sh{};
    PFHE_TRY(keyswitch_check<W>(len_in, in_dimension, len_ksk, out_dimension, log_basis, decompose_length, len_out, sh));
    if (len_in == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(ksk, len_ksk * sizeof(W)),
                             stage_out(lwe_out, len_out * sizeof(W))};
    return stateless_call(
        device, form, bufs, "key switch: the output must not overlap an input", s,
        [&](void *const *d, hipStream_t st) {
            return launch_keyswitch<W>((const W *)d[0], (const W *)d[1], (W *)d[2], sh, len_in / (in_dimension + 1), st);
        },
        [&] { return capi_check_device(device); });
}

}  // namespace
}  // namespace pfhe

// ---------------- the bootstrap handle ----------------

// Owns a blind rotation (classic or multi-bit, behind TfheRotation) and, for `chunk` ciphertexts, the accumulator, the
// switched exponents, neg_b and (when a key switch follows) the extracted LWE ciphertexts: all allocated at creation.
template <class W>
struct TfheBootstrapCore : TfheBootstrapBase<W> {
    u32 log_luts = 0;  // many-LUT: 2^log_luts outputs per input, extracted at indices 0..2^log_luts-1 of one accumulator
    bool with_keyswitch = false;
    KsShape ks{};
};
struct pfhe_tfhe_bootstrap_handle : TfheBootstrapCore<u64> {};
struct pfhe_tfhe32_bootstrap_handle : TfheBootstrapCore<u32> {};

namespace {

constexpr const char *kBootstrapBusy = "TFHE bootstrap handle in use by another thread (one handle per thread)";
constexpr const char *kBootstrapLengths =
    "TFHE bootstrap: lwe_in must be batch*(n+1) words, bsk n*(k+1)*ell*(k+1)*N complex values, tv (k+1)*N or batch*(k+1)*N "
    "words, ksk k*N*ks_ell*(n+1) words (0 without a key switch) and lwe_out batch*(n+1) (batch*(k*N+1) without)";
constexpr size_t kDefaultAccBytes = 256ull << 20;

// The rotation's create first (its statuses, in its order), then what is the bootstrap's own.  With a grouping factor the
// rotation is the multi-bit one, whose key has (lwe_dimension / g) 2^g keys; everything that decides before the device
// is then decided first: the rotation's own checks in its order, then the divisibility.  many_lut (create_many_lut): the
// classic rotation's checks run here too, and log_luts above log N is refused right behind the rotation's, before the device
template <class W, class H>
int bootstrap_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                     size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, int with_keyswitch,
                     std::optional<size_t> grouping_factor, size_t chunk, H **out, bool many_lut = false,
                     uint32_t log_luts = 0) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    auto h = std::make_unique<H>();
    if (many_lut || grouping_factor) {  // the plain create leaves every check to the rotation's create
        Shape sh{};
        PFHE_TRY(tfhe_bootstrap_check<W>(fft, glwe_dimension, log_basis, decompose_length, grouping_factor, lwe_dimension,
                                         "TFHE multi-bit bootstrap: lwe_dimension must be a multiple of grouping_factor", sh));
    }
    if (many_lut && log_luts > fft->log_n) {
        set_last_error("TFHE many-LUT bootstrap: log_luts must be at most log N");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    h->log_luts = log_luts;
    TfheRotation<W> *rotation = nullptr;
    PFHE_TRY(tfhe_rotation_create<W>(fft, glwe_dimension, log_basis, decompose_length, grouping_factor, chunk, &rotation));
    h->rotation.reset(rotation);
    const TfheRotation<W> &rot = *h->rotation;
    h->fft = fft;
    h->k = (u32)glwe_dimension;
    h->with_keyswitch = with_keyswitch != 0;
    const size_t glwe = rot.glwe, ext = glwe_dimension * fft->n + 1;
    // a zero glwe_dimension is refused as a zero lwe_dimension is: one message for both
    PFHE_TRY(require_lwe_dimension(glwe_dimension ? lwe_dimension : 0,
                                   "TFHE bootstrap: glwe_dimension must be at least 1 and lwe_dimension in 1..2^31-2"));
    h->n = (u32)lwe_dimension;
    h->bsk_len = tfhe_bootstrap_keys(grouping_factor, lwe_dimension) * rot.key_len;
    if (h->with_keyswitch) PFHE_TRY(keyswitch_shape<W>(ext - 1, lwe_dimension, ks_log_basis, ks_decompose_length, h->ks));
    // chunk 0: the rotation's default, capped at about 256 MiB of accumulator
    h->chunk = chunk ? rot.chunk : std::min(rot.chunk, std::max<size_t>(1, kDefaultAccBytes / (glwe * sizeof(W))));
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->bufs.bind(fft->device);
    PFHE_TRY(h->bufs.add(h->acc, h->chunk * glwe));
    PFHE_TRY(h->bufs.add(h->extracted, h->with_keyswitch ? (h->chunk << log_luts) * ext : 0));
    PFHE_TRY(h->bufs.add(h->exps, h->chunk * lwe_dimension));
    PFHE_TRY(h->bufs.add(h->neg_b, h->chunk));
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

template <class W, class H>
int bootstrap_check(const H *h, size_t len_in, size_t len_bsk, size_t len_tv, size_t len_ksk, size_t len_out, u64 &batch) {
    const size_t glwe = h->rotation->glwe, ext = (size_t)h->k * h->fft->n + 1;
    const size_t out_words = h->with_keyswitch ? (size_t)h->n + 1 : ext;
    const size_t ksk_words = h->with_keyswitch ? (ext - 1) * h->ks.ell * ((size_t)h->n + 1) : 0;
    batch = len_in / ((size_t)h->n + 1);
    if (len_in % ((size_t)h->n + 1) != 0 || len_bsk != h->bsk_len || (len_tv != glwe && len_tv != batch * glwe) ||
        len_ksk != ksk_words || len_out != (batch << h->log_luts) * out_words) {
        set_last_error(kBootstrapLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    return PFHE_OK;
}

// Both forms refuse alike up to the null test; the device form then looks at its pointers.
template <class W, class H>
int bootstrap(Form form, H *h, const W *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const W *tv, size_t len_tv,
              const W *ksk, size_t len_ksk, W *lwe_out, size_t len_out, hipStream_t s) {
    if (!h || !h->rotation) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kBootstrapBusy);
    if (!h->with_keyswitch && (ksk || len_ksk)) {
        set_last_error("TFHE bootstrap: a handle without a key switch takes no key-switch key");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    u64 batch = 0;
    PFHE_TRY((bootstrap_check<W>(h, len_in, len_bsk, len_tv, len_ksk, len_out, batch)));
    if (batch == 0) return PFHE_OK;
    if (!lwe_in || !bsk || !tv || !lwe_out || (h->with_keyswitch && !ksk)) return PFHE_ERR_BAD_ARGUMENT;
    if (form == Form::kDevice) {
        PFHE_REQUIRE_ALIGNED(bsk);
        const size_t out_bytes = len_out * sizeof(W);
        if (overlaps(lwe_in, len_in * sizeof(W), lwe_out, out_bytes) || overlaps(tv, len_tv * sizeof(W), lwe_out, out_bytes) ||
            overlaps(bsk, len_bsk * 2 * sizeof(double), lwe_out, out_bytes) ||
            (ksk && overlaps(ksk, len_ksk * sizeof(W), lwe_out, out_bytes))) {
            set_last_error("TFHE bootstrap: the output must not overlap an input");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const pfhe_fft &f = *h->fft;
    const size_t glwe = h->rotation->glwe, ext = (size_t)h->k * f.n + 1, in_words = (size_t)h->n + 1;
    const size_t out_words = (h->with_keyswitch ? in_words : ext) << h->log_luts;  // of one input's 2^log_luts outputs
    const u64 tv_stride = len_tv == glwe ? 0 : glwe;
    // without a key switch ksk is empty: the host form does not stage it and the launches get a null pointer
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(bsk, len_bsk * sizeof(double2)),
                             stage_in(tv, len_tv * sizeof(W)), stage_in(ksk, len_ksk * sizeof(W)),
                             stage_out(lwe_out, len_out * sizeof(W))};
    return handle_call(h->guard, f.device, form, bufs, s, [&](void *const *d, hipStream_t st) -> int {
        const W *in = (const W *)d[0], *vec = (const W *)d[2], *key = (const W *)d[3];
        W *out = (W *)d[4];
        const u32 luts = 1u << h->log_luts;  // outputs per input: indices 0..luts-1 of its one accumulator
        // chunk after chunk; every stage of a chunk is queued before the next chunk starts
        for (u64 done = 0; done < batch; done += h->chunk) {
            const u64 cur = std::min<u64>(h->chunk, batch - done);
            PFHE_TRY(launch_modswitch<W>(in + done * in_words, h->n, f.log_n, h->log_luts, (W)0, 1, h->exps, h->neg_b, cur, st));
            PFHE_TRY(launch_acc_init<W>(vec + done * tv_stride, tv_stride, h->acc, h->neg_b, h->k + 1, f.log_n, cur, st));
            PFHE_TRY(h->rotation->rotate_dev(h->acc, cur * glwe, (const double *)d[1], len_bsk, h->exps, cur * h->n, st));
            W *lwe = h->with_keyswitch ? h->extracted : out + done * out_words;
            PFHE_TRY(launch_extract<W>(h->acc, nullptr, lwe, h->k, f.log_n, ExtractRule{luts, 0, luts, 0, 0, 0}, cur * luts, st));
            if (h->with_keyswitch)
                PFHE_TRY(launch_keyswitch<W>(lwe, key, out + done * out_words, h->ks, cur << h->log_luts, st));
        }
        return PFHE_OK;
    });
}

}  // namespace

// The entry points of one word width.  P: pfhe_tfhe / pfhe_tfhe32; CW / W: the word as pfhe.h and as the library spell it.
#define PFHE_BOOTSTRAP_FAMILY(P, CW, W)                                                                                 \
    PFHE_ENTRY(P##_modswitch_dev, (int device, const CW *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n, \
                uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev, size_t len_neg_b, void *stream),              \
               modswitch_dev<W>(device, (const W *)lwe_dev, len_lwe, lwe_dimension, log_n, exps_dev, len_exps,          \
                                neg_b_dev, len_neg_b, (hipStream_t)stream))                                             \
    PFHE_ENTRY(P##_sample_extract_dev, (const pfhe_fft *fft, size_t glwe_dimension, const CW *glwe_dev,                 \
                size_t len_glwe, size_t index, CW *lwe_dev, size_t len_lwe, void *stream),                              \
               sample_extract<W>(Form::kDevice, fft, glwe_dimension, (const W *)glwe_dev, len_glwe, index,              \
                                 (W *)lwe_dev, len_lwe, (hipStream_t)stream))                                           \
    PFHE_ENTRY(P##_sample_extract, (const pfhe_fft *fft, size_t glwe_dimension, const CW *glwe, size_t len_glwe,        \
                size_t index, CW *lwe, size_t len_lwe),                                                                 \
               sample_extract<W>(Form::kHost, fft, glwe_dimension, (const W *)glwe, len_glwe, index, (W *)lwe, len_lwe, \
                                 nullptr))                                                                              \
    PFHE_ENTRY(P##_keyswitch_dev, (int device, const CW *lwe_in_dev, size_t len_in, size_t in_dimension,                \
                const CW *ksk_dev, size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length,   \
                CW *lwe_out_dev, size_t len_out, void *stream),                                                         \
               keyswitch<W>(Form::kDevice, device, (const W *)lwe_in_dev, len_in, in_dimension, (const W *)ksk_dev,     \
                            len_ksk, out_dimension, log_basis, decompose_length, (W *)lwe_out_dev, len_out,             \
                            (hipStream_t)stream))                                                                       \
    PFHE_ENTRY(P##_keyswitch, (int device, const CW *lwe_in, size_t len_in, size_t in_dimension, const CW *ksk,         \
                size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length, CW *lwe_out,         \
                size_t len_out),                                                                                        \
               keyswitch<W>(Form::kHost, device, (const W *)lwe_in, len_in, in_dimension, (const W *)ksk, len_ksk,      \
                            out_dimension, log_basis, decompose_length, (W *)lwe_out, len_out, nullptr))                \
    PFHE_ENTRY(P##_bootstrap_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                   \
                size_t decompose_length, size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length,       \
                int with_keyswitch, size_t chunk, P##_bootstrap_handle **out),                                          \
               bootstrap_create<W>(fft, glwe_dimension, log_basis, decompose_length, lwe_dimension, ks_log_basis,       \
                                   ks_decompose_length, with_keyswitch, std::nullopt, chunk, out))                      \
    int P##_bootstrap_create_multibit(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                   \
                                      size_t decompose_length, size_t lwe_dimension, uint32_t ks_log_basis,             \
                                      size_t ks_decompose_length, int with_keyswitch, size_t grouping_factor,           \
                                      size_t chunk, P##_bootstrap_handle **out) {                                       \
        PFHE_GUARD_BEGIN                                                                                                \
        if (out) *out = nullptr;                                                                                        \
        return bootstrap_create<W>(fft, glwe_dimension, log_basis, decompose_length, lwe_dimension, ks_log_basis,       \
                                   ks_decompose_length, with_keyswitch, grouping_factor, chunk, out);                   \
        PFHE_GUARD_END                                                                                                  \
    }                                                                                                                   \
    int P##_bootstrap_create_many_lut(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis,                   \
                                      size_t decompose_length, size_t lwe_dimension, uint32_t ks_log_basis,             \
                                      size_t ks_decompose_length, int with_keyswitch, size_t grouping_factor,           \
                                      uint32_t log_luts, size_t chunk, P##_bootstrap_handle **out) {                    \
        PFHE_GUARD_BEGIN                                                                                                \
        if (out) *out = nullptr;                                                                                        \
        return bootstrap_create<W>(fft, glwe_dimension, log_basis, decompose_length, lwe_dimension, ks_log_basis,       \
                                   ks_decompose_length, with_keyswitch,                                                 \
                                   grouping_factor > 1 ? std::optional<size_t>(grouping_factor) : std::nullopt, chunk,  \
                                   out, true, log_luts);                                                                \
        PFHE_GUARD_END                                                                                                  \
    }                                                                                                                   \
    PFHE_HANDLE_TRIO(P##_bootstrap, P##_bootstrap_handle, tfhe_bootstrap_scratch(h))                                    \
    PFHE_ENTRY(P##_bootstrap_dev, (P##_bootstrap_handle *h, const CW *lwe_in_dev, size_t len_in, const double *bsk_dev, \
                size_t len_bsk, const CW *tv_dev, size_t len_tv, const CW *ksk_dev, size_t len_ksk, CW *lwe_out_dev,    \
                size_t len_out, void *stream),                                                                          \
               bootstrap<W>(Form::kDevice, h, (const W *)lwe_in_dev, len_in, bsk_dev, len_bsk, (const W *)tv_dev,       \
                            len_tv, (const W *)ksk_dev, len_ksk, (W *)lwe_out_dev, len_out, (hipStream_t)stream))       \
    PFHE_ENTRY(P##_bootstrap, (P##_bootstrap_handle *h, const CW *lwe_in, size_t len_in, const double *bsk,             \
                size_t len_bsk, const CW *tv, size_t len_tv, const CW *ksk, size_t len_ksk, CW *lwe_out,                \
                size_t len_out),                                                                                        \
               bootstrap<W>(Form::kHost, h, (const W *)lwe_in, len_in, bsk, len_bsk, (const W *)tv, len_tv,             \
                            (const W *)ksk, len_ksk, (W *)lwe_out, len_out, nullptr))

extern "C" {

PFHE_BOOTSTRAP_FAMILY(pfhe_tfhe, uint64_t, u64)
PFHE_BOOTSTRAP_FAMILY(pfhe_tfhe32, uint32_t, u32)
#undef PFHE_BOOTSTRAP_FAMILY

}  // extern "C"
