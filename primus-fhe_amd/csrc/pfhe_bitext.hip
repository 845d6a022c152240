// pfhe_bitext.hip — bit extraction: from an LWE ciphertext of a multi-bit message under the extracted GLWE key to one LWE
// ciphertext per bit under the LWE key, each with its bit at 2^(BITS-1) as the circuit bootstrap takes it (include/pfhe.h:
// pfhe_bitext{,32}_*).  No reference counterpart; DESIGN.md §24 states the rule.
//
// Per input e (k N + 1 words, phase m 2^delta + noise) and bit i = 0 .. bits-1, least significant first, c_0 the input:
//   shifted key switch   out[e bits + i] = keyswitch(c_i << sigma_i), sigma_i = BITS - 1 - delta - i: every word shifted as a
//                        wrapping word, then the LWE key switch's rule word for word (the digits of init_carry /
//                        digit_word, the tile of pfhe_tfhe_exact_device.hpp).  Unless i is the last bit, the thread that
//                        stores an output word also stores its modulus switch (switch_rounded at stride 0, the body with
//                        2^(BITS-2) added and negated): the quarter turn of DESIGN.md §19 costs no launch.
//   accumulator          ACC_e = X^{neg_b[e]} TV_i, TV_i = (0, .., 0, -2^(delta+i-1) on every coefficient), written from
//                        constants by pfhe_tfhe_stages.hip's kernel at one level (launch_const_acc_init).
//   blind rotation       the classic handle behind TfheRotation, called as it is.
//   extract and subtract c_{i+1} = c_i - (extraction of ACC_e at index 0, with 2^(delta+i-1) added to the body): bit i cleared
//                        (launch_extract with a source, pfhe_tfhe_stages.hip's extraction kernel in its subtracting form).
// Every step is exact integer arithmetic modulo 2^BITS except the rotation; no atomics, no scratch memory.  Launches and
// the two forms of the call (handle_call) go through pfhe_tfhe_host.hpp; the key switch keeps its own 2-D grid.
#include <algorithm>
#include <cstdint>
#include <memory>

#include "pfhe_tfhe_exact_device.hpp"
#include "pfhe_tfhe_handles.hpp"

using namespace pfhe;

namespace pfhe {
namespace {

// ---------------- shifted key switch, with the modulus switch of what it stores ----------------
//
// The key-switch tile with M = batch, K = in_dimension * ell, out_dimension + 1 columns, as tfhe_keyswitch_kernel; the
// mask words and the body are shifted left by `shift` first.  Output row e starts at lwe_out + e * out_stride (the bits of
// an input are neighbours in the caller's output).  exps != null: output word (e, col) also goes through switch_rounded to
// exps[e n + col], the body (col = n) with 2^(BITS-2) added and negated to neg_b[e]; every word has one thread.

// Two things about the form, both measured on the u64 kernel, whose row loop the compiler schedules by what surrounds it
// (DESIGN.md §24).  The body is shifted behind the select, not in front of it: with `col == n ? body << shift : 0` the loop
// takes 110 registers (four waves per SIMD) instead of tfhe_keyswitch_kernel's 92 (five).  And the modulus switch is a
// pass of its own over the words the thread has just stored, read back from memory (a thread sees its own stores): with
// the switch inside the storing loop, the sums stay live into it and every launch ran 3.5 % longer than tfhe_keyswitch_kernel.
template <class W>
__global__ __launch_bounds__(kThreads) void tfhe_bitext_keyswitch_kernel(
    const W *__restrict__ lwe_in, const W *__restrict__ ksk, W *__restrict__ lwe_out, u32 *__restrict__ exps,
    u32 *__restrict__ neg_b, KsShape s, u32 shift, u32 log_n, u64 out_stride, u64 batch) {
    __shared__ W dig[kKsMaxRows * kKsTileM];
    const u32 lane = threadIdx.x % kKsLanes, wave = threadIdx.x / kKsLanes;
    const u32 cols = s.out_dim + 1;
    const u32 c0 = blockIdx.x * kKsTileN + lane;
    const u64 e0 = (u64)blockIdx.y * kKsTileM;
    const u64 in_stride = (u64)s.in_dim + 1;
    W acc[kKsRows][kKsCols] = {};
    // a column past the end reads the last one instead (its sums are never stored), as tfhe_keyswitch_kernel
    const W *key[kKsCols];
#pragma unroll
    for (int c = 0; c < kKsCols; ++c) key[c] = ksk + min(c0 + c * kKsLanes, cols - 1);
    ks_tile_sums(dig, lwe_in, in_stride, s.in_dim, e0, batch, key, cols, s.log_basis, s.ell, s.drop_bits, s.ki, acc, shift);
#pragma unroll
    for (int r = 0; r < kKsRows; ++r) {
        const u64 e = e0 + wave * kKsRows + r;
        if (e >= batch) continue;
#pragma unroll
        for (int c = 0; c < kKsCols; ++c) {
            const u32 col = c0 + c * kKsLanes;
            if (col >= cols) continue;
            const W b = (W)((col == s.out_dim ? lwe_in[e * in_stride + s.in_dim] : (W)0) << shift);
            lwe_out[e * out_stride + col] = b - acc[r][c];
        }
    }
    if (!exps) return;
    const u32 two_n_mask = (2u << log_n) - 1;
#pragma unroll
    for (int r = 0; r < kKsRows; ++r) {
        const u64 e = e0 + wave * kKsRows + r;
        if (e >= batch) continue;
#pragma unroll
        for (int c = 0; c < kKsCols; ++c) {
            const u32 col = c0 + c * kKsLanes;
            if (col >= cols) continue;
            const W word = lwe_out[e * out_stride + col];  // this thread's own store of the loop above
            if (col < s.out_dim) {
                exps[e * s.out_dim + col] = switch_rounded<W>(word, log_n, 0) & two_n_mask;
            } else {
                const u32 v = switch_rounded<W>((W)(word + ((W)1 << (8 * sizeof(W) - 2))), log_n, 0) & two_n_mask;
                neg_b[e] = ((2u << log_n) - v) & two_n_mask;
            }
        }
    }
}

// ---------------- launches (arguments already checked) ----------------

// exps / neg_b null: the last bit, whose output nobody switches
template <class W>
int launch_bitext_keyswitch(const W *lwe_in, const W *ksk, W *lwe_out, u32 *exps, u32 *neg_b, KsShape sh, u32 shift,
                            u32 log_n, u64 out_stride, u64 batch, hipStream_t s) {
    const u64 gx = ((u64)sh.out_dim + 1 + kKsTileN - 1) / kKsTileN;
    return launch_y_slices((batch + kKsTileM - 1) / kKsTileM, [&](u64 first_tile, u32 tiles) {
        const u64 done = first_tile * kKsTileM, cur = std::min<u64>(batch - done, (u64)tiles * kKsTileM);
        return launch_grid(tfhe_bitext_keyswitch_kernel<W>, dim3((u32)gx, tiles), 0, s, lwe_in + done * ((u64)sh.in_dim + 1), ksk,
                           lwe_out + done * out_stride, exps ? exps + done * sh.out_dim : nullptr,
                           neg_b ? neg_b + done : nullptr, sh, shift, log_n, out_stride, cur);
    });
}

}  // namespace
}  // namespace pfhe

// ---------------- the bit-extraction handle ----------------

// Owns a classic blind rotation (behind TfheRotation) and, for `chunk` inputs, one accumulator each, the switched exponents,
// neg_b and the running ciphertexts of k N + 1 words (TfheBootstrapBase's `extracted`): all allocated at creation.
template <class W>
struct TfheBitextCore : TfheBootstrapBase<W> {
    KsShape ks{};
};
struct pfhe_bitext : TfheBitextCore<u64> {};
struct pfhe_bitext32 : TfheBitextCore<u32> {};

namespace {

constexpr const char *kBitextBusy = "TFHE bit extraction handle in use by another thread (one handle per thread)";
constexpr const char *kBitextLengths =
    "TFHE bit extraction: lwe_in must be batch*(k*N+1) words, bsk n*(k+1)*ell*(k+1)*N complex values, ksk k*N*ks_ell*(n+1) "
    "words and bits_out batch*bits*(n+1)";
constexpr size_t kBitextDefaultAccBytes = 256ull << 20;

// Everything that decides before the device first, in bootstrap_create's order: a null out pointer, the product plan's
// checks, the dimensions, the key-switch basis's assert!s; then the rotation's create
template <class W, class H>
int bitext_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t lwe_dimension,
                  uint32_t ks_log_basis, size_t ks_decompose_length, size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    Shape sh{};
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    // a zero glwe_dimension is refused as a zero lwe_dimension is: one message for both
    PFHE_TRY(require_lwe_dimension(glwe_dimension ? lwe_dimension : 0,
                                   "TFHE bit extraction: glwe_dimension must be at least 1 and lwe_dimension in 1..2^31-2"));
    u32 ks_ell = 0, ks_drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), ks_log_basis, ks_decompose_length, ks_ell, ks_drop));
    auto h = std::make_unique<H>();
    TfheRotation<W> *rotation = nullptr;
    PFHE_TRY(tfhe_rotation_create<W>(fft, glwe_dimension, log_basis, decompose_length, std::nullopt, chunk, &rotation));
    h->rotation.reset(rotation);
    const TfheRotation<W> &rot = *h->rotation;
    h->fft = fft;
    h->k = (u32)glwe_dimension;
    h->n = (u32)lwe_dimension;
    const size_t glwe = rot.glwe, ext = glwe_dimension * fft->n + 1;
    h->ks = KsShape{(u32)(ext - 1), h->n, ks_log_basis, ks_ell, ks_drop, ks_group_words(ks_ell)};
    h->bsk_len = lwe_dimension * rot.key_len;
    // chunk 0: the rotation's default, capped at about 256 MiB of accumulators
    h->chunk = chunk ? rot.chunk : std::min(rot.chunk, std::max<size_t>(1, kBitextDefaultAccBytes / (glwe * sizeof(W))));
    DeviceGuard g(fft->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->bufs.bind(fft->device);
    PFHE_TRY(h->bufs.add(h->acc, h->chunk * glwe));
    PFHE_TRY(h->bufs.add(h->extracted, h->chunk * ext));
    PFHE_TRY(h->bufs.add(h->exps, h->chunk * lwe_dimension));
    PFHE_TRY(h->bufs.add(h->neg_b, h->chunk));
    PFHE_TRY(h->guard.init(fft->device));
    *out = h.release();
    return PFHE_OK;
}

// After a null handle and a second holder: delta_log and bits, the host form's null pointers, the lengths, the empty
// batch, the device form's null pointers, alignment, overlap; handle_call then refuses the device.
template <class W, class H>
int extract_bits(Form form, H *h, const W *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const W *ksk,
                 size_t len_ksk, uint32_t delta_log, uint32_t bits, W *bits_out, size_t len_out, hipStream_t s) {
    if (!h || !h->rotation) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kBitextBusy);
    constexpr u32 kBits = 8 * sizeof(W);
    if (delta_log == 0 || bits == 0 || delta_log > kBits || bits > kBits - delta_log) {
        set_last_error("TFHE bit extraction: delta_log and bits must be at least 1 and delta_log + bits at most BITS");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (form == Form::kHost && ((!lwe_in && len_in) || (!bsk && len_bsk) || (!ksk && len_ksk) || (!bits_out && len_out)))
        return PFHE_ERR_BAD_ARGUMENT;
    const pfhe_fft &f = *h->fft;
    const size_t glwe = h->rotation->glwe, ext = (size_t)h->k * f.n + 1, out_words = (size_t)h->n + 1;
    const u64 batch = len_in / ext;
    if (len_in % ext != 0 || len_out != batch * bits * out_words || len_bsk != h->bsk_len ||
        len_ksk != (ext - 1) * h->ks.ell * out_words) {
        set_last_error(kBitextLengths);
        return PFHE_ERR_BAD_LENGTH;
    }
    if (batch == 0) return PFHE_OK;
    if (form == Form::kDevice) {
        if (!lwe_in || !bsk || !ksk || !bits_out) return PFHE_ERR_BAD_ARGUMENT;
        PFHE_REQUIRE_ALIGNED(lwe_in);
        PFHE_REQUIRE_ALIGNED(bsk);
        PFHE_REQUIRE_ALIGNED(ksk);
        PFHE_REQUIRE_ALIGNED(bits_out);
        const size_t out_bytes = len_out * sizeof(W);
        if (overlaps(lwe_in, len_in * sizeof(W), bits_out, out_bytes) ||
            overlaps(bsk, len_bsk * 2 * sizeof(double), bits_out, out_bytes) ||
            overlaps(ksk, len_ksk * sizeof(W), bits_out, out_bytes)) {
            set_last_error("TFHE bit extraction: the output must not overlap an input");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    const StageBuf bufs[] = {stage_in(lwe_in, len_in * sizeof(W)), stage_in(bsk, len_bsk * sizeof(double2)),
                             stage_in(ksk, len_ksk * sizeof(W)), stage_out(bits_out, len_out * sizeof(W))};
    return handle_call(h->guard, f.device, form, bufs, s, [&](void *const *d, hipStream_t st) -> int {
        const W *in = (const W *)d[0], *key = (const W *)d[2];
        W *out = (W *)d[3];
        const u64 out_stride = (u64)bits * out_words;
        // chunk after chunk, all bits of a chunk first; the running ciphertexts are the caller's input until bit 0 is
        // cleared into the owned buffer, so the input is neither copied nor written
        for (u64 done = 0; done < batch; done += h->chunk) {
            const u64 cur = std::min<u64>(h->chunk, batch - done);
            const W *run = in + done * ext;
            for (u32 i = 0; i < bits; ++i) {
                const bool last = i + 1 == bits;
                PFHE_TRY(launch_bitext_keyswitch<W>(run, key, out + (done * bits + i) * out_words, last ? nullptr : h->exps,
                                                    last ? nullptr : h->neg_b, h->ks, kBits - 1 - delta_log - i, f.log_n,
                                                    out_stride, cur, st));
                if (last) break;
                const u32 half_shift = delta_log + i - 1;
                PFHE_TRY(launch_const_acc_init<W>(h->acc, h->neg_b, h->k, f.log_n, 1, 0, 1, 0, half_shift, cur, st));
                PFHE_TRY(h->rotation->rotate_dev(h->acc, cur * glwe, (const double *)d[1], len_bsk, h->exps, cur * h->n, st));
                PFHE_TRY(launch_extract<W>(h->acc, run, h->extracted, h->k, f.log_n, ExtractRule{1, 0, 1, 1, 0, half_shift}, cur,
                                           st));
                run = h->extracted;
            }
        }
        return PFHE_OK;
    });
}

}  // namespace

// The entry points of one word width.  P: pfhe_bitext / pfhe_bitext32, the handle type and the prefix; CW / W: the word as
// pfhe.h and as the library spell it.
#define PFHE_BITEXT_FAMILY(P, CW, W)                                                                                     \
    PFHE_ENTRY(P##_create, (const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,    \
                size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, size_t chunk, P **out),         \
               bitext_create<W>(fft, glwe_dimension, log_basis, decompose_length, lwe_dimension, ks_log_basis,           \
                                ks_decompose_length, chunk, out))                                                        \
    PFHE_HANDLE_TRIO(P, P, tfhe_bootstrap_scratch(h))                                                                    \
    PFHE_ENTRY(P##_extract_bits_dev, (P *h, const CW *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk,  \
                const CW *ksk_dev, size_t len_ksk, uint32_t delta_log, uint32_t bits, CW *bits_out_dev, size_t len_out,  \
                void *stream),                                                                                           \
               extract_bits<W>(Form::kDevice, h, (const W *)lwe_in_dev, len_in, bsk_dev, len_bsk, (const W *)ksk_dev,    \
                               len_ksk, delta_log, bits, (W *)bits_out_dev, len_out, (hipStream_t)stream))               \
    PFHE_ENTRY(P##_extract_bits, (P *h, const CW *lwe_in, size_t len_in, const double *bsk, size_t len_bsk,              \
                const CW *ksk, size_t len_ksk, uint32_t delta_log, uint32_t bits, CW *bits_out, size_t len_out),         \
               extract_bits<W>(Form::kHost, h, (const W *)lwe_in, len_in, bsk, len_bsk, (const W *)ksk, len_ksk,         \
                               delta_log, bits, (W *)bits_out, len_out, nullptr))

extern "C" {

PFHE_BITEXT_FAMILY(pfhe_bitext, uint64_t, u64)
PFHE_BITEXT_FAMILY(pfhe_bitext32, uint32_t, u32)
#undef PFHE_BITEXT_FAMILY

}  // extern "C"
