// pfhe_tfhe_handles.hpp — what the torus-side handles own (pfhe_fft, the TFHE product plan, the two blind-rotation handles) and
// the basis check they share.  Seen by pfhe_fft.hip, which implements them, and by pfhe_bootstrap.hip, whose bootstrap
// handle is built around a blind-rotation handle, and by pfhe_keygen.hip, which writes the keys they consume.  Host only.
#pragma once

#include "pfhe_capi_internal.hpp"
#include "pfhe_plan_guard.hpp"
#include "pfhe_staging.hpp"

struct pfhe_fft {
    int device = 0;
    pfhe::u32 log_n = 0;
    size_t n = 0;
    double2 *tw = nullptr;  // device: cis(pi j / N), j < N
    ~pfhe_fft() {
        if (!tw) return;
        pfhe::DeviceGuard g(device);
        (void)pfhe::counted_free(tw);
    }
};

// TfheFftContext<T> + ApproxSignedBasis<T> (power-of-two modulus): the shape of the product and its device scratch.
template <class W>
struct TfhePlanCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the plan)
    pfhe::PlanGuard guard;          // one holder at a time (&mut TfheFftContext), successive calls ordered across streams
    pfhe::u32 k = 1, log_basis = 0, ell = 0, drop_bits = 0;
    size_t chunk = 1;
    bool fused = false;
    // general form only: digit spectra (chunk x (k+1) x ell x N/2), accumulators (chunk x (k+1) x N/2) and the key's
    // Hermitian part ((k+1) x ell x (k+1) x N/2), complex f64
    double2 *spec = nullptr, *acc = nullptr, *keyh = nullptr;
    size_t scratch = 0;
    ~TfhePlanCore() {
        if (!fft) return;
        pfhe::DeviceGuard g(fft->device);
        for (double2 *b : {spec, acc, keyh})
            if (b) (void)pfhe::counted_free(b);
    }
};
struct pfhe_tfhe_plan : TfhePlanCore<pfhe::u64> {};
struct pfhe_tfhe32_plan : TfhePlanCore<pfhe::u32> {};

// The blind rotation over the TFHE product: owns a product plan and, in the per-step form, three glue buffers of chunk
// ciphertexts (D, E and the second accumulator of the ping-pong), all allocated at creation.
template <class P, class W>
struct TfheBlindRotCore {
    P *plan = nullptr;     // owned
    pfhe::PlanGuard guard; // one holder at a time and cross-stream ordering of successive calls, as the plan
    bool whole_loop = false;
    size_t chunk = 1;
    W *d = nullptr, *e = nullptr, *ping = nullptr;  // per-step form only: chunk * (k+1) * N words each
    size_t glwe = 0, key_len = 0, glue_bytes = 0;
    ~TfheBlindRotCore() {
        if (!plan) return;
        {
            pfhe::DeviceGuard g(plan->fft->device);
            for (W *b : {d, e, ping})
                if (b) (void)pfhe::counted_free(b);
        }
        delete plan;
    }
};
struct pfhe_tfhe_blindrot : TfheBlindRotCore<pfhe_tfhe_plan, pfhe::u64> {};
struct pfhe_tfhe32_blindrot : TfheBlindRotCore<pfhe_tfhe32_plan, pfhe::u32> {};

// The multi-bit blind rotation: the mask is consumed grouping_factor elements at a time against 2^g keys per group.  Owns,
// in the per-group form, the digit spectra and accumulators of `chunk` ciphertexts and the Hermitian parts of one group's
// 2^g keys; nothing in the whole-loop form.  All allocated at creation.
template <class W>
struct TfheMultiBitCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the handle)
    pfhe::PlanGuard guard;          // one holder at a time and cross-stream ordering of successive calls, as the plan
    pfhe::u32 k = 1, log_basis = 0, ell = 0, drop_bits = 0, g = 1;
    bool whole_loop = false;
    size_t chunk = 1, glwe = 0, key_len = 0, scratch = 0;
    // per-group form only: chunk x (k+1) x ell x N/2, chunk x (k+1) x N/2 and 2^g x (k+1) x ell x (k+1) x N/2 complex f64
    double2 *spec = nullptr, *acc = nullptr, *keyh = nullptr;
    ~TfheMultiBitCore() {
        if (!fft) return;
        pfhe::DeviceGuard dg(fft->device);
        for (double2 *b : {spec, acc, keyh})
            if (b) (void)pfhe::counted_free(b);
    }
};
struct pfhe_tfhe_mbrot : TfheMultiBitCore<pfhe::u64> {};
struct pfhe_tfhe32_mbrot : TfheMultiBitCore<pfhe::u32> {};

namespace pfhe {

// ApproxSignedBasis::new (basis.rs:47-177) with modulus None: its assert!s become PFHE_ERR_BAD_ARGUMENT (log_basis = BITS
// overflows the basis there too); decompose_length 0 = the full length BITS / log_basis
inline int basis_shape(u32 bits, u32 log_basis, size_t length, u32 &ell, u32 &drop) {
    if (log_basis == 0 || log_basis >= bits) {
        set_last_error("log_basis must be in 1..BITS-1");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    const u32 full = bits / log_basis;
    if (length > full) {
        set_last_error("decompose_length exceeds BITS / log_basis");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    ell = length ? (u32)length : full;
    drop = bits - ell * log_basis;
    return PFHE_OK;
}

// The blind rotation's own create and device call (pfhe_fft.hip), as pfhe_tfhe{,32}_blindrot_create / _rotate_dev run them.
int tfhe_blindrot_create_handle(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                size_t chunk, pfhe_tfhe_blindrot **out);
int tfhe_blindrot_create_handle(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                                size_t chunk, pfhe_tfhe32_blindrot **out);
int tfhe_blindrot_rotate_handle(pfhe_tfhe_blindrot *h, u64 *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                                const uint32_t *exps, size_t len_exps, hipStream_t s);
int tfhe_blindrot_rotate_handle(pfhe_tfhe32_blindrot *h, u32 *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                                const uint32_t *exps, size_t len_exps, hipStream_t s);

// true when the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// What pfhe_tfhe{,32}_plan_create decides before it touches the device, in its order (bits: 32 or 64): the basis's assert!s,
// glwe_dimension above 64, the table; for pfhe_keygen.hip, whose GGSW calls start with the same checks.
int tfhe_plan_check_args(u32 bits, const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         u32 &ell, u32 &drop);

// The multi-bit rotation's create and device call (pfhe_fft.hip), as pfhe_tfhe{,32}_mbrot_create / _rotate_dev run them;
// tfhe_mbrot_check_args is what the create decides before it touches the device (bits: 32 or 64).
int tfhe_mbrot_check_args(u32 bits, const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                          size_t grouping_factor);
int tfhe_mbrot_create_handle(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                             size_t grouping_factor, size_t chunk, pfhe_tfhe_mbrot **out);
int tfhe_mbrot_create_handle(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                             size_t grouping_factor, size_t chunk, pfhe_tfhe32_mbrot **out);
int tfhe_mbrot_rotate_handle(pfhe_tfhe_mbrot *h, u64 *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                             const uint32_t *exps, size_t len_exps, hipStream_t s);
int tfhe_mbrot_rotate_handle(pfhe_tfhe32_mbrot *h, u32 *acc, size_t len_acc, const double *bsk, size_t len_bsk,
                             const uint32_t *exps, size_t len_exps, hipStream_t s);

}  // namespace pfhe
