// pfhe_tfhe_handles.hpp — what the torus-side handles own: the FFT table, the TFHE product plan, and the two blind
// rotations behind the one interface the bootstrap handle holds (TfheRotation); and the argument checks their creates
// share.  pfhe_fft.hip implements them; pfhe_bootstrap.hip and pfhe_cbs.hip see a rotation only as a TfheRotation;
// pfhe_cmux.hip owns a product plan and queues the product's launches itself, and pfhe_lut.hip runs the CMUX's launches on a
// core it owns; pfhe_keygen.hip, which writes the keys they consume, starts its GGSW calls with the plan's checks.  Host
// only; the host layer under the entry points of all of them is pfhe_tfhe_host.hpp.
#pragma once

#include <memory>
#include <optional>

#include "pfhe_capi_internal.hpp"
#include "pfhe_device_buffers.hpp"
#include "pfhe_plan_guard.hpp"
#include "pfhe_tfhe_host.hpp"

struct pfhe_fft {
    int device = 0;
    pfhe::u32 log_n = 0;
    size_t n = 0;
    double2 *tw = nullptr;  // device: cis(pi j / N), j < N
    pfhe::DeviceBuffers bufs;
};

// The device scratch of the general product, shared by the product plan and the per-group multi-bit rotation: digit spectra
// (chunk x (k+1) x ell x N/2), accumulators (chunk x (k+1) x N/2) and the Hermitian parts of `key_copies` keys
// ((k+1) x ell x (k+1) x N/2 each), complex f64.  All of it is allocated by create() or none.
struct TfheProductScratch {
    static constexpr size_t kDefaultBytes = 256ull << 20;
    double2 *spec = nullptr, *acc = nullptr, *keyh = nullptr;
    pfhe::DeviceBuffers bufs;
    size_t bytes() const { return bufs.bytes(); }

    // Sizes `chunk` (0: the default — what fits kDefaultBytes of spectra and accumulators, or 65536 ciphertexts for a form
    // that needs no scratch; never more than one launch's grid holds) and, when the form needs it, allocates the three
    // buffers on the current device, which must be the table's.
    int create(const pfhe_fft &f, const pfhe::Shape &sh, size_t key_copies, bool needed, size_t &chunk) {
        const size_t m = f.n / 2, rows = sh.k + 1, digits = rows * sh.ell;
        if (!chunk) chunk = needed ? std::max<size_t>(1, kDefaultBytes / ((digits + rows) * m * sizeof(double2))) : 65536;
        chunk = std::min<size_t>(chunk, needed ? 0x7fffffffull / digits : 0x7fffffffull);
        if (!needed) return PFHE_OK;
        bufs.bind(f.device);
        PFHE_TRY(bufs.add(spec, chunk * digits * m));
        PFHE_TRY(bufs.add(acc, chunk * rows * m));
        return bufs.add(keyh, key_copies * digits * rows * m);
    }
};

// TfheFftContext<T> + ApproxSignedBasis<T> (power-of-two modulus): the shape of the product and its device scratch (the
// general form's; the fused form has none).
template <class W>
struct TfhePlanCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the plan)
    pfhe::PlanGuard guard;          // one holder at a time (&mut TfheFftContext), successive calls ordered across streams
    pfhe::Shape shape{};
    size_t chunk = 1;
    bool fused = false;
    TfheProductScratch scratch;
};
struct pfhe_tfhe_plan : TfhePlanCore<pfhe::u64> {};
struct pfhe_tfhe32_plan : TfhePlanCore<pfhe::u32> {};

// A blind rotation as the bootstrap handle sees it: the classic one or the multi-bit one.  rotate_dev is the handle's own
// device call (its lease, checks and stream order), scratch_bytes what its create allocated.
template <class W>
struct TfheRotation {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the handle)
    pfhe::PlanGuard guard;          // one holder at a time and cross-stream ordering of successive calls, as the plan
    bool whole_loop = false;
    size_t chunk = 1, glwe = 0, key_len = 0;  // words of a ciphertext, complex values of one Fourier GGSW key
    virtual ~TfheRotation() = default;
    virtual int rotate_dev(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps,
                           hipStream_t s) = 0;
    virtual size_t scratch_bytes() const = 0;
};

// The blind rotation over the TFHE product: owns a product plan and, in the per-step form, three glue buffers of chunk
// ciphertexts (D, E and the second accumulator of the ping-pong), all allocated at creation.
template <class W>
struct TfheBlindRotCore : TfheRotation<W> {
    std::unique_ptr<TfhePlanCore<W>> plan;          // owned
    W *d = nullptr, *e = nullptr, *ping = nullptr;  // per-step form only: chunk * (k+1) * N words each
    pfhe::DeviceBuffers bufs;                       // after the plan: the glue buffers are freed first, then the plan
    int rotate_dev(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps,
                   hipStream_t s) override;
    size_t scratch_bytes() const override { return plan->scratch.bytes() + bufs.bytes(); }
};
struct pfhe_tfhe_blindrot : TfheBlindRotCore<pfhe::u64> {};
struct pfhe_tfhe32_blindrot : TfheBlindRotCore<pfhe::u32> {};

// The multi-bit blind rotation: the mask is consumed grouping_factor elements at a time against 2^g keys per group.  Owns,
// in the per-group form, the product's scratch for `chunk` ciphertexts with the Hermitian parts of one group's 2^g keys;
// nothing in the whole-loop form.  All allocated at creation.
template <class W>
struct TfheMultiBitCore : TfheRotation<W> {
    pfhe::Shape shape{};
    pfhe::u32 g = 1;
    TfheProductScratch scratch;
    int rotate_dev(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps,
                   hipStream_t s) override;
    size_t scratch_bytes() const override { return scratch.bytes(); }
};
struct pfhe_tfhe_mbrot : TfheMultiBitCore<pfhe::u64> {};
struct pfhe_tfhe32_mbrot : TfheMultiBitCore<pfhe::u32> {};

// What the bootstrap handle (pfhe_bootstrap.hip) and the circuit bootstrap handle (pfhe_cbs.hip) share: a blind rotation
// they own (classic or multi-bit, behind TfheRotation) and, sized by their creates for `chunk` inputs, the accumulators,
// the extracted LWE ciphertexts, the switched exponents and neg_b, all allocated at creation.  Destroyed in the order
// buffers, rotation, guard.
template <class W>
struct TfheBootstrapBase {
    pfhe::PlanGuard guard;                      // one holder at a time, successive calls on different streams ordered
    std::unique_ptr<TfheRotation<W>> rotation;  // owned
    const pfhe_fft *fft = nullptr;
    pfhe::u32 k = 1, n = 0;          // GLWE and LWE dimensions
    size_t chunk = 1, bsk_len = 0;   // bsk_len: complex values of the whole key
    W *acc = nullptr, *extracted = nullptr;
    pfhe::u32 *exps = nullptr, *neg_b = nullptr;
    pfhe::DeviceBuffers bufs;
};

// The CMUX tree handle (pfhe_cmux.hip), which the look-up handle (pfhe_lut.hip) owns one of as well.  Owns, for `chunk`
// inputs of a tree of depth d: the two ping-pong node buffers (chunk * 2^(d-1) and chunk * 2^(d-2)
// ciphertexts; the last level writes into the caller's output) and, in the general form, a product plan and the D and E
// buffers of chunk * 2^(d-1) ciphertexts.  All allocated at creation.
template <class W>
struct TfheCmuxTreeCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the handle)
    pfhe::PlanGuard guard;          // one holder at a time, successive calls on different streams ordered
    pfhe::Shape shape{};
    pfhe::u32 depth = 1;
    bool fused = false;
    size_t chunk = 1, glwe = 0, key_len = 0;
    std::unique_ptr<TfhePlanCore<W>> plan;  // owned, general form only; its launches run under this handle's guard
    W *node[2] = {nullptr, nullptr}, *d = nullptr, *e = nullptr;
    pfhe::DeviceBuffers bufs;  // after the plan: the four buffers are freed first, then the plan
    size_t launch_nodes() const { return chunk << (depth - 1); }
};

// The GLWE trace handle (pfhe_trace.hip), which the ring-packing handle (pfhe_ring_pack.hip) owns one of off the fused
// shape.  Owns, in the general form, for `chunk` ciphertexts: the product's scratch (digit spectra, accumulators, the
// Hermitian parts of one key) and three word buffers: D (k polynomials per ciphertext), the gathered bodies (one) and E
// (k+1).  Nothing in the fused form.  All allocated at creation.
template <class W>
struct TfheTraceCore {
    const pfhe_fft *fft = nullptr;  // borrowed (must outlive the handle)
    pfhe::PlanGuard guard;          // one holder at a time, successive calls on different streams ordered
    pfhe::Shape shape{};
    bool fused = false;
    size_t chunk = 1, glwe = 0, key_len = 0;
    TfheProductScratch scratch;
    W *d = nullptr, *body = nullptr, *e = nullptr;
    pfhe::DeviceBuffers bufs;  // after the scratch: the word buffers are freed first
};

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

// What pfhe_tfhe{,32}_plan_create decides before it touches the device, in its order: the basis's assert!s, glwe_dimension
// above 64, the table.  The rotations' creates and pfhe_keygen.hip's GGSW calls start with the same checks.
template <class W>
int tfhe_plan_check(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, Shape &sh) {
    u32 ell = 0, drop = 0;
    PFHE_TRY(basis_shape(8 * sizeof(W), log_basis, decompose_length, ell, drop));
    if (glwe_dimension > kMaxGlweDimension) {
        set_last_error("glwe_dimension above 64 is not supported");
        return PFHE_ERR_UNSUPPORTED;
    }
    if (!fft) return PFHE_ERR_BAD_ARGUMENT;
    sh = Shape{fft->log_n, (u32)glwe_dimension, log_basis, ell, drop};
    return PFHE_OK;
}

// ... and the multi-bit rotation's: the plan's checks, then the grouping factor, all before the device
template <class W>
int tfhe_mbrot_check(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                     size_t grouping_factor, Shape &sh) {
    PFHE_TRY(tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh));
    if (grouping_factor == 0 || grouping_factor > kMaxGrouping) {
        set_last_error("grouping_factor must be in 1..4");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    return PFHE_OK;
}

// The "classic or multi-bit" head of the two bootstrap creates, all before the device: with a grouping factor the multi-bit
// rotation's checks and then the divisibility, refused with the caller's own message; without one the plan's checks
template <class W>
int tfhe_bootstrap_check(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         std::optional<size_t> grouping_factor, size_t lwe_dimension, const char *not_a_multiple, Shape &sh) {
    if (!grouping_factor) return tfhe_plan_check<W>(fft, glwe_dimension, log_basis, decompose_length, sh);
    PFHE_TRY(tfhe_mbrot_check<W>(fft, glwe_dimension, log_basis, decompose_length, *grouping_factor, sh));
    if (lwe_dimension % *grouping_factor != 0) {
        set_last_error(not_a_multiple);
        return PFHE_ERR_BAD_ARGUMENT;
    }
    return PFHE_OK;
}

// What the key switches into a GLWE and their keys decide first (packing and private key switch, pfhe_pack.hip and
// pfhe_cbs.hip): ApproxSignedBasis::new's assert!s, the two dimensions refused with the caller's own message, then the table
template <class W>
int tfhe_keyswitch_dimensions(const char *message, const pfhe_fft *f, size_t k, size_t in_dimension, uint32_t log_basis,
                              size_t decompose_length, u32 &ell, u32 &drop) {
    PFHE_TRY(basis_shape(8 * sizeof(W), log_basis, decompose_length, ell, drop));
    PFHE_TRY(require_glwe_dimension(k, message));
    PFHE_TRY(require_lwe_dimension(in_dimension, message));
    if (!f) return PFHE_ERR_BAD_ARGUMENT;
    return PFHE_OK;
}

// B += sum_r A_r z_r on every GLWE row of a key under generation (pfhe_keygen.hip's body call, adding), for either word
inline int glwe_body_add(const pfhe_fft *f, size_t k, u64 *glwe, size_t len, const u64 *key, size_t len_key, hipStream_t s) {
    return pfhe_tfhe_glwe_body_mac_dev(f, k, (uint64_t *)glwe, len, (const uint64_t *)key, len_key, 0, s);
}
inline int glwe_body_add(const pfhe_fft *f, size_t k, u32 *glwe, size_t len, const u32 *key, size_t len_key, hipStream_t s) {
    return pfhe_tfhe32_glwe_body_mac_dev(f, k, glwe, len, key, len_key, 0, s);
}

// keys of a bootstrapping key: lwe_dimension, or (lwe_dimension / g) 2^g multi-bit ones
inline size_t tfhe_bootstrap_keys(std::optional<size_t> grouping_factor, size_t lwe_dimension) {
    return grouping_factor ? (lwe_dimension / *grouping_factor) << *grouping_factor : lwe_dimension;
}

// *_scratch_bytes of both: the rotation's plus the handle's own buffers
template <class W>
size_t tfhe_bootstrap_scratch(const TfheBootstrapBase<W> *h) {
    return h && h->rotation ? h->rotation->scratch_bytes() + h->bufs.bytes() : 0;
}

// The rotation of a bootstrap handle (pfhe_fft.hip, instantiated for u32 and u64): what pfhe_tfhe{,32}_blindrot_create
// runs when there is no grouping factor, pfhe_tfhe{,32}_mbrot_create with one.
template <class W>
int tfhe_rotation_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         std::optional<size_t> grouping_factor, size_t chunk, TfheRotation<W> **out);

// The product plan a handle owns (pfhe_fft.hip, instantiated for P = TfhePlanCore<W>, u32 and u64): what
// pfhe_tfhe{,32}_plan_create runs, and the product's launches on `batch` ciphertexts, arguments already checked and the
// device current.  The owner calls the launches inside its own ordered_on; the plan's own guard stays unused.
template <class W, class P>
int tfhe_plan_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t chunk,
                     P **out);
template <class W>
int tfhe_product_impl(TfhePlanCore<W> *p, const W *in, const double2 *key, W *out, u64 batch, hipStream_t s);

// The four launches of the general product for a caller that decomposes fewer rows than k+1 (pfhe_trace.hip: the k mask
// rows): the Hermitian parts of `polys` key polynomials, the digit transforms of `polys` torus polynomials (polys * ell
// workgroups, spectra in natural order polynomial after polynomial, level after level), the multiply-accumulate of `batch`
// ciphertexts' in_rows * ell digit spectra into their k+1 accumulators, and the half-spectrum inverses of `polys`
// accumulators.  pfhe_fft.hip; the device is current.
int tfhe_key_herm_launch(const pfhe_fft &f, const double2 *key, double2 *keyh, u64 polys, hipStream_t s);
int tfhe_mulacc_launch(const pfhe_fft &f, const double2 *spec, const double2 *keyh, double2 *acc, u32 k, u32 ell, u32 in_rows,
                       u64 batch, hipStream_t s);
template <class W>
int tfhe_digit_fwd_launch(const pfhe_fft &f, const Shape &sh, const W *in, double2 *spec, u64 polys, hipStream_t s);
template <class W>
int tfhe_half_inverse_launch(const pfhe_fft &f, const double2 *acc, W *out, u64 polys, hipStream_t s);

// The exact stages around a rotation, one kernel each (pfhe_tfhe_stages.hip, instantiated for u32 and u64), arguments
// already checked and the device current.
//   launch_modswitch       the modulus switch to multiples of 2^log_stride (body_offset is added to the body word first);
//                          input e's exponents go to exps[(e copies + c) n ..] for every c < copies, its body to neg_b[e].
//   launch_acc_init        ACC_e = X^{neg_b[e]} TV_e on the caller's test vector(s), tv_stride words apart (0: one for all).
//   launch_const_acc_init  `accs` accumulators X^{neg_b[a / per_input]} TV written from constants: body coefficient c of TV
//                          is -2^(half_shift + level log_basis) at level = a mod per_input + c mod 2^log_stride, 0 from
//                          `levels` on.
//   launch_extract         `rows` output rows of k N + 1 words by the rule below; src null: the rows go to dst; src given:
//                          dst = src - rows, and dst may be exactly src.
// Row a of an extraction reads accumulator a / per_acc at index first_index + a mod per_acc (below N); add_half: plus
// 2^(half_shift + (a mod level_period) log_basis) on the body.
struct ExtractRule {
    u32 per_acc, first_index, level_period, add_half, log_basis, half_shift;
};
template <class W>
int launch_modswitch(const W *lwe, u32 n, u32 log_n, u32 log_stride, W body_offset, u32 copies, u32 *exps, u32 *neg_b,
                     u64 batch, hipStream_t s);
template <class W>
int launch_acc_init(const W *tv, u64 tv_stride, W *acc, const u32 *neg_b, u32 rows, u32 log_n, u64 batch, hipStream_t s);
template <class W>
int launch_const_acc_init(W *acc, const u32 *neg_b, u32 k, u32 log_n, u32 per_input, u32 log_stride, u32 levels, u32 log_basis,
                          u32 half_shift, u64 accs, hipStream_t s);
template <class W>
int launch_extract(const W *glwe, const W *src, W *dst, u32 k, u32 log_n, const ExtractRule &rule, u64 rows, hipStream_t s);

// The CMUX of a handle that owns a TfheCmuxTreeCore without being one (pfhe_cmux.hip, instantiated for u32 and u64): what
// pfhe_tfhe{,32}_cmux_tree_create runs, its checks and allocations for `chunk` inputs of a tree of `depth` levels, and rule 1
//  on `count` nodes, arguments already checked and the device current: tfhe_cmux_kernel on the fused shape,
// the general form's launches otherwise, at most launch_nodes() nodes per launch.  Node b reads d0 / d1 at
// (period ? b mod period : b) * stride words, takes keys + (b / per_key) * key_stride and writes out at b * (k+1) N.  The
// owner calls it inside its own ordered_on; the core's own guard stays unused.
struct CmuxSources {
    u64 stride, per_key, key_stride;
    u32 period;
};
template <class W>
int tfhe_cmux_core_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t depth,
                          size_t chunk, TfheCmuxTreeCore<W> **out);
template <class W>
int tfhe_cmux_launch(TfheCmuxTreeCore<W> *h, const W *d0, const W *d1, const double2 *keys, W *out, u64 count,
                     const CmuxSources &at, hipStream_t s);

// The trace of a handle that owns a TfheTraceCore without being one (pfhe_trace.hip, instantiated for u32 and u64): what
// pfhe_tfhe{,32}_glwe_trace_create runs; one step of the general form on `cur` ciphertexts (at most the core's chunk):
// dst = [src +] (0, .., 0, sigma_t(gathered_B)) - to_torus(product of sigma_t(gathered_A) with the key), the bracketed term
// when the step accumulates, and dst may be exactly src; and `steps` on `batch` ciphertexts in either form.  Arguments
// already checked and the device current; the owner calls them inside its own ordered_on, the core's own guard stays unused.
struct TraceSteps;  // pfhe_trace_device.hpp
template <class W>
int tfhe_trace_core_create(const pfhe_fft *fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length, size_t chunk,
                           TfheTraceCore<W> **out);
template <class W>
int tfhe_trace_general_step(TfheTraceCore<W> *h, const W *gathered, const W *src, W *dst, const double2 *key, u32 t,
                            u32 accumulate, u64 cur, hipStream_t s);
template <class W>
int tfhe_trace_steps(TfheTraceCore<W> *h, const W *in, const double2 *keys, W *out, u64 batch, const TraceSteps &steps,
                     hipStream_t s);

}  // namespace pfhe
