// pfhe_capi_rns.hip — extern "C" boundary for RNSBase, BigUintApproxSignedBasis and the RNS gadget
// external product (include/pfhe.h, second half).  Every entry point of both widths comes out of one of three families,
// each expanded for u64 and u32: PFHE_RNS_FAMILY, PFHE_EXTPROD_FAMILY, PFHE_BLINDROT_FAMILY; the profile entry and the
// test hold of the u64 plan are written out.
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <new>

#include <cstring>
#include <type_traits>

#include "pfhe_capi_internal.hpp"
#include "pfhe_ntt_device.hpp"
#include "pfhe_plan_guard.hpp"
#include "pfhe_rns.hpp"
#include "pfhe_staging.hpp"

using namespace pfhe;

// The RNS gadget external product's plan, for both word widths (W = u64: pfhe_extprod_plan over a U64DcrtTable;
// W = u32: pfhe_extprod32_plan, CrtGlwe<u32>::mul_dcrt_ggsw_to over a U32DcrtTable, glwe/crt.rs:200-227,
// dcrt/prime32.rs:11).  The plan owns the product's scratch (digit buffers); `guard` keeps it to one holder at a time.
template <class W>
struct ExtprodPlanCore {
    using Word = W;
    const TableSet *table = nullptr;  // borrowed from the pfhe_dcrt / pfhe_dcrt32 (must outlive the plan)
    PlanGuard guard;
    RnsParams rns;
    BasisParams basis_par;
    BasisCore basis{};  // the scalar constants of basis_par
    u32 k = 1;
    size_t chunk = 1;
    // digit buffer of chunk * (k+1) * ell * L * N words.  Chunks run one after the other on the caller's stream (every
    // kernel of the product is bound by the same integer ALU: a two-stream software pipeline over two buffers measured
    // 20.9 ms per 1024 products at N = 2^16 against 20.4 ms in order, and is gone).
    // PFHE_DISABLE_FUSED_EXTPROD, read at plan creation: the unfused transform + multiply-accumulate kernels (the form
    // k > 1 takes) for every shape — the parity tests compare the two
    bool use_fused = true;
    // workgroups a call must offer before the fused block + multiply-accumulate kernel is taken (N = 2^16, 3 limbs,
    // coefficient form: 1 / 2 / 4 / 5 ciphertexts take 97 / 121 / 165 / 190 us unfused and 141 / 144 / 158 / 164 us fused)
    static constexpr u64 fused_min_wgs = 160;
    // measurement aid (pfhe_extprod_profile_dev, u64 only): when non-null, run_product records an event before the
    // decomposition, between the decomposition and the transform / multiply-accumulate, and after it, per chunk
    std::vector<hipEvent_t> *prof = nullptr;
    W *digits = nullptr;
    // compact signed digits of one chunk (chunk * (k+1) * ell * N words of sdigit_bytes), or null.  u64: int32 when
    // log_basis <= 31, else int64; u32: balanced int32 digits, for N = 2^16, k = 1 (the fused kernels)
    void *sdigits = nullptr;
    size_t sdigit_bytes = 0;
    DeviceBuffers bufs;
};
struct pfhe_extprod_plan : ExtprodPlanCore<u64> {};
struct pfhe_extprod32_plan : ExtprodPlanCore<u32> {};

namespace {

constexpr const char *kPlanBusy =
    "external-product plan in use by another thread (one plan per thread, like &mut DcrtGlevContext)";

template <class Plan>
int plan_check(const Plan *p) {
    if (!p || !p->table) return PFHE_ERR_BAD_ARGUMENT;
    return PFHE_OK;
}

// one row of the product: acc[e] += glev[e or shared] (x) crt_poly[e]   (glwe/dcrt.rs:178-255)
// rows == k+1 without `accumulate` gives CrtGlwe::mul_dcrt_ggsw_to (glwe/crt.rs:200-227).
// Chunks of ciphertexts run one after the other on the caller's stream.
// `into_coeff`: the caller wants coefficient-form output; *coeff_passes reports how many passes of the inverse
// transform this function already ran on the result: -1 = all of them (small-ring kernel), 1 = the block pass
// (fused into the multiply-accumulate kernel; the caller runs the remaining strided pass), 0 = none.
// `big_input`: the input polynomials are BigUintPolynomials (value_len limbs per coefficient) instead of CRT ones.
int run_product(pfhe_extprod_plan *p, const u64 *crt_polys, u32 rows, const u64 *keys, bool keys_shared, u64 *result,
                u64 batch, bool accumulate, hipStream_t s, bool big_input, bool into_coeff = false,
                int *coeff_passes = nullptr) {
    return ordered_on(p->guard, s, [&]() -> int {
        if (coeff_passes) *coeff_passes = 0;
        const TableSet &t = *p->table;
        const u64 W = (u64)t.L * t.n;
        RnsParams rns = p->rns;
        rns.dev.big_input = rns.wide_tab.big_input = big_input ? 1u : 0u;
        const u64 in_words = big_input ? (u64)rns.dev.value_len * t.n : W;  // words per input polynomial
        const u32 ell = p->basis.ell;
        const u64 key_words = (u64)rows * ell * (p->k + 1) * W;
        // Everything runs chunk after chunk on the caller's stream (also while the caller captures a HIP graph).
        // small rings: digit extraction + ONE kernel for everything else
        // (one workgroup per (ciphertext, limb) runs 12+ transforms back to back: it needs a batch that fills the chip)
        if (p->sdigits != nullptr && extprod_small_supported(t.log_n, p->k, p->rns.dev.value_len, p->basis.log_basis) &&
            batch * t.L >= 1024 && p->use_fused) {
            for (u64 done = 0; done < batch; done += p->chunk) {
                const u64 cur = std::min<u64>(p->chunk, batch - done);
                PFHE_TRY(gadget_signed_digits_dev(rns, p->basis_par, t.log_n, crt_polys + done * rows * in_words, (int *)p->sdigits, cur * rows, s));
                PFHE_TRY(extprod_small_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, p->k, rows, ell, (const int *)p->sdigits,
                                           keys + (keys_shared ? 0 : done * key_words), keys_shared,
                                           result + done * (p->k + 1) * W, cur, accumulate, into_coeff, s));
            }
            if (coeff_passes) *coeff_passes = into_coeff ? -1 : 0;
            return PFHE_OK;
        }
        const bool fused = gadget_fused_supported(t.log_n, p->k) && p->use_fused &&
                           ((std::min<u64>(batch, p->chunk) * t.L) << (t.log_n - 12)) >= p->fused_min_wgs;
        const int passes = ntt_num_passes(t.log_n, t.ntt_arith);
        // One arithmetic for everything in here — the gadget kernels and the plain transform passes around them: the table's
        // transform arithmetic t.ntt_arith (pseudo-Mersenne, Montgomery form for generic primes below 2^61, or the
        // reference's Shoup form).
        // coefficient-form output: the inverse transform's block pass runs inside the fused kernel, on the accumulators
        const bool inv_tail = fused && into_coeff && !accumulate && coeff_passes != nullptr && passes == 2;
        if (inv_tail) *coeff_passes = 1;
        const bool fused_decompose = gadget_decompose_strided_supported(t.log_n, p->rns.dev.value_len) && p->sdigits != nullptr;
        u64 *dg = p->digits;
        for (u64 done = 0; done < batch; done += p->chunk) {
            const u64 cur = std::min<u64>(p->chunk, batch - done);
            const u64 npolys = cur * rows * ell * t.L;
            const auto stamp = [&]() -> int {
                if (p->prof == nullptr) return PFHE_OK;
                hipEvent_t ev = nullptr;
                PFHE_HIP(hipEventCreate(&ev));
                p->prof->push_back(ev);
                PFHE_HIP(hipEventRecord(ev, s));
                return PFHE_OK;
            };
            PFHE_TRY(stamp());
            // ---- steps (1)-(4) + strided passes into the digit buffer ----
            if (fused_decompose) {
                PFHE_TRY(gadget_decompose_strided_dev(rns, p->basis_par, t.primes_dev, t.log_n, t.ntt_arith,
                                                      crt_polys + done * rows * in_words, dg, cur * rows, s, p->sdigits));
            } else {
                PFHE_TRY(gadget_decompose_dev(rns, p->basis_par, t.log_n, crt_polys + done * rows * in_words, dg, cur * rows, s));
                for (int i = 0; i < passes - 1; ++i)
                    PFHE_TRY(ntt_pass_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, dg, npolys, false, i, false, s));
            }
            PFHE_TRY(stamp());
            // ---- block pass (last pass of the transform) + multiply-accumulate ----
            if (fused) {
                PFHE_TRY(gadget_block_mulacc_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, p->k, rows * ell, dg,
                                                 keys + (keys_shared ? 0 : done * key_words), keys_shared,
                                                 result + done * (p->k + 1) * W, cur, accumulate, s, inv_tail));
            } else {
                PFHE_TRY(ntt_pass_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, dg, npolys, false, passes - 1, false, s));
                PFHE_TRY(gadget_mulacc_dev(t.primes_dev, t.L, t.log_n, p->k, rows, ell, dg,
                                           keys + (keys_shared ? 0 : done * key_words), keys_shared,
                                           result + done * (p->k + 1) * W, cur, accumulate, s));
            }
            PFHE_TRY(stamp());
        }
        return PFHE_OK;
    });
}

}  // namespace

// ---- RNSBase<W> / BigUintApproxSignedBasis<W> behind both word widths of the C ABI (W = uint64_t: pfhe_rns / pfhe_basis;
//      W = uint32_t: pfhe_rns32 / pfhe_basis32).  One implementation, instantiated twice. ----
namespace {

template <class W>
using DevWord = typename std::conditional<sizeof(W) == 8, u64, u32>::type;
template <class W>
size_t words_per_value(const RnsHost &h) { return sizeof(W) == 8 ? h.par.dev.value_len : h.par.dev.value_words; }
template <class W>
size_t words_per_value(const BasisHost &h) { return sizeof(W) == 8 ? h.par.dev.value_len : h.par.dev.value_words; }

// word j (of the caller's width) of a big integer held as 64-bit limbs
template <class W>
W word_of(const std::vector<u64> &limbs, size_t base, size_t j) {
    if (sizeof(W) == 8) return (W)limbs[base + j];
    return (W)(limbs[base + j / 2] >> (32 * (j & 1)));
}

template <class W>
int rns_create_impl(const W *moduli, size_t count, int device, RnsHost &h) {
    if (!moduli && count) return PFHE_ERR_BAD_ARGUMENT;
    std::vector<u64> m(moduli, moduli + count);
    PFHE_TRY(build_rns(m.data(), count, h, 8 * sizeof(W)));
    PFHE_TRY(capi_check_device(device));
    h.device = device;
    if (h.par.wide()) {  // more than kMaxLimbs moduli: the constants live in a device table
        DeviceGuard g(device);
        if (!g.ok) return PFHE_ERR_NO_DEVICE;
        PFHE_TRY(upload_rns_wide(h));
    }
    return PFHE_OK;
}

template <class W>
int rns_moduli_product_impl(const RnsHost *h, W *out, size_t len) {
    if (!h || !out) return PFHE_ERR_BAD_ARGUMENT;
    if (len != words_per_value<W>(*h)) return PFHE_ERR_BAD_LENGTH;
    for (size_t j = 0; j < len; ++j) out[j] = word_of<W>(h->Q, 0, j);
    return PFHE_OK;
}

inline int small_modulus_check(const RnsHost &h, u64 small_value_modulus) {
    for (u64 q : h.moduli) {
        if (small_value_modulus >= q || small_value_modulus < 2) {  // base.rs:288-292, :337-341
            set_last_error("small_value_modulus must be >= 2 and smaller than every RNS modulus");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    return PFHE_OK;
}

// The eight steps below are one template each for their host and device forms.  Each refuses in this
// order: a null handle; a null pointer, when the count is not zero; a bad level or value; a wrong length; what only this
// step asks; then PFHE_OK for an empty batch, and form_call refuses a device that cannot be made current.  Where the two
// forms have always differed, a line that names `form` keeps the difference.

template <class W>
int rns_compose(Form form, const RnsHost *h, const W *in, size_t len_in, W *out, size_t len_out, size_t value_count,
                void *stream) {
    if (!h || ((!in || !out) && value_count)) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in != value_count * h->par.dev.L || len_out != value_count * words_per_value<W>(*h)) {
        set_last_error("compose: multi_residues must hold moduli_count*value_count words and the output "
                       "value_count*big_uint_value_len words");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (value_count == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(in, len_in * sizeof(W)), stage_out(out, len_out * sizeof(W))};
    return form_call(h->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return rns_compose_dev(h->par, (const DevWord<W> *)d[0], (DevWord<W> *)d[1], value_count, s);
    });
}

template <class W>
int rns_wrapping(Form form, const RnsHost *h, const W *small, size_t value_count, W *multi, size_t len_out,
                 u64 small_value_modulus, void *stream) {
    if (!h || ((!small || !multi) && value_count)) return PFHE_ERR_BAD_ARGUMENT;
    if (len_out != value_count * h->par.dev.L) return PFHE_ERR_BAD_LENGTH;
    if (form == Form::kHost && value_count == 0) return PFHE_OK;  // the device form judges the modulus first
    PFHE_TRY(small_modulus_check(*h, small_value_modulus));
    if (value_count == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(small, value_count * sizeof(W)), stage_out(multi, len_out * sizeof(W))};
    return form_call(h->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return rns_wrapping_decompose_dev(h->par, (const DevWord<W> *)d[0], (DevWord<W> *)d[1], value_count,
                                          small_value_modulus, s);
    });
}

// `factors`: L ShoupFactor<W> (value, quotient) pairs.  64-bit pairs are used as given; for 32-bit ones the 64-bit
// quotient the kernels multiply by is derived from the value (the product is the same canonical residue)
template <class W>
int rns_add_scaled(Form form, const RnsHost *h, const W *small, size_t value_count, W *acc, size_t len_acc,
                   u64 small_value_modulus, bool centred, const W *factors, void *stream) {
    if (!h || !factors || ((!small || !acc) && value_count)) return PFHE_ERR_BAD_ARGUMENT;
    const u32 L = h->par.dev.L;
    if (len_acc != value_count * L) return PFHE_ERR_BAD_LENGTH;
    if (form == Form::kHost && value_count == 0) return PFHE_OK;  // the device form judges modulus and factors first
    if (centred) PFHE_TRY(small_modulus_check(*h, small_value_modulus));
    std::vector<u64> pairs(2 * (size_t)L);
    for (u32 i = 0; i < L; ++i) {
        if (factors[2 * i] >= h->moduli[i]) {
            set_last_error("factor values must be reduced modulo their modulus");
            return PFHE_ERR_BAD_ARGUMENT;
        }
        pairs[2 * i] = factors[2 * i];
        pairs[2 * i + 1] = sizeof(W) == 8 ? (u64)factors[2 * i + 1]
                                          : (u64)((((unsigned __int128)factors[2 * i]) << 64) / h->moduli[i]);
    }
    if (value_count == 0) return PFHE_OK;
    // base.rs:343,371-378: a small modulus of two takes the unsigned branch (a 1 stays +1)
    const bool lift = centred && small_value_modulus != 2;
    const StageBuf bufs[] = {stage_in(small, value_count * sizeof(W)), stage_inout(acc, len_acc * sizeof(W))};
    return form_call(h->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return rns_add_decompose_scaled_dev(h->par, (const DevWord<W> *)d[0], (DevWord<W> *)d[1], value_count,
                                            small_value_modulus, lift, pairs.data(), s);
    });
}

template <class W>
int rns_decompose_big(Form form, const RnsHost *h, const W *values, size_t len_in, W *multi, size_t len_out,
                      size_t value_count, void *stream) {
    if (!h || ((!values || !multi) && value_count)) return PFHE_ERR_BAD_ARGUMENT;
    if (len_in != value_count * words_per_value<W>(*h) || len_out != value_count * h->par.dev.L) return PFHE_ERR_BAD_LENGTH;
    if (value_count == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(values, len_in * sizeof(W)), stage_out(multi, len_out * sizeof(W))};
    return form_call(h->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return rns_decompose_big_dev(h->par, (const DevWord<W> *)d[0], (DevWord<W> *)d[1], value_count, s);
    });
}

/* ---- BigUintApproxSignedBasis<W> ---- */

inline int basis_create_impl(const RnsHost *rns, uint32_t log_basis, size_t reverse_length, BasisHost &b) {
    if (!rns) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(build_basis(*rns, log_basis, reverse_length, b));
    if (b.par.wide()) {
        DeviceGuard g(b.device);
        if (!g.ok) return PFHE_ERR_NO_DEVICE;
        PFHE_TRY(upload_basis_wide(b));
    }
    return PFHE_OK;
}

template <class W>
int basis_scalars_impl(const BasisHost *b, W *out, size_t len) {
    if (!b || !out) return PFHE_ERR_BAD_ARGUMENT;
    const size_t vw = words_per_value<W>(*b), vl = b->par.dev.value_len, ell = b->par.dev.ell;
    if (len != ell * vw) return PFHE_ERR_BAD_LENGTH;
    for (size_t j = 0; j < ell; ++j)
        for (size_t w = 0; w < vw; ++w) out[j * vw + w] = word_of<W>(b->scalars, j * vl, w);
    return PFHE_OK;
}

template <class W>
int basis_scalars_residue_impl(const BasisHost *b, W *out, size_t len) {
    if (!b || !out) return PFHE_ERR_BAD_ARGUMENT;
    if (len != b->scalars_residue.size()) return PFHE_ERR_BAD_LENGTH;
    for (size_t i = 0; i < len; ++i) out[i] = (W)b->scalars_residue[i];
    return PFHE_OK;
}

template <class W>
int basis_init(Form form, const BasisHost *b, W *values, size_t len, uint8_t *carries, size_t count, void *stream) {
    if (!b || ((!values || !carries) && count)) return PFHE_ERR_BAD_ARGUMENT;
    if (len != count * words_per_value<W>(*b)) return PFHE_ERR_BAD_LENGTH;  // basis.rs:332
    if (count == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_inout(values, len * sizeof(W)), stage_out(carries, count)};
    return form_call(b->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return basis_init_value_carry_dev(b->par, (DevWord<W> *)d[0], (unsigned char *)d[1], count, s);
    });
}

// a copy into `adjusted`, then the in-place step on it
template <class W>
int basis_init_to(Form form, const BasisHost *b, const W *values, size_t len, W *adjusted, uint8_t *carries, size_t count,
                  void *stream) {
    if (!b || ((!values || !adjusted || !carries) && count)) return PFHE_ERR_BAD_ARGUMENT;
    if (len != count * words_per_value<W>(*b)) return PFHE_ERR_BAD_LENGTH;  // basis.rs:378-379
    if (count == 0) return PFHE_OK;
    if (adjusted != values && form == Form::kHost) std::memcpy(adjusted, values, len * sizeof(W));
    if (adjusted != values && form == Form::kDevice) {
        DeviceGuard g(b->device);
        if (!g.ok) return PFHE_ERR_NO_DEVICE;
        PFHE_HIP(hipMemcpyAsync(adjusted, values, len * sizeof(W), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return basis_init<W>(form, b, adjusted, len, carries, count, stream);
}

template <class W>
int basis_unsigned(Form form, const BasisHost *b, size_t level, const W *values, size_t len, W *digits, uint8_t *carries,
                   size_t count, void *stream) {
    if (!b || ((!values || !digits || !carries) && count)) return PFHE_ERR_BAD_ARGUMENT;
    if (level >= b->par.dev.ell) return PFHE_ERR_BAD_ARGUMENT;
    if (len != count * words_per_value<W>(*b)) return PFHE_ERR_BAD_LENGTH;  // common.rs:316-317
    if (count == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(values, len * sizeof(W)), stage_out(digits, count * sizeof(W)),
                             stage_inout(carries, count)};
    return form_call(b->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return basis_unsigned_decompose_dev(b->par, (u32)level, (const DevWord<W> *)d[0], (DevWord<W> *)d[1],
                                            (unsigned char *)d[2], count, s);
    });
}

template <class W>
int basis_signed(Form form, const BasisHost *b, size_t level, const W *values, size_t len, W *decomposed, size_t len_out,
                 uint8_t *carries, size_t count, void *stream) {
    if (!b || ((!values || !decomposed || !carries) && count)) return PFHE_ERR_BAD_ARGUMENT;
    if (level >= b->par.dev.ell) return PFHE_ERR_BAD_ARGUMENT;
    if (len != count * words_per_value<W>(*b) || len_out != len) return PFHE_ERR_BAD_LENGTH;  // common.rs:296-297
    if (form == Form::kDevice && count && values == decomposed) {  // the host form stages into separate buffers
        set_last_error("decompose_slice_to needs distinct input and output buffers");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    if (count == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_in(values, len * sizeof(W)), stage_out(decomposed, len * sizeof(W)),
                             stage_inout(carries, count)};
    return form_call(b->device, form, bufs, (hipStream_t)stream, [&](void *const *d, hipStream_t s) {
        return basis_signed_decompose_dev(b->rns, b->par, (u32)level, (const DevWord<W> *)d[0], (DevWord<W> *)d[1],
                                          (unsigned char *)d[2], count, s);
    });
}

}  // namespace

// the entry points of one word width: NS = pfhe_rns / pfhe_rns32, BS = pfhe_basis / pfhe_basis32, W = the C word type
#define H(p) ((p) ? &(p)->h : nullptr)
#define PFHE_RNS_FAMILY(NS, BS, W)                                                                                      \
    int NS##_create(const W *moduli, size_t count, int device, NS **out) {                                              \
        PFHE_GUARD_BEGIN                                                                                                \
        if (!out) return PFHE_ERR_BAD_ARGUMENT;                                                                         \
        *out = nullptr;                                                                                                 \
        auto r = std::make_unique<NS>();                                                                                \
        PFHE_TRY(rns_create_impl<W>(moduli, count, device, r->h));                                                      \
        *out = r.release();                                                                                             \
        return PFHE_OK;                                                                                                 \
        PFHE_GUARD_END                                                                                                  \
    }                                                                                                                   \
    void NS##_destroy(NS *r) { delete r; }                                                                              \
    size_t NS##_moduli_count(const NS *r) { return r ? r->h.par.dev.L : 0; }                                            \
    size_t NS##_big_uint_value_len(const NS *r) { return r ? words_per_value<W>(r->h) : 0; }                            \
    int NS##_moduli_product(const NS *r, W *out, size_t len) { return rns_moduli_product_impl<W>(H(r), out, len); }     \
    PFHE_ENTRY(NS##_compose_multiple_values_to_dev, (const NS *r, const W *multi_residues_dev, size_t len_in,           \
                W *big_uint_values_dev, size_t len_out, size_t value_count, void *stream),                              \
               rns_compose<W>(Form::kDevice, H(r), multi_residues_dev, len_in, big_uint_values_dev, len_out,            \
                              value_count, stream))                                                                     \
    PFHE_ENTRY(NS##_compose_multiple_values_to, (const NS *r, const W *multi_residues, size_t len_in,                   \
                W *big_uint_values, size_t len_out, size_t value_count),                                                \
               rns_compose<W>(Form::kHost, H(r), multi_residues, len_in, big_uint_values, len_out, value_count,         \
                              nullptr))                                                                                 \
    PFHE_ENTRY(NS##_wrapping_decompose_small_values_to_dev, (const NS *r, const W *small_values_dev,                    \
                size_t value_count, W *multi_residues_dev, size_t len_out, W small_value_modulus, void *stream),        \
               rns_wrapping<W>(Form::kDevice, H(r), small_values_dev, value_count, multi_residues_dev, len_out,         \
                               small_value_modulus, stream))                                                            \
    PFHE_ENTRY(NS##_wrapping_decompose_small_values_to, (const NS *r, const W *small_values, size_t value_count,        \
                W *multi_residues, size_t len_out, W small_value_modulus),                                              \
               rns_wrapping<W>(Form::kHost, H(r), small_values, value_count, multi_residues, len_out,                   \
                               small_value_modulus, nullptr))                                                           \
    PFHE_ENTRY(NS##_add_wrapping_decompose_small_values_scaled_dev, (const NS *r, const W *small_values_dev,            \
                size_t value_count, W *acc_dev, size_t len_acc, W small_value_modulus, const W *factors,                \
                void *stream),                                                                                          \
               rns_add_scaled<W>(Form::kDevice, H(r), small_values_dev, value_count, acc_dev, len_acc,                  \
                                 small_value_modulus, true, factors, stream))                                           \
    PFHE_ENTRY(NS##_add_decompose_small_values_scaled_dev, (const NS *r, const W *small_values_dev,                     \
                size_t value_count, W *acc_dev, size_t len_acc, const W *factors, void *stream),                        \
               rns_add_scaled<W>(Form::kDevice, H(r), small_values_dev, value_count, acc_dev, len_acc, 0, false,        \
                                 factors, stream))                                                                      \
    PFHE_ENTRY(NS##_add_wrapping_decompose_small_values_scaled, (const NS *r, const W *small_values,                    \
                size_t value_count, W *acc, size_t len_acc, W small_value_modulus, const W *factors),                   \
               rns_add_scaled<W>(Form::kHost, H(r), small_values, value_count, acc, len_acc, small_value_modulus,       \
                                 true, factors, nullptr))                                                               \
    PFHE_ENTRY(NS##_add_decompose_small_values_scaled, (const NS *r, const W *small_values, size_t value_count,         \
                W *acc, size_t len_acc, const W *factors),                                                              \
               rns_add_scaled<W>(Form::kHost, H(r), small_values, value_count, acc, len_acc, 0, false, factors,         \
                                 nullptr))                                                                              \
    PFHE_ENTRY(NS##_decompose_big_uint_values_to_dev, (const NS *r, const W *big_uint_values_dev, size_t len_in,        \
                W *multi_residues_dev, size_t len_out, size_t value_count, void *stream),                               \
               rns_decompose_big<W>(Form::kDevice, H(r), big_uint_values_dev, len_in, multi_residues_dev, len_out,      \
                                    value_count, stream))                                                               \
    PFHE_ENTRY(NS##_decompose_big_uint_values_to, (const NS *r, const W *big_uint_values, size_t len_in,                \
                W *multi_residues, size_t len_out, size_t value_count),                                                 \
               rns_decompose_big<W>(Form::kHost, H(r), big_uint_values, len_in, multi_residues, len_out,                \
                                    value_count, nullptr))                                                              \
    int BS##_create(const NS *rns, uint32_t log_basis, size_t reverse_length, BS **out) {                               \
        PFHE_GUARD_BEGIN                                                                                                \
        if (!out || !rns) return PFHE_ERR_BAD_ARGUMENT;                                                                 \
        *out = nullptr;                                                                                                 \
        auto b = std::make_unique<BS>();                                                                                \
        PFHE_TRY(basis_create_impl(H(rns), log_basis, reverse_length, b->h));                                           \
        *out = b.release();                                                                                             \
        return PFHE_OK;                                                                                                 \
        PFHE_GUARD_END                                                                                                  \
    }                                                                                                                   \
    void BS##_destroy(BS *b) { delete b; }                                                                              \
    size_t BS##_decompose_length(const BS *b) { return b ? b->h.par.dev.ell : 0; }                                      \
    uint32_t BS##_log_basis(const BS *b) { return b ? b->h.par.dev.log_basis : 0; }                                     \
    uint32_t BS##_drop_bits(const BS *b) { return b ? b->h.par.dev.drop_bits : 0; }                                     \
    W BS##_basis_value(const BS *b) { return b ? (W)b->h.par.dev.basis : 0; }                                           \
    int BS##_scalars(const BS *b, W *out, size_t len) { return basis_scalars_impl<W>(H(b), out, len); }                 \
    int BS##_scalars_residue(const BS *b, W *out, size_t len) { return basis_scalars_residue_impl<W>(H(b), out, len); } \
    PFHE_ENTRY(BS##_init_value_carry_slice_inplace_dev, (const BS *b, W *values_dev, size_t len,                        \
                uint8_t *carries_dev, size_t count, void *stream),                                                      \
               basis_init<W>(Form::kDevice, H(b), values_dev, len, carries_dev, count, stream))                         \
    PFHE_ENTRY(BS##_init_value_carry_slice_inplace, (const BS *b, W *values, size_t len, uint8_t *carries,              \
                size_t count),                                                                                          \
               basis_init<W>(Form::kHost, H(b), values, len, carries, count, nullptr))                                  \
    PFHE_ENTRY(BS##_unsigned_decompose_slice_to_dev, (const BS *b, size_t level, const W *values_dev, size_t len,       \
                W *digits_dev, uint8_t *carries_dev, size_t count, void *stream),                                       \
               basis_unsigned<W>(Form::kDevice, H(b), level, values_dev, len, digits_dev, carries_dev, count,           \
                                 stream))                                                                               \
    PFHE_ENTRY(BS##_unsigned_decompose_slice_to, (const BS *b, size_t level, const W *values, size_t len, W *digits,    \
                uint8_t *carries, size_t count),                                                                        \
               basis_unsigned<W>(Form::kHost, H(b), level, values, len, digits, carries, count, nullptr))               \
    PFHE_ENTRY(BS##_init_value_carry_slice_to_dev, (const BS *b, const W *values_dev, size_t len, W *adjusted_dev,      \
                uint8_t *carries_dev, size_t count, void *stream),                                                      \
               basis_init_to<W>(Form::kDevice, H(b), values_dev, len, adjusted_dev, carries_dev, count, stream))        \
    PFHE_ENTRY(BS##_init_value_carry_slice_to, (const BS *b, const W *values, size_t len, W *adjusted,                  \
                uint8_t *carries, size_t count),                                                                        \
               basis_init_to<W>(Form::kHost, H(b), values, len, adjusted, carries, count, nullptr))                     \
    PFHE_ENTRY(BS##_decompose_slice_to_dev, (const BS *b, size_t level, const W *values_dev, size_t len,                \
                W *decomposed_dev, size_t len_out, uint8_t *carries_dev, size_t count, void *stream),                   \
               basis_signed<W>(Form::kDevice, H(b), level, values_dev, len, decomposed_dev, len_out, carries_dev,       \
                               count, stream))                                                                          \
    PFHE_ENTRY(BS##_decompose_slice_to, (const BS *b, size_t level, const W *values, size_t len, W *decomposed,         \
                size_t len_out, uint8_t *carries, size_t count),                                                        \
               basis_signed<W>(Form::kHost, H(b), level, values, len, decomposed, len_out, carries, count, nullptr))

extern "C" {

PFHE_RNS_FAMILY(pfhe_rns, pfhe_basis, uint64_t)
PFHE_RNS_FAMILY(pfhe_rns32, pfhe_basis32, uint32_t)
#undef PFHE_RNS_FAMILY
#undef H

}  // extern "C"

/* ------------------------------ external product ------------------------------ */

namespace {

// The <u32> product.  N = 2^16, k = 1 (the bench shape) takes the 64-bit plan's kernels on B32Arith: balanced int32
// digits, lift + strided pass, block pass + multiply-accumulate (+ inverse block pass) with the transformed digits on chip.
// Every other shape: steps (1)-(4) fused (gadget_decompose_kernel on u32 words), the table's forward transform over the
// lifted digit polynomials, one multiply-accumulate kernel.  Chunk after chunk on the caller's stream.
// *coeff_passes (when the caller wants coefficient form): 1 = the inverse transform's block pass ran inside the fused
// kernel (the caller runs the strided pass), 0 = none
int run_product(pfhe_extprod32_plan *p, const u32 *polys, u32 rows, const u32 *keys, bool keys_shared, u32 *result,
                u64 batch, bool accumulate, hipStream_t s, bool big_input, bool into_coeff = false,
                int *coeff_passes = nullptr) {
    return ordered_on(p->guard, s, [&]() -> int {
        if (coeff_passes) *coeff_passes = 0;
        const TableSet &t = *p->table;
        const u64 W = (u64)t.L * t.n;
        RnsParams rns = p->rns;
        rns.dev.big_input = rns.wide_tab.big_input = big_input ? 1u : 0u;
        const u64 in_words = big_input ? (u64)rns.dev.value_words * t.n : W;
        const u32 ell = p->basis.ell;
        const u64 key_words = (u64)rows * ell * (p->k + 1) * W;
        int *sdigits = (int *)p->sdigits;
        // the fused kernels launch one workgroup per (ciphertext, limb, block): they pay once that fills the chip
        const bool fused = sdigits != nullptr && p->use_fused && extprod32_fused_supported(t.log_n, p->k) &&
                           ((std::min<u64>(batch, p->chunk) * t.L) << (t.log_n - 12)) >= p->fused_min_wgs;
        const bool inv_tail = fused && into_coeff && !accumulate && coeff_passes != nullptr;
        if (inv_tail) *coeff_passes = 1;
        for (u64 done = 0; done < batch; done += p->chunk) {
            const u64 cur = std::min<u64>(p->chunk, batch - done);
            const u32 *kp = keys + (keys_shared ? 0 : done * key_words);
            u32 *rp = result + done * (p->k + 1) * W;
            if (fused) {
                PFHE_TRY(gadget_signed_digits_dev<u32>(rns, p->basis_par, t.log_n, polys + done * rows * in_words, sdigits, cur * rows, s));
                PFHE_TRY(digits_strided32_dev(t.primes_dev, t.L, t.log_n, ell, sdigits, p->digits, cur * rows, s));
                PFHE_TRY(gadget_block_mulacc32_dev(t.primes_dev, t.L, t.log_n, rows * ell, p->digits, kp, keys_shared, rp, cur,
                                                   accumulate, inv_tail, s));
                continue;
            }
            PFHE_TRY(gadget_decompose_dev<u32>(rns, p->basis_par, t.log_n, polys + done * rows * in_words, p->digits, cur * rows, s));
            PFHE_TRY(ntt32_transform_dev(t.primes_dev, t.L, t.log_n, p->digits, cur * rows * ell * t.L, false, false, s, t.tune));
            PFHE_TRY(gadget_mulacc32_dev(t.primes_dev, t.L, t.log_n, p->k, rows, ell, p->digits, kp, keys_shared, rp, cur, accumulate, s));
        }
        return PFHE_OK;
    });
}

// The rest of DcrtGlwe::into_coeff_form (macros/mod.rs:901-911) after a product that reported `coeff_passes`.
// u64: nothing ran -> the whole inverse; the block pass ran -> the remaining passes
int finish_coeff_form(const pfhe_extprod_plan *plan, u64 *result, u64 batch, int coeff_passes, hipStream_t s) {
    const TableSet &t = *plan->table;
    if (coeff_passes == 0)
        PFHE_TRY(ntt_inverse_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, result, batch * (plan->k + 1) * t.L, false, s, t.tune));
    for (int i = coeff_passes; i > 0 && i < ntt_num_passes(t.log_n, t.ntt_arith); ++i)
        PFHE_TRY(ntt_pass_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, result, batch * (plan->k + 1) * t.L, true, i, false, s));
    return PFHE_OK;
}
// u32: nothing ran -> the table's inverse; the block pass ran inside the fused kernel -> the strided pass finishes
int finish_coeff_form(const pfhe_extprod32_plan *plan, u32 *result, u64 batch, int coeff_passes, hipStream_t s) {
    const TableSet &t = *plan->table;
    if (coeff_passes == 0)
        PFHE_TRY(ntt32_transform_dev(t.primes_dev, t.L, t.log_n, result, batch * (plan->k + 1) * t.L, true, false, s, t.tune));
    if (coeff_passes == 1)
        PFHE_TRY(ntt_pass_dev(t.primes_dev, t.L, t.log_n - 1, kArithB32, reinterpret_cast<u64 *>(result),
                              batch * (plan->k + 1) * t.L, true, 1, false, s));
    return PFHE_OK;
}

// bytes per compact signed digit when one of the width's kernels wants them for this shape, else 0 (no buffer)
size_t sdigit_bytes_for(const pfhe_extprod_plan &p) {
    const TableSet &t = *p.table;
    return gadget_decompose_strided_supported(t.log_n, p.rns.dev.value_len) ||
                   extprod_small_supported(t.log_n, p.k, p.rns.dev.value_len, p.basis.log_basis)
               ? gadget_digit_bytes(p.basis.log_basis)
               : 0;
}
size_t sdigit_bytes_for(const pfhe_extprod32_plan &p) {
    return p.use_fused && extprod32_fused_supported(p.table->log_n, p.k) ? sizeof(int) : 0;
}

inline const TableSet *table_of(const pfhe_dcrt *t) { return capi_table_of(t); }
inline const TableSet *table_of(const pfhe_dcrt32 *t) { return capi_table32_of(t); }

template <class Plan, class Table, class Rns, class Basis>
int plan_create(const Table *table, const Rns *rns, const Basis *basis, size_t glwe_dimension, size_t chunk, Plan **out) {
    using W = typename Plan::Word;
    if (!out || !table || !rns || !basis || glwe_dimension == 0 || glwe_dimension > 64) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    const TableSet *t = table_of(table);
    if (t->L != rns->h.par.dev.L) {
        set_last_error("DCRT table and RNS base have different moduli counts");
        return PFHE_ERR_BAD_ARGUMENT;
    }
    for (u32 i = 0; i < t->L; ++i) {
        if (t->primes[i].q != rns->h.moduli[i]) {
            set_last_error("DCRT table and RNS base must use the same moduli in the same order");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    if (basis->h.rns.dev.L != rns->h.par.dev.L || basis->h.Q != rns->h.Q) return PFHE_ERR_BAD_ARGUMENT;  // basis.rs:52
    for (u32 i = 0; i < t->L; ++i) {
        if (basis->h.par.dev.basis >= t->primes[i].q) {  // wrapping_decompose needs B < q_i (base.rs:288-292)
            set_last_error("gadget basis must be smaller than every RNS modulus");
            return PFHE_ERR_BAD_ARGUMENT;
        }
    }
    auto p = std::make_unique<Plan>();
    p->table = t;
    p->rns = rns->h.par;
    p->basis_par = basis->h.par;
    p->basis = basis->h.par.dev;
    p->k = (u32)glwe_dimension;
    // default: about 2 GiB (u64) / 1 GiB (u32) of digit polynomials per buffer, at least 128 ciphertexts — measured at
    // N = 2^16, 3 limbs, u64, with today's kernels (ms per 1024 products): 32: 21.7, 64: 21.2, 128: 20.8, 256: 20.9,
    // 1024: 20.8 (round 1, slower kernels: 64 was the optimum); small rings need many more ciphertexts per launch to
    // amortise the launches
    if (chunk == 0) {
        const size_t per_ct = (size_t)(glwe_dimension + 1) * p->basis.ell * t->L * t->n * sizeof(W);
        const size_t budget = sizeof(W) == 8 ? (size_t)2 << 30 : (size_t)1 << 30;
        chunk = std::max<size_t>(128, std::min<size_t>(65536, budget / per_ct));
    }
    p->chunk = chunk;
    const size_t digits_words = p->chunk * (p->k + 1) * p->basis.ell * t->L * t->n;
    DeviceGuard g(t->device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    // read here, once, and kept in the plan (nothing on the launch path calls getenv)
    p->use_fused = std::getenv("PFHE_DISABLE_FUSED_EXTPROD") == nullptr;
    p->bufs.bind(t->device);
    PFHE_TRY(p->bufs.add(p->digits, digits_words));
    p->sdigit_bytes = sdigit_bytes_for(*p);
    PFHE_TRY(p->bufs.add(p->sdigits, p->chunk * (p->k + 1) * p->basis.ell * t->n * p->sdigit_bytes));
    PFHE_TRY(p->guard.init(t->device));
    *out = p.release();
    return PFHE_OK;
}

template <class Plan>
size_t plan_scratch_bytes(const Plan *p) {
    return p ? p->bufs.bytes() : 0;
}

template <class Plan, class W>
int mul_dcrt_ggsw_to_dev(Plan *plan, const W *crt_glwe_dev, size_t len_glwe, const W *dcrt_ggsw_dev, size_t len_ggsw,
                         W *result_dev, size_t len_result, int into_coeff_form, hipStream_t stream) {
    PFHE_TRY(plan_check(plan));
    PFHE_PLAN_LEASE(plan->guard, kPlanBusy);
    const TableSet &t = *plan->table;
    const size_t words = (size_t)t.L * t.n, glwe = (plan->k + 1) * words;
    const size_t ggsw = (size_t)(plan->k + 1) * plan->basis.ell * glwe;
    if (len_glwe % glwe != 0 || len_result != len_glwe || (len_ggsw != ggsw && len_ggsw != len_glwe / glwe * ggsw)) {
        set_last_error("external product: glwe/result must be batch*(k+1)*L*N words and the GGSW one or batch "
                       "ciphertexts of (k+1)*ell*(k+1)*L*N words");
        return PFHE_ERR_BAD_LENGTH;
    }
    const u64 batch = len_glwe / glwe;
    if (batch == 0) return PFHE_OK;
    if (!crt_glwe_dev || !dcrt_ggsw_dev || !result_dev) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(crt_glwe_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_ggsw_dev);
    PFHE_REQUIRE_ALIGNED(result_dev);
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    // result.set_zero() (glwe/crt.rs:217) is implied: the first accumulation overwrites
    int coeff_passes = 0;
    PFHE_TRY(run_product(plan, crt_glwe_dev, plan->k + 1, dcrt_ggsw_dev, len_ggsw == ggsw, result_dev, batch, false, stream,
                         false, into_coeff_form != 0, &coeff_passes));
    if (into_coeff_form) PFHE_TRY(finish_coeff_form(plan, result_dev, batch, coeff_passes, stream));
    return PFHE_OK;
}

template <class Plan, class W>
int mul_dcrt_ggsw_to(Plan *plan, const W *crt_glwe, size_t len_glwe, const W *dcrt_ggsw, size_t len_ggsw, W *result,
                     size_t len_result, int into_coeff_form) {
    PFHE_TRY(plan_check(plan));
    PFHE_PLAN_LEASE(plan->guard, kPlanBusy);
    if ((!crt_glwe || !dcrt_ggsw || !result) && len_glwe) return PFHE_ERR_BAD_ARGUMENT;
    const StageBuf bufs[] = {stage_in(crt_glwe, len_glwe * sizeof(W)), stage_in(dcrt_ggsw, len_ggsw * sizeof(W)),
                             stage_out(result, len_result * sizeof(W))};
    return staged_call(plan->table->device, bufs, [&](void *const *d, hipStream_t s) {
        return mul_dcrt_ggsw_to_dev(plan, (const W *)d[0], len_glwe, (const W *)d[1], len_ggsw, (W *)d[2], len_result,
                                    into_coeff_form, s);
    });
}

// The GLev rows against `batch` polynomials, accumulating or overwriting (`out_name`: what the length message calls the output).  CRT residues: DcrtGlwe::
// add_dcrt_glev_mul_crt_poly_assign (glwe/dcrt.rs:178-255); big integers modulo Q (`big_input`): DcrtGlwe::
// add_dcrt_glev_mul_big_uint_poly_assign (glwe/dcrt.rs:258-338) / DcrtGlev::mul_big_uint_poly_to (glev/dcrt.rs:113-175)
template <class Plan, class W>
int glev_common(Plan *plan, W *out_dev, size_t len_out, const W *dcrt_glev_dev, size_t len_glev, const W *poly_dev,
                size_t len_poly, bool accumulate, bool big_input, const char *out_name, void *stream) {
    PFHE_TRY(plan_check(plan));
    PFHE_PLAN_LEASE(plan->guard, kPlanBusy);
    const TableSet &t = *plan->table;
    const size_t words = (size_t)t.L * t.n, glwe = (plan->k + 1) * words, glev = plan->basis.ell * glwe;
    const size_t value_words = sizeof(W) == 8 ? plan->rns.dev.value_len : plan->rns.dev.value_words;
    const size_t in_words = big_input ? value_words * t.n : words;
    if (len_poly % in_words != 0) return PFHE_ERR_BAD_LENGTH;  // glwe/dcrt.rs:277
    const u64 batch = len_poly / in_words;
    if (len_out != batch * glwe || (len_glev != glev && len_glev != batch * glev)) {
        set_last_error(std::string("glev product: ") + out_name +
                       " must be batch*(k+1)*L*N words and the GLev one or batch of ell*(k+1)*L*N");
        return PFHE_ERR_BAD_LENGTH;
    }
    if (batch == 0) return PFHE_OK;
    if (!out_dev || !dcrt_glev_dev || !poly_dev) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(out_dev);
    PFHE_REQUIRE_ALIGNED(dcrt_glev_dev);
    PFHE_REQUIRE_ALIGNED(poly_dev);
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    return run_product(plan, poly_dev, 1, dcrt_glev_dev, len_glev == glev, out_dev, batch, accumulate, (hipStream_t)stream,
                       big_input);
}

}  // namespace

// The external product's entry points of one word width.  P: pfhe_extprod / pfhe_extprod32; TB, NS, BS: the width's table,
// RNS-base and basis handles; CW / W: the word as pfhe.h and as the library spell it.
// Kept on purpose: what the length message of a glev call names its output.  u64 says "acc" in the accumulating CRT call
// and "result" in the overwriting one, u32 "acc/result" in both; the two big-integer calls say "acc/result" at either width.
#define PFHE_EXTPROD_FAMILY(P, TB, NS, BS, CW, W)                                                                      \
    PFHE_ENTRY(P##_plan_create, (const TB *table, const NS *rns, const BS *basis, size_t glwe_dimension, size_t chunk, \
                P##_plan **out),                                                                                       \
               plan_create(table, rns, basis, glwe_dimension, chunk, out))                                             \
    PFHE_HANDLE_TRIO(P##_plan, P##_plan, plan_scratch_bytes(h))                                                        \
    PFHE_ENTRY(P##_mul_dcrt_ggsw_to_dev, (P##_plan *plan, const CW *crt_glwe_dev, size_t len_glwe,                     \
                const CW *dcrt_ggsw_dev, size_t len_ggsw, CW *result_dev, size_t len_result, int into_coeff_form,      \
                void *stream),                                                                                         \
               mul_dcrt_ggsw_to_dev(plan, (const W *)crt_glwe_dev, len_glwe, (const W *)dcrt_ggsw_dev, len_ggsw,       \
                                    (W *)result_dev, len_result, into_coeff_form, (hipStream_t)stream))                \
    PFHE_ENTRY(P##_mul_dcrt_ggsw_to, (P##_plan *plan, const CW *crt_glwe, size_t len_glwe, const CW *dcrt_ggsw,        \
                size_t len_ggsw, CW *result, size_t len_result, int into_coeff_form),                                  \
               mul_dcrt_ggsw_to(plan, (const W *)crt_glwe, len_glwe, (const W *)dcrt_ggsw, len_ggsw, (W *)result,      \
                                len_result, into_coeff_form))                                                          \
    PFHE_ENTRY(P##_add_dcrt_glev_mul_crt_poly_assign_dev, (P##_plan *plan, CW *acc_dev, size_t len_acc,                \
                const CW *dcrt_glev_dev, size_t len_glev, const CW *crt_poly_dev, size_t len_poly, void *stream),      \
               glev_common(plan, (W *)acc_dev, len_acc, (const W *)dcrt_glev_dev, len_glev, (const W *)crt_poly_dev,   \
                           len_poly, true, false, sizeof(W) == 8 ? "acc" : "acc/result", stream))                      \
    PFHE_ENTRY(P##_glev_mul_crt_poly_to_dev, (P##_plan *plan, const CW *dcrt_glev_dev, size_t len_glev,                \
                const CW *crt_poly_dev, size_t len_poly, CW *result_dev, size_t len_result, void *stream),             \
               glev_common(plan, (W *)result_dev, len_result, (const W *)dcrt_glev_dev, len_glev,                      \
                           (const W *)crt_poly_dev, len_poly, false, false, sizeof(W) == 8 ? "result" : "acc/result",  \
                           stream))                                                                                    \
    PFHE_ENTRY(P##_add_dcrt_glev_mul_big_uint_poly_assign_dev, (P##_plan *plan, CW *acc_dev, size_t len_acc,           \
                const CW *dcrt_glev_dev, size_t len_glev, const CW *big_uint_poly_dev, size_t len_poly, void *stream), \
               glev_common(plan, (W *)acc_dev, len_acc, (const W *)dcrt_glev_dev, len_glev,                            \
                           (const W *)big_uint_poly_dev, len_poly, true, true, "acc/result", stream))                  \
    PFHE_ENTRY(P##_glev_mul_big_uint_poly_to_dev, (P##_plan *plan, const CW *dcrt_glev_dev, size_t len_glev,           \
                const CW *big_uint_poly_dev, size_t len_poly, CW *result_dev, size_t len_result, void *stream),        \
               glev_common(plan, (W *)result_dev, len_result, (const W *)dcrt_glev_dev, len_glev,                      \
                           (const W *)big_uint_poly_dev, len_poly, false, true, "acc/result", stream))

extern "C" {

PFHE_EXTPROD_FAMILY(pfhe_extprod, pfhe_dcrt, pfhe_rns, pfhe_basis, uint64_t, u64)
PFHE_EXTPROD_FAMILY(pfhe_extprod32, pfhe_dcrt32, pfhe_rns32, pfhe_basis32, uint32_t, u32)
#undef PFHE_EXTPROD_FAMILY

/* ------------------------------ what only the u64 plan has ------------------------------ */

// test aid: hold != 0 takes the plan for the calling thread as an entry point would (PFHE_ERR_BUSY if another thread has
// it) and keeps it until the same thread calls with hold == 0
int pfhe_extprod_plan_debug_hold(pfhe_extprod_plan *p, int hold) {
    if (plan_check(p) != PFHE_OK) return PFHE_ERR_BAD_ARGUMENT;
    if (hold) return p->guard.acquire() ? PFHE_OK : PFHE_ERR_BUSY;
    if (!p->guard.held_by_caller()) return PFHE_ERR_BAD_ARGUMENT;
    p->guard.release();
    return PFHE_OK;
}
int pfhe_extprod_profile_dev(pfhe_extprod_plan *plan, const uint64_t *crt_glwe_dev, size_t len_glwe,
                             const uint64_t *dcrt_ggsw_dev, size_t len_ggsw, uint64_t *result_dev, size_t len_result,
                             double *ms_out, size_t *launches_out, void *stream) {
    PFHE_GUARD_BEGIN
    PFHE_TRY(plan_check(plan));
    PFHE_PLAN_LEASE(plan->guard, kPlanBusy);
    if (!ms_out || !launches_out) return PFHE_ERR_BAD_ARGUMENT;
    std::vector<hipEvent_t> ev;
    plan->prof = &ev;
    // coefficient-form output, as bench.py times it: the second group includes the inverse block pass fused into the
    // multiply-accumulate kernel; the final strided inverse pass runs after the last stamp
    int rc = pfhe_extprod_mul_dcrt_ggsw_to_dev(plan, crt_glwe_dev, len_glwe, dcrt_ggsw_dev, len_ggsw, result_dev,
                                               len_result, 1, stream);
    plan->prof = nullptr;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    ms_out[0] = ms_out[1] = 0.0;
    *launches_out = ev.size() / 3;
    for (size_t i = 0; rc == PFHE_OK && e == hipSuccess && i + 2 < ev.size(); i += 3) {
        float a = 0, b = 0;
        e = hipEventElapsedTime(&a, ev[i], ev[i + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]);
        ms_out[0] += a;  // digit extraction + lifting strided pass
        ms_out[1] += b;  // block pass of the transform + multiply-accumulate
    }
    for (hipEvent_t x : ev) (void)hipEventDestroy(x);
    if (e != hipSuccess) return hip_fail(e, "external-product profile", __FILE__, __LINE__);
    return rc;
    PFHE_GUARD_END
}

}  // extern "C"

/* ------------------------------ batched blind rotation ------------------------------ */

// The blind-rotation (CMUX) loop of a bootstrap over the external product: for every step i and ciphertext e,
//   ACC_e <- ACC_e + coeff_form(((X^{exps[e*n_steps+i]} - 1) * ACC_e) (x) BSK_i)
// (CrtGlwe::mul_monic_monomial_assign, glwe/crt.rs:76-114; sub_element_wise_assign, macros/mod.rs:438;
// CrtGlwe::mul_dcrt_ggsw_to, glwe/crt.rs:200-227; DcrtGlwe::write_coeff_form, macros/mod.rs:921;
// add_element_wise_assign, macros/mod.rs:410).  The handle owns an external-product plan and three glue buffers of
// chunk ciphertexts (D, E and the second accumulator of the ping-pong), all allocated at creation; a call allocates
// nothing and synchronises with nothing, so one whole rotation can be captured into a HIP graph.
template <class Plan, class W>
struct BlindRotCore {
    PlanGuard guard;             // one holder at a time and cross-stream ordering of successive calls, as the plan
    std::unique_ptr<Plan> plan;  // owned
    W *d = nullptr, *e = nullptr, *ping = nullptr;  // chunk * glwe words each
    size_t glwe = 0, ggsw = 0;
    DeviceBuffers bufs;  // after the plan: the glue buffers are freed first, then the plan, then the guard's event
};
struct pfhe_blindrot : BlindRotCore<pfhe_extprod_plan, u64> {};
struct pfhe_blindrot32 : BlindRotCore<pfhe_extprod32_plan, u32> {};

namespace {

template <class H, class Table, class Rns, class Basis>
int blindrot_create(const Table *table, const Rns *base, const Basis *basis, size_t glwe_dimension, size_t chunk, H **out) {
    if (!out) return PFHE_ERR_BAD_ARGUMENT;
    *out = nullptr;
    auto h = std::make_unique<H>();
    decltype(h->plan.get()) plan = nullptr;
    PFHE_TRY(plan_create(table, base, basis, glwe_dimension, chunk, &plan));
    h->plan.reset(plan);
    const TableSet &t = *h->plan->table;
    h->glwe = (size_t)(h->plan->k + 1) * t.L * t.n;
    h->ggsw = (size_t)(h->plan->k + 1) * h->plan->basis.ell * h->glwe;
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    h->bufs.bind(t.device);
    for (auto **b : {&h->d, &h->e, &h->ping}) PFHE_TRY(h->bufs.add(*b, h->plan->chunk * h->glwe));
    PFHE_TRY(h->guard.init(t.device));
    *out = h.release();
    return PFHE_OK;
}
template <class H>
size_t blindrot_scratch_bytes(const H *h) {
    if (!h || !h->plan) return 0;
    return h->plan->bufs.bytes() + h->bufs.bytes();
}

// Fused small-ring step (u64 only): taken under exactly the condition run_product takes extprod_small_kernel under.
// Two launches per step, no D or E buffer: digits of X^r * ACC - ACC, then the product whose epilogue adds E to ACC.
bool blindrot_small_fused(const pfhe_blindrot *h, u64 cur) {
    const pfhe_extprod_plan *p = h->plan.get();
    const TableSet &t = *p->table;
    return p->sdigits != nullptr && extprod_small_supported(t.log_n, p->k, p->rns.dev.value_len, p->basis.log_basis) &&
           cur * t.L >= 1024 && p->use_fused;
}
bool blindrot_small_fused(const pfhe_blindrot32 *, u64) { return false; }
int blindrot_small_steps(pfhe_blindrot *h, u64 *acc, const u64 *bsk, const u32 *exps, u64 n_steps, u64 cur, hipStream_t s) {
    const pfhe_extprod_plan *p = h->plan.get();
    const TableSet &t = *p->table;
    RnsParams rns = p->rns;
    rns.dev.big_input = rns.wide_tab.big_input = 0u;
    for (u64 i = 0; i < n_steps; ++i) {
        PFHE_TRY(blindrot_small_digits_dev(rns, p->basis_par, t.log_n, acc, (int *)p->sdigits, cur, exps + i, (u32)n_steps, s));
        PFHE_TRY(blindrot_small_product_dev(t.primes_dev, t.L, t.log_n, t.ntt_arith, p->basis.ell, (const int *)p->sdigits,
                                            bsk + i * h->ggsw, acc, cur, s));
    }
    return PFHE_OK;
}
int blindrot_small_steps(pfhe_blindrot32 *, u32 *, const u32 *, const u32 *, u64, u64, hipStream_t) {
    return PFHE_ERR_UNSUPPORTED;
}

// the rotation's length test, for both of its forms
template <class H>
int blindrot_lengths(const H *h, size_t len_acc, size_t len_bsk, size_t len_exps) {
    const bool whole = len_acc % h->glwe == 0 && len_bsk % h->ggsw == 0;
    if (whole && len_exps == (len_acc / h->glwe) * (len_bsk / h->ggsw)) return PFHE_OK;
    set_last_error("blind rotation: acc must be batch*(k+1)*L*N words, bsk n_steps*(k+1)*ell*(k+1)*L*N and exps "
                   "batch*n_steps exponents");
    return PFHE_ERR_BAD_LENGTH;
}

template <class H, class W>
int blindrot_rotate_dev(H *h, W *acc, size_t len_acc, const W *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps,
                        hipStream_t s) {
    if (!h || !h->plan) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kPlanBusy);
    const TableSet &t = *h->plan->table;
    PFHE_TRY(blindrot_lengths(h, len_acc, len_bsk, len_exps));
    const u64 batch = len_acc / h->glwe, n_steps = len_bsk / h->ggsw;
    if (batch == 0 || n_steps == 0) return PFHE_OK;
    if (!acc || !bsk || !exps) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_REQUIRE_ALIGNED(acc);
    PFHE_REQUIRE_ALIGNED(bsk);
    DeviceGuard g(t.device);
    if (!g.ok) return PFHE_ERR_NO_DEVICE;
    const u32 rows = h->plan->k + 1;
    return ordered_on(h->guard, s, [&]() -> int {
        int rc = PFHE_OK;
        // chunk after chunk; every step of a chunk runs before the next chunk starts
        for (u64 done = 0; done < batch && rc == PFHE_OK; done += h->plan->chunk) {
            const u64 cur = std::min<u64>(h->plan->chunk, batch - done);
            W *a0 = acc + done * h->glwe;
            const uint32_t *ex = exps + done * n_steps;
            if (blindrot_small_fused(h, cur)) {
                rc = blindrot_small_steps(h, a0, bsk, ex, n_steps, cur, s);
                continue;
            }
            // ping-pong between the caller's accumulator and the handle's: every step writes ACC' to the other one, so the
            // gather of a rotated word never sees a word already updated; an odd step count starts in the handle's buffer
            // so that the last step ends in the caller's
            W *src = a0;
            if (n_steps % 2) {
                rc = blindrot_glue_dev<W>(t, BlindRotGlue::kFirstCopy, a0, nullptr, h->ping, h->d, ex, (u32)n_steps, rows, cur, s);
                src = h->ping;
            } else {
                rc = blindrot_glue_dev<W>(t, BlindRotGlue::kFirst, a0, nullptr, nullptr, h->d, ex, (u32)n_steps, rows, cur, s);
            }
            for (u64 i = 0; i < n_steps && rc == PFHE_OK; ++i) {
                // the product of one step: E = coeff_form(D (x) BSK_i) for `cur` ciphertexts
                rc = mul_dcrt_ggsw_to_dev(h->plan.get(), h->d, cur * h->glwe, bsk + i * h->ggsw, h->ggsw, h->e, cur * h->glwe, 1, s);
                if (rc != PFHE_OK) break;
                W *dst = src == a0 ? h->ping : a0;
                rc = i + 1 < n_steps
                         ? blindrot_glue_dev<W>(t, BlindRotGlue::kStep, src, h->e, dst, h->d, ex + i + 1, (u32)n_steps, rows, cur, s)
                         : blindrot_glue_dev<W>(t, BlindRotGlue::kLast, src, h->e, dst, nullptr, ex, (u32)n_steps, rows, cur, s);
                src = dst;
            }
        }
        return rc;
    });
}

// host form: every exponent must be below 2N (the reference's debug_assert!(r < 2N)); staged through the pooled context
template <class H, class W>
int blindrot_rotate_host(H *h, W *acc, size_t len_acc, const W *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
    if (!h || !h->plan) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_PLAN_LEASE(h->guard, kPlanBusy);
    if ((!acc && len_acc) || (!bsk && len_bsk) || (!exps && len_exps)) return PFHE_ERR_BAD_ARGUMENT;
    PFHE_TRY(require_exps_below_2n(exps, len_exps, h->plan->table->n, "blind rotation: every exponent must be below 2N"));
    PFHE_TRY(blindrot_lengths(h, len_acc, len_bsk, len_exps));
    if (len_acc == 0 || len_bsk == 0) return PFHE_OK;
    const StageBuf bufs[] = {stage_inout(acc, len_acc * sizeof(W)), stage_in(bsk, len_bsk * sizeof(W)),
                             stage_in(exps, len_exps * sizeof(uint32_t))};
    return staged_call(h->plan->table->device, bufs, [&](void *const *d, hipStream_t s) {
        return blindrot_rotate_dev<H, W>(h, (W *)d[0], len_acc, (const W *)d[1], len_bsk, (const uint32_t *)d[2], len_exps,
                                         s);
    });
}

}  // namespace

// The rotation's entry points of one word width.  P: pfhe_blindrot / pfhe_blindrot32, also the handle type; the rest as
// PFHE_EXTPROD_FAMILY.
#define PFHE_BLINDROT_FAMILY(P, TB, NS, BS, CW, W)                                                                  \
    PFHE_ENTRY(P##_create, (const TB *table, const NS *base, const BS *basis, size_t glwe_dimension, size_t chunk,  \
                P **out),                                                                                           \
               blindrot_create(table, base, basis, glwe_dimension, chunk, out))                                     \
    PFHE_HANDLE_TRIO(P, P, blindrot_scratch_bytes(h))                                                               \
    PFHE_ENTRY(P##_rotate_dev, (P *h, CW *acc_dev, size_t len_acc, const CW *bsk_dev, size_t len_bsk,               \
                const uint32_t *exps_dev, size_t len_exps, void *stream),                                           \
               blindrot_rotate_dev<P, W>(h, (W *)acc_dev, len_acc, (const W *)bsk_dev, len_bsk, exps_dev, len_exps, \
                                         (hipStream_t)stream))                                                      \
    PFHE_ENTRY(P##_rotate, (P *h, CW *acc, size_t len_acc, const CW *bsk, size_t len_bsk, const uint32_t *exps,     \
                size_t len_exps),                                                                                   \
               blindrot_rotate_host(h, (W *)acc, len_acc, (const W *)bsk, len_bsk, exps, len_exps))

extern "C" {

PFHE_BLINDROT_FAMILY(pfhe_blindrot, pfhe_dcrt, pfhe_rns, pfhe_basis, uint64_t, u64)
PFHE_BLINDROT_FAMILY(pfhe_blindrot32, pfhe_dcrt32, pfhe_rns32, pfhe_basis32, uint32_t, u32)
#undef PFHE_BLINDROT_FAMILY

}  // extern "C"
