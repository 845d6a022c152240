// pfhe.hpp — header-only C++17 mirror of the reference's operator interface over the C ABI
// (include/pfhe.h).  Same type names, method names and argument meaning as the Rust traits:
//   U64NttTable   — primus_ntt::NttTable for U64NttTable   (crates/primus_ntt/src/ntt/mod.rs:16-113)
//   U64DcrtTable  — primus_ntt::DcrtTable for U64DcrtTable (crates/primus_ntt/src/dcrt/mod.rs:19-135)
//   U32NttTable, U32DcrtTable — the u32 / low-q tables (ntt/prime32/table.rs, dcrt/prime32.rs)
//   RNSBase, BaseConverter, BigUintApproxSignedBasis, DcrtGlevContext, mul_dcrt_ggsw_to
//                 — primus_rns / primus_decompose / primus_lattice entry points of the RNS
//                   gadget external product (crates/primus_lattice/src/glwe/crt.rs:200-227)
//   FullComplex64FftTable, TfheFftContext, external_product_to and the Tfhe* handles — the torus side
// The two word widths: every operator after the four tables is written once, over the word type W.  A class is a template
// NameT<W> with the two public names as aliases, Name = NameT<uint64_t> and Name32 = NameT<uint32_t> (u32 words in memory:
// residues, digits, limbs, torus words); a free function is a template whose first word pointer (or whose context) selects
// W, so the same name serves uint64_t and uint32_t buffers.  detail::Fns<W> names the C functions of each width
// (pfhe_x_ / pfhe_x32_).
// Errors: constructors throw pfhe::Error carrying the pfhe_status (the reference returns
// Result<_, NttError>); in-place transforms throw on length mismatch where the reference
// debug_asserts.  Slices are (pointer, length-in-words) pairs, in place, like `&mut [u64]`.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pfhe.h"

namespace pfhe {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string &what) : std::runtime_error(what), status_(status) {}
    int status() const noexcept { return status_; }

  private:
    int status_;
};

inline void check(int status) {
    if (status != PFHE_OK) {
        std::string msg = pfhe_status_string(status);
        const char *detail = pfhe_last_error();
        if (detail && *detail) msg += std::string(": ") + detail;
        throw Error(status, msg);
    }
}

namespace detail {

// W again, where a word pointer must not take part in deducing W: only the first word pointer of a free function does, so
// a literal nullptr or a non-const pointer converts as it would for a plain function.
template <class W>
struct same_type {
    using type = W;
};
template <class W>
using same = typename same_type<W>::type;

// The one owner of a C handle H: destroys it with the handle's destroy function, move only.  handle() gives P, `const H *`
// for the immutable handles.
template <class H, void (*Destroy)(H *), class P = const H *>
class Owner {
  public:
    ~Owner() {
        if (h_) Destroy(h_);
    }
    Owner(Owner &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &) = delete;
    P handle() const { return h_; }

  protected:
    Owner() = default;
    H *h_ = nullptr;
};

// ... of a handle with one holder at a time, like the `&mut` it mirrors: a call from a second thread while one is inside
// throws (PFHE_ERR_BUSY); in_use() tells whether some thread is inside a call on it.
template <class H, void (*Destroy)(H *), int (*InUse)(const H *)>
class Busy : public Owner<H, Destroy, H *> {
  public:
    bool in_use() const { return InUse(this->h_) != 0; }
};

// ... that also reports the device scratch it owns
template <class H, void (*Destroy)(H *), int (*InUse)(const H *), size_t (*ScratchBytes)(const H *)>
class Plan : public Busy<H, Destroy, InUse> {
  public:
    size_t scratch_bytes() const { return ScratchBytes(this->h_); }
};

// The C functions of one table handle, by name: PRE is the symbol prefix of the handle type H over the word type W.
#define PFHE_TABLE_TRAITS(NAME, PRE, H, W)                                                   \
    struct NAME {                                                                            \
        using Handle = H;                                                                    \
        using Word = W;                                                                      \
        static constexpr auto destroy = PRE##destroy;                                        \
        static constexpr auto poly_length = PRE##poly_length;                                \
        static constexpr auto transform_slice = PRE##transform_slice;                        \
        static constexpr auto inverse_transform_slice = PRE##inverse_transform_slice;        \
        static constexpr auto lazy_transform_slice = PRE##lazy_transform_slice;              \
        static constexpr auto lazy_inverse_transform_slice = PRE##lazy_inverse_transform_slice; \
        static constexpr auto transform_monomial = PRE##transform_monomial;                  \
        static constexpr auto transform_coeff_one_monomial = PRE##transform_coeff_one_monomial; \
        static constexpr auto transform_coeff_minus_one_monomial = PRE##transform_coeff_minus_one_monomial; \
        static constexpr auto transform_dev = PRE##transform_dev;                            \
        static constexpr auto inverse_transform_dev = PRE##inverse_transform_dev;            \
        static constexpr auto mul_assign_dev = PRE##mul_assign_dev;                          \
        static constexpr auto add_mul_assign_dev = PRE##add_mul_assign_dev;                  \
    }
PFHE_TABLE_TRAITS(NttFns, pfhe_ntt_, pfhe_ntt, uint64_t);
PFHE_TABLE_TRAITS(DcrtFns, pfhe_dcrt_, pfhe_dcrt, uint64_t);
PFHE_TABLE_TRAITS(Ntt32Fns, pfhe_ntt32_, pfhe_ntt32, uint32_t);
PFHE_TABLE_TRAITS(Dcrt32Fns, pfhe_dcrt32_, pfhe_dcrt32, uint32_t);
#undef PFHE_TABLE_TRAITS

// What the four tables share: the host slices, the monomial shortcuts and the device-resident forms.  F names the C functions.
template <class F>
class Table : public Owner<typename F::Handle, F::destroy> {
  public:
    using H = typename F::Handle;
    using W = typename F::Word;

    size_t poly_length() const { return F::poly_length(h_); }
    void transform_slice(W *poly, size_t len) const { check(F::transform_slice(h_, poly, len)); }
    void inverse_transform_slice(W *v, size_t len) const { check(F::inverse_transform_slice(h_, v, len)); }
    void lazy_transform_slice(W *poly, size_t len) const { check(F::lazy_transform_slice(h_, poly, len)); }
    void lazy_inverse_transform_slice(W *v, size_t len) const { check(F::lazy_inverse_transform_slice(h_, v, len)); }
    void transform_monomial(W coeff, size_t degree, W *values, size_t len) const {
        check(F::transform_monomial(h_, coeff, degree, values, len));
    }
    void transform_coeff_one_monomial(size_t degree, W *values, size_t len) const {
        check(F::transform_coeff_one_monomial(h_, degree, values, len));
    }
    void transform_coeff_minus_one_monomial(size_t degree, W *values, size_t len) const {
        check(F::transform_coeff_minus_one_monomial(h_, degree, values, len));
    }
    // device-resident batches (asynchronous on `stream`)
    void transform_dev(W *poly_dev, size_t len, bool lazy = false, void *stream = nullptr) const {
        check(F::transform_dev(h_, poly_dev, len, lazy, stream));
    }
    void inverse_transform_dev(W *v_dev, size_t len, bool lazy = false, void *stream = nullptr) const {
        check(F::inverse_transform_dev(h_, v_dev, len, lazy, stream));
    }
    // NttPolynomial / DcrtPolynomial::mul_assign, add_mul_assign (crates/primus_poly/src/dcrt/mul.rs:176, mod.rs:105)
    void mul_assign_dev(W *a, size_t len_a, const W *b, size_t len_b, void *stream = nullptr) const {
        check(F::mul_assign_dev(h_, a, len_a, b, len_b, stream));
    }
    void add_mul_assign_dev(W *acc, const W *a, size_t len_a, const W *b, size_t len_b, void *stream = nullptr) const {
        check(F::add_mul_assign_dev(h_, acc, a, len_a, b, len_b, stream));
    }

  protected:
    Table() = default;
    using Owner<H, F::destroy>::h_;
};

}  // namespace detail

class U64NttTable : public detail::Table<detail::NttFns> {
  public:
    U64NttTable(uint32_t log_n, uint64_t modulus, int device = 0) { check(pfhe_ntt_create(log_n, modulus, device, &h_)); }
    size_t n() const { return poly_length(); }
    uint32_t log_n() const { return pfhe_ntt_log_n(h_); }
    uint64_t modulus() const { return pfhe_ntt_modulus(h_); }
    uint64_t root() const { return pfhe_ntt_root(h_); }
    uint64_t inv_root() const { return pfhe_ntt_inv_root(h_); }
    uint64_t inv_n() const { return pfhe_ntt_inv_n(h_); }
};

class U64DcrtTable : public detail::Table<detail::DcrtFns> {
  public:
    U64DcrtTable(uint32_t log_n, const std::vector<uint64_t> &moduli, int device = 0) {
        check(pfhe_dcrt_create(log_n, moduli.data(), moduli.size(), device, &h_));
    }
    size_t moduli_count() const { return pfhe_dcrt_moduli_count(h_); }
    size_t crt_poly_length() const { return pfhe_dcrt_crt_poly_length(h_); }
    uint64_t modulus(size_t i) const { return pfhe_dcrt_modulus(h_, i); }

    // device-pointer form (launches on `stream` only: capturable); minus_one selects -X^degree
    void transform_monomial_dev(uint64_t coeff, size_t degree, uint64_t *values_dev, size_t len, bool minus_one = false,
                                void *stream = nullptr) const {
        check(pfhe_dcrt_transform_monomial_dev(h_, coeff, degree, values_dev, len, minus_one ? 1 : 0, stream));
    }
    // CrtRlwe::mul_dcrt_polynomial_to + into_coeff_form (crates/primus_lattice/src/rlwe/crt.rs:42-65)
    void mul_dcrt_polynomial_dev(uint64_t *crt_poly, size_t len, const uint64_t *dcrt_poly, size_t len_b,
                                 void *stream = nullptr) const {
        check(pfhe_dcrt_mul_dcrt_polynomial_dev(h_, crt_poly, len, dcrt_poly, len_b, stream));
    }
    // CrtPolynomial / DcrtPolynomial / CrtGlwe element-wise family (crates/primus_poly/src/crt/{add,sub,neg,mul}.rs,
    // dcrt/inv.rs; primus_lattice/src/macros/mod.rs:367-531, glwe/crt.rs:59-175).  `out` may alias `a`.
    void add_to_dev(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t len, void *stream = nullptr) const {
        check(pfhe_dcrt_add_to_dev(h_, a, b, out, len, stream));
    }
    void sub_to_dev(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t len, void *stream = nullptr) const {
        check(pfhe_dcrt_sub_to_dev(h_, a, b, out, len, stream));
    }
    void neg_to_dev(const uint64_t *a, uint64_t *out, size_t len, void *stream = nullptr) const {
        check(pfhe_dcrt_neg_to_dev(h_, a, out, len, stream));
    }
    void mul_scalar_to_dev(const uint64_t *a, const std::vector<uint64_t> &scalars, uint64_t *out, size_t len,
                           void *stream = nullptr) const {
        require_count(scalars.size(), moduli_count());
        check(pfhe_dcrt_mul_scalar_to_dev(h_, a, scalars.data(), out, len, stream));
    }
    void add_mul_scalar_assign_dev(uint64_t *acc, const uint64_t *rhs, const std::vector<uint64_t> &scalars, size_t len,
                                   void *stream = nullptr) const {
        require_count(scalars.size(), moduli_count());
        check(pfhe_dcrt_add_mul_scalar_assign_dev(h_, acc, rhs, scalars.data(), len, stream));
    }
    // factors: (value, quotient) per modulus, ShoupFactor (crates/primus_factor/src/shoup_factor/mod.rs:22)
    void mul_factor_to_dev(const uint64_t *a, const std::vector<uint64_t> &factors, uint64_t *out, size_t len,
                           void *stream = nullptr) const {
        require_count(factors.size(), 2 * moduli_count());
        check(pfhe_dcrt_mul_factor_to_dev(h_, a, factors.data(), out, len, stream));
    }
    void add_mul_factor_assign_dev(uint64_t *acc, const uint64_t *rhs, const std::vector<uint64_t> &factors, size_t len,
                                   void *stream = nullptr) const {
        require_count(factors.size(), 2 * moduli_count());
        check(pfhe_dcrt_add_mul_factor_assign_dev(h_, acc, rhs, factors.data(), len, stream));
    }
    void mul_monomial_to_dev(const uint64_t *a, size_t r, uint64_t *out, size_t len, void *stream = nullptr) const {
        check(pfhe_dcrt_mul_monomial_to_dev(h_, a, r, out, len, stream));
    }
    void mul_monomial_assign_dev(uint64_t *data, size_t r, size_t len, void *stream = nullptr) const {
        check(pfhe_dcrt_mul_monomial_assign_dev(h_, data, r, len, stream));
    }
    // throws Error(PFHE_ERR_NO_INVERSE) where the reference panics
    void inv_to_dev(const uint64_t *a, uint64_t *out, size_t len, void *stream = nullptr) const {
        check(pfhe_dcrt_inv_to_dev(h_, a, out, len, stream));
    }

  private:
    static void require_count(size_t got, size_t want) {
        if (got != want) throw Error(PFHE_ERR_BAD_LENGTH, "expected one entry per modulus");
    }
};

// primus_ntt::U32NttTable (crates/primus_ntt/src/ntt/prime32/table.rs:37) — q < 2^30, u32 data
class U32NttTable : public detail::Table<detail::Ntt32Fns> {
  public:
    U32NttTable(uint32_t log_n, uint32_t modulus, int device = 0) { check(pfhe_ntt32_create(log_n, modulus, device, &h_)); }
    size_t n() const { return poly_length(); }
    uint32_t log_n() const { return pfhe_ntt32_log_n(h_); }
    uint32_t modulus() const { return pfhe_ntt32_modulus(h_); }
    uint32_t root() const { return pfhe_ntt32_root(h_); }
    uint32_t inv_root() const { return pfhe_ntt32_inv_root(h_); }
    uint32_t inv_n() const { return pfhe_ntt32_inv_n(h_); }
};

// primus_ntt::U32DcrtTable (crates/primus_ntt/src/dcrt/prime32.rs:11)
class U32DcrtTable : public detail::Table<detail::Dcrt32Fns> {
  public:
    U32DcrtTable(uint32_t log_n, const std::vector<uint32_t> &moduli, int device = 0) {
        check(pfhe_dcrt32_create(log_n, moduli.data(), moduli.size(), device, &h_));
    }
    size_t moduli_count() const { return pfhe_dcrt32_moduli_count(h_); }
    size_t crt_poly_length() const { return pfhe_dcrt32_crt_poly_length(h_); }
    uint32_t modulus(size_t i) const { return pfhe_dcrt32_modulus(h_, i); }
};

namespace detail {

// The C functions and handle owners of everything after the tables, by name, for the word type W: Fns<uint64_t> names
// pfhe_rns_*, pfhe_tfhe_*, ..., Fns<uint32_t> names pfhe_rns32_*, pfhe_tfhe32_*, ....  S is the width's infix (empty or 32)
// and TABLE the DCRT table over W.  An entry is FAMILY_NAME for pfhe_FAMILY{,32}_NAME.
template <class W>
struct Fns;
#define PFHE_FN(FAM, S, NAME) static constexpr auto FAM##_##NAME = pfhe_##FAM##S##_##NAME
#define PFHE_TFHE_PLAN(S, TYPE, STEM)                                                                          \
    Plan<pfhe_tfhe##S##_##TYPE, pfhe_tfhe##S##_##STEM##_destroy, pfhe_tfhe##S##_##STEM##_in_use, \
         pfhe_tfhe##S##_##STEM##_scratch_bytes>
#define PFHE_WORD_TRAITS(W, S, TABLE)                                                                          \
    template <>                                                                                                \
    struct Fns<W> {                                                                                            \
        using DcrtTable = TABLE;                                                                               \
        using Rns = Owner<pfhe_rns##S, pfhe_rns##S##_destroy>;                                                 \
        using Conv = Owner<pfhe_conv##S, pfhe_conv##S##_destroy>;                                              \
        using Basis = Owner<pfhe_basis##S, pfhe_basis##S##_destroy>;                                           \
        using ExtprodBusy = Busy<pfhe_extprod##S##_plan, pfhe_extprod##S##_plan_destroy, pfhe_extprod##S##_plan_in_use>; \
        using ExtprodPlan = Plan<pfhe_extprod##S##_plan, pfhe_extprod##S##_plan_destroy, pfhe_extprod##S##_plan_in_use, \
                                 pfhe_extprod##S##_plan_scratch_bytes>;                                        \
        using Blindrot = Plan<pfhe_blindrot##S, pfhe_blindrot##S##_destroy, pfhe_blindrot##S##_in_use,         \
                              pfhe_blindrot##S##_scratch_bytes>;                                               \
        using TfhePlan = PFHE_TFHE_PLAN(S, plan, plan);                                                        \
        using TfheBlindrot = PFHE_TFHE_PLAN(S, blindrot, blindrot);                                            \
        using TfheMbrot = PFHE_TFHE_PLAN(S, mbrot, mbrot);                                                     \
        using TfheBootstrap = PFHE_TFHE_PLAN(S, bootstrap_handle, bootstrap);                                  \
        using TfhePackfftPlan = PFHE_TFHE_PLAN(S, packfft_plan, packfft_plan);                                 \
        using TfheCbs = PFHE_TFHE_PLAN(S, cbs_handle, cbs);                                                    \
        using TfheCmuxTree = PFHE_TFHE_PLAN(S, cmux_tree_handle, cmux_tree);                                   \
        using TfheGlweTrace = PFHE_TFHE_PLAN(S, glwe_trace_handle, glwe_trace);                                \
        using TfheRingPack = Plan<pfhe_ringpack##S, pfhe_ringpack##S##_destroy, pfhe_ringpack##S##_in_use,     \
                                  pfhe_ringpack##S##_scratch_bytes>;                                   \
        using TfheLut = PFHE_TFHE_PLAN(S, lut_handle, lut);                                                    \
        using TfheBitext = Plan<pfhe_bitext##S, pfhe_bitext##S##_destroy, pfhe_bitext##S##_in_use,             \
                                pfhe_bitext##S##_scratch_bytes>;                                       \
        PFHE_FN(rns, S, create);                                                                               \
        PFHE_FN(rns, S, moduli_count);                                                                         \
        PFHE_FN(rns, S, big_uint_value_len);                                                                   \
        PFHE_FN(rns, S, moduli_product);                                                                       \
        PFHE_FN(rns, S, compose_multiple_values_to);                                                           \
        PFHE_FN(rns, S, wrapping_decompose_small_values_to);                                                   \
        PFHE_FN(rns, S, add_wrapping_decompose_small_values_scaled);                                           \
        PFHE_FN(rns, S, add_decompose_small_values_scaled);                                                    \
        PFHE_FN(rns, S, decompose_big_uint_values_to);                                                         \
        PFHE_FN(conv, S, create);                                                                              \
        PFHE_FN(conv, S, input_moduli_count);                                                                  \
        PFHE_FN(conv, S, output_moduli_count);                                                                 \
        PFHE_FN(conv, S, fast_convert_array);                                                                  \
        PFHE_FN(conv, S, exact_convert_array);                                                                 \
        PFHE_FN(conv, S, fast_convert_array_dev);                                                              \
        PFHE_FN(conv, S, exact_convert_array_dev);                                                             \
        PFHE_FN(basis, S, create);                                                                             \
        PFHE_FN(basis, S, decompose_length);                                                                   \
        PFHE_FN(basis, S, log_basis);                                                                          \
        PFHE_FN(basis, S, drop_bits);                                                                          \
        PFHE_FN(basis, S, basis_value);                                                                        \
        PFHE_FN(basis, S, init_value_carry_slice_inplace);                                                     \
        PFHE_FN(basis, S, unsigned_decompose_slice_to);                                                        \
        PFHE_FN(basis, S, decompose_slice_to);                                                                 \
        PFHE_FN(extprod, S, plan_create);                                                                      \
        PFHE_FN(extprod, S, mul_dcrt_ggsw_to);                                                                 \
        PFHE_FN(extprod, S, mul_dcrt_ggsw_to_dev);                                                             \
        PFHE_FN(blindrot, S, create);                                                                          \
        PFHE_FN(blindrot, S, rotate);                                                                          \
        PFHE_FN(blindrot, S, rotate_dev);                                                                      \
        static constexpr auto fft_forward_torus_slice = pfhe_fft_forward_torus##S##_slice;                     \
        static constexpr auto fft_inverse_torus_slice = pfhe_fft_inverse_torus##S##_slice;                     \
        static constexpr auto fft_forward_torus_dev = pfhe_fft_forward_torus##S##_dev;                         \
        static constexpr auto fft_inverse_torus_dev = pfhe_fft_inverse_torus##S##_dev;                         \
        PFHE_FN(tfhe, S, plan_create);                                                                         \
        PFHE_FN(tfhe, S, external_product_to);                                                                 \
        PFHE_FN(tfhe, S, external_product_to_dev);                                                             \
        PFHE_FN(tfhe, S, blindrot_create);                                                                     \
        PFHE_FN(tfhe, S, blindrot_rotate);                                                                     \
        PFHE_FN(tfhe, S, blindrot_rotate_dev);                                                                 \
        PFHE_FN(tfhe, S, mbrot_create);                                                                        \
        PFHE_FN(tfhe, S, mbrot_rotate);                                                                        \
        PFHE_FN(tfhe, S, mbrot_rotate_dev);                                                                    \
        PFHE_FN(tfhe, S, mul_monomial_each_to_dev);                                                            \
        PFHE_FN(tfhe, S, modswitch_dev);                                                                       \
        PFHE_FN(tfhe, S, modswitch_stride_dev);                                                                \
        PFHE_FN(tfhe, S, sample_extract);                                                                      \
        PFHE_FN(tfhe, S, sample_extract_dev);                                                                  \
        PFHE_FN(tfhe, S, keyswitch);                                                                           \
        PFHE_FN(tfhe, S, keyswitch_dev);                                                                       \
        PFHE_FN(tfhe, S, bootstrap_create);                                                                    \
        PFHE_FN(tfhe, S, bootstrap_create_multibit);                                                           \
        PFHE_FN(tfhe, S, bootstrap_create_many_lut);                                                           \
        PFHE_FN(tfhe, S, bootstrap);                                                                           \
        PFHE_FN(tfhe, S, bootstrap_dev);                                                                       \
        PFHE_FN(tfhe, S, lwe_body_mac);                                                                        \
        PFHE_FN(tfhe, S, lwe_body_mac_dev);                                                                    \
        PFHE_FN(tfhe, S, glwe_body_mac);                                                                       \
        PFHE_FN(tfhe, S, glwe_body_mac_dev);                                                                   \
        PFHE_FN(tfhe, S, ggsw_add_gadget_dev);                                                                 \
        PFHE_FN(tfhe, S, bsk_generate_dev);                                                                    \
        PFHE_FN(tfhe, S, ksk_generate_dev);                                                                    \
        PFHE_FN(tfhe, S, pack_keyswitch);                                                                      \
        PFHE_FN(tfhe, S, pack_keyswitch_dev);                                                                  \
        PFHE_FN(tfhe, S, pksk_generate_dev);                                                                   \
        PFHE_FN(tfhe, S, sample_extract_first_few);                                                            \
        PFHE_FN(tfhe, S, sample_extract_first_few_dev);                                                        \
        PFHE_FN(tfhe, S, multimsg_extract);                                                                    \
        PFHE_FN(tfhe, S, multimsg_extract_dev);                                                                \
        PFHE_FN(tfhe, S, packfft_plan_create);                                                                 \
        PFHE_FN(tfhe, S, packfft_key_dev);                                                                     \
        PFHE_FN(tfhe, S, pack_keyswitch_fft);                                                                  \
        PFHE_FN(tfhe, S, pack_keyswitch_fft_dev);                                                              \
        PFHE_FN(tfhe, S, private_keyswitch);                                                                   \
        PFHE_FN(tfhe, S, private_keyswitch_dev);                                                               \
        PFHE_FN(tfhe, S, pfksk_generate_dev);                                                                  \
        PFHE_FN(tfhe, S, cbs_create);                                                                          \
        PFHE_FN(tfhe, S, cbs_create_with);                                                                     \
        PFHE_FN(tfhe, S, cbs);                                                                                 \
        PFHE_FN(tfhe, S, cbs_dev);                                                                             \
        PFHE_FN(tfhe, S, cmux_tree_create);                                                                    \
        PFHE_FN(tfhe, S, cmux);                                                                                \
        PFHE_FN(tfhe, S, cmux_dev);                                                                            \
        PFHE_FN(tfhe, S, cmux_tree);                                                                           \
        PFHE_FN(tfhe, S, cmux_tree_dev);                                                                       \
        PFHE_FN(tfhe, S, glwe_trace_create);                                                                   \
        PFHE_FN(tfhe, S, glwe_automorphism);                                                                   \
        PFHE_FN(tfhe, S, glwe_automorphism_dev);                                                               \
        PFHE_FN(tfhe, S, glwe_trace);                                                                          \
        PFHE_FN(tfhe, S, glwe_trace_dev);                                                                      \
        PFHE_FN(ringpack, S, create);                                                                  \
        PFHE_FN(ringpack, S, merge);                                                                   \
        PFHE_FN(ringpack, S, merge_dev);                                                               \
        PFHE_FN(ringpack, S, pack);                                                                    \
        PFHE_FN(ringpack, S, pack_dev);                                                                \
        PFHE_FN(tfhe, S, lut_create);                                                                          \
        PFHE_FN(tfhe, S, rotate_by_bits);                                                                      \
        PFHE_FN(tfhe, S, rotate_by_bits_dev);                                                                  \
        PFHE_FN(tfhe, S, lut_eval);                                                                            \
        PFHE_FN(tfhe, S, lut_eval_dev);                                                                        \
        PFHE_FN(bitext, S, create);                                                                            \
        PFHE_FN(bitext, S, extract_bits);                                                                      \
        PFHE_FN(bitext, S, extract_bits_dev);                                                                  \
        PFHE_FN(lwe, S, linear);                                                                               \
        PFHE_FN(lwe, S, linear_dev);                                                                           \
        PFHE_FN(lwe, S, linear_i8);                                                                            \
        PFHE_FN(lwe, S, linear_i8_dev);                                                                        \
        PFHE_FN(rand, S, uniform_dev);                                                                         \
        PFHE_FN(rand, S, binary_dev);                                                                          \
        PFHE_FN(rand, S, ternary_dev);                                                                         \
        PFHE_FN(rand, S, tuniform_dev);                                                                        \
        PFHE_FN(rand, S, fill_rows_dev);                                                                       \
        PFHE_FN(rand, S, lwe_encrypt_seeded);                                                                  \
        PFHE_FN(rand, S, lwe_encrypt_seeded_dev);                                                              \
        PFHE_FN(rand, S, seeded_expand);                                                                       \
        PFHE_FN(rand, S, seeded_expand_dev);                                                                   \
    }
PFHE_WORD_TRAITS(uint64_t, , U64DcrtTable);
PFHE_WORD_TRAITS(uint32_t, 32, U32DcrtTable);
#undef PFHE_WORD_TRAITS
#undef PFHE_TFHE_PLAN
#undef PFHE_FN

inline void require_factors(size_t got, size_t moduli_count) {
    if (got != 2 * moduli_count) throw Error(PFHE_ERR_BAD_LENGTH, "expected one factor per modulus");
}

}  // namespace detail

// RNSBase<W> (crates/primus_rns/src/base.rs).  The <u32> instantiation is the type the reference's tests/big_uint.rs:13
// runs: moduli below 2^30, up to 32 of them.
template <class W>
class RNSBaseT : public detail::Fns<W>::Rns {
    using F = detail::Fns<W>;

  public:
    explicit RNSBaseT(const std::vector<W> &moduli, int device = 0) {
        check(F::rns_create(moduli.data(), moduli.size(), device, &this->h_));
    }
    size_t moduli_count() const { return F::rns_moduli_count(this->h_); }
    size_t big_uint_value_len() const { return F::rns_big_uint_value_len(this->h_); }
    std::vector<W> moduli_product() const {
        std::vector<W> q(big_uint_value_len());
        check(F::rns_moduli_product(this->h_, q.data(), q.size()));
        return q;
    }
    void compose_multiple_values_to(const W *multi_residues, size_t len_in, W *big_uint_values, size_t len_out,
                                    size_t value_count) const {
        check(F::rns_compose_multiple_values_to(this->h_, multi_residues, len_in, big_uint_values, len_out, value_count));
    }
    void wrapping_decompose_small_values_to(const W *small_values, size_t value_count, W *multi_residues, size_t len_out,
                                            W small_value_modulus) const {
        check(F::rns_wrapping_decompose_small_values_to(this->h_, small_values, value_count, multi_residues, len_out,
                                                        small_value_modulus));
    }
    // RNSBase::add_wrapping_decompose_small_values_scaled / add_decompose_small_values_scaled
    // (crates/primus_rns/src/base.rs:326-416); factors = (value, quotient) per modulus
    void add_wrapping_decompose_small_values_scaled(const W *small_values, size_t value_count, W *acc, size_t len_acc,
                                                    W small_value_modulus, const std::vector<W> &factors) const {
        detail::require_factors(factors.size(), moduli_count());
        check(F::rns_add_wrapping_decompose_small_values_scaled(this->h_, small_values, value_count, acc, len_acc,
                                                                small_value_modulus, factors.data()));
    }
    void add_decompose_small_values_scaled(const W *small_values, size_t value_count, W *acc, size_t len_acc,
                                           const std::vector<W> &factors) const {
        detail::require_factors(factors.size(), moduli_count());
        check(F::rns_add_decompose_small_values_scaled(this->h_, small_values, value_count, acc, len_acc, factors.data()));
    }
    // RNSBase::decompose_big_uint_values_to (crates/primus_rns/src/base.rs:457-481)
    void decompose_big_uint_values_to(const W *big_uint_values, size_t len_in, W *multi_residues, size_t len_out,
                                      size_t value_count) const {
        check(F::rns_decompose_big_uint_values_to(this->h_, big_uint_values, len_in, multi_residues, len_out, value_count));
    }
};
using RNSBase = RNSBaseT<uint64_t>;
using RNSBase32 = RNSBaseT<uint32_t>;

// primus_rns::BaseConverter (crates/primus_rns/src/converter.rs:21, generic over T: FheUint): modulus-major arrays; the
// reference's `scratch` argument has no counterpart
template <class W>
class BaseConverterT : public detail::Fns<W>::Conv {
    using F = detail::Fns<W>;

  public:
    BaseConverterT(const RNSBaseT<W> &input_base, const RNSBaseT<W> &output_base) {
        check(F::conv_create(input_base.handle(), output_base.handle(), &this->h_));
    }
    size_t input_moduli_count() const { return F::conv_input_moduli_count(this->h_); }
    size_t output_moduli_count() const { return F::conv_output_moduli_count(this->h_); }
    void fast_convert_array(const W *crt_poly_in, size_t len_in, W *crt_poly_out, size_t len_out, size_t poly_length) const {
        check(F::conv_fast_convert_array(this->h_, crt_poly_in, len_in, crt_poly_out, len_out, poly_length));
    }
    void exact_convert_array(const W *crt_poly_in, size_t len_in, W *crt_poly_out, size_t len_out, size_t poly_length) const {
        check(F::conv_exact_convert_array(this->h_, crt_poly_in, len_in, crt_poly_out, len_out, poly_length));
    }
    void fast_convert_array_dev(const W *in_dev, size_t len_in, W *out_dev, size_t len_out, size_t poly_length,
                                void *stream = nullptr) const {
        check(F::conv_fast_convert_array_dev(this->h_, in_dev, len_in, out_dev, len_out, poly_length, stream));
    }
    void exact_convert_array_dev(const W *in_dev, size_t len_in, W *out_dev, size_t len_out, size_t poly_length,
                                 void *stream = nullptr) const {
        check(F::conv_exact_convert_array_dev(this->h_, in_dev, len_in, out_dev, len_out, poly_length, stream));
    }
};
using BaseConverter = BaseConverterT<uint64_t>;
using BaseConverter32 = BaseConverterT<uint32_t>;

// BigUintApproxSignedBasis<W> (primus_decompose, big_integer/common.rs); over u32 log_basis is below 32
template <class W>
class BigUintApproxSignedBasisT : public detail::Fns<W>::Basis {
    using F = detail::Fns<W>;

  public:
    BigUintApproxSignedBasisT(const RNSBaseT<W> &base, uint32_t log_basis, size_t reverse_length = 0) {
        check(F::basis_create(base.handle(), log_basis, reverse_length, &this->h_));
    }
    size_t decompose_length() const { return F::basis_decompose_length(this->h_); }
    uint32_t log_basis() const { return F::basis_log_basis(this->h_); }
    uint32_t drop_bits() const { return F::basis_drop_bits(this->h_); }
    W basis_value() const { return F::basis_basis_value(this->h_); }
    void init_value_carry_slice_inplace(W *values, size_t len, uint8_t *carries, size_t count) const {
        check(F::basis_init_value_carry_slice_inplace(this->h_, values, len, carries, count));
    }
    void unsigned_decompose_slice_to(size_t level, const W *values, size_t len, W *digits, uint8_t *carries,
                                     size_t count) const {
        check(F::basis_unsigned_decompose_slice_to(this->h_, level, values, len, digits, carries, count));
    }
    // decomposer_iter().nth(level).decompose_slice_to (big_integer/common.rs:289-306): signed digit as a residue mod Q
    void decompose_slice_to(size_t level, const W *values, size_t len, W *decomposed_values, size_t len_out,
                            uint8_t *carries, size_t count) const {
        check(F::basis_decompose_slice_to(this->h_, level, values, len, decomposed_values, len_out, carries, count));
    }
};
using BigUintApproxSignedBasis = BigUintApproxSignedBasisT<uint64_t>;
using BigUintApproxSignedBasis32 = BigUintApproxSignedBasisT<uint32_t>;

// DcrtGlevContext (crates/primus_lattice/src/context/glev.rs:4-68) + the handles the reference
// passes next to it.  One holder at a time, like the `&mut` it mirrors: a call from a second thread while one is inside throws
// (PFHE_ERR_BUSY, "plan in use"); successive calls on different streams are ordered by the library.
// scratch_bytes() is DcrtGlevContext32's alone, as it has been: the u64 context never mirrored pfhe_extprod_plan_scratch_bytes.
template <class W>
class DcrtGlevContextT : public std::conditional_t<std::is_same<W, uint64_t>::value, typename detail::Fns<W>::ExtprodBusy,
                                                   typename detail::Fns<W>::ExtprodPlan> {
    using F = detail::Fns<W>;

  public:
    DcrtGlevContextT(const typename F::DcrtTable &table, const RNSBaseT<W> &base, const BigUintApproxSignedBasisT<W> &basis,
                     size_t glwe_dimension = 1, size_t chunk = 0) {
        check(F::extprod_plan_create(table.handle(), base.handle(), basis.handle(), glwe_dimension, chunk, &this->h_));
    }
};
using DcrtGlevContext = DcrtGlevContextT<uint64_t>;
using DcrtGlevContext32 = DcrtGlevContextT<uint32_t>;

// CrtGlwe::mul_dcrt_ggsw_to (crates/primus_lattice/src/glwe/crt.rs:200-227), host slices
template <class W>
void mul_dcrt_ggsw_to(const detail::same<W> *crt_glwe, size_t len_glwe, const detail::same<W> *dcrt_ggsw, size_t len_ggsw,
                      detail::same<W> *result, size_t len_result, DcrtGlevContextT<W> &context,
                      bool into_coeff_form = false) {
    check(detail::Fns<W>::extprod_mul_dcrt_ggsw_to(context.handle(), crt_glwe, len_glwe, dcrt_ggsw, len_ggsw, result,
                                                   len_result, into_coeff_form));
}

// device-resident batches
template <class W>
void mul_dcrt_ggsw_to_dev(const detail::same<W> *crt_glwe_dev, size_t len_glwe, const detail::same<W> *dcrt_ggsw_dev,
                          size_t len_ggsw, detail::same<W> *result_dev, size_t len_result, DcrtGlevContextT<W> &context,
                          bool into_coeff_form = false, void *stream = nullptr) {
    check(detail::Fns<W>::extprod_mul_dcrt_ggsw_to_dev(context.handle(), crt_glwe_dev, len_glwe, dcrt_ggsw_dev, len_ggsw,
                                                       result_dev, len_result, into_coeff_form, stream));
}

// The batched blind rotation over the external product (pfhe_blindrot_*): for every step i and ciphertext e,
// ACC_e += coeff_form(((X^{exps[e*n_steps+i]} - 1) * ACC_e) (x) BSK_i)  — CrtGlwe::mul_monic_monomial_assign
// (glwe/crt.rs:76-114), sub_element_wise_assign, CrtGlwe::mul_dcrt_ggsw_to (glwe/crt.rs:200-227), write_coeff_form,
// add_element_wise_assign.  Owns its product plan and glue buffers; one holder at a time, like DcrtGlevContext.
template <class W>
class BlindRotateT : public detail::Fns<W>::Blindrot {
    using F = detail::Fns<W>;

  public:
    BlindRotateT(const typename F::DcrtTable &table, const RNSBaseT<W> &base, const BigUintApproxSignedBasisT<W> &basis,
                 size_t glwe_dimension = 1, size_t chunk = 0) {
        check(F::blindrot_create(table.handle(), base.handle(), basis.handle(), glwe_dimension, chunk, &this->h_));
    }
    // host slices; every exponent below 2N
    void rotate(W *acc, size_t len_acc, const W *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(F::blindrot_rotate(this->h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(W *acc_dev, size_t len_acc, const W *bsk_dev, size_t len_bsk, const uint32_t *exps_dev, size_t len_exps,
                    void *stream = nullptr) {
        check(F::blindrot_rotate_dev(this->h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }
};
using BlindRotate = BlindRotateT<uint64_t>;
using BlindRotate32 = BlindRotateT<uint32_t>;

// FullComplex64FftTable — primus_fft::FftTable (crates/primus_fft/src/table.rs, complex64/table.rs:47-130): Fourier
// values as interleaved (re, im) doubles, N complex values per polynomial; lengths count complex values / torus words.
// One table serves both tori: W is the torus word, uint64_t or uint32_t.
class FullComplex64FftTable : public detail::Owner<pfhe_fft, pfhe_fft_destroy, pfhe_fft *> {
  public:
    explicit FullComplex64FftTable(uint32_t log_n, int device = 0) { check(pfhe_fft_create(log_n, device, &h_)); }
    size_t poly_length() const { return pfhe_fft_poly_length(h_); }
    size_t fourier_length() const { return pfhe_fft_fourier_length(h_); }
    template <class W>
    void forward_torus_slice(const W *in, size_t len_in, double *out, size_t len_out) const {
        check(detail::Fns<W>::fft_forward_torus_slice(h_, in, len_in, out, len_out));
    }
    template <class W>
    void inverse_torus_slice(const double *in, size_t len_in, W *out, size_t len_out) const {
        check(detail::Fns<W>::fft_inverse_torus_slice(h_, in, len_in, out, len_out));
    }
    template <class W>
    void forward_torus_dev(const W *in, size_t len_in, double *out, size_t len_out, void *stream = nullptr) const {
        check(detail::Fns<W>::fft_forward_torus_dev(h_, in, len_in, out, len_out, stream));
    }
    template <class W>
    void inverse_torus_dev(const double *in, size_t len_in, W *out, size_t len_out, void *stream = nullptr) const {
        check(detail::Fns<W>::fft_inverse_torus_dev(h_, in, len_in, out, len_out, stream));
    }
};

// TfheFftContext<W> with its power-of-two ApproxSignedBasis<W> (primus_lattice/src/context/tfhe.rs,
// primus_decompose/src/primitive/basis.rs:47-177); decompose_length 0 = the full BITS / log_basis.  One holder at a time.
template <class W>
class TfheFftContextT : public detail::Fns<W>::TfhePlan {
    using F = detail::Fns<W>;

  public:
    TfheFftContextT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length = 0,
                    size_t chunk = 0) {
        check(F::tfhe_plan_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &this->h_));
    }
};
using TfheFftContext = TfheFftContextT<uint64_t>;
using TfheFftContext32 = TfheFftContextT<uint32_t>;

// external_product_to (crates/primus_lattice/src/tfhe/external_product.rs:36-93): a batch of GLWE ciphertexts, one
// Fourier GGSW key (len_key complex values)
template <class W>
void external_product_to(const detail::same<W> *input, size_t len_input, const double *key, size_t len_key,
                         detail::same<W> *output, size_t len_output, TfheFftContextT<W> &context) {
    check(detail::Fns<W>::tfhe_external_product_to(context.handle(), input, len_input, key, len_key, output, len_output));
}
template <class W>
void external_product_to_dev(const detail::same<W> *input_dev, size_t len_input, const double *key_dev, size_t len_key,
                             detail::same<W> *output_dev, size_t len_output, TfheFftContextT<W> &context,
                             void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_external_product_to_dev(context.handle(), input_dev, len_input, key_dev, len_key, output_dev,
                                                       len_output, stream));
}

// The batched blind rotation over the TFHE product (pfhe_tfhe_blindrot_*): for every step i and ciphertext e,
// ACC_e += external_product_to(X^{exps[e*n_steps+i]} * ACC_e - ACC_e, BSK_i) on torus words (the rotation of
// CrtGlwe::mul_monic_monomial_assign, glwe/crt.rs:76-114; external_product_to, tfhe/external_product.rs:36-93).  Takes
// TfheFftContext's arguments, owns its product plan and glue buffers; one holder at a time.
template <class W>
class TfheBlindRotateT : public detail::Fns<W>::TfheBlindrot {
    using F = detail::Fns<W>;

  public:
    TfheBlindRotateT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length = 0,
                     size_t chunk = 0) {
        check(F::tfhe_blindrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &this->h_));
    }
    // host slices; every exponent below 2N
    void rotate(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(F::tfhe_blindrot_rotate(this->h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(W *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(F::tfhe_blindrot_rotate_dev(this->h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }
};
using TfheBlindRotate = TfheBlindRotateT<uint64_t>;
using TfheBlindRotate32 = TfheBlindRotateT<uint32_t>;

// The multi-bit blind rotation (pfhe_tfhe_mbrot_*): the mask is consumed grouping_factor (1..4) elements at a time; for every
// group t and ciphertext e, ACC_e = external_product_to(ACC_e, sum_j X^{r_j} * BSK[t][j]) with r_j the subset sum of the
// group's exponents at the set bits of j.  Binary LWE keys; bsk is groups x 2^g Fourier GGSW keys.  Owns the scratch of its
// form; one holder at a time.
template <class W>
class TfheMultiBitBlindRotateT : public detail::Fns<W>::TfheMbrot {
    using F = detail::Fns<W>;

  public:
    TfheMultiBitBlindRotateT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                             size_t decompose_length, size_t grouping_factor, size_t chunk = 0) {
        check(F::tfhe_mbrot_create(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor, chunk,
                                   &this->h_));
    }
    // host slices; every exponent below 2N
    void rotate(W *acc, size_t len_acc, const double *bsk, size_t len_bsk, const uint32_t *exps, size_t len_exps) {
        check(F::tfhe_mbrot_rotate(this->h_, acc, len_acc, bsk, len_bsk, exps, len_exps));
    }
    // device buffers, queued on `stream` (exponents taken modulo 2N)
    void rotate_dev(W *acc_dev, size_t len_acc, const double *bsk_dev, size_t len_bsk, const uint32_t *exps_dev,
                    size_t len_exps, void *stream = nullptr) {
        check(F::tfhe_mbrot_rotate_dev(this->h_, acc_dev, len_acc, bsk_dev, len_bsk, exps_dev, len_exps, stream));
    }
};
using TfheMultiBitBlindRotate = TfheMultiBitBlindRotateT<uint64_t>;
using TfheMultiBitBlindRotate32 = TfheMultiBitBlindRotateT<uint32_t>;

// the combined key of one ciphertext and one group as a key in the reference's layout (pfhe_tfhe_mb_combine_key_dev)
inline void tfhe_multibit_combine_key_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, size_t decompose_length,
                                          size_t grouping_factor, const double *keys_dev, size_t len_keys,
                                          const uint32_t *exps_dev, size_t len_exps, double *out_dev, size_t len_out,
                                          void *stream = nullptr) {
    check(pfhe_tfhe_mb_combine_key_dev(fft.handle(), glwe_dimension, decompose_length, grouping_factor, keys_dev, len_keys,
                                       exps_dev, len_exps, out_dev, len_out, stream));
}

// X^{exps[e]} * element e for elements of polys_per_exp torus polynomials (the X^{-b_e} * TV that starts a bootstrap)
template <class W>
void mul_monomial_each_to_dev(const FullComplex64FftTable &fft, const W *a_dev, size_t len, const uint32_t *exps_dev,
                              size_t polys_per_exp, detail::same<W> *out_dev, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_mul_monomial_each_to_dev(fft.handle(), a_dev, len, exps_dev, polys_per_exp, out_dev, stream));
}

// The project's own modulus switch (the reference has none): exps[e*n + i] = sw(a_{e,i}), neg_b[e] = (2N - sw(b_e)) mod 2N
template <class W>
void lwe_modulus_switch_dev(int device, const W *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                            uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev, size_t len_neg_b,
                            void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_modswitch_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, exps_dev, len_exps, neg_b_dev,
                                             len_neg_b, stream));
}
// ... to multiples of 2^log_stride (log_stride <= log_n), what a many-LUT rotation takes; log_stride 0 is the call above
template <class W>
void lwe_modulus_switch_strided_dev(int device, const W *lwe_dev, size_t len_lwe, size_t lwe_dimension, uint32_t log_n,
                                    uint32_t log_stride, uint32_t *exps_dev, size_t len_exps, uint32_t *neg_b_dev,
                                    size_t len_neg_b, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_modswitch_stride_dev(device, lwe_dev, len_lwe, lwe_dimension, log_n, log_stride, exps_dev,
                                                    len_exps, neg_b_dev, len_neg_b, stream));
}
// Rlwe::extract_lwe_with_index (primus_lattice/src/rlwe/coeff.rs:194-227) per mask polynomial of a GLWE ciphertext
template <class W>
void glwe_sample_extract(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *glwe, size_t len_glwe,
                         size_t index, detail::same<W> *lwe, size_t len_lwe) {
    check(detail::Fns<W>::tfhe_sample_extract(fft.handle(), glwe_dimension, glwe, len_glwe, index, lwe, len_lwe));
}
template <class W>
void glwe_sample_extract_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *glwe_dev, size_t len_glwe,
                             size_t index, detail::same<W> *lwe_dev, size_t len_lwe, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_sample_extract_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, index, lwe_dev, len_lwe,
                                                  stream));
}
// LWE key switch: out = (0, b) - sum_i sum_j d_{i,j} * KSK[i][j] (Lwe::add_mul_scalar_assign, lwe/single_message.rs:262-268,
// with ApproxSignedBasis's digits); decompose_length 0 = the full BITS / log_basis
template <class W>
void lwe_keyswitch(int device, const W *lwe_in, size_t len_in, size_t in_dimension, const detail::same<W> *ksk,
                   size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length,
                   detail::same<W> *lwe_out, size_t len_out) {
    check(detail::Fns<W>::tfhe_keyswitch(device, lwe_in, len_in, in_dimension, ksk, len_ksk, out_dimension, log_basis,
                                         decompose_length, lwe_out, len_out));
}
template <class W>
void lwe_keyswitch_dev(int device, const W *lwe_in_dev, size_t len_in, size_t in_dimension, const detail::same<W> *ksk_dev,
                       size_t len_ksk, size_t out_dimension, uint32_t log_basis, size_t decompose_length,
                       detail::same<W> *lwe_out_dev, size_t len_out, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_keyswitch_dev(device, lwe_in_dev, len_in, in_dimension, ksk_dev, len_ksk, out_dimension,
                                             log_basis, decompose_length, lwe_out_dev, len_out, stream));
}

// The linear layer with clear weights (pfhe_lwe{,32}_linear*): out[e][o] = sum_i W[o][i] * in[e][i] + (0, bias[o]), out_features
// chains of Lwe::add_mul_scalar_assign (lwe/single_message.rs:262-268) per input vector.  The weights' type picks the entry:
// words of the ciphertext's width (the reference's `scalar: T`), or int8_t, which gives the words of the sign-extended weights.
// bias: out_features torus words, or null with len_bias 0.
template <class W>
void lwe_linear(int device, const W *lwe_in, size_t len_in, size_t dimension, const detail::same<W> *weights, size_t len_weights,
                size_t in_features, size_t out_features, const detail::same<W> *bias, size_t len_bias, detail::same<W> *lwe_out,
                size_t len_out) {
    check(detail::Fns<W>::lwe_linear(device, lwe_in, len_in, dimension, weights, len_weights, in_features, out_features, bias,
                                     len_bias, lwe_out, len_out));
}
template <class W>
void lwe_linear(int device, const W *lwe_in, size_t len_in, size_t dimension, const int8_t *weights, size_t len_weights,
                size_t in_features, size_t out_features, const detail::same<W> *bias, size_t len_bias, detail::same<W> *lwe_out,
                size_t len_out) {
    check(detail::Fns<W>::lwe_linear_i8(device, lwe_in, len_in, dimension, weights, len_weights, in_features, out_features, bias,
                                        len_bias, lwe_out, len_out));
}
template <class W>
void lwe_linear_dev(int device, const W *lwe_in_dev, size_t len_in, size_t dimension, const detail::same<W> *weights_dev,
                    size_t len_weights, size_t in_features, size_t out_features, const detail::same<W> *bias_dev, size_t len_bias,
                    detail::same<W> *lwe_out_dev, size_t len_out, void *stream = nullptr) {
    check(detail::Fns<W>::lwe_linear_dev(device, lwe_in_dev, len_in, dimension, weights_dev, len_weights, in_features,
                                         out_features, bias_dev, len_bias, lwe_out_dev, len_out, stream));
}
template <class W>
void lwe_linear_dev(int device, const W *lwe_in_dev, size_t len_in, size_t dimension, const int8_t *weights_dev,
                    size_t len_weights, size_t in_features, size_t out_features, const detail::same<W> *bias_dev, size_t len_bias,
                    detail::same<W> *lwe_out_dev, size_t len_out, void *stream = nullptr) {
    check(detail::Fns<W>::lwe_linear_i8_dev(device, lwe_in_dev, len_in, dimension, weights_dev, len_weights, in_features,
                                            out_features, bias_dev, len_bias, lwe_out_dev, len_out, stream));
}

// The random layer (pfhe_csprng_keystream_dev, pfhe_rand{,32}_*): a position-addressed ChaCha20 stream on the device, exact
// samplers over it, whole ciphertext rows, and seeded LWE ciphertexts.  A RandSeed is the identity of one stream: eight key
// words (RFC 8439's key, little-endian words) and a 64-bit nonce.  It lives in host memory and reaches the kernels as a
// kernel argument; the library gathers no entropy, so the key is the caller's.  Output i of a sampler is a closed form of
// (seed, i): no state, any sub-range from any call.  A mask seed may be published; a noise seed is a secret and must differ
// from it (refused otherwise).  primus_distr's samplers draw from a stateful rand::Rng instead: binary and ternary give
// sample_binary_values_to / sample_ternary_values_to (primus_distr/src/common.rs:22-76) on the same word stream, the others
// have no counterpart there.
struct RandSeed {
    uint32_t key[8];
    uint32_t nonce[2];  // state words 14 (low) and 15 (high)
    RandSeed(const uint32_t (&key_words)[8], uint64_t nonce64) : nonce{(uint32_t)nonce64, (uint32_t)(nonce64 >> 32)} {
        for (int i = 0; i < 8; ++i) key[i] = key_words[i];
    }
};
// u32 stream words [word_offset, word_offset + n_words); a template like the rest of this header, so that a unit that does not
// call it does not reference the entry point: the stream's words are uint32_t and W is nothing else
template <class W = uint32_t>
void csprng_keystream_dev(int device, const RandSeed &seed, size_t word_offset, detail::same<W> *out_dev, size_t n_words,
                          void *stream = nullptr) {
    static_assert(std::is_same<W, uint32_t>::value, "the keystream is written as uint32_t words");
    check(pfhe_csprng_keystream_dev(device, seed.key, seed.nonce, word_offset, out_dev, n_words, stream));
}
// outputs [offset, offset + n) of a sampler: uniform words, bits, {0, 0, 1, -1} by two bits, TUniform(bound_log2)
template <class W>
void torus_uniform_dev(int device, const RandSeed &seed, size_t offset, W *out_dev, size_t n, void *stream = nullptr) {
    check(detail::Fns<W>::rand_uniform_dev(device, seed.key, seed.nonce, offset, out_dev, n, stream));
}
template <class W>
void torus_binary_dev(int device, const RandSeed &seed, size_t offset, W *out_dev, size_t n, void *stream = nullptr) {
    check(detail::Fns<W>::rand_binary_dev(device, seed.key, seed.nonce, offset, out_dev, n, stream));
}
template <class W>
void torus_ternary_dev(int device, const RandSeed &seed, size_t offset, W *out_dev, size_t n, void *stream = nullptr) {
    check(detail::Fns<W>::rand_ternary_dev(device, seed.key, seed.nonce, offset, out_dev, n, stream));
}
template <class W>
void torus_tuniform_dev(int device, const RandSeed &seed, size_t offset, uint32_t bound_log2, W *out_dev, size_t n,
                        void *stream = nullptr) {
    check(detail::Fns<W>::rand_tuniform_dev(device, seed.key, seed.nonce, offset, bound_log2, out_dev, n, stream));
}
// rows of mask_len uniform words and body_len TUniform words (stored, or added when `add`), absolute rows from first_row on:
// the `rand` argument of every key generator and the buffers lwe_body_mac / glwe_body_mac take
template <class W>
void fill_rows_dev(int device, const RandSeed &mask_seed, const RandSeed &noise_seed, size_t first_row, size_t mask_len,
                   size_t body_len, uint32_t bound_log2, bool add, W *out_dev, size_t len_out, void *stream = nullptr) {
    check(detail::Fns<W>::rand_fill_rows_dev(device, mask_seed.key, mask_seed.nonce, noise_seed.key, noise_seed.nonce, first_row,
                                             mask_len, body_len, bound_log2, add ? 1 : 0, out_dev, len_out, stream));
}
// bodies[r] += <mask(first_row + r), lwe_key> + noise(first_row + r): the mask never leaves registers
template <class W>
void lwe_encrypt_seeded(int device, const RandSeed &mask_seed, const RandSeed &noise_seed, size_t first_row, const W *lwe_key,
                        size_t dimension, uint32_t bound_log2, detail::same<W> *bodies, size_t rows) {
    check(detail::Fns<W>::rand_lwe_encrypt_seeded(device, mask_seed.key, mask_seed.nonce, noise_seed.key, noise_seed.nonce,
                                                  first_row, lwe_key, dimension, bound_log2, bodies, rows));
}
template <class W>
void lwe_encrypt_seeded_dev(int device, const RandSeed &mask_seed, const RandSeed &noise_seed, size_t first_row,
                            const W *lwe_key_dev, size_t dimension, uint32_t bound_log2, detail::same<W> *bodies_dev, size_t rows,
                            void *stream = nullptr) {
    check(detail::Fns<W>::rand_lwe_encrypt_seeded_dev(device, mask_seed.key, mask_seed.nonce, noise_seed.key, noise_seed.nonce,
                                                      first_row, lwe_key_dev, dimension, bound_log2, bodies_dev, rows, stream));
}
// the full rows of seeded ciphertexts: masks from the stream, bodies copied; what the receiving side runs
template <class W>
void seeded_expand(int device, const RandSeed &mask_seed, size_t first_row, size_t mask_len, size_t body_len, const W *bodies,
                   size_t len_bodies, detail::same<W> *out, size_t len_out) {
    check(detail::Fns<W>::rand_seeded_expand(device, mask_seed.key, mask_seed.nonce, first_row, mask_len, body_len, bodies,
                                             len_bodies, out, len_out));
}
template <class W>
void seeded_expand_dev(int device, const RandSeed &mask_seed, size_t first_row, size_t mask_len, size_t body_len,
                       const W *bodies_dev, size_t len_bodies, detail::same<W> *out_dev, size_t len_out, void *stream = nullptr) {
    check(detail::Fns<W>::rand_seeded_expand_dev(device, mask_seed.key, mask_seed.nonce, first_row, mask_len, body_len, bodies_dev,
                                                 len_bodies, out_dev, len_out, stream));
}

// The batched programmable bootstrap (pfhe_tfhe_bootstrap_*): modulus switch, ACC = X^{-b~} * TV, the blind rotation over
// lwe_dimension steps, sample extraction at index 0 and, with a key switch, the switch back to lwe_dimension.  Owns a
// blind-rotation handle and every buffer between the stages; one holder at a time.
template <class W>
class TfheBootstrapT : public detail::Fns<W>::TfheBootstrap {
    using F = detail::Fns<W>;

  public:
    TfheBootstrapT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                   size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, bool with_keyswitch = true,
                   size_t chunk = 0, size_t grouping_factor = 1, uint32_t log_luts = 0) {
        // grouping_factor 1: the classic rotation; above 1 the multi-bit one, on (lwe_dimension / g) * 2^g keys.  log_luts
        // above 0: the many-LUT bootstrap, 2^log_luts outputs per input (output (e, i) at e * 2^log_luts + i)
        check(log_luts != 0
                  ? F::tfhe_bootstrap_create_many_lut(fft.handle(), glwe_dimension, log_basis, decompose_length,
                                                      lwe_dimension, ks_log_basis, ks_decompose_length,
                                                      with_keyswitch ? 1 : 0, grouping_factor, log_luts, chunk, &this->h_)
              : grouping_factor == 1
                  ? F::tfhe_bootstrap_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                             ks_log_basis, ks_decompose_length, with_keyswitch ? 1 : 0, chunk, &this->h_)
                  : F::tfhe_bootstrap_create_multibit(fft.handle(), glwe_dimension, log_basis, decompose_length,
                                                      lwe_dimension, ks_log_basis, ks_decompose_length,
                                                      with_keyswitch ? 1 : 0, grouping_factor, chunk, &this->h_));
    }
    void bootstrap(const W *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const W *tv, size_t len_tv,
                   const W *ksk, size_t len_ksk, W *lwe_out, size_t len_out) {
        check(F::tfhe_bootstrap(this->h_, lwe_in, len_in, bsk, len_bsk, tv, len_tv, ksk, len_ksk, lwe_out, len_out));
    }
    void bootstrap_dev(const W *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk, const W *tv_dev,
                       size_t len_tv, const W *ksk_dev, size_t len_ksk, W *lwe_out_dev, size_t len_out,
                       void *stream = nullptr) {
        check(F::tfhe_bootstrap_dev(this->h_, lwe_in_dev, len_in, bsk_dev, len_bsk, tv_dev, len_tv, ksk_dev, len_ksk,
                                    lwe_out_dev, len_out, stream));
    }
};
using TfheBootstrap = TfheBootstrapT<uint64_t>;
using TfheBootstrap32 = TfheBootstrapT<uint32_t>;

// Key generation, encryption and phase (pfhe_tfhe{,32}_lwe_body_mac*, _glwe_body_mac*, _ggsw_add_gadget_dev, _bsk_generate_dev,
// _ksk_generate_dev).  No random number is drawn: the buffers arrive holding the caller's randomness (masks uniform, bodies
// noise + message).  body_mac adds <a,s> (A * z) into the body slot, or subtracts it (the phase); the gadget call adds
// m * 2^(drop_bits + l*log_basis); the two generators write the keys TfheBootstrap takes (grouping_factor 0: the classic
// layout, 1..4: the multi-bit one).
template <class W>
void lwe_body_mac(int device, W *lwe, size_t len_lwe, size_t dimension, const detail::same<W> *key, size_t len_key,
                  bool subtract) {
    check(detail::Fns<W>::tfhe_lwe_body_mac(device, lwe, len_lwe, dimension, key, len_key, subtract ? 1 : 0));
}
template <class W>
void lwe_body_mac_dev(int device, W *lwe_dev, size_t len_lwe, size_t dimension, const detail::same<W> *key_dev,
                      size_t len_key, bool subtract, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_lwe_body_mac_dev(device, lwe_dev, len_lwe, dimension, key_dev, len_key, subtract ? 1 : 0,
                                                stream));
}
template <class W>
void glwe_body_mac(const FullComplex64FftTable &fft, size_t glwe_dimension, W *glwe, size_t len_glwe,
                   const detail::same<W> *key, size_t len_key, bool subtract) {
    check(detail::Fns<W>::tfhe_glwe_body_mac(fft.handle(), glwe_dimension, glwe, len_glwe, key, len_key, subtract ? 1 : 0));
}
template <class W>
void glwe_body_mac_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, W *glwe_dev, size_t len_glwe,
                       const detail::same<W> *key_dev, size_t len_key, bool subtract, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_glwe_body_mac_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, key_dev, len_key,
                                                 subtract ? 1 : 0, stream));
}
template <class W>
void ggsw_add_gadget_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                         W *ggsw_dev, size_t len_ggsw, const detail::same<W> *messages_dev, size_t len_messages,
                         void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_ggsw_add_gadget_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, ggsw_dev,
                                                   len_ggsw, messages_dev, len_messages, stream));
}
template <class W>
void tfhe_generate_bsk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                           size_t decompose_length, size_t grouping_factor, const W *lwe_key_dev, size_t lwe_dimension,
                           const detail::same<W> *glwe_key_dev, size_t len_glwe_key, detail::same<W> *ggsw_torus_dev,
                           size_t len_ggsw, double *bsk_out_dev, size_t len_bsk, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_bsk_generate_dev(fft.handle(), glwe_dimension, log_basis, decompose_length, grouping_factor,
                                                lwe_key_dev, lwe_dimension, glwe_key_dev, len_glwe_key, ggsw_torus_dev,
                                                len_ggsw, bsk_out_dev, len_bsk, stream));
}
template <class W>
void tfhe_generate_ksk_dev(int device, const W *key_in_dev, size_t in_dimension, const detail::same<W> *key_out_dev,
                           size_t out_dimension, uint32_t log_basis, size_t decompose_length, detail::same<W> *ksk_dev,
                           size_t len_ksk, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_ksk_generate_dev(device, key_in_dev, in_dimension, key_out_dev, out_dimension, log_basis,
                                                decompose_length, ksk_dev, len_ksk, stream));
}

// Packing (pfhe_tfhe{,32}_pack_keyswitch*, _pksk_generate_dev, _sample_extract_first_few*, _multimsg_extract*): `count` LWE
// ciphertexts per group into one GLWE under the packing key (in_dimension x ell GLWE rows, generated in place from the
// caller's randomness), Rlwe::extract_first_few_lwe per mask polynomial (the MultiMsgLwe layout) and its expansion into
// `count` LWE ciphertexts (MultiMsgLwe::extract_rlwe_mode at every index).
template <class W>
void lwe_pack_keyswitch(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *lwe_in, size_t len_in,
                        size_t in_dimension, size_t count, const detail::same<W> *pksk, size_t len_pksk, uint32_t log_basis,
                        size_t decompose_length, detail::same<W> *glwe_out, size_t len_out) {
    check(detail::Fns<W>::tfhe_pack_keyswitch(fft.handle(), glwe_dimension, lwe_in, len_in, in_dimension, count, pksk,
                                              len_pksk, log_basis, decompose_length, glwe_out, len_out));
}
template <class W>
void lwe_pack_keyswitch_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *lwe_in_dev, size_t len_in,
                            size_t in_dimension, size_t count, const detail::same<W> *pksk_dev, size_t len_pksk,
                            uint32_t log_basis, size_t decompose_length, detail::same<W> *glwe_out_dev, size_t len_out,
                            void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_pack_keyswitch_dev(fft.handle(), glwe_dimension, lwe_in_dev, len_in, in_dimension, count,
                                                  pksk_dev, len_pksk, log_basis, decompose_length, glwe_out_dev, len_out,
                                                  stream));
}
template <class W>
void tfhe_generate_pksk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *key_in_dev, size_t in_dimension,
                            const detail::same<W> *glwe_key_dev, size_t len_glwe_key, uint32_t log_basis,
                            size_t decompose_length, detail::same<W> *pksk_dev, size_t len_pksk, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_pksk_generate_dev(fft.handle(), glwe_dimension, key_in_dev, in_dimension, glwe_key_dev,
                                                 len_glwe_key, log_basis, decompose_length, pksk_dev, len_pksk, stream));
}
template <class W>
void glwe_sample_extract_first_few(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *glwe, size_t len_glwe,
                                   size_t count, detail::same<W> *multi, size_t len_multi) {
    check(detail::Fns<W>::tfhe_sample_extract_first_few(fft.handle(), glwe_dimension, glwe, len_glwe, count, multi,
                                                        len_multi));
}
template <class W>
void glwe_sample_extract_first_few_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *glwe_dev,
                                       size_t len_glwe, size_t count, detail::same<W> *multi_dev, size_t len_multi,
                                       void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_sample_extract_first_few_dev(fft.handle(), glwe_dimension, glwe_dev, len_glwe, count,
                                                            multi_dev, len_multi, stream));
}
template <class W>
void multimsg_lwe_extract(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *multi, size_t len_multi,
                          size_t count, detail::same<W> *lwe, size_t len_lwe) {
    check(detail::Fns<W>::tfhe_multimsg_extract(fft.handle(), glwe_dimension, multi, len_multi, count, lwe, len_lwe));
}
template <class W>
void multimsg_lwe_extract_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *multi_dev, size_t len_multi,
                              size_t count, detail::same<W> *lwe_dev, size_t len_lwe, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_multimsg_extract_dev(fft.handle(), glwe_dimension, multi_dev, len_multi, count, lwe_dev,
                                                    len_lwe, stream));
}

// The packing key switch in the Fourier domain (pfhe_tfhe{,32}_packfft_*, _pack_keyswitch_fft*): lwe_pack_keyswitch's rule
// as one external product of in_dimension * ell rows against the half-spectrum key of tfhe_pack_key_fourier_dev.  Approximate
// as the TFHE product is and opt-in: 1 <= log N <= 11, 1 <= glwe_dimension <= 3; the exact call above serves every shape.
// The context owns the partial sums of `chunk` groups; one holder at a time.
template <class W>
class TfhePackFftContextT : public detail::Fns<W>::TfhePackfftPlan {
    using F = detail::Fns<W>;

  public:
    TfhePackFftContextT(const FullComplex64FftTable &fft, size_t glwe_dimension, size_t in_dimension, uint32_t log_basis,
                        size_t decompose_length = 0, size_t chunk = 0) {
        check(F::tfhe_packfft_plan_create(fft.handle(), glwe_dimension, in_dimension, log_basis, decompose_length, chunk,
                                          &this->h_));
    }
};
using TfhePackFftContext = TfhePackFftContextT<uint64_t>;
using TfhePackFftContext32 = TfhePackFftContextT<uint32_t>;

template <class W>
void tfhe_pack_key_fourier_dev(const detail::same<W> *pksk_dev, size_t len_pksk, double *fkey_dev, size_t len_fkey,
                               TfhePackFftContextT<W> &context, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_packfft_key_dev(context.handle(), pksk_dev, len_pksk, fkey_dev, len_fkey, stream));
}
template <class W>
void lwe_pack_keyswitch_fft(const detail::same<W> *lwe_in, size_t len_in, size_t count, const double *fkey, size_t len_fkey,
                            detail::same<W> *glwe_out, size_t len_out, TfhePackFftContextT<W> &context) {
    check(detail::Fns<W>::tfhe_pack_keyswitch_fft(context.handle(), lwe_in, len_in, count, fkey, len_fkey, glwe_out,
                                                  len_out));
}
template <class W>
void lwe_pack_keyswitch_fft_dev(const detail::same<W> *lwe_in_dev, size_t len_in, size_t count, const double *fkey_dev,
                                size_t len_fkey, detail::same<W> *glwe_out_dev, size_t len_out,
                                TfhePackFftContextT<W> &context, void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_pack_keyswitch_fft_dev(context.handle(), lwe_in_dev, len_in, count, fkey_dev, len_fkey,
                                                      glwe_out_dev, len_out, stream));
}

// The circuit bootstrap (pfhe_tfhe{,32}_private_keyswitch*, _pfksk_generate_dev, _cbs_*): the private functional key switch
// turns batch x levels LWE ciphertexts into GGSW-shaped blocks whose row (u, l) has the phase f_u of input (e, l), under the
// key tfhe_generate_pfksk_dev writes in place from the caller's randomness; TfheCircuitBootstrap runs, per input bit and
// level of the output basis, modulus switch, ACC = X^{-b~} * (-g_l/2), the blind rotation, extraction with g_l/2 added and
// that key switch, and gives a torus-form GGSW of the bit.
template <class W>
void lwe_private_keyswitch(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *lwe_in, size_t len_in,
                           size_t in_dimension, size_t levels, const detail::same<W> *pfksk, size_t len_pfksk,
                           uint32_t log_basis, size_t decompose_length, detail::same<W> *out, size_t len_out) {
    check(detail::Fns<W>::tfhe_private_keyswitch(fft.handle(), glwe_dimension, lwe_in, len_in, in_dimension, levels, pfksk,
                                                 len_pfksk, log_basis, decompose_length, out, len_out));
}
template <class W>
void lwe_private_keyswitch_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *lwe_in_dev, size_t len_in,
                               size_t in_dimension, size_t levels, const detail::same<W> *pfksk_dev, size_t len_pfksk,
                               uint32_t log_basis, size_t decompose_length, detail::same<W> *out_dev, size_t len_out,
                               void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_private_keyswitch_dev(fft.handle(), glwe_dimension, lwe_in_dev, len_in, in_dimension, levels,
                                                     pfksk_dev, len_pfksk, log_basis, decompose_length, out_dev, len_out,
                                                     stream));
}
template <class W>
void tfhe_generate_pfksk_dev(const FullComplex64FftTable &fft, size_t glwe_dimension, const W *key_in_dev,
                             size_t in_dimension, const detail::same<W> *glwe_key_dev, size_t len_glwe_key,
                             uint32_t log_basis, size_t decompose_length, detail::same<W> *pfksk_dev, size_t len_pfksk,
                             void *stream = nullptr) {
    check(detail::Fns<W>::tfhe_pfksk_generate_dev(fft.handle(), glwe_dimension, key_in_dev, in_dimension, glwe_key_dev,
                                                  len_glwe_key, log_basis, decompose_length, pfksk_dev, len_pfksk, stream));
}

// Owns a blind-rotation handle and every buffer between the stages for `chunk` inputs; one holder at a time.
template <class W>
class TfheCircuitBootstrapT : public detail::Fns<W>::TfheCbs {
    using F = detail::Fns<W>;

  public:
    TfheCircuitBootstrapT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                          size_t decompose_length, size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length,
                          uint32_t pfks_log_basis, size_t pfks_decompose_length, size_t chunk = 0) {
        check(F::tfhe_cbs_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension, cbs_log_basis,
                                 cbs_decompose_length, pfks_log_basis, pfks_decompose_length, chunk, &this->h_));
    }
    // with options (pfhe_tfhe_cbs_create_with): grouping_factor above 1 runs the multi-bit rotation on its key;
    // shared_rotation runs one rotation per input for all levels of the output basis (many-LUT)
    TfheCircuitBootstrapT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis,
                          size_t decompose_length, size_t lwe_dimension, uint32_t cbs_log_basis, size_t cbs_decompose_length,
                          uint32_t pfks_log_basis, size_t pfks_decompose_length, size_t chunk, size_t grouping_factor,
                          bool shared_rotation) {
        check(F::tfhe_cbs_create_with(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension,
                                      cbs_log_basis, cbs_decompose_length, pfks_log_basis, pfks_decompose_length,
                                      grouping_factor, shared_rotation ? 1 : 0, chunk, &this->h_));
    }
    void circuit_bootstrap(const W *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const W *pfksk,
                           size_t len_pfksk, W *ggsw_out, size_t len_out) {
        check(F::tfhe_cbs(this->h_, lwe_in, len_in, bsk, len_bsk, pfksk, len_pfksk, ggsw_out, len_out));
    }
    void circuit_bootstrap_dev(const W *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk, const W *pfksk_dev,
                               size_t len_pfksk, W *ggsw_out_dev, size_t len_out, void *stream = nullptr) {
        check(F::tfhe_cbs_dev(this->h_, lwe_in_dev, len_in, bsk_dev, len_bsk, pfksk_dev, len_pfksk, ggsw_out_dev, len_out,
                              stream));
    }
};
using TfheCircuitBootstrap = TfheCircuitBootstrapT<uint64_t>;
using TfheCircuitBootstrap32 = TfheCircuitBootstrapT<uint32_t>;

// The batched CMUX with a Fourier GGSW selector per group of per_key ciphertexts (out[i] = d0[i] +
// external_product_to(d1[i] - d0[i], keys[i / per_key]); out may be d0 or d1) and the tree that selects one of 2^depth GLWE
// ciphertexts by depth selectors per input (pfhe_tfhe{,32}_cmux_tree_*, _cmux, _cmux_dev).  Owns the node buffers of `chunk`
// inputs and, off the fused shape, a product plan; one holder at a time.
template <class W>
class TfheCmuxTreeT : public detail::Fns<W>::TfheCmuxTree {
    using F = detail::Fns<W>;

  public:
    TfheCmuxTreeT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                  size_t depth, size_t chunk = 0) {
        check(F::tfhe_cmux_tree_create(fft.handle(), glwe_dimension, log_basis, decompose_length, depth, chunk, &this->h_));
    }
    void cmux(const W *d0, size_t len_d0, const W *d1, size_t len_d1, const double *keys, size_t len_keys, size_t per_key,
              W *out, size_t len_out) {
        check(F::tfhe_cmux(this->h_, d0, len_d0, d1, len_d1, keys, len_keys, per_key, out, len_out));
    }
    void cmux_dev(const W *d0_dev, size_t len_d0, const W *d1_dev, size_t len_d1, const double *keys_dev, size_t len_keys,
                  size_t per_key, W *out_dev, size_t len_out, void *stream = nullptr) {
        check(F::tfhe_cmux_dev(this->h_, d0_dev, len_d0, d1_dev, len_d1, keys_dev, len_keys, per_key, out_dev, len_out,
                               stream));
    }
    void cmux_tree(const W *table, size_t len_table, const double *selectors, size_t len_selectors, W *out,
                   size_t len_out) {
        check(F::tfhe_cmux_tree(this->h_, table, len_table, selectors, len_selectors, out, len_out));
    }
    void cmux_tree_dev(const W *table_dev, size_t len_table, const double *selectors_dev, size_t len_selectors, W *out_dev,
                       size_t len_out, void *stream = nullptr) {
        check(F::tfhe_cmux_tree_dev(this->h_, table_dev, len_table, selectors_dev, len_selectors, out_dev, len_out, stream));
    }
};
using TfheCmuxTree = TfheCmuxTreeT<uint64_t>;
using TfheCmuxTree32 = TfheCmuxTreeT<uint32_t>;

// The GLWE automorphism X -> X^t with its key switch (out = (0, .., 0, sigma_t(B)) - sum_j sum_l d_l(sigma_t(A_j)) key[j][l],
// key the k*ell mask rows of a Fourier GGSW; t = 1 is a plain key switch; out may not overlap in) and the homomorphic trace
// of `steps` steps built from it (ACC += automorphism(ACC, keys[s-1], 2^(log N - s + 1) + 1); out may be in; the factor
// 2^steps stays in the result) (pfhe_tfhe{,32}_glwe_trace_*, _glwe_automorphism*).  Owns, off the fused shape, the buffers
// of `chunk` ciphertexts; one holder at a time.  The keys come from pfhe_tfhe*_gksk_generate_dev, the embedding of an LWE
// ciphertext from pfhe_tfhe*_lwe_embed*, both stateless.
template <class W>
class TfheGlweTraceT : public detail::Fns<W>::TfheGlweTrace {
    using F = detail::Fns<W>;

  public:
    TfheGlweTraceT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                   size_t chunk = 0) {
        check(F::tfhe_glwe_trace_create(fft.handle(), glwe_dimension, log_basis, decompose_length, chunk, &this->h_));
    }
    void automorphism(const W *in, size_t len_in, const double *key, size_t len_key, uint32_t t, W *out, size_t len_out) {
        check(F::tfhe_glwe_automorphism(this->h_, in, len_in, key, len_key, t, out, len_out));
    }
    void automorphism_dev(const W *in_dev, size_t len_in, const double *key_dev, size_t len_key, uint32_t t, W *out_dev,
                          size_t len_out, void *stream = nullptr) {
        check(F::tfhe_glwe_automorphism_dev(this->h_, in_dev, len_in, key_dev, len_key, t, out_dev, len_out, stream));
    }
    void trace(const W *in, size_t len_in, const double *keys, size_t len_keys, size_t steps, W *out, size_t len_out) {
        check(F::tfhe_glwe_trace(this->h_, in, len_in, keys, len_keys, steps, out, len_out));
    }
    void trace_dev(const W *in_dev, size_t len_in, const double *keys_dev, size_t len_keys, size_t steps, W *out_dev,
                   size_t len_out, void *stream = nullptr) {
        check(F::tfhe_glwe_trace_dev(this->h_, in_dev, len_in, keys_dev, len_keys, steps, out_dev, len_out, stream));
    }
};
using TfheGlweTrace = TfheGlweTraceT<uint64_t>;
using TfheGlweTrace32 = TfheGlweTraceT<uint32_t>;

// Ring packing of LWE ciphertexts by automorphisms (pfhe_ringpack{,32}_*): the
// merge at level l (out = S + automorphism(D, key, 2^l + 1), D = even - X^s odd, S = even + X^s odd, s = N / 2^l; out may be
// even) and the pack of `count` <= max_count LWE ciphertexts per output built from it, the embedding and the trailing trace
// steps, on ALL log N keys of the full trace: N times the phase of ciphertext i arrives at coefficient slot(i, count) =
// i N / 2^ceil(log2 count).  The factor N stays in the result: the message has to sit log N bits lower in the inputs, the
// price against the packing key switch and its far larger key.  Owns the node buffer of `chunk` outputs (and off the fused
// shape the general form's buffers); one holder at a time.
template <class W>
class TfheRingPackT : public detail::Fns<W>::TfheRingPack {
    using F = detail::Fns<W>;
    size_t n_ = 0;

  public:
    // max_count 0: the default, N
    TfheRingPackT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                  size_t max_count = 0, size_t chunk = 0)
        : n_(fft.poly_length()) {
        check(F::ringpack_create(fft.handle(), glwe_dimension, log_basis, decompose_length, max_count ? max_count : n_, chunk,
                                       &this->h_));
    }
    // the coefficient that holds N times the phase of input i of `count`
    size_t slot(size_t i, size_t count) const {
        size_t stride = n_;
        for (size_t c = 1; c < count; c <<= 1) stride >>= 1;
        return i * stride;
    }
    void merge(const W *even, size_t len_even, const W *odd, size_t len_odd, const double *key, size_t len_key, uint32_t level,
               W *out, size_t len_out) {
        check(F::ringpack_merge(this->h_, even, len_even, odd, len_odd, key, len_key, level, out, len_out));
    }
    void merge_dev(const W *even_dev, size_t len_even, const W *odd_dev, size_t len_odd, const double *key_dev, size_t len_key,
                   uint32_t level, W *out_dev, size_t len_out, void *stream = nullptr) {
        check(F::ringpack_merge_dev(this->h_, even_dev, len_even, odd_dev, len_odd, key_dev, len_key, level, out_dev, len_out,
                                          stream));
    }
    void pack(const W *lwe, size_t len_lwe, const double *keys, size_t len_keys, size_t count, W *glwe_out, size_t len_out) {
        check(F::ringpack_pack(this->h_, lwe, len_lwe, keys, len_keys, count, glwe_out, len_out));
    }
    void pack_dev(const W *lwe_dev, size_t len_lwe, const double *keys_dev, size_t len_keys, size_t count, W *glwe_out_dev,
                  size_t len_out, void *stream = nullptr) {
        check(F::ringpack_pack_dev(this->h_, lwe_dev, len_lwe, keys_dev, len_keys, count, glwe_out_dev, len_out, stream));
    }
};
using TfheRingPack = TfheRingPackT<uint64_t>;
using TfheRingPack32 = TfheRingPackT<uint32_t>;

// A look-up table of 2^(tree_depth + rot_bits) entries on encrypted bits: a CMUX tree over the high bits, the rotation by
// the low bits (acc += external_product_to(X^{2N - 2^(j+log_stride)} acc - acc, the input's key of bit j); out may be inp)
// and sample extraction at the indices below `extract` (pfhe_tfhe{,32}_lut_*, _rotate_by_bits*, _lut_eval*).  Owns the
// buffers of `chunk` inputs of `outputs` look-ups each; one holder at a time.
template <class W>
class TfheLutT : public detail::Fns<W>::TfheLut {
    using F = detail::Fns<W>;

  public:
    TfheLutT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
             size_t tree_depth, size_t rot_bits, size_t outputs = 1, size_t log_stride = 0, size_t chunk = 0) {
        check(F::tfhe_lut_create(fft.handle(), glwe_dimension, log_basis, decompose_length, tree_depth, rot_bits, log_stride,
                                 outputs, chunk, &this->h_));
    }
    void rotate_by_bits(const W *inp, size_t len_inp, const double *keys, size_t len_keys, size_t keys_per_input,
                        size_t first_key, W *out, size_t len_out) {
        check(F::tfhe_rotate_by_bits(this->h_, inp, len_inp, keys, len_keys, keys_per_input, first_key, out, len_out));
    }
    void rotate_by_bits_dev(const W *inp_dev, size_t len_inp, const double *keys_dev, size_t len_keys, size_t keys_per_input,
                            size_t first_key, W *out_dev, size_t len_out, void *stream = nullptr) {
        check(F::tfhe_rotate_by_bits_dev(this->h_, inp_dev, len_inp, keys_dev, len_keys, keys_per_input, first_key, out_dev,
                                         len_out, stream));
    }
    void lut_eval(const W *table, size_t len_table, const double *selectors, size_t len_selectors, size_t extract, W *out,
                  size_t len_out) {
        check(F::tfhe_lut_eval(this->h_, table, len_table, selectors, len_selectors, extract, out, len_out));
    }
    void lut_eval_dev(const W *table_dev, size_t len_table, const double *selectors_dev, size_t len_selectors,
                      size_t extract, W *out_dev, size_t len_out, void *stream = nullptr) {
        check(F::tfhe_lut_eval_dev(this->h_, table_dev, len_table, selectors_dev, len_selectors, extract, out_dev, len_out,
                                   stream));
    }
};
using TfheLut = TfheLutT<uint64_t>;
using TfheLut32 = TfheLutT<uint32_t>;

// Bit extraction: batch LWE ciphertexts of k*N + 1 words with phase m*2^delta_log + e become batch*bits LWE ciphertexts of
// lwe_dimension + 1 words, bit i of input e at e*bits + i with phase m_i*2^(BITS-1) plus noise: per bit the key switch of the
// running ciphertext shifted left and, unless it is the last, a blind rotation that clears the bit
// (pfhe_bitext{,32}_*).  Owns a classic rotation and the buffers of `chunk` inputs; one holder at a
// time.
template <class W>
class TfheBitExtractT : public detail::Fns<W>::TfheBitext {
    using F = detail::Fns<W>;

  public:
    TfheBitExtractT(const FullComplex64FftTable &fft, size_t glwe_dimension, uint32_t log_basis, size_t decompose_length,
                    size_t lwe_dimension, uint32_t ks_log_basis, size_t ks_decompose_length, size_t chunk = 0) {
        check(F::bitext_create(fft.handle(), glwe_dimension, log_basis, decompose_length, lwe_dimension, ks_log_basis,
                                    ks_decompose_length, chunk, &this->h_));
    }
    void extract_bits(const W *lwe_in, size_t len_in, const double *bsk, size_t len_bsk, const W *ksk, size_t len_ksk,
                      uint32_t delta_log, uint32_t bits, W *bits_out, size_t len_out) {
        check(F::bitext_extract_bits(this->h_, lwe_in, len_in, bsk, len_bsk, ksk, len_ksk, delta_log, bits, bits_out, len_out));
    }
    void extract_bits_dev(const W *lwe_in_dev, size_t len_in, const double *bsk_dev, size_t len_bsk, const W *ksk_dev,
                          size_t len_ksk, uint32_t delta_log, uint32_t bits, W *bits_out_dev, size_t len_out,
                          void *stream = nullptr) {
        check(F::bitext_extract_bits_dev(this->h_, lwe_in_dev, len_in, bsk_dev, len_bsk, ksk_dev, len_ksk, delta_log, bits,
                                       bits_out_dev, len_out, stream));
    }
};
using TfheBitExtract = TfheBitExtractT<uint64_t>;
using TfheBitExtract32 = TfheBitExtractT<uint32_t>;

}  // namespace pfhe
